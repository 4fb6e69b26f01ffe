"""What the tests of the wideband impulse-noise blanker share (CPU: test_wideband_blanker_model.py, GPU: test_gpu_wideband_blanker.py):
the three streams of the effect test and the streams with impulses planted at the edges of a push."""
from __future__ import annotations

import functools
from typing import List

import numpy as np

from msk144cudecoder_amd import wideband as wb

# ---- the effect test: what an impulsive stream does to every channel's level, and what is left of it behind the blanker ----

EFFECT_RATE = 240000
EFFECT_OFFSETS = np.array([-114000, -30000, 0, 12345, 114000], dtype=np.int32)
EFFECT_GAIN = 100.0
EFFECT_SIGMA = 200.0                       # cs16 steps per component
EFFECT_AMPLITUDE = 9000.0 * np.sqrt(2.0)   # |c| of an impulse: 33 dB over the noise's mean power 2 x 200^2


@functools.lru_cache(maxsize=None)
def effect_streams():
    """(clean, impulses, positions): one first push (103 680 samples) of cs16 noise, the same with N/1000 impulses of random phase
    added, and where they are.  The impulses' mean power is twice the noise's, so they triple every channel's power - less what
    int8 clips - and the blanker, which zeroes 11 samples per impulse, leaves 1 - 0.011 of the clean power.

    Every impulse is a hit: it lies at least 12 728 - 1 500 above the origin even against a 5 sigma noise sample, 1.2e8 in power,
    and T = 16 x 3 x 8e4 = 3.8e6.  No other sample is: T is 48 x the noise's mean power, and e^-48 x 1e5 samples is nothing."""
    N = wb.FIRST_OUT * EFFECT_RATE // wb.OUT_RATE
    rng = np.random.default_rng(5)
    noise = rng.normal(0.0, EFFECT_SIGMA, (N, 2))
    positions = np.sort(rng.choice(N, N // 1000, replace=False))
    phase = rng.uniform(0.0, 2.0 * np.pi, len(positions))
    hit = noise.copy()
    hit[positions, 0] += EFFECT_AMPLITUDE * np.cos(phase)
    hit[positions, 1] += EFFECT_AMPLITUDE * np.sin(phase)
    as_raw = lambda v: np.clip(np.rint(v), -32768, 32767).astype(np.int16).reshape(-1)
    return as_raw(noise), as_raw(hit), positions


def assert_effect(sum_sq_clean, sum_sq_impulses, sum_sq_blanked):
    """The per-channel assertions of the effect test, on sum_sq [channel] of the three streams."""
    clean = np.asarray(sum_sq_clean, dtype=np.float64)
    up, back = np.asarray(sum_sq_impulses) / clean, np.asarray(sum_sq_blanked) / clean
    print("impulses/clean", np.round(up, 3), "blanked/clean", np.round(back, 4))
    assert np.all(up >= 1.8), up
    assert np.all((back >= 0.97) & (back <= 1.01)), back


# ---- streams with impulses at the edges of a push ----

def edge_pushes(rate: int, fmt: str, n_pushes: int, pre: int, post: int, rng: np.random.Generator, sigma: float = 0.05, random_impulses: int = 6) -> List[np.ndarray]:
    """Raw pushes of white noise (sigma per rail, full scale 1) with full-scale impulses: a few at random, one at n = 0, N - 1 and
    N - post + 1 of some push each - so that a guard is cut at the start of a push, owes `post` and 2 samples to the next one, and a
    push begins with samples owed and a hit of its own - and two closer than pre + post.  A full-scale sample is 0.95^2 / sigma^2 =
    361 x the noise's mean power per component pair, a hit at any threshold the tests use below 4096 x."""
    P, Q = wb.rate_ratio(rate)
    out = []
    for i in range(n_pushes):
        N = (wb.FIRST_OUT if i == 0 else wb.HOP_OUT) * P // Q
        x = sigma * (rng.normal(size=N) + 1j * rng.normal(size=N))
        at = [int(v) for v in rng.integers(0, N, size=random_impulses)]
        a = int(rng.integers(N // 4, N // 2))
        at += [a, a + max(1, (pre + post) // 2)]
        if i % 3 == 0:
            at.append(0)
        if i % 3 == 1 or i == n_pushes - 1:
            at.append(N - 1)
        if i % 3 == 2 and post >= 2:
            at.append(N - post + 1)
        if i == 3:
            at += [0, N - 1]
        x[at] = 0.95 * np.exp(2j * np.pi * rng.uniform(size=len(at))) * np.sqrt(2.0)
        out.append(wb.write_samples(x, fmt))
    return out
