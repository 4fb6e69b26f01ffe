"""What the tests of the wideband input spectrum share (CPU: test_wideband_spectrum_model.py, GPU: test_gpu_wideband_spectrum.py):
the error bound of the contract (include/msk144hip.h), the test stream and its pushes.

The bound.  With T = sum_k P[k], u the relative l2 error of one f32 transform and v = 4 x 2^-24 the rounding of re^2 + im^2,

    |P^[k] - P[k]| <= 2 u sqrt(P[k] T) + u^2 T + v P[k]

(|dX_s[k]| <= ||dX_s||_2 <= u ||X_s||_2, then Cauchy-Schwarz over the segments).  U is the contract's value of u,
MSK144_SPECTRUM_U: 4 x the largest u any bin of the GPU tests' inputs needed on an MI355X (needed_u below, the figures are in
DESIGN 4.4 and in the parity report of every -m gpu run), rounded up to one significant digit.  The margin covers other seeds and
another compiler's butterfly order, not another algorithm, and U must lie below the textbook ceiling of a radix-2 transform with
f32 twiddles, window multiply and input conversion, 8 x 2^-24 x log2 B (ceiling below), at every B.

The stream: Gaussian noise of sigma 0.05 per rail, a full-scale tone on a bin centre of every B (a multiple of Fs/256), a tone
between the bins of every B (an odd multiple of Fs/16384) 40 dB below it, and one single-sample full-scale impulse per push - bins
from 0 dBFS down to the f32 floor in one spectrum.  What leaves the rails is clipped by the format, as a receiver's converter does.
"""
from __future__ import annotations

import functools
from typing import List

import numpy as np

import wideband_check as wc
from msk144cudecoder_amd import wideband as wb

V = 4.0 * 2.0 ** -24
U = 2e-7     # largest needed: 3.9e-8 (B = 8192, cs8, random window)
BINS = (256, 512, 1024, 2048, 4096, 8192)
TONE_BIN_OF_256 = 37          # the full-scale tone: +37 Fs/256
BETWEEN_BIN_OF_16384 = -2731  # the -40 dB tone: -(2731 / 16384) Fs, half way between two bins of B = 8192 and between bins of every smaller B
SIGMA = 0.05


def ceiling(bins: int) -> float:
    return 8.0 * 2.0 ** -24 * np.log2(bins)


def bound(P: np.ndarray, u: float) -> np.ndarray:
    T = float(np.sum(P))
    return 2.0 * u * np.sqrt(P * T) + u * u * T + V * P


def needed_u(got: np.ndarray, want: np.ndarray) -> float:
    """The smallest u for which every bin of `got` satisfies the bound against the exact `want`."""
    T = float(np.sum(want))
    d = np.maximum(np.abs(got - want) - V * want, 0.0)
    root = np.sqrt(want * T)
    return float(np.max(d / (np.sqrt(want * T + T * d) + root)))   # the positive root of u^2 T + 2 u sqrt(P T) - d = 0


def assert_within(got, want, u: float, what: str) -> float:
    """Print what the comparison needs, then hold every bin to the bound with u."""
    need = needed_u(got, want)
    print(f"{what}: needs u = {need:.3e} (bound with u = {u:.1e})")
    worst = int(np.argmax(np.abs(got - want) - bound(want, u)))
    assert np.all(np.abs(got - want) <= bound(want, u)), f"{what}: bin {worst} reads {got[worst]!r}, the model {want[worst]!r}; needs u = {need:.3e}"
    return need


def stream(rate: int, n_pushes: int, seed) -> np.ndarray:
    """complex128: n_pushes pushes of the test stream at `rate` (float, before the format's rounding and clipping)."""
    P, Q = wb.rate_ratio(rate)
    sizes = [k // 2 for k in wb.push_sizes_for_rate(n_pushes, rate)]
    n = sum(sizes)
    rng = np.random.default_rng(seed)
    x = SIGMA * (rng.normal(size=n) + 1j * rng.normal(size=n))
    t = np.arange(n, dtype=np.int64)
    x += np.exp(2j * np.pi * (np.mod(TONE_BIN_OF_256 * t, 256) / 256.0))
    x += 0.01 * np.exp(2j * np.pi * (np.mod(BETWEEN_BIN_OF_16384 * t, 16384) / 16384.0 + 0.123))
    start = 0
    for k in sizes:
        x[start + int(rng.integers(0, k))] = (1.0 + 1.0j) * rng.choice([-1.0, 1.0])
        start += k
    return x


@functools.lru_cache(maxsize=None)
def pushes(rate: int, fmt: str, n_pushes: int, seed: int = 0) -> tuple:
    """The raw pushes of the test stream in fmt (shared, do not modify)."""
    raw = wb.write_samples(stream(rate, n_pushes, [rate, seed]), fmt)
    raw.setflags(write=False)
    return tuple(wc.split_pushes(raw, rate, n_pushes))


def random_window(bins: int, seed: int) -> np.ndarray:
    """A seeded positive window: uniform in 0.1 .. 1."""
    return np.random.default_rng([bins, seed]).uniform(0.1, 1.0, bins)


def tone_slot(bins: int) -> int:
    """The ascending-frequency slot of the full-scale tone."""
    return bins // 2 + TONE_BIN_OF_256 * bins // 256
