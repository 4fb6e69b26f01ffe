"""Where the default ratio of msk144_set_stream_pings comes from (the table in csrc/stream_pings.h): the Python model on noise alone.

Gaussian noise band-limited to 300..2700 Hz (an SSB receiver's audio) at rms 30, 100 and 1000 LSB, one stream per level, through
stream_pings.StreamPings at shift 12, memory 8 and min_ref 1 (the floor would hide the quiet stream).  For every block E/R is taken
from the records; a block is up at ratio r iff E x 16 > R x 16r.  Prints the table and the smallest multiple of 0.25 at which no
block is up.  CPU only, numpy only:  python tools/stream_pings_sim.py [--hops 3000] [--seed 1]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msk144cudecoder_amd.stream_pings import HOP_SAMPLES, StreamPings  # noqa: E402

LEVELS = (30, 100, 1000)
RATIOS_Q4 = (32, 48, 52, 56)


def band_noise(n: int, rms: float, rng: np.random.Generator) -> np.ndarray:
    """n int16 samples at 12 kHz of Gaussian noise with nothing outside 300..2700 Hz, scaled to `rms` LSB before rounding."""
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / 12000.0)
    X[(f < 300.0) | (f > 2700.0)] = 0.0
    x = np.fft.irfft(X, n)
    return np.clip(np.rint(x * (rms / np.sqrt(np.mean(x * x)))), -32768, 32767).astype(np.int16)


def run(hops: int, seed: int):
    """Per level: (median quiet level, blocks, E x 16 and R of every block as int64 arrays)."""
    rng = np.random.default_rng(seed)
    n = (hops + 1) * HOP_SAMPLES
    x = [band_noise(n, rms, rng) for rms in LEVELS]
    sp = StreamPings(len(LEVELS), ratio_q4=16, memory=8, min_ref=1, shift=12)
    ids = list(range(len(LEVELS)))
    E16 = [[] for _ in LEVELS]
    R = [[] for _ in LEVELS]
    quiet = [[] for _ in LEVELS]
    for k in range(hops):
        first = k == 0
        lo, hi = (0, 2 * HOP_SAMPLES) if first else ((k + 1) * HOP_SAMPLES, (k + 2) * HOP_SAMPLES)
        rec, _, en, _ = sp.push(ids, [first] * len(ids), [v[lo:hi] for v in x])
        for s in ids:
            nb = int(rec["blocks"][s])
            E16[s].append(en[s, :nb] * 16)
            R[s].append(np.full(nb, int(rec["reference"][s]), dtype=np.int64))
            quiet[s].append(int(rec["quiet"][s]))
    return [(int(np.median(quiet[s])), np.concatenate(E16[s]), np.concatenate(R[s])) for s in ids]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--hops", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    worst = 0.0
    print("rms LSB  quiet (median)  blocks  worst E/R  " + "  ".join(f"up at {q / 16:g}" for q in RATIOS_Q4))
    results = run(a.hops, a.seed)
    for rms, (quiet, E16, R) in zip(LEVELS, results):
        w = float(np.max(E16 / (16.0 * R)))
        worst = max(worst, w)
        ups = "  ".join(f"{100.0 * np.count_nonzero(E16 > R * q) / E16.size:8.3f} %" for q in RATIOS_Q4)
        print(f"{rms:7d}  {quiet:14d}  {E16.size:6d}  {w:9.3f}  {ups}")
    q4 = 16
    while any(np.any(E16 > R * q4) for _, E16, R in results):   # the integer up rule itself
        q4 += 4
    print(f"worst E/R {worst:.3f}: the smallest multiple of 0.25 with no block up is {q4 / 16:g} (ratio_q4 = {q4})")


if __name__ == "__main__":
    main()
