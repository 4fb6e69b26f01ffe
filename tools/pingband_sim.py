#!/usr/bin/env python3
"""CPU simulations behind the figures that include/msk144hip.h and DESIGN.md give for the ping band.  No GPU: everything runs on the
Python models (wideband.PingBand, the rule of wideband.Pings in vectorised form).

  noise        white int8 noise per component at 3 and at 20 LSB rms, --blocks blocks each (1.66 M), memory 8, min_ref 96: the
               blocks up per ratio, for the whole-channel E and for the in-band Ef of the default band
  sensitivity  the scene of tests/wideband_pings_check.py (synth pings through the float64 channeliser model) at +10, +7, +4, +2 and
               0 dB: the share of blocks wholly inside a ping that are up, whole channel at ratio 2.0 against the band at its default

    python tools/pingband_sim.py noise
    python tools/pingband_sim.py sensitivity --seeds 8
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from msk144cudecoder_amd import wideband as wb  # noqa: E402

RATIOS_Q4 = tuple(range(24, 76, 4))   # 1.5 .. 4.5 in steps of 0.25


def up_counts(streams, ratios_q4, memory=8, min_ref=96):
    """Blocks up per ratio over a run of pushes; streams yields E [channel][nb] per push.  The rule of wideband.Pings (one scale, so
    the history restarts only at the first push), vectorised over channels."""
    hist = []
    up = np.zeros(len(ratios_q4), dtype=np.int64)
    total = 0
    for E in streams:
        nb = E.shape[1]
        quiet = np.sort(E, axis=1)[:, nb // 4]
        R = np.maximum(np.min(np.stack([quiet] + hist[-memory:] if memory else [quiet]), axis=0), min_ref)
        hist = (hist + [quiet])[-wb.PING_MAX_MEMORY:]
        for i, r in enumerate(ratios_q4):
            up[i] += int(np.count_nonzero(E * 16 > R[:, None] * r))
        total += E.size
    return up, total


def noise(args):
    taps, shift = wb.ping_band_taps(args.centre, args.halfwidth)
    C_ = 64
    pushes = max(1, (args.blocks // C_ - 54) // 27)
    print(f"band {args.centre} +-{args.halfwidth} Hz, shift {shift}; {C_} streams x (54 + 27 x {pushes}) blocks, memory 8")
    for lsb in (3.0, 20.0):
        rng = np.random.default_rng([args.seed, int(lsb)])
        band = wb.PingBand(C_, taps, shift)
        pairs = []
        for k in range(pushes + 1):
            M = wb.FIRST_OUT if k == 0 else wb.HOP_OUT
            q = np.clip(np.rint(rng.standard_normal((C_, M, 2)) * lsb), -128, 127).astype(np.int8)
            pairs.append((wb.ping_blocks(q), band.push(q)))
        up_e, total = up_counts((p[0] for p in pairs), RATIOS_Q4)
        up_f, _ = up_counts((p[1] for p in pairs), RATIOS_Q4)
        print(f"noise {lsb:g} LSB rms, {total} blocks")
        for r, a, b in zip(RATIOS_Q4, up_e, up_f):
            print(f"  ratio {r / 16:.2f}: whole channel {a} up, in band {b} up")


def sensitivity(args):
    import wideband_pings_check as pc
    taps, shift = wb.ping_band_taps(0, 1500)
    print(f"scene of wideband_pings_check, seeds {pc.SCENE_SEED}..{pc.SCENE_SEED + args.seeds - 1}; band 0 +-1500 Hz shift {shift}, ratio {wb.PING_BAND_RATIO_Q4 / 16}")
    for snr in args.snr:
        inside_n = plain_up = band_up = far_plain = far_band = 0
        for seed in range(pc.SCENE_SEED, pc.SCENE_SEED + args.seeds):
            hops = pc.scene_model_hops(snr, seed)
            _, up_e, _ = pc.model_run(hops)
            _, up_f, _ = banded_run(hops, taps, shift)
            for c, _, _ in pc.SCENE_PINGS:
                inside, far = pc.scene_blocks(c, up_e.shape[1])
                inside_n += int(inside.sum())
                plain_up += int(up_e[c][inside].sum())
                band_up += int(up_f[c][inside].sum())
                far_plain += int(up_e[c][far].sum())
                far_band += int(up_f[c][far].sum())
            for c in pc.SCENE_NOISE_CHANNELS:
                far_plain += int(up_e[c].sum())
                far_band += int(up_f[c].sum())
        print(f"  {snr:+5.1f} dB: {inside_n} blocks inside; whole channel at 2.0: {100.0 * plain_up / inside_n:5.1f} % up ({far_plain} away from a ping); "
              f"band: {100.0 * band_up / inside_n:5.1f} % up ({far_band} away)")


def banded_run(hops, taps, shift, scales=100.0, min_blocks=wb.PING_MIN_BLOCKS, ratio_q4=wb.PING_BAND_RATIO_Q4):
    """As wideband_pings_check.model_run, with the band ahead of the rule."""
    import wideband_pings_check as pc
    band = wb.PingBand(hops[0].shape[0], taps, shift)
    det = wb.Pings(hops[0].shape[0], ratio_q4=ratio_q4)
    ev = wb.PingEvents(min_blocks)
    records, events = [], []
    for q in hops:
        records.append(det.push(None, scales, energies=band.push(q)))
        events += ev.push(records[-1], det.energies)
    events += ev.close()
    return records, pc.up_matrix(records), events


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="what", required=True)
    n = sub.add_parser("noise")
    n.add_argument("--blocks", type=int, default=1660000)
    n.add_argument("--centre", type=int, default=0)
    n.add_argument("--halfwidth", type=int, default=1500)
    n.add_argument("--seed", type=int, default=1)
    s = sub.add_parser("sensitivity")
    s.add_argument("--seeds", type=int, default=8)
    s.add_argument("--snr", type=float, nargs="+", default=[10.0, 7.0, 4.0, 2.0, 0.0])
    args = ap.parse_args()
    noise(args) if args.what == "noise" else sensitivity(args)


if __name__ == "__main__":
    main()
