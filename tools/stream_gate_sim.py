"""What the stream gate keeps and what it lets through, at its own RATIO (the table in csrc/stream_gate.h and DESIGN 8 f-4): a CPU
simulation of the models against the oracle decoder.  Nothing here was run on the air.

Streams are synth.synth_audio - white noise of 1000 LSB with MSK144 pings of three frames (216 ms) at 1500 Hz, one every eight hops
at a seeded offset - behind an SSB receiver's 300..2700 Hz audio filter, so the noise is 300..2700 Hz noise and the SNR in 2500 Hz
is what synth_audio was given.  One stream per ping level from -4 to +10 dB in 2 dB steps, and one stream of noise alone.  Every
stream goes hop by hop through stream_pings.StreamPings at its defaults (ratio 3.5) and, fed those records, through one
stream_pings.StreamGate per RATIO (hold 1, min_up 1; RATIO 3.5 is ratio_q4 = 0, the detector's own mask).  The oracle decoder
(width 20 Hz, step 2 Hz, depth 4 around the ping's 1500 Hz, to keep the run short) decodes every window that overlaps a ping; a window
counts as decoded when the oracle returns the transmitted payload.  Printed per RATIO: of the windows the oracle decodes at each
level, the share the gate lists; and of the windows of the noise-only stream, the share it lists.

CPU only:  python tools/stream_gate_sim.py [--pings 40] [--noise-hops 3000] [--seed 1]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msk144cudecoder_amd import synth  # noqa: E402
from msk144cudecoder_amd.stream_pings import HOP_SAMPLES, StreamGate, StreamPings  # noqa: E402

LEVELS_DB = tuple(range(-4, 11, 2))
RATIOS = (3.5, 2.5, 2.0, 1.75, 1.5)
SIGMA = 1000.0
FRAMES = 3
PERIOD = 8            # hops between pings: far more than hold + the detector's memory of a ping needs to run out
FRAME_SAMPLES = 864


def ssb(x: np.ndarray) -> np.ndarray:
    """The stream behind a 300..2700 Hz audio filter, int16."""
    X = np.fft.rfft(x.astype(np.float64))
    f = np.fft.rfftfreq(len(x), 1.0 / 12000.0)
    X[(f < 300.0) | (f > 2700.0)] = 0.0
    return np.clip(np.rint(np.fft.irfft(X, len(x))), -32768, 32767).astype(np.int16)


def ping_stream(snr_db: float, pings: int, rng: np.random.Generator):
    """(samples, [(first sample, payload)]): `pings` pings, the k-th somewhere in hops 8k + 3 .. 8k + 4."""
    hops = PERIOD * pings + 4
    n = (hops + 1) * HOP_SAMPLES
    plist, where = [], []
    for k in range(pings):
        start = (PERIOD * k + 3) * HOP_SAMPLES + int(rng.integers(0, HOP_SAMPLES))
        msg = synth.random_message(rng)
        plist.append(synth.Ping(msg, start, FRAMES, 1500.0, float(snr_db), float(rng.uniform(0, 2 * np.pi))))
        where.append((start, msg))
    return ssb(synth.synth_audio(n, plist, SIGMA, rng)), where


def gate_lists(x: np.ndarray, ratios_q4):
    """listed[r][k]: whether the gate at ratio r lists window k (samples 2592 k .. 2592 k + 5183) of the one stream x."""
    hops = len(x) // HOP_SAMPLES - 1
    pings = StreamPings(1)
    gates = [StreamGate(1, ratio_q4=q) for q in ratios_q4]
    listed = np.zeros((len(gates), hops), dtype=bool)
    for k in range(hops):
        first = k == 0
        lo, hi = (0, 2 * HOP_SAMPLES) if first else ((k + 1) * HOP_SAMPLES, (k + 2) * HOP_SAMPLES)
        rec, _, en, _ = pings.push([0], [first], [x[lo:hi]])
        for r, g in enumerate(gates):
            listed[r, k] = len(g.push([0], [first], rec, en)[0]) == 1
    return listed


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pings", type=int, default=40, help="pings per level")
    ap.add_argument("--noise-hops", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threads", type=int, default=4)
    a = ap.parse_args()
    from oracle import oracle as orc
    o = orc.Oracle(center=1500.0, width=20.0, step=2.0, depth=4, threads=a.threads)
    rng = np.random.default_rng(a.seed)
    ratios_q4 = [0 if r == 3.5 else int(round(16 * r)) for r in RATIOS]
    print(f"{a.pings} pings of {FRAMES} frames per level, noise {SIGMA:g} LSB behind 300..2700 Hz, hold 1, min_up 1, detector at its defaults; seed {a.seed}")
    print("ping dB  windows with ping  oracle decodes  " + "  ".join(f"listed at {r:g}" for r in RATIOS))
    kept, decoded_all = np.zeros(len(RATIOS), dtype=np.int64), 0
    for db in LEVELS_DB:
        x, where = ping_stream(db, a.pings, rng)
        listed = gate_lists(x, ratios_q4)
        hops = listed.shape[1]
        with_ping = decoded = 0
        hit = np.zeros(len(RATIOS), dtype=np.int64)
        for start, msg in where:
            end = start + FRAMES * FRAME_SAMPLES
            for k in range(max(0, (start - 5184) // HOP_SAMPLES + 1), min(hops, end // HOP_SAMPLES + 1)):
                if not (k * HOP_SAMPLES < end and k * HOP_SAMPLES + 5184 > start):
                    continue
                with_ping += 1
                items, _ = o.decode_window(o.frontend_audio(x[k * HOP_SAMPLES:k * HOP_SAMPLES + 5184], 2))
                got = items["message"][items["is_message_present"] == 1]
                if any(bytes(np.asarray(m, dtype=np.uint8)) == bytes(msg) for m in got):
                    decoded += 1
                    hit += listed[:, k]
        kept += hit
        decoded_all += decoded
        print(f"{db:7d}  {with_ping:17d}  {decoded:14d}  " + "  ".join(f"{h:5d} {100.0 * h / decoded if decoded else 0.0:5.1f} %" for h in hit), flush=True)
    print(f"    all  {'':17s}  {decoded_all:14d}  " + "  ".join(f"{h:5d} {100.0 * h / decoded_all if decoded_all else 0.0:5.1f} %" for h in kept))
    noise = ssb(synth.synth_audio((a.noise_hops + 1) * HOP_SAMPLES, [], SIGMA, rng))
    listed = gate_lists(noise, ratios_q4)
    print(f"noise-only windows listed, of {listed.shape[1]}:  " + "  ".join(f"at {r:g}: {int(n)} ({100.0 * n / listed.shape[1]:.2f} %)" for r, n in zip(RATIOS, listed.sum(axis=1))))
    print("A CPU simulation of the models and the oracle decoder; nothing was run on the air.")


if __name__ == "__main__":
    main()
