#!/usr/bin/env python3
"""What the resampler in front of the hop ring costs a hop: host milliseconds of push + decode + fetch for msk144_push_rate_hops
at 48000 and 192000 Hz against msk144_push_hops on the same handle configuration (the default search: width 200, step 2, depth 4),
at 1024 and 4096 streams.  The two variants alternate hop by hop in one run, after a warm-up of both; the figure is the median of
`--reps` hops each, taken with a host clock around work that ends in msk144_fetch_wait.  Every hop is a later hop of every stream
(2592 new samples at 12 kHz, 2592 P/Q at the input rate) of white noise at 1000 LSB rms.  One JSON line per (streams, rate), with
the pinned bytes per slot of both paths.  Nothing is gated on it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msk144cudecoder_amd import input_rate as ir  # noqa: E402
from msk144cudecoder_amd.hipdecoder import HipDecoder  # noqa: E402


def hop_ms(d, push, slot, n):
    t0 = time.perf_counter()
    push(slot, n)
    d.decode()
    d.fetch_async(slot)
    d.fetch_wait(slot)
    return (time.perf_counter() - t0) * 1e3


def measure(streams, rate, reps, warmup):
    row = ir.row_samples(rate)
    rng = np.random.default_rng(streams + rate)
    with HipDecoder(channels=streams, max_results=1 << 20) as d:
        d.set_input_rate(rate)
        # slot 0 carries the hops at the input rate, slot 1 those at 12 kHz; both are filled once
        r_hops, r_first, ids, is_first = d.rate_hop_slot(0)
        hops, first, ids1, is_first1 = d.hop_slot(1)
        noise = lambda n: np.rint(rng.normal(0.0, 1000.0, size=(streams, n))).astype(np.int16)
        r_hops[:] = noise(row)
        r_first[:] = r_hops
        hops[:] = noise(2592)
        first[:] = hops
        ids[:] = np.arange(streams)
        ids1[:] = np.arange(streams)
        is_first[:] = 1
        is_first1[:] = 1
        hop_ms(d, d.push_rate_hops, 0, streams)    # every stream's first hop, both paths
        hop_ms(d, d.push_hops, 1, streams)
        is_first[:] = 0
        is_first1[:] = 0
        for _ in range(warmup):
            hop_ms(d, d.push_rate_hops, 0, streams)
            hop_ms(d, d.push_hops, 1, streams)
        a, b = [], []
        for _ in range(reps):
            a.append(hop_ms(d, d.push_rate_hops, 0, streams))
            b.append(hop_ms(d, d.push_hops, 1, streams))
        clamped = int(d.input_rate_clamped().sum())
    return {"streams": streams, "rate_hz": rate, "reps": reps, "warmup": warmup,
            "push_rate_hops_ms_median": float(np.median(a)), "push_rate_hops_ms_min": float(np.min(a)), "push_rate_hops_ms_max": float(np.max(a)),
            "push_hops_ms_median": float(np.median(b)), "push_hops_ms_min": float(np.min(b)), "push_hops_ms_max": float(np.max(b)),
            "extra_ms_median": float(np.median(a) - np.median(b)),
            "h2d_bytes_per_hop_rate": int(streams * row * 2), "h2d_bytes_per_hop_12k": int(streams * 2592 * 2),
            "pinned_bytes_per_slot_rate": int(2 * streams * row * 2), "pinned_bytes_per_slot_12k": int(2 * streams * 2592 * 2), "clamped_last_hop": clamped}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--streams", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--rates", type=int, nargs="+", default=[48000, 192000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_rate_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for n in args.streams:
            for rate in args.rates:
                line = json.dumps(measure(n, rate, args.reps, args.warmup))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
