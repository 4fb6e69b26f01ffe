#!/usr/bin/env python3
"""What the per-stream levels and pings cost a hop: host milliseconds of push + decode + fetch for msk144_push_hops with
msk144_set_stream_pings on against the same handle with it off (the default search: width 200, step 2, depth 4), at 1024 and 4096
streams.  The two variants alternate hop by hop in one run - the option is switched between the hops, outside the timed part - after
a warm-up of both; the figure is the median of `--reps` hops each, taken with a host clock around work that ends in
msk144_fetch_wait.  Every hop is a later hop of every stream, 2592 samples of white noise at 1000 LSB rms.  One JSON line per stream
count, with the bytes the option adds to the D2H of a hop.  Nothing is gated on it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msk144cudecoder_amd.hipdecoder import HipDecoder  # noqa: E402


def hop_ms(d, slot, n):
    t0 = time.perf_counter()
    d.push_hops(slot, n)
    d.decode()
    d.fetch_async(slot)
    d.fetch_wait(slot)
    return (time.perf_counter() - t0) * 1e3


def measure(streams, reps, warmup):
    rng = np.random.default_rng(streams)
    with HipDecoder(channels=streams, max_results=1 << 20) as d:
        hops, first, ids, is_first = d.hop_slot(0)
        hops[:] = np.rint(rng.normal(0.0, 1000.0, size=(streams, 2592))).astype(np.int16)
        first[:] = hops
        ids[:] = np.arange(streams)
        is_first[:] = 1
        hop_ms(d, 0, streams)           # every stream's first hop
        is_first[:] = 0
        on, off, up = [], [], 0
        for k in range(warmup + reps):
            d.set_stream_pings()
            a = hop_ms(d, 0, streams)
            rec, _, _ = d.stream_pings_slot(0)
            d.set_stream_pings(None)
            b = hop_ms(d, 0, streams)
            if k >= warmup:
                on.append(a)
                off.append(b)
                up += int(np.count_nonzero(rec["up_mask"]))
    return {"streams": streams, "reps": reps, "warmup": warmup,
            "on_ms_median": float(np.median(on)), "on_ms_min": float(np.min(on)), "on_ms_max": float(np.max(on)),
            "off_ms_median": float(np.median(off)), "off_ms_min": float(np.min(off)), "off_ms_max": float(np.max(off)),
            "extra_ms_median": float(np.median(on) - np.median(off)), "d2h_bytes_per_hop_added": int(streams * (32 + 32 + 54 * 4)), "streams_with_a_block_up": up}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--streams", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_pings_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for n in args.streams:
            line = json.dumps(measure(n, args.reps, args.warmup))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
