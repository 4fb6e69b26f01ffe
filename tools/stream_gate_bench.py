#!/usr/bin/env python3
"""What the stream gate saves and costs a hop: host milliseconds of push + decode + fetch for msk144_push_hops with
msk144_set_stream_gate on against the same handle with it off (the default search: width 200, step 2, depth 4), at 1024 and 4096
streams.  The detector is off, so the `always` flags alone decide: the share of streams listed is 0, 0.1, 0.5 and 1 (every
round(1 / share)-th stream, spread over the handle).  Gate on and gate off alternate hop by hop on one handle - the gate is switched
between the hops, outside the timed part - after a warm-up of both; the figure is the median of `--reps` hops each, with max - min
beside it, taken with a host clock around work that ends in msk144_fetch_wait.  The figure to compare against is the gate-off leg of
the same run on the same box.  Share 1 over gate-off is what the gate itself costs: the plan, the gather and the one host wait.
Every hop is a later hop of every stream, 2592 samples of white noise at 1000 LSB rms.  One JSON line per stream count and share.
Nothing is gated on it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msk144cudecoder_amd.hipdecoder import HipDecoder  # noqa: E402

SHARES = (0.0, 0.1, 0.5, 1.0)


def hop_ms(d, slot, n):
    t0 = time.perf_counter()
    d.push_hops(slot, n)
    d.decode()
    d.fetch_async(slot)
    d.fetch_wait(slot)
    return (time.perf_counter() - t0) * 1e3


def always_for(streams, share):
    if share <= 0.0:
        return []
    want = max(1, int(round(streams * share)))
    return sorted({int(i * streams / want) for i in range(want)})


def measure(streams, reps, warmup):
    rng = np.random.default_rng(streams)
    out = []
    with HipDecoder(channels=streams, max_results=1 << 20) as d:
        hops, first, ids, is_first = d.hop_slot(0)
        hops[:] = np.rint(rng.normal(0.0, 1000.0, size=(streams, 2592))).astype(np.int16)
        first[:] = hops
        ids[:] = np.arange(streams)
        is_first[:] = 1
        hop_ms(d, 0, streams)           # every stream's first hop
        is_first[:] = 0
        for share in SHARES:
            always = always_for(streams, share)
            on, off, listed = [], [], set()
            for k in range(warmup + reps):
                d.set_stream_gate(always=always)
                a = hop_ms(d, 0, streams)
                listed.add(len(d.stream_gate_slot(0)[0]))
                d.set_stream_gate(None)
                b = hop_ms(d, 0, streams)
                if k >= warmup:
                    on.append(a)
                    off.append(b)
            assert listed == {len(always)}, (listed, len(always))
            out.append({"streams": streams, "share": share, "listed": len(always), "reps": reps, "warmup": warmup,
                        "on_ms_median": float(np.median(on)), "on_ms_spread": float(np.max(on) - np.min(on)),
                        "off_ms_median": float(np.median(off)), "off_ms_spread": float(np.max(off) - np.min(off)),
                        "on_minus_off_ms": float(np.median(on) - np.median(off)), "store_bytes": int(streams) * 5184 * 8})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--streams", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_gate_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for n in args.streams:
            for row in measure(n, args.reps, args.warmup):
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
