"""What the -m gpu test files of the wideband options (levels, blanker, spectrum, pings, ping band, waterfall, capture, notch, gate
and the state table) share, each defined once: the return codes and code_of, the small shapes, the handles a module keeps, two
cached streams, and the stanzas every option's file repeats - the option leaves everything else unchanged, the same stream
twice gives the same bytes, a handle outside wideband mode refuses, a read has nothing to read.  Functions only: what is specific
to one option stays in its file."""
import contextlib
import functools

import numpy as np
import pytest

import wideband_check as wc
import wideband_gpu as wg
import wideband_levels_check as lc
import wideband_pings_check as pc
from msk144cudecoder_amd import wideband as wb

OK, EINVAL, ESTATE = 0, -1, -4
SMALL = {
    "one": dict(rate=240000, K=16, offsets=np.array([12345], dtype=np.int32)),
    "five": dict(rate=240000, K=16, offsets=pc.SCENE_OFFSETS),
}
SHAPE_NAMES = list(lc.SHAPES) + list(SMALL)


def shape_of(name):
    return lc.SHAPES[name] if name in lc.SHAPES else SMALL[name]


def code_of(hip, call):
    with pytest.raises(hip.Msk144Error) as e:
        call()
    return e.value.code


class Plain:
    """Stands for a handle where its hops are already known: the raw hops of one push."""

    def __init__(self, hops):
        self.hops, self.channels = hops, hops.shape[0]

    def dump_wideband_hop(self, c):
        return self.hops[c]


# ---- handles ----

@contextlib.contextmanager
def handle_cache(make):
    """Yields get(key): what make(key) returned on first use - a handle or a tuple of handles.  Every handle is closed on exit."""
    made = {}

    def get(key):
        if key not in made:
            made[key] = make(key)
        return made[key]

    try:
        yield get
    finally:
        for v in made.values():
            for d in v if isinstance(v, tuple) else (v,):
                d.close()


def decode_pair(hip):
    """make(C) for handle_cache: two handles of C channels with wideband_gpu.DECODE_CFG."""
    return lambda C: (hip.HipDecoder(channels=C, **wg.DECODE_CFG), hip.HipDecoder(channels=C, **wg.DECODE_CFG))


# ---- streams, built once: read-only ----

@functools.lru_cache(maxsize=None)
def rat_scene():
    """(parts, planted, format, gain): three cu8 pushes at the `rat` shape with a ping planted on channels 3, 17 and 30."""
    shape = lc.SHAPES["rat"]
    raw, planted = wg.plant_scene(wb.FIRST_OUT + 2 * wb.HOP_OUT, shape["rate"], shape["offsets"], [3, 17, 30], np.random.default_rng(55))
    raw.setflags(write=False)
    return tuple(wc.split_pushes(raw, shape["rate"], 3)), planted, "cu8", 100.0


@functools.lru_cache(maxsize=None)
def loud_push_stream(n_pushes):
    """(parts, gain): n_pushes cs16 pushes of the 5-channel scene's shape - noise at about 15 LSB rms, inside the AGC's window of
    8 .. 32, with a loud tone on channel 1 through the whole of push 2: some 120 LSB of amplitude, far above the window and
    clipping, so that the push behind it is quantised with a lower gain."""
    rate, offsets = pc.SCENE_RATE, pc.SCENE_OFFSETS
    rng = np.random.default_rng(21)
    gain = pc.burst_gain(rate)
    sizes = [k // 2 for k in wb.push_sizes_for_rate(n_pushes, rate)]
    x = (rng.standard_normal(2 * sum(sizes), dtype=np.float32) * np.float32(pc.BURST_SIGMA)).view(np.complex64)
    a0 = sizes[0] + sizes[1]
    n = np.arange(a0, a0 + sizes[2], dtype=np.int64)
    x[n] += (120.0 / (128.0 * gain) * np.exp(2j * np.pi * (np.mod(int(offsets[1]) * n, rate).astype(np.float64) / rate))).astype(np.complex64)
    raw = wb.write_samples(x, "cs16")
    raw.setflags(write=False)
    return tuple(wc.split_pushes(raw, rate, n_pushes)), gain


# ---- the stanzas ----

def _same(x, y):
    """Arrays by type, shape and bytes, tuples member by member, anything else by ==."""
    if isinstance(x, tuple):
        return isinstance(y, tuple) and len(x) == len(y) and all(_same(u, v) for u, v in zip(x, y))
    if isinstance(x, np.ndarray):
        return isinstance(y, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    return x == y


def _nonzero(x):
    """Every array and number of x has a nonzero byte."""
    if isinstance(x, tuple):
        return all(_nonzero(u) for u in x)
    return any(x.tobytes()) if isinstance(x, np.ndarray) else bool(x)


def leaves_unchanged(a, b, parts, reads=(), decode=False):
    """Push parts (the first a first push) to a, then to b - configured by the caller, the option under test on a only - and record
    after every push the hops of every channel, wideband_clip_count(), wideband_levels(), every read(d) of reads and, with `decode`,
    the sorted records of the decode.  Push by push the hops are not all zero and everything recorded on a equals what is recorded
    on b.  Returns a's [dict(hops, clip, levels, reads[, records]) per push]."""
    seen = []
    for d in (a, b):
        out = []
        for i, part in enumerate(parts):
            d.push_wideband(i % 2, part, first=i == 0)
            rec = dict(hops=wg.dump_hops(d, range(d.channels)))
            if decode:
                rec["records"] = wg._decode(d, i % 2)
            rec.update(clip=d.wideband_clip_count(), levels=d.wideband_levels(), reads=tuple(read(d) for read in reads))
            out.append(rec)
        seen.append(out)
    for i, (x, y) in enumerate(zip(*seen)):
        assert x["hops"].any(), f"push {i}: the hops are all zero"
        for what in x:
            assert _same(x[what], y[what]), f"push {i}: {what} differ with the option on"
    return seen[0]


def same_bytes_twice(d, parts, read):
    """Push parts twice, each run from a first push: read(d) after push i of the second run equals that of the first, byte for
    byte, and no array or number of it is all zero.  Returns the second run's reads."""
    runs = []
    for _ in range(2):
        out = []
        for i, part in enumerate(parts):
            d.push_wideband(i % 2, part, first=i == 0)
            out.append(read(d))
        runs.append(out)
    for i, (x, y) in enumerate(zip(*runs)):
        assert _same(x, y), f"push {i}: the second run reads other bytes"
        assert _nonzero(y), f"push {i}: all zero"
    return runs[1]


def refuses_outside_wideband_mode(hip, calls):
    """Every call(fresh) on a fresh handle, which is not in wideband mode, is refused with MSK144_EINVAL."""
    with hip.HipDecoder(channels=1, **wg.DECODE_CFG) as fresh:
        for k, call in enumerate(calls):
            assert code_of(hip, lambda: call(fresh)) == EINVAL, f"call {k}"


def unreadable(hip, reads):
    """Every read has nothing to read: MSK144_ESTATE."""
    for k, read in enumerate(reads):
        assert code_of(hip, read) == ESTATE, f"read {k}"
