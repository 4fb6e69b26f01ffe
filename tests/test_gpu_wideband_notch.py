"""-m gpu: the notch of the wideband contract (include/msk144hip.h, csrc/notch.hip) against its Python model, byte for byte and with no
tolerance.  Two handles take the same stream, the notch on handle A only; after every push wideband.Notch is fed handle B's
dump_wideband_hop of every channel, and handle A's dump and wideband_notch_stats equal what it gives
(wideband_notch_check.assert_push).

1. Shapes: the three of wideband_levels_check.py, a 1-channel and a 5-channel handle, cu8 and cs16: one first push (two staged rows)
   and three later ones of noise with two tone bursts.  Tables: no channel; one channel with the default taps and with random taps
   (-128 among them) at shifts 0 and 15; every channel, and a strict subset (the active list is shorter than the handle), each with
   those three kinds of entry dealt out over its channels.
2. Identities on the device: all-zero taps give the input delayed by 31 samples across the push boundaries; taps[31] = (64, 0) with
   shift 6 gives all zeros.
3. Extremes through the channeliser: cs16 zeros; a gain at which every component clips, with taps of +-127 and shift 0: the count of
   clamped components equals the model's.
4. What it does not touch: the channels not in the table, the levels and the clip count equal handle B's; with the ping band and the
   pings on, the models of those stages fed the notched hops match the device.
5. Switching: every EINVAL and ESTATE case; a changed entry zeroes that channel's tail only, an unchanged one keeps its tail; None
   switches the notch off; msk144_set_wideband switches it off; the same stream pushed twice gives the same bytes.
6. End to end: the scene of test_wideband_notch_decode.py as cs16 through push_wideband and decode.  With the notches every planted
   message is decoded on its own channel, without them strictly fewer are; once through the program with
   --wideband-notch=<the fixed table>: the same messages and the summary line.
"""
import numpy as np
import pytest

import wideband_gpu as wg
import wideband_levels_check as lc
import wideband_notch_check as nc
import wideband_options as wo
import wideband_pingband_check as bc
import wideband_pings_check as pc
from msk144cudecoder_amd import wideband as wb
from wideband_options import EINVAL, SMALL, Plain, code_of, shape_of

pytestmark = pytest.mark.gpu

def entry(kind: int, c: int):
    """The three kinds of entry: the default design (the bursts sit on the channel's offset: 0 Hz is among its carriers), random
    taps at shift 0, random taps at shift 15."""
    if kind == 0:
        return wb.notch_taps([0] if c % 2 == 0 else [-700 + 10 * (c % 7), 900])
    return nc.random_taps(c), 0 if kind == 1 else 15


def tables(C):
    """(name, table) of every table of test 1 for a handle of C channels."""
    out = [("none", {})]
    one = int(pc.BURSTS[0][0] * (C - 1))            # the channel of the first burst
    out += [(f"one/{kind}", {one: entry(kind, one)}) for kind in range(3)]
    out.append(("every", {c: entry(c % 3, c) for c in range(C)}))
    if C > 1:
        out.append(("subset", {c: entry((c // 2) % 3, c) for c in range(C) if c % 2 == 1 or c == one}))
    return out


@pytest.fixture(scope="module")
def handles(hip):
    """Two handles per channel count, made on first use and kept for the module."""
    with wo.handle_cache(wo.decode_pair(hip)) as get:
        yield get


# ---- 1. shapes ----

@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
@pytest.mark.parametrize("name", wo.SHAPE_NAMES)
def test_shapes_against_the_model(handles, name, fmt):
    shape = shape_of(name)
    rate, offsets = shape["rate"], shape["offsets"]
    C_ = len(offsets)
    a, b = handles(C_)
    parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), fmt)
    b.set_wideband(rate, offsets, fmt, taps_per_phase=shape["K"], gain=pc.burst_gain(rate))
    raw = []
    for i, part in enumerate(parts):
        b.push_wideband(i % 2, part, first=i == 0)
        raw.append(wg.dump_hops(b, range(C_)))
    assert [r.shape[1] for r in raw] == [5184, 2592, 2592, 2592]
    a.set_wideband(rate, offsets, fmt, taps_per_phase=shape["K"], gain=pc.burst_gain(rate))
    for tname, table in tables(C_):
        a.set_wideband_notch(table)
        model = wb.Notch(C_, table)
        changed = clamped = 0
        for i, part in enumerate(parts):
            a.push_wideband(i % 2, part, first=i == 0)
            got, _, k = nc.assert_push(a, Plain(raw[i]), model, f"{name} {fmt} {tname} push {i}")
            changed += int(np.count_nonzero(got != raw[i]))
            clamped += int(k.sum())
        print(f"{name} {fmt} {tname}: {len(table)} of {C_} channels, {changed} components changed, {clamped} clamped")
        assert (changed > 0) == bool(table)
    a.set_wideband_notch(None)
    a.synchronize()
    b.synchronize()


# ---- 2. identities on the device ----

def test_pure_delay_and_all_zeros(handles):
    shape = lc.SHAPES["rat"]
    rate, offsets = shape["rate"], shape["offsets"]
    C_ = len(offsets)
    a, b = handles(C_)
    parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), "cu8")
    for d in (a, b):
        d.set_wideband(rate, offsets, "cu8", taps_per_phase=shape["K"], gain=pc.burst_gain(rate))
    zero = np.zeros((64, 2), dtype=np.int8)
    table = {c: (zero, c % 16) if c % 3 else (nc.delta(31, 64, 0), 6) for c in range(C_) if c != 1}
    a.set_wideband_notch(table)
    model = wb.Notch(C_, table)
    stream = [np.zeros((C_, 31, 2), dtype=np.int8)]
    for i, part in enumerate(parts):
        for d in (a, b):
            d.push_wideband(i % 2, part, first=i == 0)
        got, raw, k = nc.assert_push(a, b, model, f"identities push {i}")
        stream.append(raw)
        whole = np.concatenate(stream, axis=1)
        delayed = whole[:, whole.shape[1] - raw.shape[1] - 31:whole.shape[1] - 31]
        assert raw.any() and not k.any()
        for c in range(C_):
            if c == 1:
                assert np.array_equal(got[c], raw[c])
            elif c % 3:
                assert np.array_equal(got[c], delayed[c]), f"push {i} ch={c}: not the input delayed by 31 samples"
            else:
                assert not got[c].any(), f"push {i} ch={c}: not all zero"
    a.set_wideband_notch(None)
    a.synchronize()
    b.synchronize()


# ---- 3. extremes through the channeliser ----

def test_all_zero_and_all_clipped_hops(handles):
    C_ = len(pc.SCENE_OFFSETS)
    a, b = handles(C_)
    sizes = wb.push_sizes_for_rate(2, pc.SCENE_RATE)
    table = {c: [300, -700] for c in range(C_)}
    for d in (a, b):
        d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16")
    a.set_wideband_notch(table)
    model = wb.Notch(C_, table)
    for i, n in enumerate(sizes):
        for d in (a, b):
            d.push_wideband(i % 2, np.zeros(n, dtype=np.int16), first=i == 0)
        got, _, k = nc.assert_push(a, b, model, f"zeros push {i}")
        assert not got.any() and not k.any()
    # every component clipped, taps of +-127, shift 0: nearly every output is clamped
    rng = np.random.default_rng(8)
    table = {c: ((127 * (2 * rng.integers(0, 2, size=(64, 2)) - 1)).astype(np.int8), 0) for c in range(C_)}
    for d in (a, b):
        d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16", gain=1e9)
    a.set_wideband_notch(table)
    model = wb.Notch(C_, table)
    for i, n in enumerate(sizes):
        part = rng.integers(-3000, 3000, size=n).astype(np.int16)
        for d in (a, b):
            d.push_wideband(i % 2, part, first=i == 0)
        got, raw, k = nc.assert_push(a, b, model, f"clipped push {i}")
        assert np.abs(raw.astype(np.int32)).min() >= 127, "not every component is clipped"
        print(f"clipped push {i}: clamped {list(k)} of {2 * raw.shape[1]} components per channel")
        assert k.min() > raw.shape[1] and np.abs(got.astype(np.int32)).max() == 128
    a.set_wideband_notch(None)
    a.synchronize()
    b.synchronize()


# ---- 4. what it does not touch ----

def test_what_it_does_not_touch(handles):
    shape = SMALL["five"]
    rate, offsets = shape["rate"], shape["offsets"]
    C_ = len(offsets)
    a, b = handles(C_)
    parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), "cs16")
    taps, shift = wb.ping_band_taps()
    for d in (a, b):
        d.set_wideband(rate, offsets, "cs16", taps_per_phase=shape["K"], gain=pc.burst_gain(rate))
        d.set_wideband_pings(ratio_q4=wb.PING_BAND_RATIO_Q4)
        d.set_wideband_ping_band()
    table = {1: [0], 3: [0, 1500]}                  # the bursts sit on channels 1 and 3, at their offsets
    a.set_wideband_notch(table)
    model = wb.Notch(C_, table)
    band, det = wb.PingBand(C_, taps, shift), wb.Pings(C_, ratio_q4=wb.PING_BAND_RATIO_Q4)
    band_b, det_b = wb.PingBand(C_, taps, shift), wb.Pings(C_, ratio_q4=wb.PING_BAND_RATIO_Q4)
    differ = 0
    for i, part in enumerate(parts):
        for d in (a, b):
            d.push_wideband(i % 2, part, first=i == 0)
        got, raw, _ = nc.assert_push(a, b, model, f"push {i}")
        for c in (0, 2, 4):
            assert np.array_equal(got[c], raw[c]), f"push {i}: ch={c} is not in the table"
        assert a.wideband_levels().tobytes() == b.wideband_levels().tobytes() and a.wideband_clip_count() == b.wideband_clip_count(), f"push {i}"
        # the ping band and the detector see the notched hops
        rec_a, _, _ = bc.assert_push(a, band, det, f"notched, push {i}")
        rec_b, _, _ = bc.assert_push(b, band_b, det_b, f"plain, push {i}")
        differ += int(np.count_nonzero(rec_a["peak"] != rec_b["peak"]))
        assert np.array_equal(rec_a["peak"][[0, 2, 4]], rec_b["peak"][[0, 2, 4]])
    assert differ > 0                               # the bursts are carriers to the notch: the in-band peaks of channels 1 and 3 moved
    for d in (a, b):
        d.set_wideband_ping_band(None)
        d.set_wideband_pings(None)
    a.set_wideband_notch(None)
    a.synchronize()
    b.synchronize()


# ---- 5. switching ----

def test_order_and_refusals(hip, handles):
    rate, offsets = pc.SCENE_RATE, pc.SCENE_OFFSETS
    C_ = len(offsets)
    a, b = handles(C_)
    parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), "cs16")
    gain = pc.burst_gain(rate)
    L = a.L
    import ctypes as C

    def raw_set(d, channels, params, count=None):
        ch = (C.c_int32 * max(len(channels), 1))(*channels)
        return L.msk144_set_wideband_notch(d.h, ch, len(channels) if count is None else count, params)

    good = (hip.WidebandNotchParams * C_)()
    wo.refuses_outside_wideband_mode(hip, [lambda f: f.set_wideband_notch({0: [0]}), lambda f: f.set_wideband_notch(None), hip.HipDecoder.wideband_notch_stats])
    for d in (a, b):
        d.set_wideband(rate, offsets, "cs16", gain=gain)
    assert raw_set(a, [0, 0], good) == EINVAL and b"twice" in L.msk144_last_error(a.h)
    assert raw_set(a, [C_], good) == EINVAL and raw_set(a, [-1], good) == EINVAL and raw_set(a, [0, 5], good) == EINVAL
    assert raw_set(a, list(range(C_)), good, count=C_ + 1) == EINVAL and raw_set(a, [0], good, count=-1) == EINVAL
    assert raw_set(a, [0], None) == EINVAL
    for bad in (-1, 16, 40, 1 << 20, -(1 << 31)):
        assert code_of(hip, lambda: a.set_wideband_notch({2: (nc.random_taps(0), bad)})) == EINVAL, bad
    for ok in (0, 15):
        a.set_wideband_notch({2: (np.full((64, 2), -128, dtype=np.int8), ok)})
    # ESTATE: before any push, before a push with the notch on, and again after a new table
    wo.unreadable(hip, [a.wideband_notch_stats])
    a.set_wideband_notch(None)
    a.push_wideband(0, parts[0], first=True)
    wo.unreadable(hip, [a.wideband_notch_stats])
    b.push_wideband(0, parts[0], first=True)

    # set in mid-stream: the table's channels start from silence on the next push
    t0 = {0: [300], 3: [0, 1500]}
    a.set_wideband_notch(t0)
    wo.unreadable(hip, [a.wideband_notch_stats])
    model = wb.Notch(C_, t0)
    for d in (a, b):
        d.push_wideband(1, parts[1], first=False)
    nc.assert_push(a, b, model, "set in mid-stream")
    assert model.tail[0].any() and model.tail[3].any()
    # 0 unchanged: keeps its tail; 3 changed, 1 new: zero tails.  A filter that had cleared channel 0's tail would differ
    t1 = {0: wb.notch_taps([300]), 1: [0], 3: [0, 1600]}
    a.set_wideband_notch(t1)
    wo.unreadable(hip, [a.wideband_notch_stats])
    model.set(t1)
    for d in (a, b):
        d.push_wideband(0, parts[2], first=False)
    got, raw, _ = nc.assert_push(a, b, model, "a changed, a new and an unchanged entry")
    cleared = wb.Notch(C_, t1).push(raw)[0]
    assert not np.array_equal(cleared[0], got[0]) and np.array_equal(cleared[[1, 3]], got[[1, 3]])
    # None: off from the next push, the hops are the channeliser's again
    a.set_wideband_notch(None)
    for d in (a, b):
        d.push_wideband(1, parts[3], first=False)
    assert np.array_equal(wg.dump_hops(a, range(C_)), wg.dump_hops(b, range(C_)))
    wo.unreadable(hip, [a.wideband_notch_stats])

    # the same stream pushed twice gives the same bytes: a first push zeroes every tail
    a.set_wideband_notch(t1)
    again = wo.same_bytes_twice(a, parts, lambda d: (wg.dump_hops(d, range(C_)), d.wideband_notch_stats()))
    model = wb.Notch(C_, t1)
    for i, part in enumerate(parts):
        b.push_wideband(i % 2, part, first=i == 0)
        want, _ = model.push(wg.dump_hops(b, range(C_)))
        assert np.array_equal(want, again[i][0]), f"second run, push {i}"

    # msk144_set_wideband switches it off
    a.set_wideband(rate, offsets, "cs16", gain=gain)
    a.push_wideband(0, parts[0], first=True)
    b.push_wideband(0, parts[0], first=True)
    assert np.array_equal(wg.dump_hops(a, range(C_)), wg.dump_hops(b, range(C_)))
    wo.unreadable(hip, [a.wideband_notch_stats])
    a.synchronize()
    b.synchronize()


# ---- 6. end to end ----

def test_the_notches_bring_the_decodes_back(hip):
    parts = nc.scene_parts()
    _, planted, table = nc.decode_scene()
    C_ = len(nc.SCENE_OFFSETS)
    found = []
    with hip.HipDecoder(channels=C_, read_mode=2, **nc.SCENE_CFG) as d:
        for notched in (True, False):
            d.set_wideband(nc.SCENE_RATE, nc.SCENE_OFFSETS, "cs16", gain=nc.SCENE_GAIN)
            d.set_wideband_notch(table if notched else None)
            recs, _ = wg.decode_wideband(d, parts)
            got = wg.messages_by_channel(recs)
            found.append(sorted(c for c, msg in planted.items() if msg in got.get(c, set())))
            if notched:
                clamped = d.wideband_notch_stats()
                assert list(clamped["on"]) == [1] * C_
    print(f"decoded with the notches: {found[0]}; without: {found[1]}")
    assert found[0] == sorted(planted), "a planted message is not decoded on its own channel with the notches"
    assert len(found[1]) < len(found[0])

    # the program, with the same table
    spec = ",".join(f"{c}:{f[0]}+{f[1]}" for c, f in sorted(table.items()))
    args = [f"--wideband-rate={nc.SCENE_RATE}", "--wideband-format=cs16", "--channel-offsets=" + ",".join(str(int(f)) for f in nc.SCENE_OFFSETS)] + nc.SCENE_DECODE_ARGS
    lines, err = wg.run_program(args + [f"--wideband-notch={spec}"], np.concatenate(parts).tobytes())
    got = wg.messages_by_channel_in_lines(lines)
    assert sorted(c for c, msg in planted.items() if msg in got.get(c, set())) == found[0], "the program decodes other messages than the library"
    first = sorted(table)[:3]
    assert (f"msk144hipdecoder: wideband notch: {C_} of {C_} channels notched, {2 * C_} notches of +-100 Hz, " in err
            and "components clamped; " + " ".join(f"ch={c} {table[c][0]:+d},{table[c][1]:+d} Hz" for c in first) in err), err[-800:]
