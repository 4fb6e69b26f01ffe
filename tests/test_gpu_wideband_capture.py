"""-m gpu: the capture of the wideband contract (include/msk144hip.h) against its Python model, wideband.Capture, with no tolerance.
After every push the model is fed the device's own ping records; header (count, total), descriptors and flags must be equal, and
every unit's bytes must be the dump_wideband_hop bytes saved from the push that carried that hop (run_against_model).

1. Shapes: the three of wideband_levels_check.py (240 ksps x 130 channels; 24 125 sps x 33, Q = 96; 8 Msps x 70 over ten bands with
   padded slots), cu8 and cs16, noise with two tone bursts and a detector ratio of 1.375, at which noise alone makes a good part of
   the hops active: the units are spread over the channels.
2. Channel counts 1, 63, 64, 65, 255, 256, 257: one below, at and one above the 64-lane wave and the 256 channels that are both the
   plan kernel's workgroup and its chunk (one channel per lane, so the chunk has no width of its own), and 513 and 769: three and
   four chunks, where the kernel's LDS double buffer is used a second time and the running base is carried over more than one
   chunk boundary.  Listed channels lie in every chunk.
3. The planned scene of wideband_capture_check.py: the device's own activity holds every case of its CASES - the test fails if one
   is missing.
4. Overflow on that scene: max_units at the largest push's count - 1, count and count + 1.
5. An AGC step in mid-stream; set, off and set again in mid-stream; max_units grown and shrunk between a push and a read, read
   through the C entry into buffers of exactly the max_units last set, with guard rows; the same stream pushed twice gives the
   same bytes.
6. Refusals and order.
7. It changes nothing: with capture on and off, hops, levels, clip counts, ping records and energies, waterfall rows and decoded
   records are byte-identical, per shape.
8. Replay: the program run with --wideband-pings --wideband-capture on a scene whose planted message decodes; the segment a ping
   line names, fed to msk144hipdecoder --read-mode=2, prints the same message as the live run printed for that channel.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import wideband_capture_check as cc
import wideband_gpu as wg
import wideband_levels_check as lc
import wideband_options as wo
import wideband_pings_check as pc
from msk144cudecoder_amd import wideband as wb
from wideband_options import EINVAL, ESTATE, code_of

pytestmark = pytest.mark.gpu

RATIO_Q4 = 22           # 1.375 x the reference: white noise alone puts a block up now and then
COUNTS = (1, 63, 64, 65, 255, 256, 257, 513, 769)


@pytest.fixture(scope="module")
def handles(hip):
    """Two handles per channel count, made on first use and kept for the module."""
    with wo.handle_cache(wo.decode_pair(hip)) as get:
        yield get


class Saved:
    """The dump_wideband_hop bytes of every hop of a stream, by hop."""

    def __init__(self):
        self.hops = {}

    def take(self, d, i):
        q = wg.dump_hops(d, range(d.channels))
        if i == 0:
            self.hops[0], self.hops[1] = q[:, :wb.HOP_OUT].copy(), q[:, wb.HOP_OUT:].copy()
        else:
            self.hops[i + 1] = q


def assert_capture(d, model, saved, rec, i, what):
    """The capture of push i of handle d equals the model fed `rec`, and its bytes are the saved hops'.  Returns (units, total)."""
    units, data, total = d.wideband_capture()
    assert data.shape == (len(units), wb.HOP_OUT, 2) and data.dtype == np.int8
    cc.assert_units((units, total), model.push(rec, i == 0), f"{what} push {i}")
    for u, row in zip(units, data):
        c, k = int(u["channel"]), int(u["hop"])
        assert np.array_equal(row, saved.hops[k][c]), f"{what} push {i}: the bytes of ch={c} hop={k} are not the hop's"
    return units, total


def run_against_model(d, parts, pre, post, listed, max_units=None, what="", pings=True):
    """Push parts with capture (set by the caller) and hold every push to the model.  Returns (records, [(units, total)])."""
    model = wb.Capture(d.channels, pre, post, max_units, listed)
    saved, records, out = Saved(), [], []
    for i, part in enumerate(parts):
        d.push_wideband(i % 2, part, first=i == 0)
        rec = d.wideband_pings() if pings else None
        saved.take(d, i)
        out.append(assert_capture(d, model, saved, rec, i, what))
        records.append(rec)
    d.synchronize()
    return records, out


def spread(C, n=6):
    """Up to n listed channels over the whole range, the last channel among them."""
    return sorted({int(round(f * (C - 1))) for f in np.linspace(0.1, 1.0, n)})


# ---- 1. shapes ----

@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_shapes_against_the_model(handles, name, fmt):
    shape = lc.SHAPES[name]
    rate, offsets = shape["rate"], shape["offsets"]
    d, _ = handles(len(offsets))
    listed = spread(len(offsets))
    d.set_wideband(rate, offsets, fmt, taps_per_phase=shape["K"], gain=pc.burst_gain(rate))
    d.set_wideband_pings(ratio_q4=RATIO_Q4)
    d.set_wideband_capture(1, 1, None, listed)
    records, out = run_against_model(d, pc.burst_parts(rate, tuple(int(f) for f in offsets), fmt), 1, 1, listed, what=f"{name} {fmt}")
    a = cc.activity_of(records)
    flags = np.concatenate([u["flags"] for u, _ in out])
    print(f"{name} {fmt}: {int(a.sum())} of {a.size} hops active, units per push {[t for _, t in out]}")
    # the units are no trivial set: active, tail, pre-roll and listed ones, on many channels
    assert all((flags & f).any() for f in (wb.CAPTURE_ACTIVE, wb.CAPTURE_TAIL, wb.CAPTURE_PRE, wb.CAPTURE_LISTED))
    assert len({int(c) for u, _ in out for c in u["channel"]}) > len(listed)
    d.set_wideband_capture(None)
    d.set_wideband_pings(None)


# ---- 2. channel counts around the widths of the prefix ----

@pytest.mark.parametrize("C", COUNTS)
def test_channel_counts_against_the_model(handles, C):
    rate = 240000
    grid = np.arange(-112000, 112001, 16000)
    offsets = grid[np.arange(C) % len(grid)].astype(np.int32)
    d, _ = handles(C)
    listed = spread(C, 16)
    assert C - 1 in listed and {c // 256 for c in listed} == set(range((C + 255) // 256))     # a listed channel in every chunk
    d.set_wideband(rate, offsets, "cs16", gain=pc.burst_gain(rate))
    d.set_wideband_pings(ratio_q4=RATIO_Q4)
    d.set_wideband_capture(1, 2, 2 * C, listed)
    records, out = run_against_model(d, pc.burst_parts(rate, tuple(int(f) for f in offsets), "cs16"), 1, 2, listed, 2 * C, what=f"{C} channels")
    print(f"{C} channels: units per push {[t for _, t in out]}")
    assert out[0][1] >= 2 * len(listed) and all(t >= len(listed) for _, t in out)
    d.set_wideband_capture(None)
    d.set_wideband_pings(None)


# ---- 3. the planned scene ----

def scene_setup(d, max_units=None, capture=True):
    d.set_wideband(cc.SCENE_RATE, cc.SCENE_OFFSETS, "cs16", gain=cc.SCENE_GAIN)
    d.set_wideband_pings()
    if capture:
        d.set_wideband_capture(cc.SCENE_PRE, cc.SCENE_POST, max_units, cc.SCENE_LISTED)


def test_the_planned_scene_on_the_device(handles):
    d, _ = handles(len(cc.SCENE_OFFSETS))
    scene_setup(d)
    records, out = run_against_model(d, cc.scene_parts(), cc.SCENE_PRE, cc.SCENE_POST, cc.SCENE_LISTED, what="scene")
    a = cc.activity_of(records)
    print("device activity\n", a.astype(int))
    found = cc.cases(cc.up_matrix(records), cc.SCENE_PRE, cc.SCENE_POST, cc.SCENE_LISTED)
    assert found == set(cc.CASES), f"the device's activity misses: {set(cc.CASES) - found}"
    flags = {(int(u["channel"]), int(u["hop"])): int(u["flags"]) for us, _ in out for u in us}
    assert len(flags) == sum(t for _, t in out), "a hop emitted twice"
    assert flags[(6, 0)] == wb.CAPTURE_LISTED and (7, 0) not in flags and not any(c == 7 for c, _ in flags)


# ---- 4. overflow ----

def test_overflow_at_the_count(handles):
    d, _ = handles(len(cc.SCENE_OFFSETS))
    scene_setup(d, wb.CAPTURE_MAX_UNITS)
    _, free = run_against_model(d, cc.scene_parts(), cc.SCENE_PRE, cc.SCENE_POST, cc.SCENE_LISTED, wb.CAPTURE_MAX_UNITS, what="unbounded")
    count = max(t for _, t in free)
    assert count >= 6 and all(len(u) == t for u, t in free)
    for max_units in (count - 1, count, count + 1):
        scene_setup(d, max_units)
        _, out = run_against_model(d, cc.scene_parts(), cc.SCENE_PRE, cc.SCENE_POST, cc.SCENE_LISTED, max_units, what=f"max_units {max_units}")
        for (u, t), (fu, ft) in zip(out, free):
            assert t == ft and u.tobytes() == fu[:max_units].tobytes()           # the decisions do not depend on the drops
        assert max(len(u) for u, _ in out) == min(count, max_units)
        assert (max_units < count) == any(len(u) < t for u, t in out)


# ---- 5. AGC, switching, repeatability ----

def test_an_agc_step_in_mid_stream(handles):
    d, _ = handles(len(pc.SCENE_OFFSETS))
    parts, gain = wo.loud_push_stream(6)               # a loud tone on channel 1 through the whole of push 2 (hop 3)
    d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16", gain=gain)
    d.set_wideband_agc()
    d.set_wideband_pings()
    d.set_wideband_capture(1, 2, None, [4])
    model, saved, exps, got = wb.Capture(d.channels, 1, 2, None, [4]), Saved(), [], []
    for i, part in enumerate(parts):
        d.push_wideband(i % 2, part, first=i == 0)
        saved.take(d, i)
        got.append(assert_capture(d, model, saved, d.wideband_pings(), i, "AGC"))
        exps.append([int(v) for v in d.wideband_levels()["exponent"]])
    d.synchronize()
    print("exponents", exps, "units", [[(int(u["channel"]), int(u["hop"]), int(u["flags"])) for u in us] for us, _ in got])
    assert exps[2][1] == 0 and exps[3][1] == -1, "no AGC step behind the loud push"
    # channel 1 is kept from its pre-roll hop 2 through the step: hops 3 (quantised before the step), 4 and 5 (after it) as they were
    mine = [(int(u["hop"]), int(u["flags"]) & wb.CAPTURE_PRE) for us, _ in got for u in us if u["channel"] == 1]
    assert mine[:4] == [(2, wb.CAPTURE_PRE), (3, 0), (4, 0), (5, 0)]
    d.set_wideband_agc(None)
    d.set_wideband_capture(None)
    d.set_wideband_pings(None)


def test_set_off_and_set_again_in_mid_stream(hip, handles):
    d, _ = handles(len(cc.SCENE_OFFSETS))
    parts = cc.scene_parts()
    scene_setup(d, capture=False)
    saved, model = Saved(), None
    seen = {}
    for i, part in enumerate(parts):
        if i == 2:
            # before the push that carries hop 3, where channel 3's event starts: the stream has hop 2, which is its pre-roll
            d.set_wideband_capture(cc.SCENE_PRE, cc.SCENE_POST, None, cc.SCENE_LISTED)
            model = wb.Capture(d.channels, cc.SCENE_PRE, cc.SCENE_POST, None, cc.SCENE_LISTED)
            model.hop = i
        if i == 4:
            d.set_wideband_capture(None)
            model = None
        if i == 5:
            # before the push that carries hop 6, with other parameters: the tails of hops 4 and 5 count as nothing
            d.set_wideband_capture(0, 1, 4, [0, 7])
            model = wb.Capture(d.channels, 0, 1, 4, [0, 7])
            model.hop = i
        d.push_wideband(i % 2, part, first=i == 0)
        saved.take(d, i)
        if model is None:
            assert code_of(hip, d.wideband_capture) == ESTATE
        else:
            units, _ = assert_capture(d, model, saved, d.wideband_pings(), i, "switching")
            seen[i] = [(int(u["channel"]), int(u["hop"]), int(u["flags"])) for u in units]
    d.synchronize()
    print(seen)
    assert (3, 2, wb.CAPTURE_PRE) in seen[2] and (3, 3, wb.CAPTURE_ACTIVE) in seen[2]
    assert not any(c == 4 for c, _, _ in seen[2]), "activity before `set` counted"       # channel 4's tail of hop 2 is forgotten
    assert seen[5] == [(0, 6, wb.CAPTURE_LISTED), (7, 6, wb.CAPTURE_LISTED)]                # channels 2, 3, 5 would be in their tails
    d.set_wideband_capture(None)


def read_into(hip, d, rows):
    """msk144_wideband_capture into buffers of exactly `rows` units, as the contract sizes them, with one guard row behind each:
    (code, units, data, total); fails if a guard row was written."""
    units = np.full(rows + 1, -1, dtype=wb.CAPTURE_DTYPE)
    data = np.full((rows + 1, wb.CAPTURE_UNIT_BYTES), 0x5A, dtype=np.int8)
    count, total = ctypes.c_int32(-1), ctypes.c_int32(-1)
    code = d.L.msk144_wideband_capture(d.h, units.ctypes.data_as(ctypes.POINTER(hip.WidebandCaptureUnit)), data.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), ctypes.byref(count),
                                       ctypes.byref(total))
    assert units[rows:].tobytes() == np.full(1, -1, dtype=wb.CAPTURE_DTYPE).tobytes() and (data[rows:] == 0x5A).all(), f"written past {rows} rows"
    if code != 0:
        assert (data == 0x5A).all() and count.value == -1, "a refused read wrote something"
        return code, None, None, None
    assert 0 <= count.value <= rows
    return code, units[:count.value], data[:count.value].reshape(-1, wb.HOP_OUT, 2), total.value


def test_max_units_grown_and_shrunk_between_a_push_and_a_read(hip, handles):
    """Every accepted `set` ends the last push's units, so a read never returns rows that no push wrote (max_units grown: new device
    rows) nor more rows than the caller's buffers for the max_units last set hold (shrunk).  All channels are listed: every push has
    one unit per channel and hop, C or 2 C of them."""
    d, _ = handles(len(cc.SCENE_OFFSETS))
    C, parts = d.channels, cc.scene_parts()
    listed = list(range(C))
    d.set_wideband(cc.SCENE_RATE, cc.SCENE_OFFSETS, "cs16", gain=cc.SCENE_GAIN)
    saved = Saved()
    # (max_units set before push i)
    plan = [2, 4 * C, 1, wb.CAPTURE_MAX_UNITS, 3, C]
    assert len(parts) > len(plan)
    for i, rows in enumerate(plan):
        d.set_wideband_capture(0, 0, rows, listed)
        # between `set` and the push: nothing to read, whatever the push before it left - and nothing is written
        assert read_into(hip, d, rows)[0] == ESTATE, f"before push {i}"
        d.push_wideband(i % 2, parts[i], first=i == 0)
        saved.take(d, i)
        code, units, data, total = read_into(hip, d, rows)
        hops = [0, 1] if i == 0 else [i + 1]
        want = [(c, k, wb.CAPTURE_LISTED) for c in range(C) for k in hops]
        assert code == 0 and total == len(want), f"push {i}"
        assert [(int(u["channel"]), int(u["hop"]), int(u["flags"])) for u in units] == want[:rows], f"push {i}"
        for u, row in zip(units, data):
            assert np.array_equal(row, saved.hops[int(u["hop"])][int(u["channel"])]), f"push {i}: the bytes of ch={u['channel']} hop={u['hop']}"
        # the wrapper sizes its buffers by the max_units last set
        again = d.wideband_capture()
        assert again[0].tobytes() == units.tobytes() and again[1].tobytes() == data.tobytes() and again[2] == total
    # after a push at a large max_units, a smaller `set` and a read with the smaller buffers: refused, not copied
    d.set_wideband_capture(0, 0, wb.CAPTURE_MAX_UNITS, listed)
    d.push_wideband(0, parts[len(plan)], first=False)
    assert read_into(hip, d, wb.CAPTURE_MAX_UNITS)[1].size == C
    d.set_wideband_capture(0, 0, 1, listed)
    assert read_into(hip, d, 1)[0] == ESTATE
    d.set_wideband_capture(None)
    assert read_into(hip, d, 1)[0] == ESTATE
    d.synchronize()


def test_the_same_stream_twice_gives_the_same_bytes(handles):
    d, _ = handles(len(cc.SCENE_OFFSETS))
    scene_setup(d)
    again = wo.same_bytes_twice(d, cc.scene_parts(), type(d).wideband_capture)
    d.synchronize()
    assert sum(t for _, _, t in again) >= 30


# ---- 6. refusals and order ----

def test_order_and_refusals(hip, handles):
    a, _ = handles(len(cc.SCENE_OFFSETS))
    parts = cc.scene_parts()
    H = hip.HipDecoder
    wo.refuses_outside_wideband_mode(hip, [H.set_wideband_capture, lambda f: f.set_wideband_capture(None), H.wideband_capture])
    a.set_wideband(cc.SCENE_RATE, cc.SCENE_OFFSETS, "cs16", gain=cc.SCENE_GAIN)
    C = a.channels
    for bad in (dict(pre=2), dict(pre=-1), dict(post=-1), dict(post=17), dict(max_units=0), dict(max_units=16385), dict(max_units=-4), dict(channels=[C]), dict(channels=[-1]),
                dict(channels=[1, 1]), dict(channels=[0, 3, 0])):
        assert code_of(hip, lambda: a.set_wideband_capture(**bad)) == EINVAL, bad
    for good in (dict(pre=0, post=0, max_units=1), dict(post=16), dict(max_units=16384), dict(channels=list(range(C))), dict()):
        a.set_wideband_capture(**good)
    a.set_wideband_capture(None)
    wo.unreadable(hip, [a.wideband_capture])                                            # before any push
    a.push_wideband(0, parts[0], first=True)
    wo.unreadable(hip, [a.wideband_capture])                                            # ... and after one made with capture off
    # without the detector only listed channels are kept; `set` takes effect at the next push and not before
    a.set_wideband_capture(1, 1, None, [2])
    assert code_of(hip, a.wideband_capture) == ESTATE
    a.push_wideband(1, parts[1], first=False)
    units, data, total = a.wideband_capture()
    assert [(int(u["channel"]), int(u["hop"]), int(u["flags"])) for u in units] == [(2, 2, wb.CAPTURE_LISTED)] and total == 1
    assert np.array_equal(data[0], a.dump_wideband_hop(2))
    # a refused `set` changes nothing; an accepted one ends the last push's units, until the next push
    assert code_of(hip, lambda: a.set_wideband_capture(post=17)) == EINVAL
    again = a.wideband_capture()
    assert again[0].tobytes() == units.tobytes() and again[1].tobytes() == data.tobytes() and again[2] == 1
    a.set_wideband_capture(1, 1, 1, [5])
    assert code_of(hip, a.wideband_capture) == ESTATE
    a.push_wideband(0, parts[2], first=False)
    units, _, total = a.wideband_capture()
    assert [(int(u["channel"]), int(u["hop"])) for u in units] == [(5, 3)] and total == 1
    # a quiet band: nothing listed, no detector - the header alone
    a.set_wideband_capture()
    a.push_wideband(1, parts[3], first=False)
    units, data, total = a.wideband_capture()
    assert len(units) == 0 and data.shape == (0, wb.HOP_OUT, 2) and total == 0
    # switched off: there is nothing to read any more, nor after the next push; msk144_set_wideband switches it off as well
    a.set_wideband_capture(None)
    wo.unreadable(hip, [a.wideband_capture])
    a.push_wideband(0, parts[4], first=False)
    wo.unreadable(hip, [a.wideband_capture])
    a.set_wideband_capture()
    a.set_wideband(cc.SCENE_RATE, cc.SCENE_OFFSETS, "cs16", gain=cc.SCENE_GAIN)
    a.push_wideband(0, parts[0], first=True)
    wo.unreadable(hip, [a.wideband_capture])
    a.synchronize()


# ---- 7. it changes nothing ----

@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_it_changes_nothing(handles, name):
    shape = lc.SHAPES[name]
    rate, offsets, K = shape["rate"], shape["offsets"], shape["K"]
    a, b = handles(len(offsets))
    if name == "rat":
        parts, planted, fmt, gain = wo.rat_scene()
    else:
        fmt, gain = "cs16", pc.burst_gain(rate)
        parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), fmt)[:3]
    for d in (a, b):
        d.set_wideband(rate, offsets, fmt, taps_per_phase=K, gain=gain)
        d.set_wideband_pings(ratio_q4=RATIO_Q4)
        d.set_wideband_waterfall()
    a.set_wideband_capture(1, 1, None, spread(len(offsets)))
    H = type(a)
    seen = wo.leaves_unchanged(a, b, parts, reads=(H.wideband_pings, H.wideband_ping_blocks, H.wideband_waterfall), decode=True)
    assert a.wideband_capture()[2] > 0
    for s in seen:
        assert s["reads"][0]["up_mask"].any() or s["reads"][1].any()
    if name == "rat":
        assert sum(len(s["records"]) for s in seen) > 0 and planted     # the scene decodes to something
    for d in (a, b):
        d.set_wideband_waterfall(None)
        d.set_wideband_pings(None)
    a.set_wideband_capture(None)


# ---- 8. replay ----

def test_a_captured_segment_replays_to_the_same_message(hip, tmp_path):
    rate, offsets, pushes = pc.SCENE_RATE, pc.SCENE_OFFSETS, 6
    raw, planted = wg.plant_scene(wb.FIRST_OUT + (pushes - 1) * wb.HOP_OUT, rate, offsets, [1, 3], np.random.default_rng(2025))
    pings, out = str(tmp_path / "pings.txt"), str(tmp_path / "cap")
    args = [f"--wideband-rate={rate}", "--wideband-format=cu8", "--channel-offsets=" + ",".join(str(int(f)) for f in offsets), "--wideband-gain=16"] + wg.SCENE_DECODE_ARGS
    lines, err = wg.run_program(args + [f"--wideband-pings={pings}", f"--wideband-capture={out}"], raw.tobytes())
    live = wg.messages_by_channel_in_lines(lines)
    assert "msk144hipdecoder: wideband capture: " in err and " 0 units dropped" in err
    with open(pings) as f:
        named = {}
        for l in f.read().splitlines():
            m = re.match(r"ping ch=(\d+) .* file=(\S+) at=(\d+)$", l)
            assert m, l
            named.setdefault(int(m.group(1)), m.group(2))
    replayed = 0
    for c, msg in planted.items():
        assert msg in live.get(c, set()), f"the live run did not decode ch={c}"
        assert c in named, f"no ping line names a file for ch={c}"
        path = os.path.join(out, named[c])
        assert os.path.getsize(path) % wb.CAPTURE_UNIT_BYTES == 0 and os.path.getsize(path) >= 2 * wb.CAPTURE_UNIT_BYTES
        with open(path, "rb") as f:
            again, _ = wg.run_program(["--read-mode=2"] + wg.SCENE_DECODE_ARGS, f.read())
        bits = {bytes(int(b) for b in m) for l in again for m in re.findall(r"bits='([01]{77})'", l)}
        print(f"ch={c}: {named[c]}, live {len(live[c])} message(s), replay {len(bits)}")
        assert bits == live[c], f"ch={c}: the replay of {named[c]} prints other messages than the live run"
        replayed += 1
    assert replayed == 2
