"""CPU: the capture rule of the wideband contract (include/msk144hip.h) in its three forms - the definitions of W and P evaluated
by brute force (wideband_capture_check.brute), the Python state machine wideband.Capture, and the C++ rule the plan kernel runs,
through libmsk144host.so - and the file rule, wideband.CaptureSegments against the C++ CaptureSegments.

1. Random activity: 1..70 channels, 1..40 pushes, pre in {0, 1}, post in {0, 1, 3, 16}, lists that include a silent listed channel:
   all three forms give the same units, flags and totals, push by push.
2. Overflow: max_units at the largest push's count exactly, one below it, and 1: the stored units are the first max_units of the
   unbounded run's and the totals are unchanged - decisions do not depend on drops.
3. Details the random runs may miss: the detector off (records None), restart() in mid-stream with its pre-roll, the documented
   single-hop segments, parameters out of range, and the stop of `since`: post = 16 behind one active hop, with and without restart().
4. CaptureSegments: names, gaps, capture.log lines and at= offsets, Python and C++ writing the same bytes.
5. The planned scene through the float64 channeliser model and wideband.Pings: its activity equals the plan and holds every case of
   wideband_capture_check.CASES, so the GPU test's scene is known to be a good one.
"""
import os

import numpy as np
import pytest

import wideband_capture_check as cc
from msk144cudecoder_amd import wideband as wb


def random_case(rng):
    C_, pushes = int(rng.integers(1, 71)), int(rng.integers(1, 41))
    density = float(rng.choice([0.03, 0.1, 0.3, 0.7]))
    a = rng.random((C_, pushes + 1)) < density
    listed = sorted(int(c) for c in rng.choice(C_, size=min(C_, int(rng.integers(0, 5))), replace=False))
    if listed:
        a[listed[0]] = False                      # a silent listed channel
    return a, listed


@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("post", [0, 1, 3, 16])
def test_state_machines_equal_the_definitions(pre, post):
    rng = np.random.default_rng([pre, post, 5])
    silent_listed = 0
    for trial in range(12):
        a, listed = random_case(rng)
        recs = cc.push_records(a, rng)
        assert np.array_equal(cc.activity_of(recs), a)
        want = cc.brute(a, pre, post, listed)
        py, cpp = wb.Capture(a.shape[0], pre, post, listed=listed), cc.HostCapture(a.shape[0], pre, post, listed=listed)
        emitted = set()
        for i, r in enumerate(recs):
            got = py.push(r, i == 0)
            cc.assert_units(got, want[i], f"pre {pre} post {post} trial {trial} push {i}: wideband.Capture")
            cc.assert_units(cpp.push(r, i == 0), want[i], f"pre {pre} post {post} trial {trial} push {i}: the C++ rule")
            assert py.hop == i + 1
            if got[1] == len(got[0]):
                keys = {(int(u["channel"]), int(u["hop"])) for u in got[0]}
                assert len(keys) == len(got[0]) and not keys & emitted, "a hop emitted twice"
                emitted |= keys
        silent_listed += bool(listed)
    assert silent_listed >= 3


@pytest.mark.parametrize("pre, post", [(1, 1), (0, 3), (1, 16)])
def test_overflow_drops_the_tail_and_changes_no_decision(pre, post):
    rng = np.random.default_rng([pre, post, 9])
    a = rng.random((40, 13)) < 0.3
    listed = [7, 21]
    a[7] = False
    recs = cc.push_records(a, rng)
    free = cc.brute(a, pre, post, listed, max_units=wb.CAPTURE_MAX_UNITS)
    largest = max(t for _, t in free)
    assert largest >= 8
    for max_units in (largest, largest - 1, 1):
        want = cc.brute(a, pre, post, listed, max_units=max_units)
        py, cpp = wb.Capture(40, pre, post, max_units, listed), cc.HostCapture(40, pre, post, max_units, listed)
        stored = []
        for i, r in enumerate(recs):
            got = py.push(r, i == 0)
            cc.assert_units(got, want[i], f"max_units {max_units} push {i}: wideband.Capture")
            cc.assert_units(cpp.push(r, i == 0), want[i], f"max_units {max_units} push {i}: the C++ rule")
            # the first max_units of what an unbounded run stores, and its total: nothing depends on what was dropped
            assert got[1] == free[i][1] and got[0].tobytes() == free[i][0][:max_units].tobytes()
            stored.append(len(got[0]))
        assert max(stored) == min(largest, max_units)
        if max_units == largest:
            assert all(s == t for s, (_, t) in zip(stored, free))       # count = max_units exactly drops nothing
        else:
            assert any(s < t for s, (_, t) in zip(stored, free))


def test_detector_off_restart_and_single_hop_segments():
    a = np.zeros((3, 8), dtype=bool)
    a[0, [3, 6]] = True
    a[1, 5] = True
    recs = cc.push_records(a)
    # the detector off for the push that carried hop 3 (push 2): a(3) = 0
    on = np.ones(8, dtype=bool)
    on[3] = False
    want = cc.brute(a, 1, 1, [2], on=on)
    for make in (wb.Capture, cc.HostCapture):
        m = make(3, 1, 1, listed=[2])
        for i, r in enumerate(recs):
            cc.assert_units(m.push(None if i == 2 else r, i == 0), want[i], f"{make.__name__} push {i}")
    # channel 2 always; channel 1 hops 4 (pre-roll) and 5 in push 4; channel 0 hops 5 (pre-roll) and 6 and channel 1's tail in push 5
    assert [int(t) for _, t in want] == [2, 1, 1, 1, 3, 4, 2]

    # restart() before the push that carries hop 5: activity before it counts as none, hop 4 is pre-roll for a(5) once more
    b = np.zeros((1, 8), dtype=bool)
    b[0, [4, 5]] = True
    recs = cc.push_records(b)
    for make in (wb.Capture, cc.HostCapture):
        m = make(1, 1, 0)
        out = []
        for i, r in enumerate(recs):
            if i == 4:
                m.restart()
            out.append([(int(u["hop"]), int(u["flags"])) for u in m.push(r, i == 0)[0]])
        assert out == [[], [], [], [(3, wb.CAPTURE_PRE), (4, wb.CAPTURE_ACTIVE)], [(4, wb.CAPTURE_PRE), (5, wb.CAPTURE_ACTIVE)], [], []], make.__name__

    # a rule that joins a stream in mid-stream is told the hop count
    m, h = wb.Capture(1, 1, 0), cc.HostCapture(1, 1, 0)
    m.hop = 4
    h.set_hop(4)
    for x in (m, h):
        assert [(int(u["hop"]), int(u["flags"])) for u in x.push(recs[4], False)[0]] == [(4, wb.CAPTURE_PRE), (5, wb.CAPTURE_ACTIVE)]

    # the documented single-hop segments: hop 0 active alone with post = 0, and pre = 0 with post = 0
    c = np.zeros((1, 5), dtype=bool)
    c[0, 0] = True
    assert [len(u) for u, _ in cc.brute(c, 1, 0)] == [1, 0, 0, 0]
    c[0, 0], c[0, 3] = False, True
    assert [[int(k) for k in u["hop"]] for u, _ in cc.brute(c, 0, 0)] == [[], [], [3], []]
    assert [[int(k) for k in u["hop"]] for u, _ in cc.brute(c, 1, 0)] == [[], [], [2, 3], []]


def test_since_saturates_one_hop_past_the_longest_post():
    """Hop 0 active alone, 20 silent hops, post = 16: the tail runs through hop 16 and `since` then stays at its stop.  restart()
    ahead of the push that carries hop 5 ends the tail there: earlier activity counts as none."""
    a = np.zeros((1, 21), dtype=bool)
    a[0, 0] = True
    recs = cc.push_records(a)
    for pre in (0, 1):
        whole = cc.brute(a, pre, 16)
        assert [[int(k) for k in u["hop"]] for u, _ in whole] == [[0, 1]] + [[k] for k in range(2, 17)] + [[]] * 4
        for restart_at, want in ((None, whole), (4, whole[:4] + cc.brute(np.zeros_like(a), pre, 16)[4:])):
            py, cpp = wb.Capture(1, pre, 16), cc.HostCapture(1, pre, 16)
            for i, r in enumerate(recs):
                if i == restart_at:
                    py.restart()
                    cpp.restart()
                cc.assert_units(py.push(r, i == 0), want[i], f"pre {pre} restart {restart_at} push {i}: wideband.Capture")
                cc.assert_units(cpp.push(r, i == 0), want[i], f"pre {pre} restart {restart_at} push {i}: the C++ rule")
            assert restart_at is None or all(t == 0 for _, t in want[4:])


def test_parameters_out_of_range_are_refused():
    for bad in (dict(pre=2), dict(pre=-1), dict(post=-1), dict(post=17), dict(max_units=0), dict(max_units=16385), dict(listed=[4]), dict(listed=[-1]), dict(listed=[1, 1])):
        with pytest.raises(ValueError):
            wb.Capture(4, **bad)
        assert not cc.HostCapture(4, **bad).m, bad
    with pytest.raises(ValueError):
        wb.Capture(40, listed=list(range(17)))
    assert not cc.HostCapture(40, listed=list(range(17))).m
    for good in (dict(pre=0, post=0, max_units=1), dict(post=16, max_units=16384, listed=[0, 3])):
        assert wb.Capture(4, **good) and cc.HostCapture(4, **good).m
    assert wb.Capture(300).max_units == 512 and wb.Capture(3).max_units == 6


def test_segments_names_gaps_log_lines_and_offsets(tmp_path):
    offsets = [-24000, 0, 36000]
    rng = np.random.default_rng(4)
    # (channel, hop) per push: channel 0 runs 1..3, pauses, runs 6..7; channel 2 has hop 0 alone, then 2 (a gap of one hop)
    pushes = [[(0, 1), (2, 0)], [(0, 2), (2, 2)], [(0, 3)], [], [], [(0, 6)], [(0, 7)]]
    rows = {}
    dirs = []
    for k, make in enumerate((wb.CaptureSegments, cc.HostSegments)):
        d = tmp_path / f"d{k}"
        os.makedirs(d)
        dirs.append(d)
        seg = make(str(d), offsets)
        for units in pushes:
            u = np.array([(c, 1, h) for c, h in units], dtype=wb.CAPTURE_DTYPE)
            data = np.stack([rows.setdefault(x, rng.integers(-128, 128, size=(wb.HOP_OUT, 2)).astype(np.int8)) for x in units]) if units else np.zeros((0, wb.HOP_OUT, 2), dtype=np.int8)
            seg.push(u, data)
            if units == [(0, 3)]:
                # block g = 27 hop + b: hop 2 of channel 0 is the second hop of its open segment, hop 2 of channel 2 the first of its
                assert seg.locate(0, 27 * 2 + 5) == " file=ch0_hop1.cs8 at=%d" % (2592 + 5 * 96)
                assert seg.locate(2, 27 * 2) == " file=ch2_hop2.cs8 at=0"
                assert seg.locate(2, 26) == " file=ch2_hop0.cs8 at=%d" % (26 * 96)       # an ended segment is remembered
                assert seg.locate(2, 27) == " file=-" and seg.locate(1, 0) == " file=-" and seg.locate(0, 26) == " file=-"
        assert seg.locate(0, 27 * 3 + 26) == " file=ch0_hop1.cs8 at=%d" % (2 * 2592 + 26 * 96)
        seg.close()
        assert seg.locate(0, 27 * 7) == " file=ch0_hop6.cs8 at=2592"
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) == ["capture.log", "ch0_hop1.cs8", "ch0_hop6.cs8", "ch2_hop0.cs8", "ch2_hop2.cs8"]
    for n in names:
        assert (dirs[0] / n).read_bytes() == (dirs[1] / n).read_bytes(), n
    assert (dirs[0] / "ch0_hop1.cs8").read_bytes() == b"".join(rows[(0, h)].tobytes() for h in (1, 2, 3))
    assert (dirs[0] / "ch2_hop0.cs8").read_bytes() == rows[(2, 0)].tobytes()
    assert (dirs[0] / "capture.log").read_text().splitlines() == [
        "capture ch=2 offset=36000 hop=0 t=0.000 hops=1 file=ch2_hop0.cs8",
        "capture ch=0 offset=-24000 hop=1 t=0.216 hops=3 file=ch0_hop1.cs8",
        "capture ch=0 offset=-24000 hop=6 t=1.296 hops=2 file=ch0_hop6.cs8",
        "capture ch=2 offset=36000 hop=2 t=0.432 hops=1 file=ch2_hop2.cs8"]
    s = wb.CaptureSegments(str(dirs[0]), offsets)
    assert (s.segments, s.hops, s.bytes) == (0, 0, 0)
    assert wb.capture_log_line(4095, -5, 123456, 7) == "capture ch=4095 offset=-5 hop=123456 t=26666.496 hops=7 file=ch4095_hop123456.cs8"


def test_the_planned_scene_has_the_planned_activity_and_every_case():
    m = wb.Channeliser(cc.SCENE_RATE, cc.SCENE_OFFSETS, gain=cc.SCENE_GAIN)
    det = wb.Pings(len(cc.SCENE_OFFSETS))
    records = []
    for i, part in enumerate(cc.scene_parts()):
        q = m.push(wb.read_samples(part, "cs16"), first=i == 0)[0]
        assert np.abs(q.astype(np.int16)).max() < 127, "the scene clips"
        records.append(det.push(q, cc.SCENE_GAIN))
    a = cc.activity_of(records)
    plan = cc.planned_activity()
    assert np.array_equal(a, plan), f"activity\n{a.astype(int)}\nplanned\n{plan.astype(int)}"
    up = cc.up_matrix(records)
    found = cc.cases(up, cc.SCENE_PRE, cc.SCENE_POST, cc.SCENE_LISTED)
    assert found == set(cc.CASES), f"missing: {set(cc.CASES) - found}"
    # ... and what the rule makes of it, spelled out: (channel, hop) of every unit, push by push
    cap = wb.Capture(len(cc.SCENE_OFFSETS), cc.SCENE_PRE, cc.SCENE_POST, listed=cc.SCENE_LISTED)
    got = [[(int(u["channel"]), int(u["hop"])) for u in cap.push(r, i == 0)[0]] for i, r in enumerate(records)]
    assert got == [
        [(0, 0), (0, 1), (1, 0), (1, 1), (6, 0), (6, 1)],
        [(0, 2), (1, 2), (4, 1), (4, 2), (5, 1), (5, 2), (6, 2)],
        [(1, 3), (3, 2), (3, 3), (4, 3), (5, 3), (6, 3)],
        [(3, 4), (4, 4), (5, 4), (6, 4)],
        [(2, 4), (2, 5), (3, 5), (5, 5), (6, 5)],
        [(2, 6), (3, 6), (5, 6), (6, 6)],
        [(2, 7), (6, 7)],
        [(6, 8)]]
    for i, (u, t) in enumerate(cc.brute(a, cc.SCENE_PRE, cc.SCENE_POST, cc.SCENE_LISTED)):
        assert [(int(x["channel"]), int(x["hop"])) for x in u] == got[i] and t == len(got[i])
