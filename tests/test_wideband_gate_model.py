"""CPU: the gate rule of the wideband contract (include/msk144hip.h) in its three forms - the contract's sentence evaluated by brute
force (wideband_gate_check.brute), the Python state machine wideband.Gate, and the C++ rule the plan kernel runs, through
libmsk144host.so.

1. Random up masks: 1, 63, 64, 65, 256, 257 and 1000 channels x 40 pushes, hold in {0, 1, 3, 16}, min_up in {1, 3, 27}, random
   always sets: all three forms give the same lists and totals, push by push, byte for byte.
2. max_channels below the qualifying count: the first max_channels in ascending order, the totals unchanged - `since` moves for
   every channel whatever was dropped.
3. The first push walks hops 0 and 1 in that order; restart() (msk144_set_wideband_gate in mid-stream) forgets earlier activity; the
   detector off (records None) leaves the always channels; `since` stops one hop past hold = 16, against the brute force.
4. The coverage property for hold >= 1: every window that contains an active hop is decoded.  Its converse: no window is decoded
   more than `hold` hops after the last activity.  hold = 0 decodes exactly the windows whose newest hop is active.
5. check_gate's refusals, and the same parameters refused by wideband.Gate.
"""
import numpy as np
import pytest

import wideband_gate_check as gc
from msk144cudecoder_amd import wideband as wb

COUNTS = (1, 63, 64, 65, 256, 257, 1000)
PUSHES = 40


def three_forms(records, channels, hold, min_up, always=(), max_channels=None, restart_at=None, what=""):
    """Push the records through wideband.Gate and the C++ rule, hold both to the brute force; returns the lists."""
    py, cpp = wb.Gate(channels, hold, min_up, max_channels, always), gc.HostGate(channels, hold, min_up, max_channels, always)
    assert cpp.m, what
    a = gc.hop_activity(records, min_up)
    want = gc.brute(a, hold, always, max_channels)
    if restart_at is not None:
        want[restart_at:] = gc.brute(a, hold, always, max_channels, since_push=restart_at)[restart_at:]
    out = []
    for i, r in enumerate(records):
        if i == restart_at:
            py.restart()
            cpp.restart()
        got_py, got_cpp = py.push(r, i == 0), cpp.push(r, i == 0)
        gc.assert_list(got_py, want[i], f"{what} push {i}: wideband.Gate")
        gc.assert_list(got_cpp, want[i], f"{what} push {i}: the C++ rule")
        assert got_py[0].tobytes() == got_cpp[0].tobytes()
        out.append(got_py)
    return out, a


@pytest.mark.parametrize("C", COUNTS)
def test_the_three_forms_agree_on_random_records(C):
    rng = np.random.default_rng([C, 31])
    seen = set()
    combos = [(h, u) for h in (0, 1, 3, 16) for u in (1, 3, 27)]
    if C == 1000:
        combos = [(0, 1), (1, 3), (3, 27), (16, 1)]           # the brute force over 1000 channels is what takes the time
    for hold, min_up in combos:
        density = float(rng.choice([0.02, 0.1, 0.4]))
        records = gc.random_records(rng, C, PUSHES, density)
        always = sorted(int(c) for c in rng.choice(C, size=int(rng.integers(0, min(C, 40) + 1)), replace=False))
        lists, a = three_forms(records, C, hold, min_up, always, what=f"{C} channels hold {hold} min_up {min_up}")
        seen |= {len(l) for l, _ in lists}
        assert all(t == len(l) for l, t in lists)
    assert len(seen) > 1 or C == 1


@pytest.mark.parametrize("hold, min_up", [(1, 1), (0, 3), (16, 1)])
def test_a_budget_drops_the_tail_and_changes_no_decision(hold, min_up):
    C = 257
    rng = np.random.default_rng([hold, min_up, 9])
    records = gc.random_records(rng, C, 20, 0.3)
    always = [0, 100, 256]
    free, _ = three_forms(records, C, hold, min_up, always, what="no budget")
    smallest = min(t for _, t in free)
    assert smallest >= 4
    for cap in (smallest, smallest - 1, 1):
        got, _ = three_forms(records, C, hold, min_up, always, cap, what=f"max_channels {cap}")
        for (l, t), (fl, ft) in zip(got, free):
            assert t == ft and len(l) == cap and list(l) == list(fl[:cap])
    # max_channels 0 and None stand for every channel
    assert [t for _, t in three_forms(records, C, hold, min_up, always, 0, what="max_channels 0")[0]] == [t for _, t in free]


def one_channel(masks, first_two=True):
    """Records of a one-channel stream from a list of up masks, one per push."""
    out = []
    for i, m in enumerate(masks):
        r = np.zeros(1, dtype=wb.PING_DTYPE)
        r["up_mask"], r["blocks"] = m, 54 if i == 0 else 27
        out.append(r)
    return out


def test_the_first_push_walk_restart_and_the_detector_off():
    lo, hi = 1 << 5, 1 << (27 + 5)
    for make in (wb.Gate, gc.HostGate):
        # hop 0 active alone: after hop 1 the channel is one hop past its activity
        assert [len(make(1, hold=h).push(one_channel([lo])[0], True)[0]) for h in (0, 1)] == [0, 1], make.__name__
        # hop 1 active alone: hold 0 takes it.  A walk of hop 1 alone would give the same; one in the other order would not
        assert [len(make(1, hold=h).push(one_channel([hi])[0], True)[0]) for h in (0, 1)] == [1, 1], make.__name__
        # hop 0 active, then three quiet pushes at hold 2: since = 1, 2, 3, 4
        g = make(1, hold=2)
        assert [len(g.push(r, i == 0)[0]) for i, r in enumerate(one_channel([lo, 0, 0, 0]))] == [1, 1, 0, 0], make.__name__
        # restart() before the push after the activity: it counts as none
        g = make(1, hold=3)
        recs = one_channel([0, lo, 0, 0])
        assert len(g.push(recs[0], True)[0]) == 0 and len(g.push(recs[1], False)[0]) == 1
        g.restart()
        assert len(g.push(recs[2], False)[0]) == 0 and len(g.push(recs[3], False)[0]) == 0
        # a new first push clears as well
        g = make(1, hold=16)
        g.push(one_channel([lo])[0], True)
        assert len(g.push(one_channel([0])[0], True)[0]) == 0
        # the detector off: only the always channels
        g = make(5, hold=16, always=(1, 3))
        assert [list(g.push(None, i == 0)[0]) for i in range(3)] == [[1, 3]] * 3
        # `since` saturates: activity 40 pushes ago does not come back at hold 16
        g = make(1, hold=16)
        got = [len(g.push(r, i == 0)[0]) for i, r in enumerate(one_channel([hi] + [0] * 40))]
        assert got == [1] * 17 + [0] * 24, make.__name__
    # restart in mid-stream against the brute force
    rng = np.random.default_rng(12)
    records = gc.random_records(rng, 65, 12, 0.2)
    three_forms(records, 65, 3, 1, (7,), restart_at=5, what="restart at push 5")


def test_since_saturates_one_hop_past_the_longest_hold():
    """Hop 0 active alone, 20 silent hops, hold = 16: the channel is listed through hop 16 and `since` then stays at its stop.
    restart() ahead of the push that carries hop 5 ends that there: earlier activity counts as none."""
    records = one_channel([1 << 5] + [0] * 19)
    lists, a = three_forms(records, 1, 16, 1, what="hold 16")
    assert a.shape == (1, 21) and a[0].tolist() == [True] + [False] * 20
    assert [t for _, t in lists] == [1] * 16 + [0] * 4           # push p carries hop p + 1
    lists, _ = three_forms(records, 1, 16, 1, restart_at=4, what="hold 16, restart at push 4")
    assert [t for _, t in lists] == [1] * 4 + [0] * 16


@pytest.mark.parametrize("hold", [0, 1, 3, 16])
@pytest.mark.parametrize("min_up", [1, 3])
def test_coverage_and_its_converse(hold, min_up):
    rng = np.random.default_rng([hold, min_up, 77])
    C = 64
    records = gc.random_records(rng, C, PUSHES, 0.08)
    a = gc.hop_activity(records, min_up)
    g = wb.Gate(C, hold, min_up)
    decoded = np.zeros((C, PUSHES), dtype=bool)
    for i, r in enumerate(records):
        decoded[g.push(r, i == 0)[0], i] = True
    assert a.any() and not a.all()
    for c in range(C):
        for p in range(PUSHES):
            window = a[c, p] or a[c, p + 1]                            # the window of push p covers hops p and p + 1
            if hold >= 1:
                assert decoded[c, p] or not window, f"ch={c} push {p}: a window with an active hop is not decoded"
            recent = a[c, max(0, p + 1 - hold):p + 2].any()            # activity within `hold` hops of the newest
            assert recent or not decoded[c, p], f"ch={c} push {p}: decoded more than {hold} hops after the last activity"
            if hold == 0:
                assert decoded[c, p] == a[c, p + 1]
    if hold >= 1:
        assert (decoded & ~(a[:, :-1] | a[:, 1:])).any() == (hold >= 2)    # hold 1 decodes nothing but windows that hold activity


def test_check_gate_refusals():
    assert gc.host_check(8) == "" and gc.host_check(8, 0, 27, 8) == "" and gc.host_check(8, 16, 1, 1) == "" and gc.host_check(1, 1, 1, 1) == ""
    assert gc.host_check(8, -1) == gc.host_check(8, 17) == "gate hold must lie within 0..16 hops"
    assert gc.host_check(8, 1, 0) == gc.host_check(8, 1, 28) == "gate min_up must lie within 1..27 blocks"
    assert gc.host_check(8, 1, 1, -1) == gc.host_check(8, 1, 1, 9) == "gate max_channels must lie within 1..8, or be 0 for all"
    for bad in (dict(hold=-1), dict(hold=17), dict(min_up=0), dict(min_up=28), dict(max_channels=-1), dict(max_channels=9), dict(always=[8]), dict(always=[-1])):
        with pytest.raises(ValueError):
            wb.Gate(8, **bad)
        assert not gc.HostGate(8, **bad).m, bad
    # always is any subset, more than the 16 a capture list holds
    g = wb.Gate(40, always=range(40))
    assert len(g.push(None, True)[0]) == 40 and wb.Gate(8).max_channels == 8 and wb.Gate(8, max_channels=0).max_channels == 8
