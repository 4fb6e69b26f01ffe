"""The stream gate rule (include/msk144hip.h "Stream gate"): stream_pings.StreamGate in Python integers against msk144sg::Model of
libmsk144host.so (csrc/stream_gate.h), over seeded pushes fed by stream_pings.StreamPings; what unlisted streams keep, what an absent
detector leaves, and every refusal of the parameter check.  CPU only."""
import numpy as np
import pytest

from msk144cudecoder_amd import stream_pings as sp
from msk144cudecoder_amd.wideband import SINCE_QUIET


def noise_row(rng, n, sigma, loud):
    """Gaussian noise of `sigma` LSB with `loud` blocks of 96 samples eight times as strong."""
    x = rng.normal(0.0, sigma, size=n)
    for b in rng.integers(0, n // 96, size=loud):
        x[96 * b:96 * (b + 1)] *= 8.0
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def plan(C, pushes, rng):
    """Per push (ids, firsts): every stream first at push 0, later a seeded subset that always holds stream 0; the last stream
    starts over at push 5, stream min(1, C - 1) at push 9."""
    out = [(list(range(C)), [1] * C)]
    for k in range(1, pushes):
        ids = [0] + [s for s in range(1, C) if rng.random() < 0.6]
        firsts = [0] * len(ids)
        for at, s in ((5, C - 1), (9, min(1, C - 1))):
            if k == at:
                if s not in ids:
                    ids = sorted(ids + [s])
                    firsts = [0] * len(ids)
                firsts[ids.index(s)] = 1
        out.append((ids, firsts))
    return out


CASES = [dict(hold=1, min_up=1), dict(hold=0, min_up=1), dict(hold=16, min_up=1), dict(hold=1, min_up=27), dict(hold=1, min_up=2, max_streams=2),
         dict(hold=1, min_up=1, ratio_q4=24), dict(hold=0, min_up=3, ratio_q4=160, max_streams=3), dict(hold=2, min_up=1, ratio_q4=65535)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_python_model_equals_the_host_model(case):
    """Sixteen pushes of seven streams: partial lists, mixed first and later hops, a stream restarted in mid-run, and a new gate (the
    `set`) at push 11 while the detector keeps its history.  List, total and every stream's `since` agree after every push."""
    C = 7
    rng = np.random.default_rng(5)
    always = [3]
    pings = sp.StreamPings(C, ratio_q4=40, memory=4)
    a, b = sp.StreamGate(C, always=always, **case), sp.HostStreamGate(C, always=always, **case)
    listed = dropped = 0
    for k, (ids, firsts) in enumerate(plan(C, 16, rng)):
        if k == 11:
            a, b = sp.StreamGate(C, always=always, **case), sp.HostStreamGate(C, always=always, **case)
        # quiet hops and hops with loud blocks, so that `since` runs up and falls back
        rows = [noise_row(rng, 5184 if f else 2592, 300.0, int(rng.choice([0, 0, 1, 4]))) for f in firsts]
        rec, _, en, _ = pings.push(ids, firsts, rows)
        got_a, got_b = a.push(ids, firsts, rec, en), b.push(ids, firsts, rec, en)
        assert got_a[0].dtype == np.int32 and got_a[0].tolist() == got_b[0].tolist() and got_a[1] == got_b[1], (k, got_a, got_b)
        assert a.since == b.since, (k, a.since, b.since)
        assert got_a[0].tolist() == sorted(got_a[0].tolist()) and len(got_a[0]) == min(got_a[1], a.max_streams)
        assert 3 not in ids or got_a[1] >= 1                     # the always stream qualifies whenever it is listed
        listed += len(got_a[0])
        dropped += got_a[1] - len(got_a[0])
    assert listed > 0
    if case.get("max_streams"):
        assert dropped > 0                                       # the cap did drop
    if case.get("min_up") == 27 or case.get("ratio_q4") == 65535:
        assert a.since == [SINCE_QUIET] * C                      # nothing is ever active


def test_the_gates_own_ratio_lists_what_the_detectors_does_not():
    """One block at 3 x the quiet level: not up at the detector's 3.5, up at the gate's 2.0."""
    x = np.where(np.arange(5184) % 2 == 0, 400, -400).astype(np.int16)
    x[96 * 30:96 * 31] = np.where(np.arange(96) % 2 == 0, 693, -693)          # 693^2 / 400^2 = 3.0
    rec, _, en, _ = sp.StreamPings(1).push([0], [1], [x])
    assert int(rec["up_mask"][0]) == 0
    for make in (sp.StreamGate, sp.HostStreamGate):
        strict, loose = make(1).push([0], [1], rec, en), make(1, ratio_q4=32).push([0], [1], rec, en)
        assert strict[0].tolist() == [] and strict[1] == 0
        assert loose[0].tolist() == [0] and loose[1] == 1


@pytest.mark.parametrize("make", [sp.StreamGate, sp.HostStreamGate])
def test_unlisted_streams_keep_since(make):
    """Stream 1 is active at push 0 and sits out four pushes: it comes back with since = 1 and is in at hold 1; stream 0, quiet in
    every one of them, stays saturated and is out."""
    rec = np.zeros(2, dtype=sp.PING_DTYPE)
    rec["blocks"], rec["reference"] = 54, 96
    rec["up_mask"][1] = 1 << 40                                                   # hop 1 of the first push
    en = np.zeros((2, 54), dtype=np.int64)
    g = make(2)
    assert g.push([0, 1], [1, 1], rec, en)[0].tolist() == [1] and g.since == [SINCE_QUIET, 0]
    quiet = np.zeros(1, dtype=sp.PING_DTYPE)
    quiet["blocks"], quiet["reference"] = 27, 96
    for _ in range(4):
        assert g.push([0], [0], quiet, en[:1])[1] == 0
    assert g.since == [SINCE_QUIET, 0]                                              # stream 0 saturated, stream 1 untouched
    two = np.zeros(2, dtype=sp.PING_DTYPE)
    two["blocks"], two["reference"] = 27, 96
    assert g.push([0, 1], [0, 0], two, en)[0].tolist() == [1] and g.since == [SINCE_QUIET, 1]   # position 1: one quiet hop behind its active one
    assert g.push([0, 1], [0, 0], two, en)[1] == 0 and g.since == [SINCE_QUIET, 2]


@pytest.mark.parametrize("make", [sp.StreamGate, sp.HostStreamGate])
@pytest.mark.parametrize("ratio_q4", [0, 32])
def test_without_the_detectors_records_only_always_streams_are_listed(make, ratio_q4):
    g = make(6, hold=16, ratio_q4=ratio_q4, always=[1, 4])
    got = g.push([0, 1, 2, 3, 4, 5], [1] * 6)
    assert got[0].tolist() == [1, 4] and got[1] == 2
    got = g.push([0, 2, 4, 5], [0, 0, 0, 1])
    assert got[0].tolist() == [2] and got[1] == 1                                  # POSITION 2 is stream 4
    assert g.since == [SINCE_QUIET] * 6


REFUSED = [dict(hold=-1), dict(hold=17), dict(min_up=0), dict(min_up=28), dict(max_streams=-1), dict(max_streams=9), dict(ratio_q4=-1), dict(ratio_q4=1), dict(ratio_q4=15),
           dict(ratio_q4=65536)]
TAKEN = [dict(), dict(hold=0), dict(hold=16), dict(min_up=27), dict(max_streams=8), dict(max_streams=1), dict(ratio_q4=16), dict(ratio_q4=65535)]


@pytest.mark.parametrize("bad", REFUSED, ids=str)
def test_every_refusal_of_the_params_check(bad):
    assert sp.host_gate_check(8, **bad) != "" and sp.stream_gate_check(8, **bad) != ""
    with pytest.raises(ValueError):
        sp.HostStreamGate(8, **bad)
    with pytest.raises(ValueError):
        sp.StreamGate(8, **bad)


@pytest.mark.parametrize("make", [sp.StreamGate, sp.HostStreamGate])
@pytest.mark.parametrize("always", [[8], [-1], [0, 3, 100]])
def test_an_always_stream_out_of_range_is_refused(make, always):
    with pytest.raises(ValueError):
        make(8, always=always)


@pytest.mark.parametrize("good", TAKEN, ids=str)
def test_what_the_params_check_takes(good):
    assert sp.host_gate_check(8, **good) == "" and sp.stream_gate_check(8, **good) == ""
    sp.HostStreamGate(8, **good), sp.StreamGate(8, **good)
