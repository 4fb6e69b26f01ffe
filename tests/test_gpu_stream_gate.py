"""-m gpu: the stream gate (include/msk144hip.h "Stream gate") - list, total and, through them, `since` against
stream_pings.StreamGate in integer equality after every push, behind msk144_push_hops and msk144_push_rate_hops, pipelined, capped,
with a ratio of its own; the gated decode against the ungated one; switched off, refused, and the program with --stream-gate."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from msk144cudecoder_amd import stream_pings as sp
from msk144cudecoder_amd import synth

import input_rate_scene as S
import test_gpu_stream_pings as P   # its push plan, noise rows and push helper

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "msk144cudecoder_amd", "msk144hipdecoder")
EINVAL, ESTATE = -1, -4
PINGS = dict(ratio_q4=40, memory=16, min_ref=96, shift=12)


def _code(hip, fn):
    with pytest.raises(hip.Msk144Error) as e:
        fn()
    return e.value.code


def same_list(got, want):
    return got[0].dtype == np.int32 and got[0].tolist() == want[0].tolist() and got[1] == want[1]


@pytest.mark.parametrize("C", [1, 5, 67, 300])
def test_list_and_total_equal_the_model(hip, C):
    """Twenty pushes with partial lists, mixed first and later hops and restarts (the plan and the rows of test_gpu_stream_pings):
    list and total equal StreamGate fed the model detector's records after every push (the `since` of every stream is pinned by
    test_since_of_every_stream_read_off_a_quiet_tail; here the `always` streams are in whatever theirs is) - through
    msk144_stream_gate at the push and through msk144_stream_gate_slot behind the fetch, with the other slot pushed meanwhile.  300 positions make the plan walk take a second chunk: 256, then 44 with a ragged last wave."""
    rng = np.random.default_rng(100 + C)
    always = sorted({C - 1, C // 2})
    pings, gate = sp.StreamPings(C, **PINGS), sp.StreamGate(C, always=always)
    at_push, of_slot, sizes = [], [], set()
    with hip.HipDecoder(channels=C, **S.CFG) as d:
        d.set_stream_pings(**PINGS)
        d.set_stream_gate(always=always)
        for k, (ids, firsts) in enumerate(P.plan(C, 20, rng)):
            s = k % 2
            # quiet hops among the ones with loud blocks, so that streams drop out of the list and come back
            rows = [P.noise_row(rng, 5184 if f else 2592, float(rng.choice([150.0, 400.0, 1200.0])), loud=int(rng.choice([0, 0, 0, 2]))) for f in firsts]
            P.push(d, s, ids, firsts, rows)
            rec, _, en, _ = pings.push(ids, firsts, rows)
            want = gate.push(ids, firsts, rec, en)
            got = d.stream_gate()
            assert same_list(got, want), (k, got, want)
            assert d.stream_pings()[0].tobytes() == rec.tobytes()
            at_push.append(got)
            sizes.add(len(got[0]))
            d.decode()
            d.fetch_async(s)
            if k >= 1:
                d.fetch_wait(1 - s)
                of_slot.append(d.stream_gate_slot(1 - s))
        d.fetch_wait(19 % 2)
        of_slot.append(d.stream_gate_slot(19 % 2))
    assert all(same_list(a, b) for a, b in zip(of_slot, at_push)) and len(of_slot) == 20
    assert C == 1 or len(sizes) > 2               # the list did change from push to push


def flat_row(n):
    """Every block the same energy: nothing is up, whatever the history."""
    return np.where(np.arange(n) % 2 == 0, 400, -400).astype(np.int16)


def test_since_of_every_stream_read_off_a_quiet_tail(hip):
    """`since` has no read entry, so it is read off the lists: hold 16 and no `always` stream, eight mixed pushes with partial lists
    and a restart, then seventeen pushes of every stream with no block up.  A stream leaves the list at the tail push at which its
    `since` passes 16, so the push at which each of the 67 streams leaves gives its `since` behind the mixed pushes exactly; the
    lists equal the model's after every push, and the streams do leave at different pushes."""
    rng = np.random.default_rng(17)
    C = 67
    pings, gate = sp.StreamPings(C, **PINGS), sp.StreamGate(C, hold=16)
    left_at = {}
    with hip.HipDecoder(channels=C, **S.CFG) as d:
        d.set_stream_pings(**PINGS)
        d.set_stream_gate(hold=16)
        mixed = P.plan(C, 8, rng)
        tail = [(list(range(C)), [0] * C)] * 17
        since_before_tail = None
        for k, (ids, firsts) in enumerate(mixed + tail):
            if k == len(mixed):
                since_before_tail = list(gate.since)
            quiet = k >= len(mixed)
            rows = [flat_row(5184 if f else 2592) if quiet else P.noise_row(rng, 5184 if f else 2592, 400.0, loud=int(rng.choice([0, 0, 0, 2]))) for f in firsts]
            P.push(d, k % 2, ids, firsts, rows)
            rec, _, en, _ = pings.push(ids, firsts, rows)
            want = gate.push(ids, firsts, rec, en)
            got = d.stream_gate()
            assert same_list(got, want), (k, got, want)
            if quiet:
                assert not np.any(rec["up_mask"])
                for s in range(C):
                    if s not in got[0].tolist() and s not in left_at:
                        left_at[s] = k - len(mixed)
            d.decode()
            d.fetch_async(k % 2)
            d.fetch_wait(k % 2)
    # tail push t leaves a stream at since + t + 1: it is out once that passes 16
    assert left_at == {s: max(0, 16 - since_before_tail[s]) for s in range(C)}
    assert len(set(left_at.values())) > 3 and len(left_at) == C


def ratio_row(n):
    """One block at 3.0 x the level of the others: not up at the detector's 3.5, up at a gate ratio of 2.0."""
    x = np.where(np.arange(n) % 2 == 0, 400, -400).astype(np.int16)
    x[96 * 20:96 * 21] = np.where(np.arange(96) % 2 == 0, 693, -693)
    return x


def test_the_gates_own_ratio(hip):
    """ratio_q4 = 32 on a detector at its default 56: the lists are the model's on the energies and references the detector
    reported, and stream 1's one block at 3 x its quiet level is listed by the gate while the detector's mask has nothing."""
    rng = np.random.default_rng(9)
    C = 6
    pings, gate = sp.StreamPings(C), sp.StreamGate(C, ratio_q4=32)
    with hip.HipDecoder(channels=C, **S.CFG) as d:
        d.set_stream_pings()
        d.set_stream_gate(ratio_q4=32)
        for k, (ids, firsts) in enumerate([(list(range(C)), [1] * C), ([0, 1, 4], [0, 0, 0]), ([1, 2, 3, 5], [0, 1, 0, 0]), (list(range(C)), [0] * C)]):
            rows = [ratio_row(5184 if f else 2592) if s == 1 and k != 1 else P.noise_row(rng, 5184 if f else 2592, 500.0, loud=int(rng.choice([0, 1]))) for s, f in zip(ids, firsts)]
            P.push(d, k % 2, ids, firsts, rows)
            rec, _, en, _ = pings.push(ids, firsts, rows)
            got_rec, _ = d.stream_pings()
            _, _, got_en = d.stream_pings_slot(k % 2)
            assert got_rec.tobytes() == rec.tobytes() and np.array_equal(got_en, en)
            want = gate.push(ids, firsts, got_rec, got_en)
            got = d.stream_gate()
            assert same_list(got, want), (k, got, want)
            if k != 1:
                j = ids.index(1)
                assert int(rec["up_mask"][j]) == 0 and j in got[0].tolist()


def test_the_cap_lists_the_first_positions_and_moves_the_same_state(hip):
    """max_streams 5 of 67: count < total, the listed positions are the first five of the uncapped handle's list, and the totals
    stay equal push after push - the state moves the same."""
    rng = np.random.default_rng(67)
    C = 67
    dropped = 0
    with hip.HipDecoder(channels=C, **S.CFG) as capped, hip.HipDecoder(channels=C, **S.CFG) as free:
        for d, m in ((capped, 5), (free, None)):
            d.set_stream_pings(**PINGS)
            d.set_stream_gate(max_streams=m, always=[66])
        for k, (ids, firsts) in enumerate(P.plan(C, 8, rng)):
            rows = [P.noise_row(rng, 5184 if f else 2592, 400.0, loud=int(rng.choice([0, 0, 2]))) for f in firsts]
            P.push(capped, k % 2, ids, firsts, rows)
            P.push(free, k % 2, ids, firsts, rows)
            a, b = capped.stream_gate(), free.stream_gate()
            assert a[1] == b[1] == len(b[0]) and a[0].tolist() == b[0].tolist()[:5]
            dropped += a[1] - len(a[0])
            for d in (capped, free):
                d.decode()
                d.fetch_async(k % 2)
            rec = capped.fetch_wait(k % 2)[0]
            free.fetch_wait(k % 2)
            assert len(rec) == 0 or int(rec["channel"].max()) < len(a[0])
    assert dropped > 0


@functools.lru_cache(maxsize=None)
def ping_scene():
    """The three streams of test_program_logs_and_summaries_equal_the_model: seed 31, 6 hops; noise with one +20 dB ping at sample
    7000, noise alone, silence."""
    rng = np.random.default_rng(31)
    hops = 6
    n = 5184 + (hops - 1) * 2592
    ping = synth.Ping(synth.random_message(rng), 7000, 8, 1500.0, 20.0, 0.3)
    x = (synth.synth_audio(n, [ping], 300.0, rng), synth.synth_audio(n, [], 300.0, rng), np.zeros(n, dtype=np.int16))
    return hops, tuple(v.astype(np.int16) for v in x)


def scene_rows(x, k):
    return [v[:5184] if k == 0 else v[(k + 1) * 2592:(k + 2) * 2592] for v in x]


def hop(d, k, ids, rows):
    """Push k of the listed streams, decoded and fetched: (records, segment powers of the n positions)."""
    s = k % 2
    P.push(d, s, ids, [k == 0] * len(ids), rows)
    d.decode()
    d.fetch_async(s)
    rec, seg = d.fetch_wait(s)
    return rec, seg[:len(ids)]


def as_multiset(records):
    return sorted(r.tobytes() for r in records)


@pytest.mark.parametrize("always", [(0,), (0, 2)])
def test_gated_decode_equals_ungated_decode(hip, always):
    """Two handles on the same hops: the ungated handle's records of the listed positions, their channel mapped to the list index,
    are the gated handle's records as multisets, byte for byte, and the segment powers of all positions are equal."""
    hops, x = ping_scene()
    compared = 0
    with hip.HipDecoder(channels=3, **S.CFG) as gated, hip.HipDecoder(channels=3, **S.CFG) as plain:
        gated.set_stream_pings()
        gated.set_stream_gate(always=always)
        for k in range(hops):
            rows = scene_rows(x, k)
            got, got_seg = hop(gated, k, [0, 1, 2], rows)
            want, want_seg = hop(plain, k, [0, 1, 2], rows)
            positions, total = gated.stream_gate_slot(k % 2)
            assert set(always) <= set(positions.tolist()) and total == len(positions)
            index = {int(j): i for i, j in enumerate(positions)}
            kept = want[np.isin(want["channel"], positions)].copy()
            kept["channel"] = [index[int(c)] for c in kept["channel"]]
            assert as_multiset(got) == as_multiset(kept)
            assert got_seg.tobytes() == want_seg.tobytes()
            assert gated.copy_count() >= 0
            compared += len(kept)
    assert compared > 0


def test_a_push_that_lists_nothing_leaves_no_records(hip):
    """The scene without `always`: its first window is noise alone - count 0, no launch, 0 records, the fetch succeeds with the
    segment powers of every position - and a later push, with the ping, still decodes."""
    hops, x = ping_scene()
    counts, records = [], []
    with hip.HipDecoder(channels=3, **S.CFG) as d, hip.HipDecoder(channels=3, **S.CFG) as plain:
        d.set_stream_pings()
        d.set_stream_gate()
        for k in range(hops):
            rec, seg = hop(d, k, [0, 1, 2], scene_rows(x, k))
            _, want_seg = hop(plain, k, [0, 1, 2], scene_rows(x, k))
            counts.append(len(d.stream_gate()[0]))
            records.append(len(rec))
            assert seg.tobytes() == want_seg.tobytes()
            assert counts[-1] > 0 or (len(rec) == 0 and d.result_count() == 0 and d.copy_count() == 0)
    assert counts[0] == 0 and max(counts) == 1 and sum(records[1:]) > 0


def test_behind_the_resampler(hip):
    """msk144_push_rate_hops at 48000 Hz: the list is that of the model fed the resampled rows (msk144_dump_rate_hop)."""
    inputs, _ = S.scene(48000)
    row = 2592 * 4
    C = S.CHANNELS
    pings, gate = sp.StreamPings(C, ratio_q4=32), sp.StreamGate(C, ratio_q4=20, always=[3])
    listed = set()
    with hip.HipDecoder(channels=C, **S.CFG) as d:
        d.set_input_rate(48000)
        d.set_stream_pings(ratio_q4=32)
        d.set_stream_gate(ratio_q4=20, always=[3])
        for k, ids in enumerate([[0, 1, 2, 3, 4], [0, 2, 3], [0, 1, 2, 3, 4], [1, 2, 4]]):
            firsts = [k == 0] * len(ids)
            hops, first_halves, streams, is_first = d.rate_hop_slot(k % 2)
            for j, s in enumerate(ids):
                v = inputs[s]
                if k == 0:
                    first_halves[j, :] = v[:row]
                hops[j, :] = v[(k + 1) * row:(k + 2) * row]
                streams[j] = s
                is_first[j] = 1 if k == 0 else 0
            d.push_rate_hops(k % 2, len(ids))
            rows = [d.dump_rate_hop(j) for j in range(len(ids))]
            rec, _, en, _ = pings.push(ids, firsts, rows)
            want = gate.push(ids, firsts, rec, en)
            got = d.stream_gate()
            assert same_list(got, want), (k, got, want)
            listed |= {ids[j] for j in got[0]}
            d.decode()
            d.fetch_async(k % 2)
            rec_out, _ = d.fetch_wait(k % 2)
            assert len(rec_out) == 0 or int(rec_out["channel"].max()) < len(got[0])
    assert 3 in listed and len(listed) > 1


def test_off_is_the_parent(hip):
    """The decode records of the input-rate scene's 12 kHz hops: a handle whose gate decoded a push and was switched off again, one
    whose gate was set and switched off before any push, and one that never had the entry called give the same bytes."""
    model_hops = S.scene(48000)[1]
    with hip.HipDecoder(channels=S.CHANNELS, **S.CFG) as was_on, hip.HipDecoder(channels=S.CHANNELS, **S.CFG) as set_off, hip.HipDecoder(channels=S.CHANNELS, **S.CFG) as never:
        was_on.set_stream_pings()
        was_on.set_stream_gate(always=[1])
        P.scene_push(was_on, 1, 0, model_hops)
        ids, rows = list(range(S.CHANNELS)), [model_hops[0][c] for c in range(S.CHANNELS)]
        rec, _, en, _ = sp.StreamPings(S.CHANNELS).push(ids, [1] * S.CHANNELS, rows)
        want = sp.StreamGate(S.CHANNELS, always=[1]).push(ids, [1] * S.CHANNELS, rec, en)
        assert same_list(was_on.stream_gate(), want) and 1 in want[0].tolist() and len(want[0]) < S.CHANNELS
        was_on.decode()
        was_on.fetch_async(1)
        was_on.fetch_wait(1)
        was_on.set_stream_gate(None)
        was_on.set_stream_pings(None)
        assert _code(hip, was_on.stream_gate) == ESTATE
        set_off.set_stream_gate(hold=3, max_streams=2, ratio_q4=32, always=[0])
        set_off.set_stream_gate(None)
        a, b, want = P.decode_hops(was_on, model_hops), P.decode_hops(set_off, model_hops), P.decode_hops(never, model_hops)
    assert sum(len(r) for r in want) > 0
    for x, y, w in zip(a, b, want):
        assert x.tobytes() == w.tobytes() and y.tobytes() == w.tobytes()


def test_state_and_refusals(hip):
    zeros = [np.zeros(5184, dtype=np.int16)] * 2
    with hip.HipDecoder(channels=2, **S.CFG) as d:
        assert _code(hip, d.stream_gate) == ESTATE                       # never set
        assert _code(hip, lambda: d.stream_gate_slot(0)) == ESTATE
        d.set_stream_gate(hold=16, min_up=27, max_streams=2, ratio_q4=65535, always=[1])
        assert _code(hip, d.stream_gate) == ESTATE                       # no push since the `set`
        P.push(d, 0, [0, 1], [1, 1], zeros)
        assert d.stream_gate()[0].tolist() == [1]                        # stream pings are off: only the always stream
        for bad in (dict(hold=-1), dict(hold=17), dict(min_up=0), dict(min_up=28), dict(max_streams=-1), dict(max_streams=3), dict(ratio_q4=15), dict(ratio_q4=65536), dict(ratio_q4=-1)):
            assert _code(hip, lambda: d.set_stream_gate(**bad)) == EINVAL
        assert d.stream_gate()[0].tolist() == [1]                        # a refused call changes nothing
        assert _code(hip, lambda: d.stream_gate_slot(1)) == ESTATE       # this slot has had no push
        assert _code(hip, lambda: d.stream_gate_slot(2)) == EINVAL
        d.decode()
        d.fetch_async(0)
        assert len(d.fetch_wait(0)[0]) == 0 and d.stream_gate_slot(0)[0].tolist() == [1]
        # a whole-window submit is not gated, moves no state and leaves the last push's list
        d.submit_audio(np.zeros((2, 5184), dtype=np.int16))
        d.decode()
        assert d.result_count() == 0 and d.stream_gate()[0].tolist() == [1]
        P.push(d, 1, [1], [0], zeros[:1])
        got = d.stream_gate()
        assert got[0].tolist() == [0] and got[1] == 1                    # POSITION 0 is stream 1
        d.set_stream_gate()
        assert _code(hip, d.stream_gate) == ESTATE                       # an accepted `set` ends the list
        assert _code(hip, lambda: d.stream_gate_slot(0)) == ESTATE
        d.set_stream_gate(None)
        assert _code(hip, d.stream_gate) == ESTATE                       # off
    with hip.HipDecoder(channels=2, read_mode=2, center=0.0, width=20.0, step=2.0, depth=2) as d:
        assert _code(hip, d.set_stream_gate) == EINVAL                   # read_mode 2
        d.set_wideband(48000, [-6000, 6000], "cu8")
        assert _code(hip, d.set_stream_gate) == EINVAL                   # and in wideband mode


# ---- the program ----
ARGS = ["--search-width=20", "--search-step=2", "--scan-depth=2"]


def _run(args):
    p = subprocess.run([EXE] + ARGS + args, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().strip().split("\n")
    assert lines[-1] == "Done"
    return [re.sub(r"date=\d{14}", "date=X", l) for l in lines[:-1]], p.stderr.decode()


def test_program_prints_the_ungated_lines_and_the_summary(tmp_path):
    """The three --inputs streams of the stream-pings program test with --stream-gate: every decode of the run lies in a window the
    gate lists, so stdout is the ungated run's, and the summary line carries the counts of StreamGate on the same samples - 5 of 18
    stream windows, stream 0 at pushes 1..5."""
    hops, x = ping_scene()
    paths = []
    for c, v in enumerate(x):
        f = tmp_path / f"s{c}.raw"
        f.write_bytes(v.tobytes())
        paths.append(str(f))
    want_out, _ = _run(["--inputs=" + ",".join(paths)])
    got_out, err = _run(["--inputs=" + ",".join(paths), "--stream-gate"])
    assert len(want_out) > 0 and got_out == want_out

    pings, gate = sp.StreamPings(3), sp.StreamGate(3)
    decoded = busiest = 0
    for k in range(hops):
        rec, _, en, _ = pings.push([0, 1, 2], [k == 0] * 3, scene_rows(x, k))
        positions, total = gate.push([0, 1, 2], [k == 0] * 3, rec, en)
        assert total == len(positions) and (positions.tolist() == ([0] if k >= 1 else []))
        decoded += len(positions)
        busiest = max(busiest, len(positions))
    assert (decoded, busiest) == (5, 1)
    line = [l for l in err.splitlines() if l.startswith("msk144hipdecoder: stream gate:")]
    assert len(line) == 1
    assert line[0].startswith(f"msk144hipdecoder: stream gate: {decoded} of {3 * hops} stream windows decoded, 0 dropped over max, busiest hop {busiest} (hold 1, min up 1, max 0, ")
