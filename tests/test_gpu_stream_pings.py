"""-m gpu: per-stream levels and pings of the audio hops (include/msk144hip.h "Stream levels and pings") - the kernel against
stream_pings.StreamPings in integer equality, behind msk144_push_hops and msk144_push_rate_hops, pipelined, switched off, refused,
and the program with --stream-pings and --stream-levels."""
import os
import re
import subprocess

import numpy as np
import pytest

from msk144cudecoder_amd import input_rate as ir
from msk144cudecoder_amd import stream_pings as sp
from msk144cudecoder_amd import synth

import input_rate_scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "msk144cudecoder_amd", "msk144hipdecoder")
EINVAL, ESTATE = -1, -4
CAP = sp.ENERGY_CAP


def _code(hip, fn):
    with pytest.raises(hip.Msk144Error) as e:
        fn()
    return e.value.code


def noise_row(rng, n, sigma, loud=3):
    """Gaussian noise of `sigma` LSB with `loud` blocks of 96 samples eight times as strong."""
    x = rng.normal(0.0, sigma, size=n)
    for b in rng.integers(0, n // 96, size=loud):
        x[96 * b:96 * (b + 1)] *= 8.0
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def push(d, slot, ids, firsts, rows):
    """One msk144_push_hops of the rows (5184 samples where first, else 2592) of the listed streams."""
    hops, first_halves, streams, is_first = d.hop_slot(slot)
    for j, (s, f, x) in enumerate(zip(ids, firsts, rows)):
        if f:
            first_halves[j, :] = x[:2592]
        hops[j, :] = x[-2592:]
        streams[j] = s
        is_first[j] = 1 if f else 0
    d.push_hops(slot, len(ids))


def check_push(d, slot, want):
    """What the last push left, through all three read entries, against the model's (records, levels, energies, events)."""
    w_rec, w_lev, w_en, _ = want
    rec, lev = d.stream_pings()
    assert rec.dtype == w_rec.dtype and lev.dtype == w_lev.dtype
    assert rec.tobytes() == w_rec.tobytes(), (rec, w_rec)
    assert lev.tobytes() == w_lev.tobytes(), (lev, w_lev)
    s_rec, s_lev, s_en = d.stream_pings_slot(slot)      # the call above has waited
    assert s_rec.tobytes() == w_rec.tobytes() and s_lev.tobytes() == w_lev.tobytes()
    assert s_en.shape == w_en.shape and np.array_equal(s_en, w_en)          # all 54 or 27 energies, and zeros behind them
    for j in (0, len(rec) - 1):
        e = d.stream_ping_blocks(j)
        assert len(e) == int(w_rec["blocks"][j]) and np.array_equal(e, w_en[j, :len(e)])


def plan(C, pushes, rng):
    """Per push (ids, firsts): every stream first at push 0; later a seeded subset that always holds stream 0 (so that its ring of
    16 wraps), for five streams 0, 2, 3 at push 1; first and later hops mixed in push 5 (the last stream starts over); stream
    min(1, C - 1) restarted at push 9."""
    out = [(list(range(C)), [1] * C)]
    for k in range(1, pushes):
        ids = [0] + [s for s in range(1, C) if rng.random() < 0.6]
        if C == 5 and k == 1:
            ids = [0, 2, 3]
        firsts = [0] * len(ids)
        for at, s in ((5, C - 1), (9, min(1, C - 1))):
            if k == at:
                if s not in ids:
                    ids = sorted(ids + [s])
                    firsts = [0] * len(ids)
                firsts[ids.index(s)] = 1
        out.append((ids, firsts))
    return out


@pytest.mark.parametrize("C", [1, 5, 67])
def test_records_levels_and_energies_equal_the_model(hip, C):
    """Twenty pushes with partial lists, mixed first and later hops, a restart and a history longer than the ring of 16: records,
    levels and energies equal StreamPings after every push.  67 streams fill sixteen workgroups of four waves and leave the last
    one ragged.  A stream the pushes skipped continues its history where it left it: the model's `history` says so."""
    rng = np.random.default_rng(100 + C)
    params = dict(ratio_q4=40, memory=16, min_ref=96, shift=12)
    model = sp.StreamPings(C, **params)
    skipped_then_continued = 0
    last_history = {}
    with hip.HipDecoder(channels=C, **S.CFG) as d:
        d.set_stream_pings(**params)
        for k, (ids, firsts) in enumerate(plan(C, 20, rng)):
            rows = [noise_row(rng, 5184 if f else 2592, float(rng.choice([150.0, 400.0, 1200.0]))) for f in firsts]
            push(d, k % 2, ids, firsts, rows)
            want = model.push(ids, firsts, rows)
            check_push(d, k % 2, want)
            for j, (s, f) in enumerate(zip(ids, firsts)):
                h = int(want[0]["history"][j])
                if not f and s in last_history and last_history[s][0] < k - 1:
                    assert h == min(16, last_history[s][1] + 1)      # untouched while unlisted
                    skipped_then_continued += 1
                last_history[s] = (k, h)
        if C == 1:
            assert int(want[0]["history"][0]) == 10                    # the one stream: restarted at push 9, ten pushes since
        else:
            assert int(want[0]["history"][0]) == 16 and skipped_then_continued > 0     # stream 0: twenty pushes, the ring of 16 has wrapped


@pytest.mark.parametrize("shift", [0, 12, 24])
def test_extremes_in_one_push(hip, shift):
    """All -32768, all zero, constant magnitude and two equal largest blocks, as a first push (54 blocks) and a later one (27)."""
    rng = np.random.default_rng(7 + shift)
    params = dict(ratio_q4=32, memory=8, min_ref=96, shift=shift)
    model = sp.StreamPings(4, **params)

    def rows(n):
        const = np.where(np.arange(n) % 2 == 0, 1000, -1000).astype(np.int16)
        twin = rng.integers(-100, 101, size=n).astype(np.int16)
        loud = rng.integers(-20000, 20001, size=96).astype(np.int16)
        twin[96 * 5:96 * 6] = loud
        twin[96 * 20:96 * 21] = loud
        return [np.full(n, -32768, dtype=np.int16), np.zeros(n, dtype=np.int16), const, twin]

    with hip.HipDecoder(channels=4, **S.CFG) as d:
        d.set_stream_pings(**params)
        for k, first in enumerate((1, 0)):
            x = rows(5184 if first else 2592)
            nb = 54 if first else 27
            push(d, k, [0, 1, 2, 3], [first] * 4, x)
            want = model.push([0, 1, 2, 3], [first] * 4, x)
            check_push(d, k, want)
            rec, lev = d.stream_pings()
            en = d.stream_pings_slot(k)[2]
            # full scale: the exact sum, every sample counted, every block at the cap for shifts up to 14
            assert int(lev["sum_sq"][0]) == nb * 96 * 2 ** 30 and int(lev["sum"][0]) == -32768 * 96 * nb
            assert int(lev["peak"][0]) == 32768 and int(lev["full_scale"][0]) == int(lev["samples"][0]) == 96 * nb
            assert int(lev["saturated_blocks"][0]) == (nb if shift <= 14 else 0)
            assert np.all(en[0, :nb] == (CAP if shift <= 14 else (96 * 2 ** 30) >> shift))
            # zeros: R is the floor
            assert int(rec["reference"][1]) == 96 and int(rec["up_mask"][1]) == 0 and int(lev["peak"][1]) == 0
            # every E equal: the quiet level is E, nothing is up, the peak is block 0
            assert np.all(en[2, :nb] == en[2, 0]) and int(rec["quiet"][2]) == int(en[2, 0]) == min(CAP, (96 * 1000 * 1000) >> shift)
            assert int(rec["up_mask"][2]) == 0 and int(rec["peak_block"][2]) == 0 and int(rec["peak"][2]) == int(en[2, 0])
            # two equal largest blocks: the lower one is the peak
            assert int(en[3, 5]) == int(en[3, 20]) == int(en[3, :nb].max()) > 0
            assert int(rec["peak_block"][3]) == 5 and int(rec["peak"][3]) == int(en[3, 5])


@pytest.mark.parametrize("rate,K", [(48000, 16), (96125, 4)])
def test_behind_the_resampler(hip, rate, K):
    """msk144_push_rate_hops: the records are those of the model fed the resampled samples (msk144_dump_rate_hop).  96125 Hz has
    rows of 20763 samples, an odd length."""
    rng = np.random.default_rng(rate)
    row = ir.row_samples(rate)
    params = dict(ratio_q4=32, memory=8, min_ref=96, shift=12)
    model = sp.StreamPings(5, **params)
    pushes = [([0, 1, 2, 3, 4], [1, 1, 1, 1, 1]), ([0, 2, 4], [0, 0, 0]), ([1, 2, 3], [0, 1, 0])]
    assert rate != 96125 or row == 20763
    with hip.HipDecoder(channels=5, **S.CFG) as d:
        d.set_input_rate(rate, taps_per_phase=K)
        d.set_stream_pings(**params)
        for k, (ids, firsts) in enumerate(pushes):
            hops, first_halves, streams, is_first = d.rate_hop_slot(k % 2)
            for j, (s, f) in enumerate(zip(ids, firsts)):
                x = noise_row(rng, 2 * row, 3000.0 if s == 4 else 600.0, loud=4)
                first_halves[j, :] = x[:row]
                hops[j, :] = x[row:]
                streams[j] = s
                is_first[j] = f
            d.push_rate_hops(k % 2, len(ids))
            rows = [d.dump_rate_hop(j) for j in range(len(ids))]
            assert [len(r) for r in rows] == [5184 if f else 2592 for f in firsts]
            check_push(d, k % 2, model.push(ids, firsts, rows))


def scene_push(d, s, k, model_hops):
    """Hop k of the five streams of the input-rate scene, as 12 kHz hops."""
    push(d, s, list(range(S.CHANNELS)), [k == 0] * S.CHANNELS, [model_hops[k][c] for c in range(S.CHANNELS)])


def decode_hops(d, model_hops):
    recs = []
    for k in range(S.HOPS):
        scene_push(d, k % 2, k, model_hops)
        d.decode()
        d.fetch_async(k % 2)
        recs.append(d.fetch_wait(k % 2)[0])
    return recs


def test_pipelined_slots_keep_their_own_results(hip):
    """Both slots in flight: what msk144_stream_pings_slot gives behind msk144_fetch_wait equals msk144_stream_pings taken at the
    push, although the other slot has been pushed since."""
    model_hops = S.scene(48000)[1]
    model = sp.StreamPings(S.CHANNELS)
    with hip.HipDecoder(channels=S.CHANNELS, **S.CFG) as d:
        d.set_stream_pings()
        assert _code(hip, lambda: d.stream_pings_slot(0)) == ESTATE
        at_push, of_slot = [], []
        for k in range(S.HOPS):
            s = k % 2
            scene_push(d, s, k, model_hops)
            at_push.append(d.stream_pings())
            want = model.push(list(range(S.CHANNELS)), [k == 0] * S.CHANNELS, [model_hops[k][c] for c in range(S.CHANNELS)])
            assert at_push[-1][0].tobytes() == want[0].tobytes() and at_push[-1][1].tobytes() == want[1].tobytes()
            d.decode()
            d.fetch_async(s)
            if k >= 1:
                d.fetch_wait(1 - s)
                of_slot.append(d.stream_pings_slot(1 - s))
        d.fetch_wait((S.HOPS - 1) % 2)
        of_slot.append(d.stream_pings_slot((S.HOPS - 1) % 2))
    for (rec, lev), (s_rec, s_lev, _) in zip(at_push, of_slot):
        assert len(s_rec) == S.CHANNELS and rec.tobytes() == s_rec.tobytes() and lev.tobytes() == s_lev.tobytes()


def test_off_is_the_parent(hip):
    """The decode records of the scene: a handle whose option was used and switched off again, one with the option on, and one that
    never had it give the same bytes."""
    model_hops = S.scene(48000)[1]
    with hip.HipDecoder(channels=S.CHANNELS, **S.CFG) as was_on, hip.HipDecoder(channels=S.CHANNELS, **S.CFG) as on, hip.HipDecoder(channels=S.CHANNELS, **S.CFG) as never:
        was_on.set_stream_pings()
        scene_push(was_on, 1, 0, model_hops)
        was_on.stream_pings()
        was_on.decode()
        was_on.fetch_async(1)
        was_on.fetch_wait(1)
        was_on.set_stream_pings(None)
        assert _code(hip, was_on.stream_pings) == ESTATE
        on.set_stream_pings()
        got_off, got_on, want = decode_hops(was_on, model_hops), decode_hops(on, model_hops), decode_hops(never, model_hops)
    assert sum(len(r) for r in want) > 0
    for a, b, w in zip(got_off, got_on, want):
        assert a.tobytes() == w.tobytes() and b.tobytes() == w.tobytes()


def test_state_and_refusals(hip):
    zeros = [np.zeros(5184, dtype=np.int16)] * 2
    with hip.HipDecoder(channels=2, **S.CFG) as d:
        for bad in (dict(ratio_q4=15), dict(ratio_q4=65536), dict(memory=-1), dict(memory=17), dict(min_ref=0), dict(min_ref=(1 << 22) + 1), dict(shift=-1), dict(shift=25)):
            assert _code(hip, lambda: d.set_stream_pings(**bad)) == EINVAL
        assert _code(hip, d.stream_pings) == ESTATE                     # never set
        d.set_stream_pings(shift=24, ratio_q4=65535, memory=0, min_ref=1 << 22)
        assert _code(hip, d.stream_pings) == ESTATE                     # no push since the `set`
        assert _code(hip, lambda: d.stream_ping_blocks(0)) == ESTATE
        assert _code(hip, lambda: d.stream_pings_slot(0)) == ESTATE
        push(d, 0, [0, 1], [1, 1], zeros)
        rec, lev = d.stream_pings()
        assert len(rec) == 2 and int(rec["reference"][0]) == 1 << 22
        assert _code(hip, lambda: d.stream_ping_blocks(2)) == EINVAL    # past n of the push
        assert _code(hip, lambda: d.stream_pings_slot(1)) == ESTATE     # this slot has had no push
        # a whole-window submit leaves no records and the last push's stay
        d.submit_audio(np.zeros((2, 5184), dtype=np.int16))
        assert d.stream_pings()[0].tobytes() == rec.tobytes()
        d.set_stream_pings()
        assert _code(hip, d.stream_pings) == ESTATE                     # a new `set`
        assert _code(hip, lambda: d.stream_pings_slot(0)) == ESTATE
    with hip.HipDecoder(channels=2, read_mode=2, center=0.0, width=20.0, step=2.0, depth=2) as d:
        assert _code(hip, d.set_stream_pings) == EINVAL                 # read_mode 2
        d.set_wideband(48000, [-6000, 6000], "cu8")
        assert _code(hip, d.set_stream_pings) == EINVAL                 # and in wideband mode


# ---- the program ----
ARGS = ["--search-width=20", "--search-step=2", "--scan-depth=2"]


def _run(args):
    p = subprocess.run([EXE] + ARGS + args, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().strip().split("\n")
    assert lines[-1] == "Done"
    return [re.sub(r"date=\d{14}", "date=X", l) for l in lines[:-1]], p.stderr.decode()


def test_program_logs_and_summaries_equal_the_model(tmp_path):
    """Three --inputs streams - noise with a strong ping, noise alone, silence - with --stream-pings and --stream-levels: the log
    and both summaries are the model's on the same samples, stdout is that of the run without the options."""
    rng = np.random.default_rng(31)
    hops = 6
    n = 5184 + (hops - 1) * 2592
    ping = synth.Ping(synth.random_message(rng), 7000, 8, 1500.0, 20.0, 0.3)
    x = [synth.synth_audio(n, [ping], 300.0, rng), synth.synth_audio(n, [], 300.0, rng), np.zeros(n, dtype=np.int16)]
    paths = []
    for c, v in enumerate(x):
        f = tmp_path / f"s{c}.raw"
        f.write_bytes(v.astype(np.int16).tobytes())
        paths.append(str(f))
    log = tmp_path / "pings.log"
    want_out, _ = _run(["--inputs=" + ",".join(paths)])
    got_out, err = _run(["--inputs=" + ",".join(paths), f"--stream-pings={log}", "--stream-levels"])
    assert len(want_out) > 0 and got_out == want_out

    defaults = dict(sp.STREAM_PINGS_DEFAULTS)
    model, report, events = sp.StreamPings(3), sp.StreamReport(3), []
    for k in range(hops):
        rows = [v[:5184] if k == 0 else v[(k + 1) * 2592:(k + 2) * 2592] for v in x]
        _, lev, _, ev = model.push([0, 1, 2], [k == 0] * 3, rows)
        report.add([0, 1, 2], lev, ev)
        events += ev
    tail = model.close()
    report.add_events(tail)
    events += tail
    got_log = log.read_text().splitlines()
    # the streams of a batch are those whose hop was ready: the order of the lines between streams is the run's, within a stream the model's
    for c in range(3):
        assert [l for l in got_log if l.startswith(f"ping ch={c} ")] == [sp.stream_ping_line(e) for e in events if e["channel"] == c]
    assert len(got_log) == len(events)
    assert any(l.startswith("ping ch=0 ") for l in got_log) and not any(l.startswith("ping ch=2 ") for l in got_log)
    err_lines = err.splitlines()
    assert report.pings_line(model, dict(defaults, min_blocks=2)) in err_lines
    want_levels = report.levels_lines()
    assert [l for l in err_lines if l.startswith("msk144hipdecoder: stream levels:")] == want_levels
    assert want_levels[-1].endswith("all hops zero ch=2")
