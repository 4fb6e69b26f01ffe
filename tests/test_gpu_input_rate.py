"""-m gpu: audio input at 24 to 192 kHz (include/msk144hip.h) - the resampler kernel bit for bit against input_rate.Resampler, the
decode behind it against a handle fed the model's output, the state rules, and the program with --input-rate."""
import os
import re
import subprocess

import numpy as np
import pytest

from msk144cudecoder_amd import input_rate as ir

import input_rate_scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "msk144cudecoder_amd", "msk144hipdecoder")
CH = S.CHANNELS
EINVAL, ESTATE = -1, -4

# three pushes: all five first; then streams 0, 2, 4; then 1, 2, 3 with stream 2 restarted
PUSHES = [([0, 1, 2, 3, 4], [1, 1, 1, 1, 1]), ([0, 2, 4], [0, 0, 0]), ([1, 2, 3], [0, 1, 0])]


def held_noise(rng, n, hold):
    """Uniform full-range int16 noise, every value held for `hold` samples."""
    return np.repeat(rng.integers(-32768, 32768, size=-(-n // hold)), hold)[:n].astype(np.int16)


def stream_rows(rate, seed):
    """Per stream a function n -> the next n input samples.  Stream 0: white uniform full-range noise.  Stream 1: the same noise
    with each value held for ceil(P/Q) samples - white noise at the input rate is averaged over P/Q samples by any of these filters
    and cannot reach the clamp above 48 kHz, held noise does at every rate: its reference clamp count must be non-zero.  Stream 2:
    constant +32767.  Stream 3: constant -32768.  Stream 4: white noise at a quarter of full scale."""
    rng = np.random.default_rng(seed)
    P, Q = ir.rate_ratio(rate)
    hold = -(-P // Q)
    return [lambda n: rng.integers(-32768, 32768, size=n).astype(np.int16), lambda n: held_noise(rng, n, hold), lambda n: np.full(n, 32767, dtype=np.int16),
            lambda n: np.full(n, -32768, dtype=np.int16), lambda n: rng.integers(-8192, 8192, size=n).astype(np.int16)]


def run_pushes(hip, rate, taps, shift, seed):
    """The three pushes on the device and through the model: per push (device hops, device counts, model hops, model counts)."""
    row = ir.row_samples(rate)
    gen = stream_rows(rate, seed)
    model = ir.Resampler(CH, rate, taps, shift)
    out = []
    with hip.HipDecoder(channels=CH, **S.CFG) as d:
        d.set_input_rate(rate, taps=taps, shift=shift)
        for b, (streams, firsts) in enumerate(PUSHES):
            s = b % 2
            hops, first_halves, ids, is_first = d.rate_hop_slot(s)
            assert hops.shape == (CH, row) and first_halves.shape == (CH, row)
            rows = []
            for j, (c, f) in enumerate(zip(streams, firsts)):
                x = gen[c]((2 if f else 1) * row)
                rows.append(x)
                if f:
                    first_halves[j, :] = x[:row]
                hops[j, :] = x[-row:]
                ids[j] = c
                is_first[j] = f
            d.push_rate_hops(s, len(streams))
            got = [d.dump_rate_hop(j) for j in range(len(streams))]
            counts = d.input_rate_clamped()
            # the slot's own copy (complete, as the call above has waited), and the other slot's still that of the push before
            assert np.array_equal(d.input_rate_slot_clamped(s), counts)
            assert b == 0 or np.array_equal(d.input_rate_slot_clamped(1 - s), out[-1][1])
            want, want_counts = model.push(rows, streams, firsts)
            out.append((got, counts, want, want_counts))
    return out


def check_pushes(results):
    for got, counts, want, want_counts in results:
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == np.int16 and g.shape == w.shape
            assert np.array_equal(g, w)
        assert np.array_equal(counts, want_counts)


CASES = [(r, k) for r in (24000, 32000, 48000, 96125, 192000) for k in (1, 16)] + [(24000, 64), (48000, 64), (96125, 64)]


@pytest.mark.parametrize("rate,K", CASES)
def test_hops_are_bit_exact(hip, rate, K):
    """msk144_dump_rate_hop and msk144_input_rate_clamped equal input_rate.Resampler on every row, with partial batches and a
    restarted stream."""
    results = run_pushes(hip, rate, ir.default_taps(rate, K), 14, seed=rate + K)
    check_pushes(results)
    # The noise rows clamp now and then: the model's count must be non-zero, or the comparison of the counts shows nothing.  Not at
    # K = 1: those P taps are all positive and sum to about 2^14, so an output is an average of inputs and stays in range.  The
    # held-noise row (stream 1) at every rate; the white row (stream 0) where it can: white uniform noise has sigma 18918, the filter
    # passes at most Q/P of its power, so full scale lies no nearer than 2.4 sigma at 24000 Hz and 2.8 at 32000 Hz, within reach of
    # the row's 7776 outputs, but 3.5 sigma and more from 48000 Hz on, 6.9 at 192000 Hz.
    if K >= 16:
        count = lambda stream: sum(int(results[b][3][j]) for b, (streams, _) in enumerate(PUSHES) for j, s in enumerate(streams) if s == stream)
        assert count(1) > 0
        if rate in (24000, 32000):
            assert count(0) > 0


# 24000 Hz: one branch of three taps.  32000 Hz (P/Q = 8/3, K = 2): branch 0 has six taps, 10925 + 5 x 10922; branches 1 and 2 five of 13107
EDGE_TAPS = {24000: [32767, 32767, 1, 0], 32000: [10925 if k == 0 else 10922 if k % 3 == 0 else 13107 for k in range(16)]}


@pytest.mark.parametrize("rate", sorted(EDGE_TAPS))
def test_custom_filter_at_the_headroom_edge(hip, rate):
    """Every branch sums to exactly 65535 and s = 15: constant -32768 drives the accumulator to -(2^31 - 32768)."""
    taps = np.array(EDGE_TAPS[rate], dtype=np.int16)
    P, Q = ir.rate_ratio(rate)
    assert ir.check_config(rate, taps, 15) == "" and all(int(np.abs(taps[r::Q].astype(np.int64)).sum()) == 65535 for r in range(Q))
    results = run_pushes(hip, rate, taps, 15, seed=rate)
    check_pushes(results)
    assert sum(int(c.sum()) for _, _, _, c in results) > 0


def _decode_hops(d, push):
    """The records of the scene's four hops; push(d, slot, k) hands hop k of every stream to the handle."""
    recs = []
    for k in range(S.HOPS):
        s = k % 2
        push(d, s, k)
        d.decode()
        d.fetch_async(s)
        recs.append(d.fetch_wait(s)[0])
    return recs


def _push_model(model_hops):
    """The parent's msk144_push_hops sequence on the model's 12 kHz output."""
    def push(d, s, k):
        hops, first_halves, ids, is_first = d.hop_slot(s)
        for c in range(CH):
            y = model_hops[k][c]
            if k == 0:
                first_halves[c, :] = y[:2592]
            hops[c, :] = y[-2592:]
        ids[:CH] = np.arange(CH)
        is_first[:CH] = 1 if k == 0 else 0
        d.push_hops(s, CH)
    return push


@pytest.mark.parametrize("rate", [48000, 32000])
def test_decode_identity(hip, rate):
    """The records of msk144_push_rate_hops -> decode -> fetch over four hops equal, byte for byte, those of a second handle fed
    the model's output through msk144_push_hops."""
    inputs, model_hops = S.scene(rate)
    row = ir.row_samples(rate)

    def push_rate(d, s, k):
        hops, first_halves, ids, is_first = d.rate_hop_slot(s)
        for c in range(CH):
            if k == 0:
                first_halves[c, :] = inputs[c][:row]
            hops[c, :] = inputs[c][(k + 1) * row:(k + 2) * row]
        ids[:CH] = np.arange(CH)
        is_first[:CH] = 1 if k == 0 else 0
        d.push_rate_hops(s, CH)

    counts = []     # per hop: (right behind the push, waiting for it; the slot's own copy behind fetch_wait)

    def push_rate_counted(d, s, k):
        push_rate(d, s, k)
        counts.append([d.input_rate_clamped()])

    with hip.HipDecoder(channels=CH, **S.CFG) as d, hip.HipDecoder(channels=CH, **S.CFG) as ref:
        d.set_input_rate(rate)
        assert _code(hip, lambda: d.input_rate_slot_clamped(0)) == ESTATE
        got = []
        for k in range(S.HOPS):
            s = k % 2
            push_rate_counted(d, s, k)
            d.decode()
            d.fetch_async(s)
            if k >= 1:      # the other slot's hop is fetched with this one already pushed: its counts are still its own
                got.append(d.fetch_wait(1 - s)[0])
                counts[k - 1].append(d.input_rate_slot_clamped(1 - s))
        got.append(d.fetch_wait((S.HOPS - 1) % 2)[0])
        counts[-1].append(d.input_rate_slot_clamped((S.HOPS - 1) % 2))
        for at_push, of_slot in counts:
            assert len(of_slot) == CH and np.array_equal(at_push, of_slot)
        want = _decode_hops(ref, _push_model(model_hops))
    assert sum(len(r) for r in want) > 0
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


def _code(hip, fn):
    with pytest.raises(hip.Msk144Error) as e:
        fn()
    return e.value.code


def test_state_and_refusals(hip):
    rate = 48000
    row = ir.row_samples(rate)
    h48 = ir.default_taps(48000, 16)
    with hip.HipDecoder(channels=CH, **S.CFG) as d:
        # the bad configurations
        for bad in (12000, 44100, 22050, 23875, 192125, 384000):
            assert _code(hip, lambda: d.set_input_rate(bad, taps=h48)) == EINVAL
        assert _code(hip, lambda: d.set_input_rate(48000, taps=h48[:-1])) == EINVAL               # L not a multiple of P
        assert _code(hip, lambda: d.set_input_rate(48000, taps=np.zeros(65 * 4, dtype=np.int16))) == EINVAL   # K = 65
        assert _code(hip, lambda: d.set_input_rate(48000, taps=h48, shift=0)) == EINVAL
        assert _code(hip, lambda: d.set_input_rate(48000, taps=h48, shift=16)) == EINVAL
        assert _code(hip, lambda: d.set_input_rate(24000, taps=[32767, 32767, 1, 1], shift=15)) == EINVAL     # a branch sum of 65536
        assert _code(hip, lambda: d.rate_hop_slot(0)) == ESTATE                                   # nothing is set
        # a later hop before a first one
        d.set_input_rate(rate)
        hops, first_halves, ids, is_first = d.rate_hop_slot(0)
        hops[:] = 0
        first_halves[:] = 0
        ids[:2] = [0, 1]
        is_first[:2] = [1, 0]
        assert _code(hip, lambda: d.push_rate_hops(0, 2)) == ESTATE
        is_first[:2] = [1, 1]
        d.push_rate_hops(0, 2)
        is_first[:2] = [0, 0]
        d.push_rate_hops(0, 2)
        ids[:2] = [1, 0]
        assert _code(hip, lambda: d.push_rate_hops(0, 2)) == EINVAL                               # not ascending
        # ... and after a new `set`, which resets every stream
        d.set_input_rate(rate)
        hops, first_halves, ids, is_first = d.rate_hop_slot(0)
        ids[:2] = [0, 1]
        is_first[:2] = [0, 0]
        assert _code(hip, lambda: d.push_rate_hops(0, 2)) == ESTATE
        assert _code(hip, lambda: d.dump_rate_hop(0)) == ESTATE                                   # no push since the `set`
    with hip.HipDecoder(channels=2, read_mode=2, center=0.0, width=20.0, step=2.0, depth=2) as d:
        assert _code(hip, lambda: d.set_input_rate(48000)) == EINVAL                              # read_mode 2
        d.set_wideband(48000, [-6000, 6000], "cu8")
        assert _code(hip, lambda: d.set_input_rate(48000)) == EINVAL                              # and in wideband mode


def test_switched_off_the_handle_is_the_parent(hip):
    """set(None) followed by the parent's msk144_push_hops sequence gives the records of a handle that never had an input rate."""
    push_model = _push_model(S.scene(48000)[1])
    with hip.HipDecoder(channels=CH, **S.CFG) as d, hip.HipDecoder(channels=CH, **S.CFG) as ref:
        d.set_input_rate(96125, taps_per_phase=4)
        hops, first_halves, ids, is_first = d.rate_hop_slot(1)
        hops[:] = 1000
        first_halves[:] = -1000
        ids[:CH] = np.arange(CH)
        is_first[:CH] = 1
        d.push_rate_hops(1, CH)
        d.decode()
        d.fetch_async(1)
        d.fetch_wait(1)
        d.set_input_rate(None)
        assert _code(hip, lambda: d.push_rate_hops(0, CH)) == ESTATE
        got = _decode_hops(d, push_model)
        want = _decode_hops(ref, push_model)
    assert sum(len(r) for r in want) > 0
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


# ---- the program ----
ARGS = ["--search-width=20", "--search-step=2", "--scan-depth=2"]


def _run(args, data=b""):
    p = subprocess.run([EXE] + ARGS + args, input=data, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().strip().split("\n")
    assert lines[-1] == "Done"
    return [re.sub(r"date=\d{14}", "date=X", l) for l in lines[:-1]], p.stderr.decode()


def _model_12k(c, hops):
    """Stream c of the 48 kHz scene as the model resamples it, its first `hops` hops."""
    _, model_hops = S.scene(48000)
    return np.concatenate([model_hops[k][c] for k in range(hops)])


def test_program_stdin_and_wav_header():
    """--input-rate=48000 on stdin prints what the program without the option prints for the model-resampled stream; so does
    --skip-wav-header --input-rate=wav with the rate in the header."""
    inputs, _ = S.scene(48000)
    want, _ = _run([], _model_12k(0, S.HOPS).tobytes())
    got, err = _run(["--input-rate=48000"], inputs[0].tobytes())
    assert len(want) > 0 and got == want
    assert "input rate 48000 Hz = 12000 x 4/1, 64 taps (16 per phase), shift 14, " in err
    header = b"RIFF" + (36 + inputs[0].nbytes).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little") + (1).to_bytes(2, "little") + \
        (48000).to_bytes(4, "little") + (96000).to_bytes(4, "little") + (2).to_bytes(2, "little") + (16).to_bytes(2, "little") + b"data" + inputs[0].nbytes.to_bytes(4, "little")
    got_wav, _ = _run(["--skip-wav-header", "--input-rate=wav"], header + inputs[0].tobytes())
    assert got_wav == want


def test_program_two_inputs_of_different_length(tmp_path):
    inputs, _ = S.scene(48000)
    row = ir.row_samples(48000)
    hops = (S.HOPS, S.HOPS - 2)                  # the second file ends two hops early
    at_rate, at_12k = [], []
    for j, (c, n) in enumerate(zip((1, 0), hops)):
        a, b = tmp_path / f"r{j}.raw", tmp_path / f"m{j}.raw"
        a.write_bytes(inputs[c][:(n + 1) * row].tobytes())
        b.write_bytes(_model_12k(c, n).tobytes())
        at_rate.append(str(a))
        at_12k.append(str(b))
    want, _ = _run(["--inputs=" + ",".join(at_12k)])
    got, _ = _run(["--input-rate=48000", "--inputs=" + ",".join(at_rate)])
    per = lambda lines, c: [l for l in lines if f"ch={c}; " in l]
    assert len(per(want, 0)) > 0 and len(per(want, 1)) > 0
    for c in range(2):
        assert per(got, c) == per(want, c)
