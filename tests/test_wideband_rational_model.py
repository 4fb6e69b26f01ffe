"""Wideband channeliser at rational rates Fs = 12000 P/Q, on the CPU: the rate ratio, the default prototype filter, the float64
model of the contract (msk144cudecoder_amd/wideband.py) against a naive zero-stuff -> filter -> decimate, and hop-by-hop
filtering against the whole stream."""
import os
import subprocess

import numpy as np
import pytest

from msk144cudecoder_amd import wideband as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "msk144cudecoder_amd", "host")


@pytest.fixture(scope="module", autouse=True)
def host_lib():
    subprocess.run(["make", "-s", "-C", HOST, "../libmsk144host.so"], check=True)


@pytest.mark.parametrize("rate, ratio", [(2048000, (512, 3)), (2500000, (625, 3)), (250000, (125, 6)), (24125, (193, 96)),
                                         (1920000, (160, 1)), (6142000, (3071, 6))])
def test_rate_ratio(rate, ratio):
    assert wb.rate_ratio(rate) == ratio


@pytest.mark.parametrize("D", [2, 80, 160, 512])
def test_integer_rate_taps_are_the_integer_design(D):
    assert np.array_equal(wb.default_taps_for_rate(D * 12000, 16), wb.default_taps(D, 16))


def _response_db(h, fs, freqs):
    n = np.arange(len(h))
    H = np.array([abs(np.sum(h * np.exp(-2j * np.pi * f * n / fs))) for f in freqs])
    return 20 * np.log10(np.maximum(H, 1e-300) / abs(h.sum()))


@pytest.mark.parametrize("rate", [2048000, 2500000, 250000, 24125, 96125])
def test_rational_default_taps_meet_the_filter_spec(rate):
    P, Q = wb.rate_ratio(rate)
    h = wb.default_taps_for_rate(rate, 16)
    assert len(h) == 16 * P
    assert np.allclose(h, h[::-1], atol=1e-15)
    assert abs(h.sum() - Q) < 1e-9
    for r in range(Q):
        assert abs(h[r::Q].sum() - 1.0) < 1e-3, r            # every branch about unit DC gain
    fs = 12000 * P                                           # the prototype rate Q Fs
    passband = _response_db(h, fs, np.linspace(0, 4000, 81))
    assert passband.max() - passband.min() <= 0.1
    stop = _response_db(h, fs, np.linspace(8000, fs / 2, 3000))
    assert stop.max() <= -60.0


def test_rational_default_taps_refuse_out_of_range():
    for rate in (44100, 2048001, 23875, 6144125, 0):
        with pytest.raises(ValueError):
            wb.default_taps_for_rate(rate, 16)
    with pytest.raises(ValueError):
        wb.default_taps_for_rate(2048000, 65)


def _noise(n, rng, scale=0.3):
    return scale * (rng.normal(size=n) + 1j * rng.normal(size=n))


def _offsets(rate):
    lim = rate // 2 - 6000
    return [0, -lim, lim, 5999, -5999, 1234, -(lim // 3) - 7]


@pytest.mark.parametrize("rate", [24125, 250000, 2048000])
def test_model_equals_naive_zero_stuff_filter_decimate(rate):
    P, Q = wb.rate_ratio(rate)
    rng = np.random.default_rng(rate)
    M = 2 * 96                                               # outputs: a multiple of every Q
    x = _noise(M * P // Q, rng)
    offsets = _offsets(rate)
    ch = wb.Channeliser(rate, offsets, K=16)
    y = ch.filter(x)
    assert y.shape == (len(offsets), M)
    for c, f in enumerate(offsets):
        ref = wb.naive_resampled_channel(x, rate, f, ch.taps)
        assert np.max(np.abs(y[c] - ref)) < 1e-12, f


@pytest.mark.parametrize("rate", [24125, 250000, 2048000])
def test_hop_by_hop_equals_whole_stream(rate):
    P, Q = wb.rate_ratio(rate)
    rng = np.random.default_rng(7 + rate)
    offsets = _offsets(rate)
    sizes = [n // 2 for n in wb.push_sizes_for_rate(4, rate)]
    assert sizes == [wb.FIRST_OUT * P // Q] + [wb.HOP_OUT * P // Q] * 3
    x = _noise(sum(sizes), rng, 0.02)
    whole = wb.Channeliser(rate, offsets)
    q_all, clip_all = wb.quantise(whole.filter(x), whole.gain)
    hop = wb.Channeliser(rate, offsets)
    pos, got, clips = 0, [], 0
    for i, n in enumerate(sizes):
        q, cl = hop.push(x[pos:pos + n], first=(i == 0))
        got.append(q)
        clips += cl
        pos += n
    assert np.array_equal(np.concatenate(got, axis=1), q_all)
    assert clips == clip_all


def test_integer_rate_model_is_unchanged_by_the_rational_path():
    """A rate that is a multiple of 12000 keeps the integer formula: the same output as mix -> filter -> decimate by D."""
    rng = np.random.default_rng(3)
    x = _noise(300 * 80, rng)
    ch = wb.Channeliser(960000, [0, 12345, -400000])
    assert ch.Q == 1 and ch.D == 80
    y = ch.filter(x)
    for c, f in enumerate([0, 12345, -400000]):
        assert np.max(np.abs(y[c] - wb.naive_channel(x, 960000, f, ch.taps))) < 1e-9


@pytest.mark.parametrize("rate", [250000, 2048000])
def test_synth_wideband_rational_length_and_tone(rate):
    """A rational-rate scene has n_out P/Q samples, and a planted tone lands in its channel at the planted level."""
    from msk144cudecoder_amd import synth
    P, Q = wb.rate_ratio(rate)
    rng = np.random.default_rng(11)
    n_out = wb.FIRST_OUT
    msg = synth.random_message(rng)
    f_c = 24000
    raw = wb.synth_wideband(n_out, rate, [(f_c, synth.Ping(msg, 500, 2, 300.0, 20.0, 0.0))], 0.02, rng, "cs16")
    assert raw.size == 2 * n_out * P // Q
    ch = wb.Channeliser(rate, [f_c, -f_c])
    y = ch.filter(wb.read_samples(raw, "cs16"))
    p_on = np.mean(np.abs(y[0, 600:2000]) ** 2)
    p_off = np.mean(np.abs(y[1, 600:2000]) ** 2)
    assert p_on > 20 * p_off


def test_integer_scene_is_byte_identical_to_the_integer_synthesiser():
    """synth_wideband at D x 12000 keeps its integer path (seeded scenes of existing tests depend on it)."""
    from msk144cudecoder_amd import synth
    msg = synth.random_message(np.random.default_rng(1))
    pings = [(12000, synth.Ping(msg, 300, 2, 100.0, 10.0, 0.5))]
    a = wb.synth_wideband(wb.FIRST_OUT, 48000, pings, 0.05, np.random.default_rng(9), "cu8")
    # the integer path by hand: noise, then the ping spectrum zero-padded by D = 4, placed at start * D
    rng = np.random.default_rng(9)
    N = wb.FIRST_OUT * 4
    x = rng.normal(0.0, 0.05, N) + 1j * rng.normal(0.0, 0.05, N)
    p = pings[0][1]
    bb = synth._ping_baseband(p)
    up = wb._upsample(bb, 4)
    amp = np.sqrt(2.0 * 0.05 ** 2 * (2500.0 / 48000) * 10.0 ** (p.snr_db / 10.0))
    n = np.arange(p.start * 4, min(N, p.start * 4 + len(up)))
    x[n] += amp * up[:len(n)] * np.exp(1j * (2 * np.pi * (12000 + p.freq_hz) * n / 48000 + p.phase))
    assert np.array_equal(a, wb.write_samples(x, "cu8"))
