"""Wideband channeliser on the CPU: the default prototype filter meets its spec, the float64 model of the contract
(msk144cudecoder_amd/wideband.py) equals mix -> filter -> decimate, and pushing hop by hop equals filtering the whole stream."""
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


def _response_db(h, fs, freqs):
    n = np.arange(len(h))
    H = np.array([abs(np.sum(h * np.exp(-2j * np.pi * f * n / fs))) for f in freqs])
    return 20 * np.log10(np.maximum(H, 1e-300))


@pytest.mark.parametrize("D", [40, 80, 160, 200])
def test_default_taps_meet_the_filter_spec(D):
    h = wb.default_taps(D, 16)
    fs = D * 12000
    assert len(h) == 16 * D
    assert abs(h.sum() - 1.0) < 1e-12                      # unit DC gain
    assert np.allclose(h, h[::-1], atol=1e-15)             # linear phase
    passband = _response_db(h, fs, np.linspace(0, 4000, 81))
    assert passband.max() - passband.min() <= 0.1
    stop = _response_db(h, fs, np.linspace(8000, fs / 2, 4000))
    assert stop.max() <= -60.0


def test_default_taps_refuse_out_of_range():
    with pytest.raises(ValueError):
        wb.default_taps(1, 16)
    with pytest.raises(ValueError):
        wb.default_taps(160, 65)


def _noise(n, rng, scale=0.3):
    return scale * (rng.normal(size=n) + 1j * rng.normal(size=n))


@pytest.mark.parametrize("D", [2, 40, 80])
def test_model_equals_naive_mix_filter_decimate(D):
    rng = np.random.default_rng(D)
    rate = D * 12000
    lim = rate // 2 - 6000
    offsets = [0, -lim, lim, 5999, -12345 % lim, 3 * 12000 // 2 + 7] if lim > 0 else [0]
    offsets = [o for o in offsets if abs(o) <= lim]
    x = _noise(600 * D, rng)
    ch = wb.Channeliser(rate, offsets, K=16)
    y = ch.filter(x)
    for c, f in enumerate(offsets):
        ref = wb.naive_channel(x, rate, f, ch.taps)
        assert np.max(np.abs(y[c] - ref)) < 1e-9


@pytest.mark.parametrize("D", [40, 160])
def test_hop_by_hop_equals_whole_stream(D):
    rng = np.random.default_rng(100 + D)
    rate = D * 12000
    lim = rate // 2 - 6000
    offsets = [0, 5999, -5999, -lim, lim, 1234, -77777 % lim]
    x = _noise((wb.FIRST_OUT + 5 * wb.HOP_OUT) * D, rng, 0.02)
    whole = wb.Channeliser(rate, offsets)
    y_all = whole.filter(x)
    q_all, clip_all = wb.quantise(y_all, whole.gain)
    hop = wb.Channeliser(rate, offsets)
    pos, got, clips = 0, [], 0
    for i, n in enumerate([wb.FIRST_OUT * D] + [wb.HOP_OUT * D] * 5):
        q, cl = hop.push(x[pos:pos + n], first=(i == 0))
        got.append(q)
        clips += cl
        pos += n
    got = np.concatenate(got, axis=1)
    assert got.shape == (len(offsets), wb.FIRST_OUT + 5 * wb.HOP_OUT, 2)
    assert np.array_equal(got, q_all)
    assert clips == clip_all
    assert hop.m == wb.FIRST_OUT + 5 * wb.HOP_OUT
    # a first push restarts the stream: zero history and m = 0
    q0, _ = hop.push(x[:wb.FIRST_OUT * D], first=True)
    assert np.array_equal(q0, q_all[:, :wb.FIRST_OUT])


def test_output_phase_is_exact_for_large_m():
    # (f_c m) mod 12000 in integers: hours into a stream the rotation is still the exact root of unity
    m = np.array([0, 12000, 12000 * 10 ** 8, 12000 * 10 ** 8 + 1], dtype=np.int64)
    r = wb.output_rotation([5999], m)[0]
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == 1.0
    assert abs(r[3] - np.exp(-2j * np.pi * 5999 / 12000)) < 1e-15


@pytest.mark.parametrize("fmt", wb.FORMATS)
def test_formats_round_trip(fmt):
    rng = np.random.default_rng(7)
    x = _noise(1000, rng, 0.2)
    raw = wb.write_samples(x, fmt)
    y = wb.read_samples(raw.tobytes(), fmt)
    step = 1 / 128 if fmt != "cs16" else 1 / 32768
    assert np.max(np.abs(y.real - x.real)) <= step / 2 + 1e-12
    assert np.max(np.abs(y.imag - x.imag)) <= step / 2 + 1e-12
    if fmt == "cu8":
        assert wb.read_samples(bytes([0, 255]), fmt)[0] == complex(-127.5 / 128, 127.5 / 128)


def test_synth_wideband_puts_the_ping_in_its_channel():
    from msk144cudecoder_amd import synth
    rng = np.random.default_rng(3)
    D = 40
    msg = synth.random_message(rng)
    raw = wb.synth_wideband(5184, D * 12000, [(30000, synth.Ping(msg, 100, 4, 500.0, 20.0))], 0.01, rng, "cs16")
    assert raw.dtype == np.int16 and len(raw) == 2 * 5184 * D
    x = wb.read_samples(raw, "cs16")
    ch = wb.Channeliser(D * 12000, [30000, -30000, 30000 - 12000])
    p = np.mean(np.abs(ch.filter(x)) ** 2, axis=1)
    assert p[0] > 5 * p[1] and p[0] > 5 * p[2]          # 20 dB in 2500 Hz for two thirds of the window
