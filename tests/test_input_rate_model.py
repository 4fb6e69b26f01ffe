"""The input-rate contract on the CPU (include/msk144hip.h, "Audio input at 24 to 192 kHz"): input_rate.Resampler against a direct
evaluation of the formula, the host library's C++ against Resampler, the default taps, their response, the headroom rule and every
refusal of check_config."""
import numpy as np
import pytest

from msk144cudecoder_amd import input_rate as ir
from msk144cudecoder_amd.wideband import default_taps_for_rate, rate_ratio

RATES = (24000, 32000, 44000, 48000, 96000, 96125, 192000)


def direct(x, h, P, Q, s, M):
    """y[0..M) of one stream from its whole input x, by the contract's formula in Python integers / int64; x[n < 0] = 0."""
    L = len(h)
    x = [int(v) for v in x]
    h = [int(v) for v in h]
    y = np.zeros(M, dtype=np.int64)
    clamped = 0
    for m in range(M):
        n, r = divmod(m * P, Q)
        acc, k = 0, 0
        while r + k * Q < L:
            if 0 <= n - k:
                acc += h[r + k * Q] * x[n - k]
            k += 1
        assert abs(acc) <= 2**31 - 32768
        v = (acc + (1 << (s - 1))) >> s
        if v > 32767 or v < -32768:
            clamped += 1
        y[m] = min(max(v, -32768), 32767)
    return y, clamped


def cut(x, row, hops):
    """The stream as a first hop and `hops - 1` later ones."""
    return [x[:2 * row]] + [x[(k + 1) * row:(k + 2) * row] for k in range(1, hops)]


@pytest.mark.parametrize("rate,K,shift", [(24000, 1, 14), (32000, 3, 14), (44000, 16, 14), (48000, 16, 14), (96125, 2, 14), (96125, 16, 13), (192000, 5, 14)])
def test_resampler_equals_the_formula_and_the_host_library(rate, K, shift):
    P, Q = rate_ratio(rate)
    h = ir.default_taps(rate, K)
    row = ir.row_samples(rate)
    assert row * Q == 2592 * P
    rng = np.random.default_rng(rate + K)
    hops = 3
    x = rng.integers(-32768, 32768, size=(hops + 1) * row).astype(np.int16)
    M = 2592 * (hops + 1)
    want, want_clamped = direct(x, h, P, Q, shift, M)

    model = ir.Resampler(2, rate, h, shift)
    host = ir.HostResampler(2, rate, h, shift)
    got, got_clamped, got_host, host_clamped = [], 0, [], 0
    for k, part in enumerate(cut(x, row, hops)):
        y, c = model.push([part], [1], [1 if k == 0 else 0])
        assert y[0].dtype == np.int16 and len(y[0]) == (5184 if k == 0 else 2592)
        got.append(y[0])
        got_clamped += int(c[0])
        yh, ch = host.push_one(1, part, k == 0)
        got_host.append(yh)
        host_clamped += ch
    assert np.array_equal(np.concatenate(got).astype(np.int64), want)
    assert got_clamped == want_clamped
    assert np.array_equal(np.concatenate(got_host), np.concatenate(got)) and host_clamped == got_clamped
    host.close()


def test_streams_are_independent_and_a_restart_starts_from_zero_history():
    rate = 32000
    row = ir.row_samples(rate)
    rng = np.random.default_rng(5)
    a = rng.integers(-20000, 20000, size=4 * row).astype(np.int16)
    b = rng.integers(-20000, 20000, size=4 * row).astype(np.int16)
    alone = ir.Resampler(1, rate)
    ya = [alone.push([p], [0], [k == 0])[0][0] for k, p in enumerate(cut(a, row, 3))]
    both = ir.Resampler(3, rate)
    pa, pb = cut(a, row, 3), cut(b, row, 3)
    y0, _ = both.push([pa[0], pb[0]], [0, 2], [1, 1])
    assert np.array_equal(y0[0], ya[0])
    y1, _ = both.push([pb[1]], [2], [0])          # stream 0 sits this one out and keeps its history
    y2, _ = both.push([pa[1], pb[2]], [0, 2], [0, 0])
    assert np.array_equal(y2[0], ya[1])
    y3, _ = both.push([pa[0]], [0], [1])          # restarted: the first hop again, whatever the history held
    assert np.array_equal(y3[0], ya[0])
    with pytest.raises(RuntimeError):
        both.push([pa[1]], [1], [0])              # stream 1 never had a first hop
    with pytest.raises(ValueError):
        both.push([pa[1], pa[1]], [2, 0], [0, 0])


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("K", [4, 16, 64])
def test_default_taps_are_the_rounded_design_with_headroom(rate, K):
    P, Q = rate_ratio(rate)
    d = default_taps_for_rate(rate, K)
    h = ir.default_taps(rate, K)
    assert h.dtype == np.int16 and len(h) == K * P
    assert np.array_equal(h.astype(np.int64), np.rint(d * 2.0**14).astype(np.int64))
    worst = max(int(np.abs(h[r::Q].astype(np.int64)).sum()) for r in range(Q))
    assert worst <= 38342                         # the worst branch sum of these designs; the rule allows 65535
    assert ir.check_config(rate, h) == ""


def response_db(h, fs_up, f):
    k = np.arange(len(h))
    return 20 * np.log10(np.maximum(np.abs(np.exp(-2j * np.pi * np.outer(f, k) / fs_up) @ h), 1e-300))


@pytest.mark.parametrize("rate", RATES)
def test_integer_taps_keep_the_design_pass_and_stop_band(rate):
    P, Q = rate_ratio(rate)
    fs_up = 12000.0 * P
    d = default_taps_for_rate(rate, 16) / Q
    h = ir.default_taps(rate, 16).astype(np.float64) / 2.0**14 / Q
    f_pass = np.linspace(0.0, 4000.0, 161)
    f_stop = np.linspace(8000.0, fs_up / 2, 2000)
    for taps in (d, h):
        assert np.max(np.abs(response_db(taps, fs_up, f_pass))) <= 0.1
        assert np.max(response_db(taps, fs_up, f_stop)) <= -60.0


def test_headroom_rule_at_the_edge():
    # 24000 Hz: P = 2, Q = 1, one branch.  Two taps 32767 + 32767 = 65534 and three taps + 1 = 65535 pass, one more does not
    assert ir.check_config(24000, np.array([32767, 32767], dtype=np.int16), 15) == ""
    assert ir.check_config(24000, np.array([32767, 32767, 1, 0], dtype=np.int16), 15) == ""
    assert "65536" in ir.check_config(24000, np.array([32767, 32767, 1, 1], dtype=np.int16), 15)
    assert "sum" in ir.check_config(24000, np.array([32767, -32768, 1, 0], dtype=np.int16), 15)
    # 32000 Hz: P = 8, Q = 3: branches h[r], h[r + 3], h[r + 6].  Branch 1 = taps 1, 4, 7
    t = np.zeros(8, dtype=np.int16)
    t[[1, 4, 7]] = (32767, -32767, 1)
    assert ir.check_config(32000, t, 15) == ""
    t[7] = 2
    assert "branch 1" in ir.check_config(32000, t, 15)
    # at the edge the accumulator of the worst input stays inside 32 bits, and the model agrees with the formula
    edge = np.array([32767, 32767, 1, 0], dtype=np.int16)
    x = np.full(2 * ir.row_samples(24000), -32768, dtype=np.int16)
    y, c = ir.Resampler(1, 24000, edge, 15).push([x], [0], [1])
    want, wc = direct(x, edge, 2, 1, 15, 5184)
    assert np.array_equal(y[0].astype(np.int64), want) and int(c[0]) == wc and wc > 0


@pytest.mark.parametrize("rate,why", [(12000, "12000"), (44100, "multiple of 125"), (22050, "outside"), (23875, "outside"), (192125, "outside"), (384000, "outside"),
                                      (0, "outside"), (-48000, "outside")])
def test_check_config_refuses_the_rates(rate, why):
    assert why in ir.check_config(rate, np.ones(64, dtype=np.int16))
    with pytest.raises(ValueError):
        ir.default_taps(rate, 16)


def test_check_config_refuses_taps_and_shifts():
    h = ir.default_taps(48000, 16)
    assert ir.check_config(48000, h, 14) == ""
    assert ir.check_config(48000, h, 1) == "" and ir.check_config(48000, h, 15) == ""
    assert "shift" in ir.check_config(48000, h, 0) and "shift" in ir.check_config(48000, h, 16)
    assert "K x P" in ir.check_config(48000, h[:-1])             # L not a multiple of P
    assert "K x P" in ir.check_config(48000, np.zeros(65 * 4, dtype=np.int16))   # K = 65
    assert ir.check_config(48000, np.zeros(64 * 4, dtype=np.int16)) == ""
    assert "K x P" in ir.check_config(96125, np.zeros(768, dtype=np.int16))      # P = 769
    assert "int16" in ir.check_config(48000, np.array([40000, 0, 0, 0]))
    assert "int16" in ir.check_config(48000, np.array([0.5, 0, 0, 0]))
    assert "int16" in ir.check_config(48000, np.zeros(0, dtype=np.int16))
    with pytest.raises(ValueError):
        ir.default_taps(48000, 0)
    with pytest.raises(ValueError):
        ir.default_taps(48000, 65)
    with pytest.raises(ValueError):
        ir.Resampler(1, 48000, h, 16)
