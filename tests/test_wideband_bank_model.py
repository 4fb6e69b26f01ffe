"""The two-stage wideband bank on the CPU: the float64 model (msk144cudecoder_amd/wideband.py AnalysisBank, TwoStage) against a
direct evaluation of the contract's two formulas, the default bank filter's specification, the composite channel, the band rule at
its edges, and the two-stage near-tie rule (tests/wideband_bank_check.py) against deliberate slips in the very configuration the
GPU test runs."""
import numpy as np
import pytest

import wideband_bank_check as bc
import wideband_check as wc
from msk144cudecoder_amd import wideband as wb

BANK_RATES = [6152000, 8000000, 10000000, 20000000, 61440000]


def _naive_stage1(x, h1, k, n):
    """s_k[n] = (-1)^{kn} sum_l h1[l] e^{+j2pi (k l mod 64)/64} x[32n - l], x[< 0] = 0, straight from the contract."""
    out = []
    for nn in n:
        acc = 0j
        for l in range(len(h1)):
            i = 32 * nn - l
            if i >= 0:
                acc += h1[l] * np.exp(2j * np.pi * ((k * l) % 64) / 64) * x[i]
        out.append((-1) ** ((k * nn) % 2) * acc)
    return np.array(out)


def _naive_stage2(s, rate2, d, h, m):
    """The single-stage contract at rate2 = 12000 P/Q on the stream s at offset d, output m (rational form; Q = 1 included)."""
    P, Q = wb.rate_ratio(rate2)
    n_m, r = (m * P) // Q, (m * P) % Q
    acc = 0j
    for k in range((len(h) - r + Q - 1) // Q):
        if n_m - k >= 0:
            acc += h[r + k * Q] * np.exp(2j * np.pi * ((d * k) % rate2) / rate2) * s[n_m - k]
    return np.exp(-2j * np.pi * ((d * n_m) % rate2) / rate2) * acc


def test_two_stage_model_matches_direct_evaluation():
    rate = 8000000
    rng = np.random.default_rng(8)
    h1 = rng.normal(size=512) / np.sqrt(512)
    P2, Q2 = wb.rate_ratio(rate // 32)
    h2 = rng.normal(size=2 * P2) / np.sqrt(2 * P2)
    offsets = np.array([0, rate // 2 - 6000, -(rate // 2 - 6000), rate // 128, rate // 128 - 1, -987654], dtype=np.int64)
    n_in = (wb.FIRST_OUT + wb.HOP_OUT) * rate // 12000
    x = rng.normal(size=n_in) + 1j * rng.normal(size=n_in)
    model = wb.TwoStage(rate, offsets, taps=h2, K=2, bank_taps=h1)
    n1 = wb.FIRST_OUT * rate // 12000
    y = np.concatenate([model.filter(x[:n1]), model.filter(x[n1:])], axis=1)
    k = wb.bank_band(rate, offsets)
    d = wb.bank_residual(rate, offsets)
    for c in range(len(offsets)):
        for m in (0, 7, wb.FIRST_OUT - 1, wb.FIRST_OUT, wb.FIRST_OUT + 1234):
            n_m = (m * P2) // Q2
            lo = max(0, n_m - len(h2) // Q2 - 1)
            s = np.zeros(n_m + 1, dtype=np.complex128)
            s[lo:] = _naive_stage1(x, h1, int(k[c]), range(lo, n_m + 1))
            want = _naive_stage2(s, rate // 32, int(d[c]), h2, m)
            assert abs(y[c, m] - want) < 1e-9 * max(1.0, abs(want)), (c, m)


def _response_db(h, f, fs):
    return 20 * np.log10(np.abs(np.exp(-2j * np.pi * np.outer(f / fs, np.arange(len(h)))) @ h))


@pytest.mark.parametrize("rate", BANK_RATES)
def test_default_bank_meets_its_specification(rate):
    h1 = wb.default_bank_taps(rate)
    assert len(h1) == 512 and abs(h1.sum() - 1.0) < 1e-12 and np.allclose(h1, h1[::-1])
    fp, fs = rate / 128 + 4000, 3 * rate / 128 - 8000
    ripple = _response_db(h1, np.linspace(-fp, fp, 801), rate)
    assert np.abs(ripple).max() <= 0.1
    stop = _response_db(h1, np.concatenate([np.linspace(fs, rate / 2, 4000), -np.linspace(fs, rate / 2, 4000)]), rate)
    assert stop.max() <= -60.0


def _dense_response(h, rate, nfft=1 << 20):
    """|H| on nfft points over one period [0, rate) and a lookup at any frequency in Hz (nearest bin)."""
    H = np.abs(np.fft.fft(h, nfft))
    return lambda f: H[np.rint(np.mod(f, rate) / rate * nfft).astype(np.int64) % nfft]


@pytest.mark.parametrize("rate", BANK_RATES)
def test_composite_channel_is_flat_to_4_khz_and_60_db_down_from_8_khz(rate):
    """A tone at f reaches channel f_c as |H1(f - k_c Fs/64)| x sum_j |H2(f - f_c + j Fs/32)| / Q2 (stage 2 sees it at f - k_c Fs/64
    at rate Fs/32, images Fs/32 apart after its upsampling by Q2): flat within 0.1 dB for |f - f_c| <= 4 kHz, <= -60 dB for
    |f - f_c| >= 8 kHz anywhere in the wideband, the aliases of the decimation by 32 included."""
    rate2 = rate // 32
    P2, Q2 = wb.rate_ratio(rate2)
    H1 = _dense_response(wb.default_bank_taps(rate), rate)
    H2 = _dense_response(wb.default_taps_for_rate(rate2) if Q2 > 1 else wb.default_taps(P2), 12000 * P2)
    lim = rate // 2 - 6000
    step = rate // 128
    for fc in (0, lim, -lim, step, step - 1, -step, 5 * step - 1, 1234567 % lim):
        k = int(wb.bank_band(rate, [fc])[0])
        nu = np.concatenate([np.linspace(-4000, 4000, 161), np.linspace(-rate / 2, rate / 2, 40001)])
        nu = np.concatenate([nu] + [j * rate2 + np.linspace(-8000, 8000, 161) for j in range(-32, 33) if j])
        nu = np.mod(nu + rate / 2, rate) - rate / 2          # a tone's distance from f_c, as the input sampled at Fs sees it
        f = fc + nu
        comp = H1(f - k * (rate // 64)) * sum(H2(nu + j * rate2) for j in range(Q2)) / Q2
        db = 20 * np.log10(np.maximum(comp, 1e-300))
        assert np.abs(db[np.abs(nu) <= 4000]).max() <= 0.1, fc
        assert db[np.abs(nu) >= 8000].max() <= -60.0, fc


@pytest.mark.parametrize("rate", BANK_RATES)
def test_band_assignment_at_its_edges(rate):
    lim = rate // 2 - 6000
    half = rate // 128            # band k covers (2k-1) Fs/128 <= f < (2k+1) Fs/128
    assert wb.bank_band(rate, [lim])[0] == 32 and wb.bank_band(rate, [-lim])[0] == -32
    for k in (-31, -2, -1, 0, 1, 31):
        edge = -(-(2 * k + 1) * rate // 128)      # the first integer at or above (2k+1) Fs/128
        assert list(wb.bank_band(rate, [edge - 1, edge, edge + 1])) == [k, k + 1, k + 1]
    f = np.random.default_rng(rate).integers(-lim, lim + 1, size=2000)
    f = np.concatenate([f, [0, lim, -lim, half, -half, half - 1, -half - 1]])
    k = wb.bank_band(rate, f)
    d = wb.bank_residual(rate, f)
    assert k.min() >= -32 and k.max() <= 32
    assert np.all(np.abs(d) <= rate // 128) and np.all(d + k * (rate // 64) == f)
    assert rate // 128 < rate // 64 - 6000
    # the library's rule (csrc/wideband.h, through libmsk144host.so) is the same
    lib = wb._host_lib()
    import ctypes as C
    lib.msk144host_wideband_band.argtypes = [C.c_int64, C.c_int64]
    lib.msk144host_wideband_band.restype = C.c_int
    assert [lib.msk144host_wideband_band(rate, int(v)) for v in f] == [int(v) for v in k]


def test_band_32_is_band_minus_32():
    rate = 10000000
    x = np.random.default_rng(3).normal(size=4096 * 32) * (1 + 1j)
    h1 = wb.default_bank_taps(rate)
    a = wb.AnalysisBank(h1, [32]).push(x)
    b = wb.AnalysisBank(h1, [-32]).push(x)
    assert np.array_equal(a, b)
    lim = rate // 2 - 6000
    assert wb.TwoStage(rate, [lim, -lim], K=4).bands == [32]      # one stream for both edges


def test_new_rates_pass_the_rules_and_old_refusals_stay():
    for rate in (6152000, 8000000, 10000000, 20000000, 61440000):
        assert wb.check_config(rate, "cu8", 16, 100.0, [0, rate // 2 - 6000, -(rate // 2 - 6000)]) == ""
        assert wb.check_config(rate, "cu8", 16, 100.0, [rate // 2 - 5999]) != ""
    for rate in (6156000, 6144125, 12500000, 61448000, 64000000):
        assert "2 <= D <= 512" in wb.check_config(rate, "cu8", 16, 100.0, [0])
    for rate in (6152001, 10000001):
        assert "multiple of 125" in wb.check_config(rate, "cu8", 16, 100.0, [0])


# ---- the two-stage near-tie rule ----

def _run(model_or_ref, raw, rate, fmt, n_pushes):
    out = []
    for i, part in enumerate(wc.split_pushes(raw, rate, n_pushes)):
        out.append(model_or_ref.push(wb.read_samples(part, fmt), first=i == 0))
    return out


@pytest.fixture(scope="module")
def gpu_case():
    """The 10 Msps configuration of test_gpu_wideband_bank.py::test_hops_match_the_two_stage_model: reference outputs and tolerances."""
    rate, fmt, n = bc.CASES[1]
    offsets, taps, bank_taps, gain, raw = bc.case(rate, fmt, n)
    ref = bc.BankReference(rate, offsets, taps=taps, K=bc.K2, gain=gain, bank_taps=bank_taps)
    return dict(rate=rate, fmt=fmt, n=n, offsets=offsets, taps=taps, bank_taps=bank_taps, gain=gain, raw=raw, ref=_run(ref, raw, rate, fmt, n))


def test_the_model_passes_its_own_rule(gpu_case):
    for y, d in gpu_case["ref"]:
        q, clip = wb.quantise(y, wc.f32(gpu_case["gain"]))
        rep = wc.check_hops(q, y, d, gpu_case["gain"], clip)
        assert rep["ok"]
        assert rep["max_delta_lsb"] < 0.5 and rep["near_ties"] < 0.5 * rep["components"]


@pytest.mark.parametrize("kind", bc.SLIPS)
def test_slips_fail_the_rule(gpu_case, kind):
    g = gpu_case
    m = bc.slipped_model(kind, g["rate"], g["offsets"], g["taps"], bc.K2, wc.f32(g["gain"]), g["bank_taps"])
    bad = 0
    for i, ((y, d), part) in enumerate(zip(g["ref"], wc.split_pushes(g["raw"], g["rate"], g["n"]))):
        q, clip = m.push(wb.read_samples(part, g["fmt"]), first=i == 0)
        bad += wc.check_hops(q, y, d, g["gain"], clip)["mismatches"]
    assert bad > 0, kind
