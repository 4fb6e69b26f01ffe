"""The wideband channeliser's references on the CPU (tests/wideband_check.py), before the device is held to them:

1. The float64 model (Channeliser) equals the naive mix -> filter -> decimate with random non-symmetric taps at the shape edges.
2. The impulse closed forms equal the model at every tap position the GPU tests use.
3. Sensitivity: each simulated indexing or format slip fails the near-tie rule in the configuration the matching GPU test runs;
   the slips the old |dq| <= 1 / 99.9 % check could not see still pass that check with the default taps.
4. The contract refuses a gain for which 128 x gain is not finite in f32.
"""
import os
import subprocess

import numpy as np
import pytest

import wideband_check as wc
from msk144cudecoder_amd import wideband as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "msk144cudecoder_amd", "host")


@pytest.fixture(scope="module", autouse=True)
def host_lib():
    subprocess.run(["make", "-s", "-C", HOST, "../libmsk144host.so"], check=True)


def _offsets(rate):
    lim = rate // 2 - 6000
    return [0, lim, -lim, 1234567 % lim, -(7777 % lim) - 1]


# ---- 1. the model against the naive channel ----

@pytest.mark.parametrize("D, K", [(2, 1), (2, 64), (3, 5), (33, 64), (512, 1), (512, 5)])
def test_integer_model_equals_naive_channel_random_taps(D, K):
    rate = D * 12000
    rng = np.random.default_rng([D, K])
    h = wc.random_taps(K * D, rng)
    n_out = 2 * K + 40
    x = 0.1 * (rng.normal(size=n_out * D) + 1j * rng.normal(size=n_out * D))
    offs = _offsets(rate)
    model = wb.Channeliser(rate, offs, taps=h)
    cut = (K + 7) * D                                       # two pushes: the second reads the history
    y = np.concatenate([model.filter(x[:cut]), model.filter(x[cut:])], axis=1)
    for c, f in enumerate(offs):
        ref = wb.naive_channel(x, rate, f, h)
        assert np.max(np.abs(y[c] - ref)) <= 1e-9, (f, np.max(np.abs(y[c] - ref)))


@pytest.mark.parametrize("rate, K, periods", [(30000, 16, 40), (24125, 16, 6), (2048000, 5, 10), (6143875, 1, 1)])
def test_rational_model_equals_naive_resampled_channel_random_taps(rate, K, periods):
    """30000 = 5/2 (fewer phases than one 32-phase chunk), 24125 = 193/96 (the largest Q), 2048000 = 512/3, 6143875 = 49151/96
    (the largest P); short inputs, two pushes of `periods` x P samples each."""
    P, Q = wb.rate_ratio(rate)
    rng = np.random.default_rng([rate, K])
    h = wc.random_taps(K * P, rng)
    n = periods * P
    x = 0.1 * (rng.normal(size=2 * n) + 1j * rng.normal(size=2 * n))
    offs = _offsets(rate)
    model = wb.Channeliser(rate, offs, taps=h)
    y = np.concatenate([model.filter(x[:n]), model.filter(x[n:])], axis=1)
    for c, f in enumerate(offs):
        ref = wb.naive_resampled_channel(x, rate, f, h)
        assert np.max(np.abs(y[c] - ref)) <= 1e-9, (f, np.max(np.abs(y[c] - ref)))


# ---- 2. the impulse closed forms ----

@pytest.mark.parametrize("rate, K, j", wc.impulse_cases())
def test_impulse_closed_form_equals_the_model(rate, K, j):
    P, Q = wb.rate_ratio(rate)
    raw = wc.random_cs8(rate, wc.IMPULSE_PUSHES, np.random.default_rng([rate, j]))
    model = wb.Channeliser(rate, [0], taps=wc.unit_taps(K * P, j), gain=1.0)
    for i, part in enumerate(wc.split_pushes(raw, rate, wc.IMPULSE_PUSHES)):
        q, clipped = model.push(wb.read_samples(part, "cs8"), first=i == 0)
        want = wc.impulse_expected(raw, rate, j, wc.push_m0(i), q.shape[1])
        assert clipped == 0
        assert np.array_equal(q[0], want), (i, int(np.count_nonzero(q[0] != want)))


def test_impulse_taps_cover_the_branch_bookkeeping():
    """At 2.048 Msps (K = 16: K_r = 2731 or 2730, Kq = 6, s_full = 171 or 170) the rational taps include a long and a short phase's
    last tap and phase 32; at 24125 (K_r 32 or 33 over 193 phases) phase 32 of the branches that have it."""
    js = wc.branch_impulse_taps(2048000, 16, [0])
    assert js == sorted({0, 3 * 2730, 3 * 5 * 512, 3 * (170 + 5 * 512), 3 * (171 + 4 * 512), 3 * 32, 3 * (32 + 5 * 512)})
    js = wc.branch_impulse_taps(24125, 16, [0, 1, 47, 95])       # r = mr; branches 0 and 1 have 33 phases of one tap
    assert {0 + 32 * 96, 1 + 32 * 96, 47 + 31 * 96, 95 + 31 * 96} <= set(js)


# ---- 3. sensitivity: each slip fails its configuration's check ----

def _zero(h, idx):
    h = h.copy()
    h[np.asarray(list(idx), dtype=np.int64)] = 0.0
    return h


def _branch_taps(P, Q, L):
    """Per branch residue r: the tap indices j = r + kQ, k < K_r, and the phase of each (k mod P) and its index within the phase."""
    out = []
    for mr in range(Q):
        r = mr * P % Q
        k = np.arange((L - r + Q - 1) // Q)
        out.append((r + k * Q, k % P, k // P))
    return out


def _slipped_taps(slip, h, P, Q):
    L = len(h)
    if slip == "taps_reversed":
        return h[::-1].copy()
    if slip == "tap0_dropped":
        return _zero(h, [0])
    if slip == "tapL1_dropped":
        return _zero(h, [L - 1])
    if slip == "branch_last_dropped":                     # the last tap of every branch: k = K_r - 1
        return _zero(h, [j[-1] for j, _, _ in _branch_taps(P, Q, L)])
    if slip == "phase_last_dropped":                      # q = (taps of the phase) - 1 in every phase of every branch
        idx = []
        for j, p, q in _branch_taps(P, Q, L):
            for pp in np.unique(p):
                idx.append(j[p == pp][-1])
        return _zero(h, idx)
    if slip == "phase_first_dropped":                     # q = 0 in every phase of every branch
        return _zero(h, [jj for j, _, q in _branch_taps(P, Q, L) for jj in j[q == 0]])
    return h


def _slipped_push(slip, rate, offsets, taps, gain, part, fmt, first, state):
    """The int8 hops a device with `slip` would produce for one push (state carries the slipped model between pushes)."""
    P, Q = wb.rate_ratio(rate)
    if "model" not in state:
        m = wb.Channeliser(rate, offsets, taps=_slipped_taps(slip, taps, P, Q), gain=gain)
        if slip == "n0_plus_one":
            m.branches = [(r, n0 + 1, G) for r, n0, G in m.branches]
        state["model"] = m
    m = state["model"]
    x = wb.read_samples(part, fmt)
    if slip == "cu8_centre_127":
        x = x + (0.5 + 0.5j) / 128.0                      # (u - 127)/128 instead of (u - 127.5)/128
    if slip == "iq_swap":
        x = x.imag + 1j * x.real
    if first:
        m.reset()
    m0 = m.m
    y = m.filter(x)
    if slip == "rotation_sign":                           # e^{+j phi} instead of e^{-j phi}: y e^{+2j phi}
        mm = m0 + np.arange(y.shape[1], dtype=np.int64)
        n = (mm * P) // Q
        ph = np.mod(np.mod(np.asarray(offsets, dtype=np.int64), rate)[:, None] * np.mod(n, rate)[None, :], rate) / rate
        y = y * np.exp(4j * np.pi * ph)
    return wb.quantise(y, wc.f32(gain))


# (slip, the GPU test configuration it must fail: (rate, K, format, channels)); the model runs on the first 8 channels of it
INT_CASE = (33 * 12000, 16, "cs8", wc.GRID_CHANNELS)            # INT_GRID
CU8_CASE = (31 * 12000, 7, "cu8", wc.GRID_CHANNELS)             # INT_GRID
RAT_CASE = (2048000, 16, "cs16", 31)                             # the channel tiling test at 2.048 Msps, C = 31
SLIPS = [("taps_reversed", INT_CASE), ("tap0_dropped", INT_CASE), ("tapL1_dropped", INT_CASE), ("phase_last_dropped", INT_CASE),
         ("phase_first_dropped", INT_CASE), ("rotation_sign", INT_CASE), ("iq_swap", INT_CASE), ("cu8_centre_127", CU8_CASE),
         ("taps_reversed", RAT_CASE), ("tap0_dropped", RAT_CASE), ("tapL1_dropped", RAT_CASE), ("branch_last_dropped", RAT_CASE),
         ("phase_last_dropped", RAT_CASE), ("phase_first_dropped", RAT_CASE), ("n0_plus_one", RAT_CASE), ("rotation_sign", RAT_CASE),
         ("iq_swap", RAT_CASE)]


@pytest.mark.parametrize("slip, case", SLIPS, ids=[f"{s}-{c[0]}" for s, c in SLIPS])
def test_slip_fails_the_near_tie_rule(slip, case):
    rate, K, fmt, C = case
    offsets, taps, gain, raw = wc.grid_case(rate, K, fmt, C=C)
    offsets = offsets[:8]
    ref = wc.Reference(rate, offsets, taps=taps, gain=gain)
    state = {}
    parts = wc.split_pushes(raw, rate, wc.GRID_PUSHES)[:2]
    failed = []
    for i, part in enumerate(parts):
        y, d = ref.push(wb.read_samples(part, fmt), first=i == 0)
        ok_rep = wc.check_hops(wb.quantise(y, wc.f32(gain))[0], y, d, gain)
        assert ok_rep["ok"], ok_rep                        # the unslipped model passes its own rule
        q, clip = _slipped_push(slip, rate, offsets, taps, gain, part, fmt, i == 0, state)
        rep = wc.check_hops(q, y, d, gain, clip)
        failed.append(not rep["ok"])
    assert all(failed), f"{slip} passes the near-tie rule on push(es) {[i for i, f in enumerate(failed) if not f]}"


def test_impulse_references_see_the_tap_slips():
    """The exact impulse references fail for the index slips too: e_j read reversed, or with tap j dropped, is another output."""
    for rate, K, j in wc.impulse_cases():
        P, Q = wb.rate_ratio(rate)
        L = K * P
        h = wc.unit_taps(L, j)
        raw = wc.random_cs8(rate, 2, np.random.default_rng([rate, j]))
        part = wc.split_pushes(raw, rate, 2)[0]
        want = wc.impulse_expected(raw, rate, j, 0, wb.FIRST_OUT)
        for slip in ("taps_reversed", "branch_last_dropped", "phase_last_dropped", "phase_first_dropped"):
            hs = _slipped_taps(slip, h, P, Q)
            if np.array_equal(hs, h):
                continue                                   # the slip does not touch tap j
            q, _ = wb.Channeliser(rate, [0], taps=hs, gain=1.0).push(wb.read_samples(part, "cs8"), first=True)
            assert not np.array_equal(q[0], want), (rate, K, j, slip)


OLD_CASES = [("taps_reversed", 960000), ("tap0_dropped", 960000), ("tapL1_dropped", 960000), ("branch_last_dropped", 2048000)]


@pytest.mark.parametrize("slip, rate", OLD_CASES)
def test_slip_passes_the_old_check_with_default_taps(slip, rate):
    """What the suite could not see before: with the default (symmetric, 70 dB edge) taps, 16 channels, cs16 at the old GPU tests'
    level and gain 100, these slips stay within |dq| <= 1 and 99.9 % exact.  The near-tie cases above catch every one of them."""
    P, Q = wb.rate_ratio(rate)
    rng = np.random.default_rng(rate)
    offsets = wc.offsets_for(rate, 16, rng)
    sigma = 0.03 * np.sqrt(rate / 1920000)
    raw = wc.raw_input(rate, 2, "cs16", rng, sigma)
    good = wb.Channeliser(rate, offsets)
    bad = wb.Channeliser(rate, offsets, taps=_slipped_taps(slip, good.taps, P, Q))
    for i, part in enumerate(wc.split_pushes(raw, rate, 2)):
        x = wb.read_samples(part, "cs16")
        assert wc.old_check_passes(bad.push(x, first=i == 0)[0], good.push(x, first=i == 0)[0]), (slip, i)


def test_near_tie_rule_accepts_only_near_ties():
    """The rule itself: an exact tie may round either way; one LSB off elsewhere fails; the clip count may differ only by ties on
    the clip edges."""
    y = np.array([[0.5, 1.25, 127.5, -128.5, 3.0]]) / 128.0 + 0j
    d = wc.delta(np.full(5, 1.0), np.full(5, 16), 1.0)
    q = wb.quantise(y, 1.0)[0]
    assert wc.check_hops(q, y, d, 1.0, 2)["ok"]
    q2 = q.copy()
    q2[0, 0, 0] = 1                                        # the other side of the tie at 0.5
    assert wc.check_hops(q2, y, d, 1.0, 2)["ok"]
    q3 = q.copy()
    q3[0, 1, 0] = 2                                        # 1.25 -> 2: not a tie
    assert not wc.check_hops(q3, y, d, 1.0, 2)["ok"]
    assert wc.check_hops(q, y, d, 1.0, 1)["ok"]         # the model clips 127.5 -> 128, not -128.5 -> -128 (half to even)
    assert wc.check_hops(q, y, d, 1.0, 3)["ok"]         # both are edge ties: 1 +- 2
    assert not wc.check_hops(q, y, d, 1.0, 4)["ok"]
    y4 = np.array([[200.0]]) / 128.0 + 0j
    assert not wc.check_hops(wb.quantise(y4, 1.0)[0], y4, d[:1], 1.0, 0)["ok"]


def test_delta_is_the_documented_bound():
    T, N, g = np.array([2.0]), np.array([100]), 3.0
    assert wc.delta(T, N, g)[0] == 16 * np.sqrt(108.0) * 2.0 ** -24 * 128 * 3.0 * 2.0


# ---- 4. the gain bound ----

def test_gain_bound_is_enforced_by_the_contract():
    ok = wb.check_config(1920000, "cs16", 16, 1e36, [0])
    assert ok == ""
    for g in (3e38, 1.01e36, float("inf"), float("nan"), 0.0, -1.0):
        why = wb.check_config(1920000, "cs16", 16, g, [0])
        assert "wideband gain must be a positive finite number" in why and "1e36" in why, (g, why)
    assert np.isfinite(np.float32(128.0) * np.float32(1e36))
    header = open(os.path.join(ROOT, "include", "msk144hip.h")).read()
    assert "0 < gain <= 1e36" in header
