"""-m gpu: the wideband channeliser (csrc/channelise.hip) at its shape, tap and quantiser edges, against references that do not
share the float64 model's blind spots (tests/wideband_check.py):

1. Impulses: taps e_j, offset 0, cs8, gain 1 - every output equals an input component or 0, exactly (closed forms, no model).
2. Random non-symmetric taps over the (D, K) and (rate, K) grid, the near-tie rule, three pushes.
3. Channel tiling: C = 1, 31, 129, 257 with random taps; C = 1024 with the default taps (sampled channels).
4. The quantiser: ties to even, full scale per format, exact per-push clip counts, a tiny gain, the top of the gain range.
5. The stream: a first push after later ones restarts it; 130 pushes across the output rotation's 125-push period.
The CPU side (test_wideband_edges_model.py) checks that each reference fails for the indexing slips these tests are meant to see.
"""
import numpy as np
import pytest

import wideband_check as wc
from msk144cudecoder_amd import wideband as wb
from wideband_gpu import DECODE_CFG, check_stream, dump_hops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def d33(hip):
    with hip.HipDecoder(channels=33, **DECODE_CFG) as d:
        yield d


def _check_stream(d, rate, offsets, fmt, taps, K, gain, parts, firsts, tally, sample=None, what=""):
    """Configure d, push parts (firsts[i]: a first push) and hold every push to the near-tie rule on the channels in sample."""
    ref = wc.Reference(rate, offsets if sample is None else np.asarray(offsets)[sample], taps=taps, K=K, gain=gain)
    d.set_wideband(rate, offsets, fmt, taps=taps, taps_per_phase=K, gain=gain)
    check_stream(d, ref, fmt, parts, firsts, what, tally, sample)


# ---- 1. impulses ----

@pytest.mark.parametrize("rate, K, j", wc.impulse_cases())
def test_impulse_is_exact(d33, rate, K, j):
    P, Q = wb.rate_ratio(rate)
    raw = wc.random_cs8(rate, wc.IMPULSE_PUSHES, np.random.default_rng([rate, j]))
    d33.set_wideband(rate, np.zeros(33, dtype=np.int32), "cs8", taps=wc.unit_taps(K * P, j), taps_per_phase=K, gain=1.0)
    for i, part in enumerate(wc.split_pushes(raw, rate, wc.IMPULSE_PUSHES)):
        d33.push_wideband(i % 2, part, first=i == 0)
        got = dump_hops(d33, range(33))
        want = wc.impulse_expected(raw, rate, j, wc.push_m0(i), got.shape[1])
        for c in range(33):
            bad = np.count_nonzero(np.any(got[c] != want, axis=1))
            assert bad == 0, f"rate {rate} K {K} tap {j} push {i} channel {c}: {bad} of {len(want)} samples differ"
        assert d33.wideband_clip_count() == 0


@pytest.mark.parametrize("rate, K, j", [(80 * 12000, 3, 80), (2048000, 16, 3 * (171 + 4 * 512))])
def test_impulse_with_offsets(d33, parity_report, rate, K, j):
    P, Q = wb.rate_ratio(rate)
    rng = np.random.default_rng([rate, j, 1])
    raw = wc.random_cs8(rate, wc.IMPULSE_PUSHES, rng)
    tally = wc.Tally()
    _check_stream(d33, rate, wc.offsets_for(rate, 33, rng), "cs8", wc.unit_taps(K * P, j), K, 1.0, wc.split_pushes(raw, rate, wc.IMPULSE_PUSHES),
                  [True, False, False], tally, what=f"impulse {rate} tap {j}")
    parity_report(f"wideband_impulse_offsets_{rate}_K{K}_j{j}", tally.report())


# ---- 2. random taps over the shape grid ----

@pytest.mark.parametrize("rate, K, fmt", wc.INT_GRID + wc.RAT_GRID)
def test_random_taps_grid(d33, parity_report, rate, K, fmt):
    offsets, taps, gain, raw = wc.grid_case(rate, K, fmt)
    tally = wc.Tally()
    _check_stream(d33, rate, offsets, fmt, taps, K, gain, wc.split_pushes(raw, rate, wc.GRID_PUSHES), [True, False, False], tally,
                  what=f"{rate} K {K} {fmt}")
    parity_report(f"wideband_grid_{rate}_K{K}_{fmt}", tally.report())


# ---- 3. channel tiling ----

TILING = [(rate, C) for rate in (80 * 12000, 2048000) for C in (1, 31, 129, 257)]


@pytest.mark.parametrize("rate, C", TILING)
def test_channel_tiling_random_taps(hip, parity_report, rate, C):
    fmt = "cs16"
    offsets, taps, gain, raw = wc.grid_case(rate, 16, fmt, C=C)
    tally = wc.Tally()
    with hip.HipDecoder(channels=C, **DECODE_CFG) as d:
        _check_stream(d, rate, offsets, fmt, taps, 16, gain, wc.split_pushes(raw, rate, wc.GRID_PUSHES), [True, False, False], tally,
                      what=f"{rate} C {C}")
    parity_report(f"wideband_tiling_{rate}_C{C}", tally.report())


@pytest.mark.parametrize("rate", [160 * 12000, 2048000])
def test_1024_channels_default_taps(hip, parity_report, rate):
    """The configuration tools/wideband_bench.py times: 1024 offsets evenly over +-(Fs/2 - 6000), cu8, K = 16, default taps and
    gain.  The model runs on the channels at every 32- and 128-boundary and 32 more."""
    C = 1024
    rng = np.random.default_rng(rate)
    lim = rate // 2 - 6000
    offsets = np.linspace(-lim, lim, C).astype(np.int32)
    raw = wc.raw_input(rate, wc.GRID_PUSHES, "cu8", rng, 0.03 * np.sqrt(rate / 1920000))
    sample = wc.sample_channels(C, rng)
    tally = wc.Tally()
    with hip.HipDecoder(channels=C, **DECODE_CFG) as d:
        _check_stream(d, rate, offsets, "cu8", None, 16, 100.0, wc.split_pushes(raw, rate, wc.GRID_PUSHES), [True, False, False], tally,
                      sample=sample, what=f"{rate} C 1024")
    parity_report(f"wideband_1024_channels_{rate}", dict(tally.report(), sampled_channels=len(sample)))


# ---- 4. the quantiser ----

QRATE = 80 * 12000


def _impulse_pushes(d, fmt, raw, gain, n_pushes=3):
    """Taps e_0 at D = 80, K = 1, 33 channels at offset 0: output m of every channel is 128 gain x (input sample 80 m), exactly."""
    d.set_wideband(QRATE, np.zeros(33, dtype=np.int32), fmt, taps=wc.unit_taps(80, 0), taps_per_phase=1, gain=gain)
    for i, part in enumerate(wc.split_pushes(raw, QRATE, n_pushes)):
        d.push_wideband(i % 2, part, first=i == 0)
        M = wb.FIRST_OUT if i == 0 else wb.HOP_OUT
        m = wc.push_m0(i) + np.arange(M)
        comp = np.asarray(raw).reshape(-1, 2)[80 * m].astype(np.float64)
        yield i, dump_hops(d, range(33)), comp, d.wideband_clip_count()


def _want(v):
    r = np.rint(v)                                   # half to even, as rintf
    return np.clip(r, -128, 127).astype(np.int8), int(np.count_nonzero((r < -128) | (r > 127)))


def test_rounding_ties_go_to_even(d33):
    raw = wc.random_cs8(QRATE, 3, np.random.default_rng(11))
    for i, got, comp, clip in _impulse_pushes(d33, "cs8", raw, 0.5):
        want, n = _want(comp / 2.0)                        # s / 2: every odd s is a tie
        assert np.count_nonzero(comp % 2) > 1000
        assert np.array_equal(got, np.broadcast_to(want, got.shape)), f"push {i}"
        assert clip == n == 0


def test_cs16_full_scale(d33):
    rng = np.random.default_rng(12)
    raw = rng.choice(np.array([32767, -32768, 32640, -32640, 0, 128, -384, 12345], dtype=np.int16), size=2 * wb.FIRST_OUT * 80 * 2)
    for i, got, comp, clip in _impulse_pushes(d33, "cs16", raw, 1.0):
        want, n = _want(comp / 256.0)      # 32767 -> 127.996 -> 128 and the tie 32640 -> 127.5 -> 128: clipped; -32768 -> -128 exactly
        assert np.array_equal(got, np.broadcast_to(want, got.shape)), f"push {i}"
        assert n == np.count_nonzero((comp == 32767) | (comp == 32640)) > 0
        assert clip == 33 * n, f"push {i}"


def test_cu8_full_scale(d33):
    raw = np.random.default_rng(13).integers(0, 256, size=2 * wb.FIRST_OUT * 80 * 2).astype(np.uint8)
    for i, got, comp, clip in _impulse_pushes(d33, "cu8", raw, 1.0):
        want, n = _want(comp - 127.5)                      # 255 -> 127.5 -> 128, clipped; 0 -> -127.5 -> -128, not clipped
        assert np.array_equal(got, np.broadcast_to(want, got.shape)), f"push {i}"
        assert n == np.count_nonzero(comp == 255) > 0
        assert clip == 33 * n, f"push {i}"


def test_all_saturating_clip_count_per_push(d33):
    rng = np.random.default_rng(14)
    raw = (rng.integers(2, 128, size=2 * wb.FIRST_OUT * 80 * 2) * rng.choice([-1, 1], size=2 * wb.FIRST_OUT * 80 * 2)).astype(np.int8)
    for i, got, comp, clip in _impulse_pushes(d33, "cs8", raw, 100.0):
        want, n = _want(comp * 100.0)                      # |v| >= 200
        assert np.array_equal(got, np.broadcast_to(want, got.shape)), f"push {i}"
        assert n == comp.size
        assert clip == 33 * n, f"push {i}: the count is per push"


def test_tiny_gain_gives_zeros(d33):
    offsets, taps, _, raw = wc.grid_case(QRATE, 16, "cs16")
    d33.set_wideband(QRATE, offsets, "cs16", taps=taps, taps_per_phase=16, gain=1e-30)
    for i, part in enumerate(wc.split_pushes(raw, QRATE, 3)):
        d33.push_wideband(i % 2, part, first=i == 0)
        assert not np.any(dump_hops(d33, range(33))), f"push {i}"
        assert d33.wideband_clip_count() == 0


def test_top_of_range_gain(hip, d33):
    """128 x gain must be finite in f32: at gain 3e38 an exact zero output (digital silence, or the zero history of a first push)
    became rint(inf x 0) = NaN and was stored as -128, uncounted.  The contract now refuses gain > 1e36; at 1e36 a zero stays 0."""
    with pytest.raises(hip.Msk144Error) as e:
        d33.set_wideband(QRATE, np.zeros(33, dtype=np.int32), "cs8", taps=wc.unit_taps(80, 0), taps_per_phase=1, gain=3e38)
    assert e.value.code == -1 and "wideband gain must be a positive finite number no larger than 1e36" in str(e.value)
    raw = np.zeros(2 * wb.FIRST_OUT * 80 * 2, dtype=np.int8)
    raw[1::4] = 1                                          # Q of every other sample: +1/128; everything else silence
    for i, got, comp, clip in _impulse_pushes(d33, "cs8", raw, 1e36, n_pushes=2):
        want, n = _want(comp * 1e36)
        assert np.array_equal(got, np.broadcast_to(want, got.shape)), f"push {i}"
        assert clip == 33 * n


# ---- 5. the stream ----

@pytest.mark.parametrize("rate", [80 * 12000, 2048000])
def test_first_push_restarts_the_stream(d33, parity_report, rate):
    """first, later, later, then first again and later: the second first push ignores the history and restarts m at 0."""
    offsets, taps, gain, raw = wc.grid_case(rate, 16, "cs8", n_pushes=3, seed=1)
    _, _, _, raw2 = wc.grid_case(rate, 16, "cs8", n_pushes=2, seed=2)
    parts = wc.split_pushes(raw, rate, 3) + wc.split_pushes(raw2, rate, 2)
    tally = wc.Tally()
    _check_stream(d33, rate, offsets, "cs8", taps, 16, gain, parts, [True, False, False, True, False], tally, what=f"{rate} restart")
    parity_report(f"wideband_restart_{rate}", tally.report())


@pytest.mark.parametrize("rate, fmt", [(2 * 12000, "cs16"), (30000, "cu8")])
def test_130_pushes(d33, parity_report, rate, fmt):
    """130 pushes cross the output rotation's period - (f_c m) mod 12000 repeats every lcm(2592, 12000) / 2592 = 125 hops - and
    carry the history many times."""
    n = 130
    offsets, taps, gain, raw = wc.grid_case(rate, 16, fmt, n_pushes=n)
    tally = wc.Tally()
    _check_stream(d33, rate, offsets, fmt, taps, 16, gain, wc.split_pushes(raw, rate, n), [True] + [False] * (n - 1), tally, what=f"{rate} stream")
    parity_report(f"wideband_130_pushes_{rate}", tally.report())
