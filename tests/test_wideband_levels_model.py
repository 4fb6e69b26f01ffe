"""CPU: the stepped AGC rule and the level statistics of the wideband channeliser (include/msk144hip.h), without a device.

1. wideband.Agc (Python integers) equals msk144host_wideband_agc_step - csrc/wideband.h agc_step, the function the device runs -
   over random statistic sequences, the clamps at min_exp and max_exp included.
2. A stationary channel, for a log sweep of powers: the exponent settles within hold x (max_exp - min_exp) pushes and never
   moves again.
3. Every validation rule is refused, by the shared C++ check and by the Python model alike.
4. Model only: the tone scenes (tests/wideband_levels_check.py) through the float64 channeliser and Agc reach the settled state the
   device is held to in test_gpu_wideband_levels.py - every non-silent channel inside the window with nothing clipped, silent
   channels at max_exp with all-zero output - and walk the ladder both ways on the way there.
5. quantise() with per-channel gains and levels() agree with the scalar forms channel by channel.
6. Silence, then the tones, at the rational rate: the model climbs to max_exp on all-zero output, then clips and walks down.
7. The faint decode scene: under the default Agc the model settles before the pings, and the oracle decodes every planted message
   from the model's hops - the scene is chosen here, not by what the device makes of it.
"""
import ctypes as C

import numpy as np
import pytest

import wideband_levels_check as lc
from msk144cudecoder_amd import wideband as wb

DEFAULTS = dict(lo_sq=64, hi_sq=1024, clip_ppm=1000, hold=4, min_exp=-20, max_exp=20)
ORDER = ("lo_sq", "hi_sq", "clip_ppm", "hold", "min_exp", "max_exp")


@pytest.fixture(scope="module")
def host():
    L = wb._host_lib()
    L.msk144host_wideband_agc_step.argtypes = [C.POINTER(C.c_int32), C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_int]
    L.msk144host_wideband_agc_step.restype = C.c_int
    L.msk144host_wideband_gain_ok.argtypes = [C.c_float, C.c_int32]
    L.msk144host_wideband_gain_ok.restype = C.c_int
    L.msk144host_wideband_agc_scale.argtypes = [C.c_float, C.c_int32]
    L.msk144host_wideband_agc_scale.restype = C.c_float
    return L


def c_step(L, p, n, S, k, e, quiet):
    arr = (C.c_int32 * 6)(*[p[name] for name in ORDER])
    ce, cq = C.c_int32(e), C.c_int32(quiet)
    why = C.create_string_buffer(256)
    rc = L.msk144host_wideband_agc_step(arr, n, S, k, C.byref(ce), C.byref(cq), why, len(why))
    return rc, ce.value, cq.value, why.value.decode()


def one_record(n, S, k):
    lv = np.zeros(1, dtype=wb.LEVEL_DTYPE)
    lv["samples"], lv["sum_sq"], lv["clipped"] = n, S, k
    return lv


def test_defaults_are_the_contracts():
    assert wb.AGC_DEFAULTS == DEFAULTS
    from msk144cudecoder_amd import hipdecoder
    assert hipdecoder.AGC_DEFAULTS == DEFAULTS
    assert C.sizeof(hipdecoder.WidebandAgc) == 24 and hipdecoder.LEVEL_DTYPE.itemsize == 32


@pytest.mark.parametrize("params", [DEFAULTS, dict(DEFAULTS, hold=1, min_exp=-2, max_exp=3), dict(lo_sq=0, hi_sq=1, clip_ppm=0, hold=2, min_exp=0, max_exp=0),
                                    dict(DEFAULTS, min_exp=1, max_exp=5), lc.AGC])
def test_python_rule_equals_the_shared_one(host, params):
    rng = np.random.default_rng([abs(v) for v in params.values()])
    a = wb.Agc(1, 1.0, **params)
    e = quiet = 0
    seen = set()
    for i in range(4000):
        n = 5184 if i % 50 == 0 else 2592
        mode = rng.integers(0, 4)                                    # long quiet and loud runs reach both clamps
        lo, hi = params["lo_sq"] * 2 * n, params["hi_sq"] * 2 * n
        S = int({0: rng.integers(0, lo + 1), 1: rng.integers(hi, 2 * hi + 2), 2: rng.integers(lo, hi + 1), 3: rng.choice([lo - 1, lo, hi, hi + 1])}[int(mode)])
        S = max(S, 0)
        if i % 400 < 200:
            S = 0
        elif i % 400 < 260:
            S = 2 * n * 128 * 128
        k = int(rng.choice([0, 0, 0, params["clip_ppm"] * 2 * n // 1000000, params["clip_ppm"] * 2 * n // 1000000 + 1, 2 * n]))
        if i % 400 < 260:
            k = 0
        rc, e, quiet, _ = c_step(host, params, n, S, k, e, quiet)
        assert rc == 0
        a.step(one_record(n, S, k))
        assert (a.e[0], a.quiet[0]) == (e, quiet), f"step {i}: n {n} S {S} k {k}"
        seen.add(e)
    assert params["min_exp"] in seen and params["max_exp"] in seen, "the sequence never reached a clamp"
    assert float(a.gains()[0]) == host.msk144host_wideband_agc_scale(1.0, a.e[0]) / 128.0


@pytest.mark.parametrize("params", [DEFAULTS, dict(DEFAULTS, hold=1), dict(DEFAULTS, lo_sq=100, hi_sq=401)])
def test_a_stationary_channel_settles_and_stays(params):
    """A channel of mean-square power p per component at exponent 0 has 4^e p at exponent e, until the int8 range ends: above
    127.5 rms everything clips.  One step multiplies the power by 4 < hi_sq / lo_sq, so the rule cannot cycle."""
    n = 2592
    limit = params["hold"] * (params["max_exp"] - params["min_exp"])
    powers = 10.0 ** np.linspace(-14, 14, 113)
    a = wb.Agc(len(powers), 1.0, **params)
    lv = np.zeros(len(powers), dtype=wb.LEVEL_DTYPE)
    lv["samples"] = n
    history = []
    for i in range(3 * limit):
        p = np.minimum(powers * 4.0 ** np.asarray(a.e, dtype=np.float64), 128.0 ** 2)
        lv["sum_sq"] = np.floor(p * 2 * n).astype(np.int64)
        lv["clipped"] = np.where(p >= 127.5 ** 2, 2 * n, 0)
        history.append(list(a.e))
        a.step(lv)
    h = np.asarray(history)
    assert np.all(h[limit:] == h[limit]), "an exponent moved after hold x (max_exp - min_exp) pushes"
    inside = (params["lo_sq"] <= p) & (p <= params["hi_sq"])
    at_clamp = (h[-1] == params["min_exp"]) | (h[-1] == params["max_exp"])
    assert np.all(inside | at_clamp) and inside.sum() > len(powers) // 2


BAD = [dict(hi_sq=256), dict(lo_sq=256, hi_sq=1024), dict(lo_sq=-1), dict(hold=0), dict(min_exp=3, max_exp=2), dict(clip_ppm=-1),
       dict(max_exp=127), dict(min_exp=-127)]


@pytest.mark.parametrize("change", BAD)
def test_bad_parameters_are_refused(host, change):
    p = dict(DEFAULTS, **change)
    rc, e, quiet, why = c_step(host, p, 2592, 0, 0, 0, 0)
    assert rc == -1 and why and (e, quiet) == (0, 0)
    with pytest.raises(ValueError):
        wb.Agc(1, 100.0, **p)


def test_gains_that_overflow_the_ladder_are_refused(host):
    assert host.msk144host_wideband_gain_ok(100.0, 20) == 1
    assert host.msk144host_wideband_gain_ok(1e36, 0) == 1                 # 128e36 is finite
    assert host.msk144host_wideband_gain_ok(1e36, 20) == 0                # 128e36 x 2^20 is not
    for g in (0.0, -1.0, float("inf"), float("nan")):
        assert host.msk144host_wideband_gain_ok(g, 0) == 0
    wb.Agc(2, [100.0, 1e30], max_exp=20)
    with pytest.raises(ValueError):
        wb.Agc(2, [100.0, 1e36], max_exp=20)
    with pytest.raises(ValueError):
        wb.Agc(2, [100.0, 0.0])
    with pytest.raises(TypeError):
        wb.Agc(1, 100.0, hi=3)


@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_the_tone_scene_settles_in_the_model(name):
    shape = lc.SHAPES[name]
    f, a = lc.tone_amplitudes(shape)
    assert abs(20 * np.log10(a[0] / a[-1]) - 60.0) < 1e-9
    lv, used, q = lc.model_agc_run(name)
    lc.settled_state(shape, lv, used, q, f"model {name}")
    e = np.asarray(used)
    assert [int(v["samples"][0]) for v in lv] == [5184] + [2592] * 11
    assert (np.diff(e, axis=0) > 0).any(), "no channel stepped up"
    if name != "rat":
        assert (np.diff(e, axis=0) < 0).any() and lv[0]["clipped"].sum() > 10000, "no channel clipped and stepped down"
        assert lc.silent_channels(shape).sum() >= 14
    assert len(set(e[-1])) >= 3


def test_per_channel_quantiser_and_levels():
    rng = np.random.default_rng(5)
    y = (rng.normal(size=(6, 500)) + 1j * rng.normal(size=(6, 500))) * 0.01
    g = np.array([1.0, 10.0, 100.0, 1000.0, 1e-9, 50.0])
    q, clipped = wb.quantise(y, g, per_channel=True)
    lv = wb.levels(q, clipped)
    for c in range(6):
        qc, kc = wb.quantise(y[c:c + 1], float(g[c]))
        assert np.array_equal(q[c], qc[0]) and clipped[c] == kc
        assert lv["sum_sq"][c] == int((qc.astype(np.int64) ** 2).sum()) and lv["samples"][c] == 500
    assert wb.quantise(y, g)[1] == clipped.sum() and clipped[3] > 0 and not q[4].any()
    same, k = wb.quantise(y, 100.0)
    assert np.array_equal(wb.quantise(y, np.full(6, 100.0))[0], same)


def test_silence_then_tones_in_the_model():
    lv, used, hops = lc.model_silence_run("rat")
    lc.silence_then_tones_checks(lv, used, hops, "model rat")


def test_the_oracle_decodes_the_faint_scene_from_the_models_hops(orc):
    from oracle import oracle_cli
    import wideband_check as wc
    import wideband_gpu as wg
    raw, planted, starts = lc.decode_scene(with_starts=True)
    m = wb.Channeliser(lc.DECODE_RATE, lc.DECODE_OFFSETS)
    a = wb.Agc(len(lc.DECODE_OFFSETS), 100.0)
    hops, used = [], []
    for i, part in enumerate(wc.split_pushes(raw, lc.DECODE_RATE, lc.DECODE_PUSHES)):
        used.append(list(a.e))
        q, clipped = wb.quantise(m.filter(wb.read_samples(part, "cs16")), a.gains(), per_channel=True)
        hops.append(q)
        a.step(wb.levels(q, clipped))
    e = np.asarray(used)
    assert np.all(e[lc.DECODE_LEAD - 1] >= 5) and np.all(e[lc.DECODE_LEAD - 1:] == e[lc.DECODE_LEAD - 1]), "not settled before the pings"
    stream = np.concatenate(hops, axis=1)                            # [C][M][2]
    cfg = {k: v for k, v in wg.DECODE_CFG.items() if k != "read_mode"}
    for c, msg in planted.items():
        w0 = max(0, starts[c] // 2592 - 1) * 2592                    # the windows that hold the ping
        pay = set()
        oracle_cli.decode_stream(stream[c, w0:w0 + 5184 + 2 * 2592].reshape(-1), cfg, read_mode=2, payloads=pay)
        assert "".join(str(int(b)) for b in msg) in pay, f"the oracle does not decode the ping of channel {c} from the model's hops"
