"""-m gpu: per-channel levels, per-channel gains and the stepped AGC of the wideband channeliser (include/msk144hip.h), at the three
shapes of tests/wideband_levels_check.py - 240 ksps with 130 channels, 24 125 sps (96 branches) with 33, 8 Msps (two-stage bank,
padded slots) with 70.

1. Default identity: a handle that also calls set_wideband_gains(all G) and reads wideband_levels() after every push writes the
   same bytes and clip counts as one configured as before, at every rate and input format.
2. Per-channel gains: every channel's bytes equal those of the scalar-gain run with its gain (device against device, exact);
   sampled channels also meet the near-tie rule against the float64 model.
3. Statistics: samples, sum_sq against the dumped hops, the clipped counts against the clip count and, per channel, the model.
4. AGC: the exponent of every push equals the Python rule replayed over the device's own statistics; the settled state is the
   model's (test_wideband_levels_model.py); a first push reproduces every byte; msk144_set_wideband returns to the scalar gain.
5. Decode: a faint scene (0.2 LSB rms at gain 100) is decoded on every planted channel under the AGC, byte-identically to the same
   hops fed through msk144_push_hops; the fixed-gain result goes into the parity report.
6. msk144hipdecoder --wideband-gain=auto --wideband-levels prints the same messages and a table that agrees with the Python run.
"""
import re

import numpy as np
import pytest

import wideband_bank_check as bc
import wideband_check as wc
import wideband_gpu as wg
import wideband_levels_check as lc
import wideband_options as wo
from msk144cudecoder_amd import wideband as wb

pytestmark = pytest.mark.gpu

NAMES = list(lc.SHAPES)


@pytest.fixture(scope="module")
def pairs(hip):
    """Two handles per shape, made on first use and kept for the module."""
    with wo.handle_cache(lambda name: wo.decode_pair(hip)(len(lc.SHAPES[name]["offsets"]))) as get:
        yield get


def noise_gain(rate):
    """About 30 LSB rms for white input of wc.SIGMA per rail behind the default filters (12 kHz of the band)."""
    return wc.f32(30.0 / (128.0 * wc.SIGMA * np.sqrt(12000.0 / rate)))


def all_hops(d):
    return wg.dump_hops(d, range(d.channels))


def reference(shape, channels, gain):
    off = shape["offsets"][channels]
    if wb.is_bank_rate(shape["rate"]):
        return bc.BankReference(shape["rate"], off, K=shape["K"], gain=gain)
    return wc.Reference(shape["rate"], off, K=shape["K"], gain=gain)


# ---- 1. default identity ----

@pytest.mark.parametrize("fmt", wb.FORMATS)
@pytest.mark.parametrize("name", NAMES)
def test_default_identity(pairs, name, fmt):
    shape = lc.SHAPES[name]
    rate, C = shape["rate"], len(shape["offsets"])
    G = noise_gain(rate)
    raw = wc.raw_input(rate, 3, fmt, np.random.default_rng([rate, wb.FORMATS.index(fmt)]))
    a, b = pairs(name)
    for d in (a, b):
        d.set_wideband(rate, shape["offsets"], fmt, taps_per_phase=shape["K"], gain=G)
    b.set_wideband_gains(np.full(C, G, dtype=np.float32))
    for i, part in enumerate(wc.split_pushes(raw, rate, 3)):
        for d in (a, b):
            d.push_wideband(i % 2, part, first=i == 0)
        lv = b.wideband_levels()
        ha, hb = all_hops(a), all_hops(b)
        assert np.array_equal(ha, hb), f"{name} {fmt} push {i}"
        assert a.wideband_clip_count() == b.wideband_clip_count() == lv["clipped"].sum()
        assert ha.any() and not lv["exponent"].any() and np.all(lv["gain"] == np.float32(G))


# ---- 2. per-channel gains ----

@pytest.mark.parametrize("name", NAMES)
def test_per_channel_gains_are_exact(pairs, parity_report, name):
    shape = lc.SHAPES[name]
    rate, C = shape["rate"], len(shape["offsets"])
    G = noise_gain(rate)
    three = [wc.f32(G), wc.f32(G / 7.0), wc.f32(G * 3.0)]
    gains = np.array([three[c % 3] for c in range(C)], dtype=np.float32)
    parts = wc.split_pushes(wc.raw_input(rate, 3, "cs16", np.random.default_rng([rate, 2])), rate, 3)
    a, b = pairs(name)
    b.set_wideband(rate, shape["offsets"], "cs16", taps_per_phase=shape["K"], gain=1.0)
    b.set_wideband_gains(gains)
    got, clips = [], []
    for i, part in enumerate(parts):
        b.push_wideband(i % 2, part, first=i == 0)
        got.append(all_hops(b))
        clips.append(b.wideband_levels()["clipped"].copy())
        assert np.all(b.wideband_levels()["gain"] == gains)
    for k, g in enumerate(three):
        mine = np.arange(C) % 3 == k
        a.set_wideband(rate, shape["offsets"], "cs16", taps_per_phase=shape["K"], gain=g)
        for i, part in enumerate(parts):
            a.push_wideband(i % 2, part, first=i == 0)
            assert np.array_equal(all_hops(a)[mine], got[i][mine]), f"{name} gain {g} push {i}"
    # sampled channels against the float64 model, gain by gain
    rng = np.random.default_rng([rate, 3])
    sample = np.unique(np.concatenate([[0, 31, 32, C - 2, C - 1], rng.choice(C, size=7, replace=False)]))
    tally = wc.Tally()
    for k, g in enumerate(three):
        ch = sample[sample % 3 == k]
        ref = reference(shape, ch, g)
        for i, part in enumerate(parts):
            y, dl = ref.push(wb.read_samples(part, "cs16"), first=i == 0)
            tally.add(wc.assert_hops(got[i][ch], y, dl, g, None, what=f"{name} gain {g} push {i}"))
    parity_report(f"wideband_levels_gains_{name}", tally.report())


# ---- 3. statistics ----

@pytest.mark.parametrize("name", NAMES)
def test_statistics_are_exact(pairs, name):
    """The tone scene at one gain for all: the strong channels clip heavily; on the second push (the tones' onset has passed) the
    channels without a tone are all zero, where the shape has any."""
    shape = lc.SHAPES[name]
    rate, C = shape["rate"], len(shape["offsets"])
    G = wc.f32(shape["stats_gain"])
    parts = lc.scene_parts(name)[:2]
    a, _ = pairs(name)
    a.set_wideband(rate, shape["offsets"], "cs16", taps_per_phase=shape["K"], gain=G)
    rng = np.random.default_rng([rate, 4])
    sample = np.unique(np.concatenate([[0, 31, 32, C - 2, C - 1], rng.choice(C, size=7, replace=False)]))
    ref = reference(shape, sample, G)
    silent = lc.silent_channels(shape)
    for i, part in enumerate(parts):
        a.push_wideband(i % 2, part, first=i == 0)
        lv = a.wideband_levels()
        hops = all_hops(a)
        assert np.all(lv["samples"] == (5184 if i == 0 else 2592))
        assert np.array_equal(lv["sum_sq"], wb.levels(hops)["sum_sq"]), f"{name} push {i}"
        assert lv["clipped"].sum() == a.wideband_clip_count()
        assert lv["clipped"].max() > 2000, "no channel clips heavily"
        if i == 1 and silent.any():
            assert not lv["sum_sq"][silent].any() and not lv["clipped"][silent].any()
        y, dl = ref.push(wb.read_samples(part, "cs16"), first=i == 0)
        for j, c in enumerate(sample):
            dj = dl if dl.ndim == 1 else dl[j:j + 1]
            wc.assert_hops(hops[c:c + 1], y[j:j + 1], dj, G, int(lv["clipped"][c]), what=f"{name} push {i} channel {c}")


# ---- 4. the AGC trajectory ----

def agc_run(d, name):
    """(levels, hops) of every push of the scene under the scene's AGC, from a first push."""
    lv, hops = [], []
    for i, part in enumerate(lc.scene_parts(name)):
        d.push_wideband(i % 2, part, first=i == 0)
        lv.append(d.wideband_levels())
        hops.append(all_hops(d))
    return lv, hops


@pytest.mark.parametrize("name", NAMES)
def test_agc_trajectory(pairs, name):
    shape = lc.SHAPES[name]
    rate, C = shape["rate"], len(shape["offsets"])
    base = lc.base_gains(shape)
    a, b = pairs(name)
    b.set_wideband(rate, shape["offsets"], "cs16", taps_per_phase=shape["K"], gain=100.0)
    b.set_wideband_gains(base)
    b.set_wideband_agc(**lc.AGC)
    lv, hops = agc_run(b, name)
    # the rule replayed over the device's own statistics
    rule = wb.Agc(C, base, **lc.AGC)
    for i in range(lc.N_PUSHES):
        assert np.array_equal(lv[i]["exponent"], rule.e), f"{name} push {i}"
        assert np.array_equal(lv[i]["gain"], rule.gains().astype(np.float32))
        assert np.array_equal(lv[i]["sum_sq"], wb.levels(hops[i])["sum_sq"])
        rule.step(lv[i])
    lc.settled_state(shape, lv, [v["exponent"] for v in lv], hops[-1], f"device {name}")
    # a first push restarts exponents and hold counters
    lv2, hops2 = agc_run(b, name)
    for i in range(lc.N_PUSHES):
        assert np.array_equal(hops2[i], hops[i]), f"{name}: push {i} after the restart"
        assert np.array_equal(lv2[i], lv[i])
    # msk144_set_wideband: the scalar gain, the AGC off
    part = lc.scene_parts(name)[0]
    for d in (a, b):
        d.set_wideband(rate, shape["offsets"], "cs16", taps_per_phase=shape["K"], gain=wc.f32(shape["g0"]))
    for i in range(2):
        for d in (a, b):
            d.push_wideband(i, part, first=True)
        assert np.array_equal(all_hops(a), all_hops(b))
        lvb = b.wideband_levels()
        assert not lvb["exponent"].any() and np.all(lvb["gain"] == np.float32(shape["g0"]))


def test_silence_then_tones_at_the_rational_rate(pairs):
    """Q = 96: in silence the 96 branches add nothing to any counter, every channel climbs to max_exp on all-zero output; the tones then
    walk the ladder down.  The model shows the same (test_wideband_levels_model.py)."""
    shape = lc.SHAPES["rat"]
    C = len(shape["offsets"])
    base = lc.base_gains(shape)
    _, b = pairs("rat")
    b.set_wideband(shape["rate"], shape["offsets"], "cs16", taps_per_phase=shape["K"], gain=100.0)
    b.set_wideband_gains(base)
    b.set_wideband_agc(**lc.AGC)
    rule = wb.Agc(C, base, **lc.AGC)
    lv, hops = [], []
    for i, part in enumerate(lc.silence_then_tones("rat")):
        b.push_wideband(i % 2, part, first=i == 0)
        lv.append(b.wideband_levels())
        hops.append(all_hops(b))
        assert np.array_equal(lv[i]["exponent"], rule.e), f"push {i}"
        assert np.array_equal(lv[i]["sum_sq"], wb.levels(hops[i])["sum_sq"]) and lv[i]["clipped"].sum() == b.wideband_clip_count()
        rule.step(lv[i])
    lc.silence_then_tones_checks(lv, [v["exponent"] for v in lv], hops, "device rat")


def test_levels_describe_the_last_push(pairs):
    """Changing the gains or the AGC after a push does not change what wideband_levels() reports for that push."""
    shape = lc.SHAPES["rat"]
    C = len(shape["offsets"])
    base = lc.base_gains(shape)
    parts = lc.scene_parts("rat")
    _, b = pairs("rat")
    b.set_wideband(shape["rate"], shape["offsets"], "cs16", taps_per_phase=shape["K"], gain=100.0)
    b.set_wideband_gains(base)
    b.set_wideband_agc(**lc.AGC)
    for i in range(3):
        b.push_wideband(i % 2, parts[i], first=i == 0)
    before = b.wideband_levels()
    assert np.all(before["exponent"] == 2)
    b.set_wideband_gains(np.full(C, 7.0))
    assert np.array_equal(b.wideband_levels(), before)
    b.set_wideband_agc(None)
    assert np.array_equal(b.wideband_levels(), before)
    b.push_wideband(1, parts[3])
    after = b.wideband_levels()
    assert not after["exponent"].any() and np.all(after["gain"] == np.float32(7.0))


def test_refusals(hip, pairs):
    shape = lc.SHAPES["rat"]
    C = len(shape["offsets"])
    a, _ = pairs("rat")
    a.set_wideband(shape["rate"], shape["offsets"], "cs16", taps_per_phase=shape["K"], gain=100.0)

    def refused(call, text):
        with pytest.raises(hip.Msk144Error) as e:
            call()
        assert e.value.code == -1 and text in str(e.value), str(e.value)

    refused(lambda: a.set_wideband_agc(hi_sq=256), "hi_sq > 4 x lo_sq")
    refused(lambda: a.set_wideband_agc(hold=0), "hold")
    refused(lambda: a.set_wideband_agc(min_exp=2, max_exp=1), "min_exp <= max_exp")
    refused(lambda: a.set_wideband_gains(np.zeros(C)), "gain of channel 0")
    a.set_wideband_gains(np.full(C, 1e36))
    refused(lambda: a.set_wideband_agc(), "not finite")
    a.set_wideband_gains(None)
    a.set_wideband_agc()
    refused(lambda: a.set_wideband_gains(np.full(C, 1e36)), "gain of channel 0")
    a.set_wideband_agc(None)
    # the configured gain is held to the ladder as well when it is restored under the AGC
    a.set_wideband(shape["rate"], shape["offsets"], "cs16", taps_per_phase=shape["K"], gain=1e36)
    a.set_wideband_gains(np.ones(C))
    a.set_wideband_agc()
    refused(lambda: a.set_wideband_gains(None), "cannot be restored")
    a.set_wideband_agc(None)
    a.set_wideband_gains(None)
    wo.unreadable(hip, [a.wideband_levels])                             # no push since the configuration
    with hip.HipDecoder(channels=1, **wg.DECODE_CFG) as plain:
        refused(lambda: plain.set_wideband_agc(), "wideband mode")
        refused(lambda: plain.set_wideband_gains(np.ones(1)), "wideband mode")
        refused(lambda: plain.wideband_levels(), "wideband mode")


# ---- 5. decode under the AGC, 6. the program ----

@pytest.fixture(scope="module")
def faint(hip):
    """The faint scene (tests/wideband_levels_check.py) through a handle with the default AGC: records, hops and levels of every
    push; and the same scene at the fixed gain 100."""
    raw, planted = lc.decode_scene()
    parts = wc.split_pushes(raw, lc.DECODE_RATE, lc.DECODE_PUSHES)
    C = len(lc.DECODE_OFFSETS)
    out = dict(raw=raw, planted=planted)
    with hip.HipDecoder(channels=C, **wg.DECODE_CFG) as d:
        for agc in (False, True):
            d.set_wideband(lc.DECODE_RATE, lc.DECODE_OFFSETS, "cs16", gain=100.0)
            if agc:
                d.set_wideband_agc()
            recs, hops, lv = [], [], []
            for i, part in enumerate(parts):
                d.push_wideband(i % 2, part, first=i == 0)
                lv.append(d.wideband_levels())
                hops.append(all_hops(d))
                recs.append(wg._decode(d, i % 2))
            out["agc" if agc else "fixed"] = dict(recs=recs, hops=hops, levels=lv)
    return out


def test_faint_scene_decodes_under_the_agc(hip, faint, parity_report):
    run, fixed = faint["agc"], faint["fixed"]
    rms0 = np.sqrt(fixed["levels"][lc.DECODE_LEAD - 1]["sum_sq"] / (2.0 * 2592))
    assert np.median(rms0) < 0.4, "the scene is not faint at gain 100"     # 0.2 LSB before the rounding, less after it
    lv = run["levels"]
    assert np.all(lv[lc.DECODE_LEAD - 1]["exponent"] >= 5) and all(np.array_equal(v["exponent"], lv[lc.DECODE_LEAD - 1]["exponent"]) for v in lv[lc.DECODE_LEAD:])
    got = wg.messages_by_channel(run["recs"])
    wg.check_channels(got, faint["planted"], lc.DECODE_OFFSETS)
    with hip.HipDecoder(channels=len(lc.DECODE_OFFSETS), **wg.DECODE_CFG) as b:
        rec_b = wg.decode_hops(b, run["hops"])
    for ra, rb in zip(run["recs"], rec_b):
        assert ra.tobytes() == rb.tobytes()
    got_fixed = wg.messages_by_channel(fixed["recs"]) if sum(len(r) for r in fixed["recs"]) else {}
    parity_report("wideband_levels_faint_scene", dict(
        planted=len(faint["planted"]), decoded_with_agc=sum(m in got.get(c, ()) for c, m in faint["planted"].items()),
        decoded_at_fixed_gain_100=sum(m in got_fixed.get(c, ()) for c, m in faint["planted"].items()),
        rms_lsb_at_fixed_gain=float(np.median(rms0)), settled_exponent=int(np.median(lv[-1]["exponent"]))))


def test_faint_scene_through_the_program(faint):
    offsets = lc.DECODE_OFFSETS
    args = ["--wideband-rate=%d" % lc.DECODE_RATE, "--wideband-format=cs16", "--channel-offsets=" + ",".join(str(int(f)) for f in offsets),
            "--wideband-gain=auto", "--wideband-levels"] + wg.SCENE_DECODE_ARGS
    lines, err = wg.run_program(args, faint["raw"].tobytes())
    got = wg.messages_by_channel_in_lines(lines)
    wg.check_channels(got, faint["planted"], offsets)
    assert got == wg.messages_by_channel(faint["agc"]["recs"])
    lv = faint["agc"]["levels"]
    table = re.findall(r"wideband level ch=(\d+) offset=(-?\d+) Hz rms=([0-9.]+) LSB clipped=(\d+) gain=([0-9.e+-]+) exp=(-?\d+)\.\.(-?\d+)", err)
    assert [int(t[0]) for t in table] == list(range(len(offsets))) and [int(t[1]) for t in table] == [int(f) for f in offsets]
    rms = {}
    for c, t in enumerate(table):
        S, n = sum(int(v["sum_sq"][c]) for v in lv), sum(int(v["samples"][c]) for v in lv)
        rms[c] = np.sqrt(S / (2.0 * n))
        assert abs(float(t[2]) - rms[c]) < 0.006 and int(t[3]) == sum(int(v["clipped"][c]) for v in lv)
        assert float(t[4]) == float(lv[-1]["gain"][c])
        assert (int(t[5]), int(t[6])) == (min(int(v["exponent"][c]) for v in lv), max(int(v["exponent"][c]) for v in lv))
    named = re.search(r"wideband levels: most clipped((?: ch=\d+ \(\d+\)){3}); quietest((?: ch=\d+ \([0-9.]+ LSB\)){3})", err)
    assert named
    quiet = [int(c) for c in re.findall(r"ch=(\d+)", named.group(2))]
    assert sorted(rms[c] for c in quiet) == sorted(rms.values())[:3]
