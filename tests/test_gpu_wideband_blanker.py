"""-m gpu: the impulse-noise blanker on the wideband input stream (include/msk144hip.h), held to its Python model byte for byte:
every decision of the contract is made in integers, so nothing here has a tolerance.

1. Stream and statistics: 240 ksps, 5 channels, 5 pushes of cu8, cs8 and cs16 noise with impulses at the edges of a push (n = 0,
   N - 1, N - post + 1, two closer than pre + post): after every push msk144_dump_wideband_blanked and every field of
   msk144_wideband_blanker_stats equal wideband.Blanker's - at the default guards, at pre = post = 4096 (a halo wider than a tile) and
   at pre = post = 0.
2. Hop identity: the hops, clip count and levels of a blanked handle fed cu8 or cs8 equal those of a plain cs16 handle fed the
   model's blanked stream (the f32 inputs of the filters are the same numbers), at the three shapes of wideband_levels_check.py:
   two channel tiles, 96 branches with a push of 10 422 samples, the two-stage bank.
3. Nothing to blank: at threshold_q4 = 65535 noise has no hit, and the hops equal those of a plain cu8 handle - the cs16 staging
   alone changes nothing.
4. Switching: set and switched off before the first push is never set; set in mid-stream leaves the running stream alone and
   takes effect at the next first push; msk144_set_wideband switches it off; the same stream pushed twice gives the same bytes.
5. Effect: the three streams of the CPU effect test through the device, the same assertions on msk144_wideband_levels.
"""
import numpy as np
import pytest

import wideband_blanker_check as kc
import wideband_gpu as wg
import wideband_levels_check as lc
import wideband_options as wo
from msk144cudecoder_amd import wideband as wb
from wideband_options import EINVAL, ESTATE, code_of

pytestmark = pytest.mark.gpu

RATE = 240000
OFFSETS = kc.EFFECT_OFFSETS


@pytest.fixture(scope="module")
def handles(hip):
    """Two handles per channel count, made on first use and kept for the module."""
    with wo.handle_cache(wo.decode_pair(hip)) as get:
        yield get


def all_hops(d):
    return wg.dump_hops(d, range(d.channels))


def push_and_compare(d, model, parts, what):
    """Push parts (the first a first push) to the blanked handle d and to the model: stream and statistics equal after every push."""
    model.reset()
    for i, part in enumerate(parts):
        d.push_wideband(i % 2, part, first=i == 0)
        want, st = model.push(part)
        got = d.dump_wideband_blanked()
        assert got.shape == (len(part) // 2, 2)
        assert np.array_equal(got.reshape(-1), want), f"{what} push {i}: {np.count_nonzero(got.reshape(-1) != want)} components differ"
        assert d.wideband_blanker_stats() == st, f"{what} push {i}"
    return st


# ---- 1. stream and statistics ----

@pytest.mark.parametrize("guards", [(2, 8), (4096, 4096), (0, 0)])
@pytest.mark.parametrize("fmt", wb.FORMATS)
def test_stream_and_stats_equal_the_model(handles, fmt, guards):
    pre, post = guards
    d, _ = handles(len(OFFSETS))
    parts = kc.edge_pushes(RATE, fmt, 5, pre, post, np.random.default_rng([wb.FORMATS.index(fmt), pre, post]))
    d.set_wideband(RATE, OFFSETS, fmt)
    d.set_wideband_blanker(pre=pre, post=post)
    st = push_and_compare(d, wb.Blanker(fmt, pre=pre, post=post), parts, f"{fmt} {guards}")
    # the stream did what it was made for: hits in every push, guards that overlap, samples owed across a push boundary
    assert st["total_hits"] >= 5 * 8 and st["total_samples"] == sum(len(p) // 2 for p in parts)
    assert st["total_blanked"] > st["total_hits"] or (pre, post) == (0, 0)
    assert st["carry_out"] == post


def test_an_odd_push_length_and_another_threshold(handles):
    """24 125 sps: pushes of 10 422 and 5 211 samples - no whole number of 64-sample words or 16-byte loads, the last tile partly
    empty - at 4 x the mean power, where noise has hits of its own."""
    shape = lc.SHAPES["rat"]
    d, _ = handles(len(shape["offsets"]))
    for fmt in ("cu8", "cs16"):
        parts = kc.edge_pushes(shape["rate"], fmt, 4, 3, 70, np.random.default_rng([7, wb.FORMATS.index(fmt)]))
        assert [len(p) // 2 for p in parts] == [10422, 5211, 5211, 5211]
        d.set_wideband(shape["rate"], shape["offsets"], fmt)
        d.set_wideband_blanker(threshold_q4=64, pre=3, post=70)
        st = push_and_compare(d, wb.Blanker(fmt, threshold_q4=64, pre=3, post=70), parts, fmt)
        assert st["total_hits"] > 2 * 44            # more than the impulses planted, at most 11 per push: noise has hits of its own


# ---- 2. hop identity ----

@pytest.mark.parametrize("fmt", ["cu8", "cs8"])
@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_hops_equal_a_plain_handle_fed_the_blanked_stream(handles, name, fmt):
    shape = lc.SHAPES[name]
    rate, offsets, K = shape["rate"], shape["offsets"], shape["K"]
    sigma = 0.05
    gain = float(np.float32(30.0 / (128.0 * sigma * np.sqrt(12000.0 / rate))))   # about 30 LSB rms behind the default filters
    parts = kc.edge_pushes(rate, fmt, 4, 2, 8, np.random.default_rng([rate, wb.FORMATS.index(fmt)]), sigma=sigma)
    a, b = handles(len(offsets))
    a.set_wideband(rate, offsets, fmt, taps_per_phase=K, gain=gain)
    a.set_wideband_blanker()
    b.set_wideband(rate, offsets, "cs16", taps_per_phase=K, gain=gain)
    model = wb.Blanker(fmt)
    for i, part in enumerate(parts):
        want, st = model.push(part)
        a.push_wideband(i % 2, part, first=i == 0)
        b.push_wideband(i % 2, want, first=i == 0)
        assert st["blanked"] > st["hits"] > 0 and a.wideband_blanker_stats() == st
        ha, hb = all_hops(a), all_hops(b)
        assert ha.any() and np.array_equal(ha, hb), f"{name} {fmt} push {i}: {np.count_nonzero(ha != hb)} components differ"
        assert a.wideband_clip_count() == b.wideband_clip_count()
        la, lb = a.wideband_levels(), b.wideband_levels()
        assert np.array_equal(la, lb) and la["sum_sq"].all()


# ---- 3. nothing to blank ----

def test_without_a_hit_the_hops_are_those_of_a_plain_handle(handles):
    a, b = handles(len(OFFSETS))
    rng = np.random.default_rng(3)
    n = (wb.FIRST_OUT + 2 * wb.HOP_OUT) * RATE // wb.OUT_RATE
    raw = wb.write_samples(0.05 * (rng.normal(size=n) + 1j * rng.normal(size=n)), "cu8")
    parts = [raw[:2 * wb.FIRST_OUT * 20], raw[2 * wb.FIRST_OUT * 20:2 * (wb.FIRST_OUT + wb.HOP_OUT) * 20], raw[2 * (wb.FIRST_OUT + wb.HOP_OUT) * 20:]]
    for d in (a, b):
        d.set_wideband(RATE, OFFSETS, "cu8")
    a.set_wideband_blanker(threshold_q4=65535)
    for i, part in enumerate(parts):
        for d in (a, b):
            d.push_wideband(i % 2, part, first=i == 0)
        st = a.wideband_blanker_stats()
        assert (st["hits"], st["blanked"], st["total_hits"], st["carry_out"]) == (0, 0, 0, 0) and st["threshold"] == ((st["sum_power"] // st["samples"]) * 65535) >> 4
        assert np.array_equal(a.dump_wideband_blanked().reshape(-1), wb.as_cs16(part, "cu8"))
        ha = all_hops(a)
        assert ha.any() and np.array_equal(ha, all_hops(b))
        assert a.wideband_clip_count() == b.wideband_clip_count() and np.array_equal(a.wideband_levels(), b.wideband_levels())


# ---- 4. switching ----

def test_switching(hip, handles):
    a, b = handles(len(OFFSETS))
    parts = kc.edge_pushes(RATE, "cu8", 3, 2, 8, np.random.default_rng(4))
    wo.refuses_outside_wideband_mode(hip, [hip.HipDecoder.set_wideband_blanker])
    for d in (a, b):
        d.set_wideband(RATE, OFFSETS, "cu8")
    for bad in (dict(threshold_q4=15), dict(threshold_q4=65536), dict(pre=-1), dict(pre=4097), dict(post=-1), dict(post=4097)):
        assert code_of(hip, lambda: a.set_wideband_blanker(**bad)) == EINVAL, bad
    wo.unreadable(hip, [a.wideband_blanker_stats])                                         # before any push

    # set, then switched off before the first push: a handle that never had one
    a.set_wideband_blanker()
    a.set_wideband_blanker(None)
    plain = []
    for i, part in enumerate(parts):
        for d in (a, b):
            d.push_wideband(i % 2, part, first=i == 0)
        plain.append(all_hops(b))
        assert np.array_equal(all_hops(a), plain[i])
        wo.unreadable(hip, [a.wideband_blanker_stats, a.dump_wideband_blanked])

    # set in mid-stream: the running stream keeps what it started with
    a.push_wideband(0, parts[0], first=True)
    a.set_wideband_blanker()
    a.push_wideband(1, parts[1], first=False)
    assert np.array_equal(all_hops(a), plain[1])
    wo.unreadable(hip, [a.wideband_blanker_stats])

    # ... and the next first push is blanked; the same stream pushed twice gives the same bytes
    runs = []
    for _ in range(2):
        model, seen = wb.Blanker("cu8"), []
        for i, part in enumerate(parts):
            a.push_wideband(i % 2, part, first=i == 0)
            want, st = model.push(part)
            assert a.wideband_blanker_stats() == st and st["hits"] > 0
            assert np.array_equal(a.dump_wideband_blanked().reshape(-1), want)
            seen.append((all_hops(a), a.wideband_clip_count(), a.wideband_levels()))
            assert not np.array_equal(seen[i][0], plain[i])
        runs.append(seen)
    for (h0, c0, l0), (h1, c1, l1) in zip(*runs):
        assert np.array_equal(h0, h1) and c0 == c1 and np.array_equal(l0, l1)

    # switched off in mid-stream: still blanked until the stream restarts
    a.set_wideband_blanker(None)
    a.push_wideband(1, parts[1], first=False)
    assert a.wideband_blanker_stats()["hits"] > 0
    a.push_wideband(0, parts[0], first=True)
    assert np.array_equal(all_hops(a), plain[0]) and code_of(hip, a.wideband_blanker_stats) == ESTATE

    # msk144_set_wideband resets the blanker to off
    a.set_wideband_blanker()
    a.set_wideband(RATE, OFFSETS, "cu8")
    a.push_wideband(0, parts[0], first=True)
    assert np.array_equal(all_hops(a), plain[0]) and code_of(hip, a.wideband_blanker_stats) == ESTATE


# ---- 5. effect ----

def test_effect_on_the_channels_levels(handles):
    clean, impulses, positions = kc.effect_streams()
    a, b = handles(len(OFFSETS))
    a.set_wideband(kc.EFFECT_RATE, kc.EFFECT_OFFSETS, "cs16", gain=kc.EFFECT_GAIN)
    a.set_wideband_blanker()
    b.set_wideband(kc.EFFECT_RATE, kc.EFFECT_OFFSETS, "cs16", gain=kc.EFFECT_GAIN)
    a.push_wideband(0, clean, first=True)
    st = a.wideband_blanker_stats()
    assert st["hits"] == 0 and st["blanked"] == 0
    sum_sq_clean = a.wideband_levels()["sum_sq"].copy()
    b.push_wideband(0, impulses, first=True)
    sum_sq_impulses = b.wideband_levels()["sum_sq"].copy()
    a.push_wideband(1, impulses, first=True)
    st = a.wideband_blanker_stats()
    print("hits", st["hits"], "blanked", st["blanked"])
    assert st["hits"] == len(positions) and st["blanked"] <= 11 * len(positions)
    kc.assert_effect(sum_sq_clean, sum_sq_impulses, a.wideband_levels()["sum_sq"])
