"""CPU: the impulse-noise blanker of the wideband contract (include/msk144hip.h) in its Python model, wideband.Blanker.

1. Hand-made pushes: a hit at n = 0 (the pre-guard is cut at the start of the push), a hit at N - 1 (the whole post-guard is owed to
   the next push, which blanks it without a hit of its own), overlapping guards, p == T is no hit, an all-zero cs16 push and an
   all-128 cu8 push have none.
2. The cs16 form of every raw value of every format reads as exactly the same number.
3. msk144host_wideband_blanker_threshold - csrc/wideband.h blanker_threshold, the function the device runs - equals Python integers,
   also at the largest sums a push can reach.
4. Effect, on the float64 Channeliser with the default taps: impulses of twice the noise's mean power raise every channel's level
   by at least 1.8 x (3 x, less what int8 clips); behind the blanker it is back within 0.97 .. 1.01 of the clean stream's
   (1 - 0.011 expected: 11 of every 1000 samples are zeroed); the clean stream has no hit.
"""
import ctypes as C

import numpy as np
import pytest

import wideband_blanker_check as kc
from msk144cudecoder_amd import wideband as wb


def cs16_push(N, at=(), value=(1000, 0), floor=(1, 0)):
    x = np.tile(np.array(floor, dtype=np.int16), (N, 1))
    for n in at:
        x[n] = value
    return x.reshape(-1)


def blanked_at(out):
    return np.flatnonzero(~out.reshape(-1, 2).any(axis=1))


def test_a_hit_at_the_start_of_a_push_has_its_pre_guard_cut():
    b = wb.Blanker("cs16", pre=2, post=3)
    out, st = b.push(cs16_push(64, at=[0]))
    assert list(blanked_at(out)) == [0, 1, 2, 3]
    assert (st["samples"], st["hits"], st["blanked"], st["carry_out"]) == (64, 1, 4, 0)
    assert st["sum_power"] == 1000 * 1000 + 63 and st["threshold"] == ((1000063 // 64) * 256) >> 4


def test_a_hit_at_the_end_of_a_push_owes_its_post_guard_to_the_next():
    b = wb.Blanker("cs16", pre=2, post=5)
    out, st = b.push(cs16_push(64, at=[63]))
    assert list(blanked_at(out)) == [61, 62, 63] and st["carry_out"] == 5
    out, st = b.push(cs16_push(64))                       # all samples alike: p = M, no hit
    assert list(blanked_at(out)) == [0, 1, 2, 3, 4]
    assert (st["hits"], st["blanked"], st["carry_out"]) == (0, 5, 0)
    assert (st["total_samples"], st["total_hits"], st["total_blanked"]) == (128, 1, 8)
    out, st = b.push(cs16_push(64))                       # nothing is owed twice
    assert st["blanked"] == 0 and len(blanked_at(out)) == 0
    # N - post + 1 owes two samples; reset() forgets what is owed and the totals
    out, st = b.push(cs16_push(64, at=[64 - 5 + 1]))
    assert st["carry_out"] == 2
    b.reset()
    out, st = b.push(cs16_push(64))
    assert st["blanked"] == 0 and st["total_samples"] == 64


def test_what_is_owed_and_a_hit_of_the_next_push_overlap():
    b = wb.Blanker("cs16", pre=1, post=4)
    b.push(cs16_push(64, at=[62]))                        # owes 62 + 4 - 63 = 3
    out, st = b.push(cs16_push(64, at=[3]))
    assert list(blanked_at(out)) == [0, 1, 2, 3, 4, 5, 6, 7] and (st["hits"], st["blanked"]) == (1, 8)


def test_overlapping_guards_are_counted_once():
    b = wb.Blanker("cs16", pre=2, post=3)
    out, st = b.push(cs16_push(64, at=[10, 14]))
    assert list(blanked_at(out)) == list(range(8, 18)) and (st["hits"], st["blanked"]) == (2, 10)
    keep = np.setdiff1d(np.arange(64), np.arange(8, 18))
    assert np.array_equal(out.reshape(-1, 2)[keep], np.tile([1, 0], (54, 1)))


def test_a_power_equal_to_the_threshold_is_no_hit():
    # powers 25, 9, 9, 9: M = 13, T = (13 x 31) >> 4 = 25
    x = np.array([[3, 4], [3, 0], [0, 3], [3, 0]], dtype=np.int16)
    out, st = wb.Blanker("cs16", threshold_q4=31, pre=0, post=0).push(x.reshape(-1))
    assert (st["sum_power"], st["threshold"], st["hits"], st["blanked"]) == (52, 25, 0, 0) and np.array_equal(out, x.reshape(-1))
    x[0] = [5, 1]                                         # 26 > 25, and M is still 13
    out, st = wb.Blanker("cs16", threshold_q4=31, pre=0, post=0).push(x.reshape(-1))
    assert (st["sum_power"], st["threshold"], st["hits"], st["blanked"]) == (53, 25, 1, 1) and list(blanked_at(out)) == [0]


def test_silence_has_no_hits():
    out, st = wb.Blanker("cs16").push(np.zeros(2 * 100, dtype=np.int16))
    assert (st["sum_power"], st["threshold"], st["hits"], st["blanked"]) == (0, 0, 0, 0)
    raw = np.full(2 * 100, 128, dtype=np.uint8)           # cu8 has no zero: c = 1, p = 2
    out, st = wb.Blanker("cu8").push(raw)
    assert (st["sum_power"], st["threshold"], st["hits"], st["blanked"]) == (200, 32, 0, 0) and np.all(out == 128)


def test_parameters_are_held_to_the_contract():
    assert wb.BLANKER_DEFAULTS == dict(threshold_q4=256, pre=2, post=8) and wb.Blanker("cu8").p == wb.BLANKER_DEFAULTS
    for bad in (dict(threshold_q4=15), dict(threshold_q4=65536), dict(pre=-1), dict(post=4097)):
        with pytest.raises(ValueError):
            wb.Blanker("cs8", **bad)
    with pytest.raises(TypeError):
        wb.Blanker("cs8", guard=3)
    wb.Blanker("cs8", threshold_q4=16, pre=4096, post=4096)
    wb.Blanker("cs8", threshold_q4=65535, pre=0, post=0)


@pytest.mark.parametrize("fmt", wb.FORMATS)
def test_the_cs16_form_of_every_raw_value_reads_the_same(fmt):
    info = np.iinfo({"cu8": np.uint8, "cs8": np.int8, "cs16": np.int16}[fmt])
    v = np.arange(info.min, info.max + 1, dtype=np.int64)
    raw = np.stack([v, v[::-1]], axis=1).astype(info.dtype).reshape(-1)       # every value as I and as Q
    conv = wb.as_cs16(raw, fmt)
    assert conv.dtype == np.int16
    assert np.array_equal(wb.read_samples(conv, "cs16"), wb.read_samples(raw, fmt))
    # and through the blanker, where nothing is blanked
    quiet = raw.reshape(-1, 2)[np.abs(wb.blanker_components(raw, fmt)).max(axis=1) < 20].reshape(-1)
    out, st = wb.Blanker(fmt, threshold_q4=65535).push(quiet)
    assert st["hits"] == 0 and np.array_equal(wb.read_samples(out, "cs16"), wb.read_samples(quiet, fmt))


def test_the_host_threshold_is_the_python_rule():
    L = wb._host_lib()
    f = L.msk144host_wideband_blanker_threshold
    f.argtypes, f.restype = [C.c_int64, C.c_int64, C.c_int32], C.c_int64
    cases = [(N << 31, N, 65535) for N in (10368, 26542080)]                  # every sample at cs16's largest power, 2 x 32768^2
    cases += [(0, 5184, 256), (1, 5184, 256), (5183, 5184, 65535), (5184, 5184, 16), (5184 * 17 + 5183, 5184, 17)]
    rng = np.random.default_rng(1)
    for _ in range(2000):
        N = int(rng.integers(1, 26542081))
        cases.append((int(rng.integers(0, (N << 31) + 1)), N, int(rng.integers(16, 65536))))
    for S, N, q in cases:
        assert f(S, N, q) == ((S // N) * q) >> 4, (S, N, q)
    assert f(10368 << 31, 10368, 65535) == (65535 << 31) >> 4
    assert f(100, 0, 256) == f(-1, 10, 256) == f(100, 10, 15) == f(100, 10, 65536) == -1


def test_effect_on_the_channels_levels():
    clean, impulses, positions = kc.effect_streams()
    ch = wb.Channeliser(kc.EFFECT_RATE, kc.EFFECT_OFFSETS, gain=kc.EFFECT_GAIN)
    sum_sq = lambda raw: wb.levels(ch.push(wb.read_samples(raw, "cs16"), first=True)[0])["sum_sq"]
    b = wb.Blanker("cs16")
    out, st = b.push(clean)
    assert st["hits"] == 0 and np.array_equal(out, clean)
    b.reset()
    out, st = b.push(impulses)
    print("hits", st["hits"], "blanked", st["blanked"])
    assert st["hits"] == len(positions) == 103 and st["blanked"] <= 11 * len(positions)
    kc.assert_effect(sum_sq(clean), sum_sq(impulses), sum_sq(out))
