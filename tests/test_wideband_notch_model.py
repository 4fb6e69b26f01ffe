"""CPU: the notch of the wideband contract (include/msk144hip.h) - wideband.Notch and wideband.notch_taps against the C++ of
csrc/wideband.h in libmsk144host.so (notch_filter, notch_design, the two checks, notch_response, NotchPlanner).

1. wideband.Notch equals notch_filter byte for byte on random int8 streams cut into pushes of 5184 + 3 x 2592 samples, with random
   taps (including -128) and shifts 0, 7 and 15.
2. notch_taps equals the C++ design; every refusal of the two checks.
3. The default design for one frequency is at least 20 dB down within +-62 Hz of it and within 0.5 dB at +-400 Hz and beyond (the
   values at +62 Hz and +400 Hz are printed; the design's own CPU check gave -23.0 dB and -0.1 dB for W = 100).
4. Identities: all-zero taps give the input delayed by 31 samples exactly, across push boundaries; taps[31] = (64, 0) with shift 6
   gives all zeros.
5. The table: a changed entry zeroes that channel's tail only, an unchanged one keeps its tail, channels not in the table pass.
6. wideband.NotchPlanner equals its C++ twin (csrc/wideband.h NotchPlanner) on constructed sums: a bin hot for PERSIST periods, hot
   for one period only, a third carrier refused, one closer than 1000 Hz refused, the interpolated frequency of a tone between two
   bins, edge bins.
"""
import numpy as np
import pytest

import wideband_notch_check as nc
from msk144cudecoder_amd import wideband as wb

PUSHES = (5184, 2592, 2592, 2592)


def stream(channels, seed, lo=-128, hi=128):
    rng = np.random.default_rng([17, seed])
    return [rng.integers(lo, hi, size=(channels, n, 2)).astype(np.int8) for n in PUSHES]


# ---- 1. the model against the C++ filter ----

def test_the_model_equals_the_host_filter_byte_for_byte():
    shifts = [0, 7, 15, 7]
    taps = np.stack([nc.random_taps(c) for c in range(4)])
    taps[3] = wb.notch_taps([300, -700])[0]
    shifts[3] = wb.notch_taps([300, -700])[1]
    model = wb.Notch(4, {c: (taps[c], shifts[c]) for c in range(4)})
    host = nc.HostNotch(taps, shifts)
    total = np.zeros(4, dtype=np.int64)
    for i, q in enumerate(stream(4, 1)):
        y, k = model.push(q)
        yh, kh = host.push(q)
        assert y.dtype == np.int8 and y.tobytes() == yh.tobytes(), f"push {i}"
        assert np.array_equal(k, kh), f"push {i}: clipped {k} != {kh}"
        assert np.array_equal(model.tail, host.tail) and np.array_equal(model.tail, q[:, -63:]), f"push {i}: the tail is the raw input's"
        total += k
    print("clamped components per channel (shifts 0, 7, 15, design):", total)
    assert total[0] > 0 and total[1] > 0        # random taps at small shifts drive the output into the clamp


# ---- 2. the design and the checks ----

@pytest.mark.parametrize("freqs, hw", [([0], 100), ([300], 100), ([-5900], 100), ([300, -700], 100), ([1200, 200], 60), ([-2500, 3500], 500), ([5500], 500), ([40], 50)])
def test_notch_taps_is_the_host_design(freqs, hw):
    taps, shift = wb.notch_taps(freqs, hw)
    ht, hs = nc.host_design(freqs, hw)
    assert taps.dtype == np.int8 and taps.shape == (64, 2) and np.array_equal(taps, ht) and shift == hs
    assert 0 <= shift <= 15 and not taps[63].any()
    top = np.abs(taps.astype(np.int32)).max()
    assert 64 <= top <= 127 or shift == 15      # s = floor(log2(127 / largest |component|)): the next shift would not fit
    # the design in numpy, to the rounding of rint at a tie
    k = np.arange(63)
    arg = 2.0 * hw * (k - 31) / 12000.0
    h = np.sinc(arg) * (0.54 - 0.46 * np.cos(2 * np.pi * k / 62))
    b = sum(h / h.sum() * np.exp(2j * np.pi * f * (k - 31) / 12000.0) for f in freqs)
    want = np.stack([b.real, b.imag], axis=1) * 2.0 ** shift
    assert np.abs(taps[:63] - want).max() <= 0.5 + 1e-9
    assert shift == min(15, int(np.floor(np.log2(127.0 / np.abs(want / 2.0 ** shift).max()))))


def test_refusals_of_the_two_checks():
    for bad in (-1, 16, 40, 1 << 20, -(1 << 31)):
        assert "0..15" in nc.host_check(bad), bad
    for good in (0, 7, 15):
        assert nc.host_check(good) == ""
    assert "1 or 2 frequencies" in nc.host_design([], 100)
    assert "1 or 2 frequencies" in nc.host_design([100, 1200, 2400], 100)
    for hw in (49, 501, 0, -100):
        assert "50..500" in nc.host_design([0], hw), hw
    assert "+-6000" in nc.host_design([5901], 100) and "+-6000" in nc.host_design([-5901], 100) and "+-6000" in nc.host_design([5501], 500)
    assert "+-6000" in nc.host_design([0, 5951], 50)
    assert "1000 Hz apart" in nc.host_design([300, 1299], 100) and "1000 Hz apart" in nc.host_design([-200, 200], 100) and "1000 Hz apart" in nc.host_design([0, 0], 100)
    assert not isinstance(nc.host_design([300, 1300], 100), str) and not isinstance(nc.host_design([5900], 100), str) and not isinstance(nc.host_design([0], 50), str)
    with pytest.raises(ValueError, match="1000 Hz apart"):
        wb.notch_taps([0, 999])
    with pytest.raises(ValueError, match="50..500"):
        wb.notch_taps([0], 600)


# ---- 3. the response of the default design ----

@pytest.mark.parametrize("f0", [300, 0, -1700])
def test_the_default_design_is_deep_at_the_carrier_and_flat_away_from_it(f0):
    taps, shift = wb.notch_taps([f0])
    near = nc.response_db(taps, shift, f0 + np.arange(-62, 63))
    far = nc.response_db(taps, shift, np.concatenate([np.arange(f0 + 400, 6000, 25), np.arange(-6000, f0 - 399, 25)]))
    at62, at400 = nc.response_db(taps, shift, [f0 + 62, f0 + 400])
    print(f"f0 = {f0}: {at62:.1f} dB at +62 Hz, {at400:.2f} dB at +400 Hz, {near.max():.1f} dB the least within +-62 Hz, {np.abs(far).max():.2f} dB the most beyond +-400 Hz")
    assert near.max() <= -20.0
    assert np.abs(far).max() <= 0.5


# ---- 4. identities ----

def test_all_zero_taps_delay_the_input_by_31_samples():
    parts = stream(2, 4)
    for shift in (0, 6, 15):
        model = wb.Notch(2, {0: (np.zeros((64, 2), dtype=np.int8), shift)})
        whole = np.concatenate([np.zeros((2, 31, 2), dtype=np.int8)] + parts, axis=1)
        pos = 0
        for i, q in enumerate(parts):
            y, k = model.push(q)
            assert np.array_equal(y[0], whole[0, pos:pos + q.shape[1]]) and np.array_equal(y[1], q[1]) and not k.any(), f"shift {shift} push {i}"
            pos += q.shape[1]


def test_a_unit_tap_at_the_delay_cancels_everything():
    model = wb.Notch(1, {0: (nc.delta(31, 64, 0), 6)})
    host = nc.HostNotch(nc.delta(31, 64, 0)[None], [6])
    for q in stream(1, 5):
        y, k = model.push(q)
        yh, kh = host.push(q)
        assert not y.any() and not k.any() and not yh.any() and not kh.any()


# ---- 5. the table ----

def test_a_changed_entry_restarts_that_channel_alone():
    parts = stream(3, 6)
    e0, e1 = wb.notch_taps([300]), wb.notch_taps([-700, 900])
    model = wb.Notch(3, {0: [300], 2: e1})
    model.push(parts[0])
    model.push(parts[1])
    tail = model.tail.copy()
    assert tail[0].any() and tail[2].any() and not tail[1].any()
    model.set({0: e0, 1: [0], 2: [-700, 1000]})          # 0 unchanged (the same taps, given as taps), 1 new, 2 changed
    assert np.array_equal(model.tail[0], tail[0]) and not model.tail[1].any() and not model.tail[2].any()
    y, _ = model.push(parts[2])
    kept = wb.Notch(3, {0: [300]})
    kept.push(parts[0])
    kept.push(parts[1])
    assert np.array_equal(y[0], kept.push(parts[2])[0][0])
    fresh = wb.Notch(3, {1: [0], 2: [-700, 1000]})
    assert np.array_equal(y[1:], fresh.push(parts[2])[0][1:])
    model.set(None)
    y, k = model.push(parts[3])
    assert np.array_equal(y, parts[3]) and not k.any()
    with pytest.raises(ValueError):
        model.set({3: [0]})
    with pytest.raises(ValueError):
        model.set({0: (np.zeros((64, 2)), 16)})


# ---- 6. the planner of --wideband-notch=auto against its C++ twin ----

def floor_sums(channels, seed):
    """A period's push: a flat floor of about 1000 per bin with 1 % ripple."""
    return 1000.0 * (1.0 + 0.01 * np.random.default_rng([23, seed]).standard_normal((channels, 96)))


def tone(s, c, f_hz, power):
    """Adds a tone at f_hz to channel c's sums as a Hann window spreads it: the main lobe over the two or three nearest bins."""
    x = f_hz / 125.0 + 48
    for j in range(96):
        d = j - x
        if abs(d) < 2.0:
            s[c, j] += power * (0.5 + 0.5 * np.cos(np.pi * d / 2.0)) ** 2
    return s


def run_both(pushes, channels, **plan):
    """Feeds both planners; returns the model's [(push, channel, hz, excess)], having held the C++ twin to the same."""
    model, host = wb.NotchPlanner(channels, **plan), nc.HostPlanner(channels, **plan)
    out = []
    for i, s in enumerate(pushes):
        got, want = model.push(s), host.push(s)
        assert [(c, hz) for c, hz, _ in got] == [(c, hz) for c, hz, _ in want], f"push {i}"
        assert all(a[2] == b[2] for a, b in zip(got, want)), f"push {i}: the excess differs"
        out += [(i, c, hz, ex) for c, hz, ex in got]
    return out, model


def test_planner_a_bin_hot_for_persist_periods_adds_a_notch():
    # period 3, persist 2: the carrier of channel 1 is there from the start, and is added at the end of the second period (push 5)
    pushes = [tone(floor_sums(3, i), 1, 750.0, 40000.0) for i in range(12)]
    added, model = run_both(pushes, 3, db=10.0, period=3, persist=2)
    assert [(i, c, hz) for i, c, hz, _ in added] == [(5, 1, 750)]
    assert 15.0 < added[0][3] < 17.0          # 3 x 41000 over a median of 3 x 1000
    assert model.notches == [[], [750], []]


def test_planner_a_bin_hot_for_one_period_only_adds_nothing():
    pushes = [floor_sums(2, i) for i in range(12)]
    for i in (3, 4, 5):                        # the second period alone
        tone(pushes[i], 0, -1500.0, 40000.0)
    for i in (6, 7, 8):                        # then another bin: the run starts again
        tone(pushes[i], 0, 2000.0, 40000.0)
    added, model = run_both(pushes, 2, db=10.0, period=3, persist=2)
    assert added == [] and model.notches == [[], []]
    # hot, quiet, hot: not consecutive
    pushes = [floor_sums(1, i) for i in range(9)]
    for i in (0, 1, 2, 6, 7, 8):
        tone(pushes[i], 0, 500.0, 40000.0)
    assert run_both(pushes, 1, db=10.0, period=3, persist=2)[0] == []
    # the same bin +-1 counts as the same carrier, two bins away does not
    for step, n in ((125.0, 1), (250.0, 0)):
        pushes = [tone(floor_sums(1, i), 0, 500.0 + step * (i // 3), 40000.0) for i in range(6)]
        assert len(run_both(pushes, 1, db=10.0, period=3, persist=2)[0]) == n, step
    # below DB: 9 dB over the median is not hot at 10, and is at 8
    pushes = [tone(floor_sums(1, i), 0, 500.0, 7000.0) for i in range(6)]
    assert run_both(pushes, 1, db=10.0, period=3, persist=2)[0] == []
    assert len(run_both(pushes, 1, db=8.0, period=3, persist=2)[0]) == 1


def test_planner_a_third_carrier_and_one_closer_than_1000_hz_are_refused():
    pushes = []
    for i in range(10):
        s = floor_sums(2, i)
        tone(s, 0, 0.0, 90000.0)
        tone(s, 0, 1500.0, 60000.0)
        tone(s, 0, -2500.0, 30000.0)             # the third: never added
        tone(s, 1, 1000.0, 90000.0)
        tone(s, 1, 1875.0, 60000.0)              # 875 Hz from the first, and outside its guard of 3 bins: refused by the spacing rule
        tone(s, 1, -3000.0, 30000.0)             # the next one the search sees only once 1875 Hz stops being the highest: never
        pushes.append(s)
    added, model = run_both(pushes, 2, db=10.0, period=1, persist=2)
    assert [(i, c, hz) for i, c, hz, _ in added] == [(1, 0, 0), (1, 1, 1000), (3, 0, 1500)]
    assert model.notches == [[0, 1500], [1000]]


def test_planner_interpolates_between_two_bins_and_handles_the_edges():
    # a tone between bins 52 and 53: nearer 52
    for f, lo, hi in ((540.0, 520, 560), (562.5, 562, 563), (600.0, 580, 620)):
        pushes = [tone(floor_sums(1, i), 0, f, 40000.0) for i in range(2)]
        added, _ = run_both(pushes, 1, db=10.0, period=1, persist=2)
        assert len(added) == 1 and lo <= added[0][2] <= hi, (f, added)
    # the edge bins: no neighbour on one side, d = 0; bin 0 is -6000 Hz, which the design rule (|f| + W <= 6000) refuses
    pushes = [floor_sums(2, i) for i in range(4)]
    for s in pushes:
        s[0, 0] += 50000.0
        s[1, 95] += 50000.0
        s[1, 94] += 20000.0
    added, model = run_both(pushes, 2, db=10.0, period=1, persist=2)
    assert [(c, hz) for _, c, hz, _ in added] == [(1, 5875)] and model.notches == [[], [5875]]
    assert wb.NotchPlanner.vertex(np.ones(96), 0) == 0.0 and wb.NotchPlanner.vertex(np.ones(96), 95) == 0.0
    a = np.ones(96)
    a[10], a[11] = 100.0, 0.0
    assert wb.NotchPlanner.vertex(a, 10) == 0.0      # a neighbour that is not positive
    a[9], a[11] = 1.0, 10.0
    assert 0.0 < wb.NotchPlanner.vertex(a, 10) < 0.5


def test_planner_defaults_and_refusals():
    assert wb.NOTCH_PLAN_DEFAULTS == dict(db=10.0, period=23, persist=2) and wb.WATERFALL_CARRIER_DB == 10.0
    got = nc.host_parse("auto")
    assert (got["db"], got["period"], got["persist"], got["halfwidth"]) == (10.0, 23, 2, 100)
    for bad in (dict(db=0.5), dict(db=101.0), dict(period=0), dict(persist=0), dict(period=100001), dict(persist=1001)):
        with pytest.raises(ValueError):
            wb.NotchPlanner(1, **bad)
        assert not nc.host().msk144host_wideband_notch_planner_new(1, bad.get("db", 10.0), bad.get("period", 23), bad.get("persist", 2), 100), bad
