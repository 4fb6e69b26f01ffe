"""The ping band of the wideband contract (include/msk144hip.h) on the CPU: the default design, the C++ filter
(csrc/wideband.h ping_band_energies through libmsk144host.so) against the Python model wideband.PingBand integer for integer, the
identities and extremes of the filter, its tail, and what the band is for - the sensitivity scene of wideband_pingband_check.py, where
the band sees both pings whole and the whole-channel detector sees nothing, and the capture that follows either.
"""
import numpy as np
import pytest

import wideband_pingband_check as bc
import wideband_pings_check as pc
from msk144cudecoder_amd import wideband as wb

DESIGNS = [(0, 1500), (0, 500), (0, 3000), (1500, 1500), (-2000, 1000), (4500, 1500), (137, 1234)]


def random_hops(rng, channels, first):
    return rng.integers(-128, 128, size=(channels, wb.FIRST_OUT if first else wb.HOP_OUT, 2)).astype(np.int8)


def delta(k, re=1, im=0):
    t = np.zeros((64, 2), dtype=np.int8)
    t[k] = (re, im)
    return t


# ---- the default design ----

@pytest.mark.parametrize("centre,halfwidth", DESIGNS)
def test_the_default_design(centre, halfwidth):
    taps, shift = wb.ping_band_taps(centre, halfwidth)
    assert taps.dtype == np.int8 and taps.shape == (64, 2) and np.abs(taps.astype(int)).max() == 127
    host_taps, host_shift = bc.host_design(centre, halfwidth)
    assert np.array_equal(taps, host_taps) and shift == host_shift
    top = float(bc.response_db(taps, centre)[0])
    assert shift == int(np.rint(top / (10.0 * np.log10(2.0)))) and 0 <= shift <= 40
    f = np.arange(-6000.0, 6000.0, 5.0)
    rel = bc.response_db(taps, f) - top
    dist = np.abs((f - centre + 6000.0) % 12000.0 - 6000.0)     # |f - centre| with frequencies wrapped to +-6000
    inside, outside = dist <= halfwidth - 400, dist >= halfwidth + 400
    print(f"{centre} +-{halfwidth}: shift {shift}, pass band {rel[inside].min():+.2f} .. {rel[inside].max():+.2f} dB, stop band {rel[outside].max():.1f} dB")
    assert inside.any() and outside.any()
    assert rel[inside].min() >= -0.5 and rel[inside].max() <= 0.5
    assert rel[outside].max() <= -30.0


def test_the_design_refuses_what_the_contract_refuses():
    for centre, halfwidth in ((0, 499), (0, 3001), (4501, 1500), (-5501, 500), (6000, 500)):
        assert isinstance(bc.host_design(centre, halfwidth), str), (centre, halfwidth)
        with pytest.raises(ValueError):
            wb.ping_band_taps(centre, halfwidth)
    for centre, halfwidth in ((0, 500), (0, 3000), (4500, 1500), (-5500, 500), (3000, 3000)):
        assert not isinstance(bc.host_design(centre, halfwidth), str), (centre, halfwidth)
    assert bc.host_check(0) == "" and bc.host_check(40) == "" and bc.host_check(-1) != "" and bc.host_check(41) != ""
    for shift in (-1, 41):
        with pytest.raises(ValueError):
            wb.PingBand(1, delta(0), shift)


# ---- two implementations ----

@pytest.mark.parametrize("shift", [0, 18, 40])
@pytest.mark.parametrize("small", [False, True])
def test_the_host_filter_equals_the_model(shift, small):
    rng = np.random.default_rng([5, shift, small])
    taps = (rng.integers(-2, 3, size=(64, 2)) if small else rng.integers(-128, 128, size=(64, 2))).astype(np.int8)
    if not small:
        taps[rng.integers(0, 64, size=4), 1] = -128     # the tap that (br, -bi) cannot hold
        taps[rng.integers(0, 64, size=4), 0] = -128
    C_ = 3
    a, b = wb.PingBand(C_, taps, shift), bc.HostPingBand(C_, taps, shift)
    for i in range(4):
        q = random_hops(rng, C_, i == 0)
        if small:
            q = (q.astype(np.int16) * 3 // 128).astype(np.int8)     # -3 .. 2: with taps of -2 .. 2 the sums stay under the clamp at shift 0
        Ea, Eb = a.push(q), b.push(q)
        assert Ea.dtype == np.int64 and Ea.shape == (C_, 54 if i == 0 else 27)
        assert np.array_equal(Ea, Eb), f"push {i}"
        assert np.array_equal(a.tail, b.tail) and np.array_equal(a.tail, q[:, -63:, :])
        assert 0 <= Ea.min() and Ea.max() <= (1 << 22) - 1
    if small and shift == 0:
        assert 0 < Ea.min() and Ea.max() < (1 << 22) - 1, "this case is meant to stay under the clamp"
    if not small and shift == 0:
        assert Ea.min() == (1 << 22) - 1, "... and this one to reach it"


# ---- identities ----

def test_identities():
    rng = np.random.default_rng(11)
    C_ = 2
    hops = [random_hops(rng, C_, i == 0) for i in range(3)]
    for model in (wb.PingBand, bc.HostPingBand):
        # b[0] = 1: Ef is E; b[0] = j turns every sample by 90 degrees: E again
        for re, im in ((1, 0), (0, 1), (-1, 0), (0, -1)):
            band = model(C_, delta(0, re, im), 0)
            for q in hops:
                assert np.array_equal(band.push(q), wb.ping_blocks(q)), (model.__name__, re, im)
        # b[63] = 1: the E of the stream delayed by 63 samples, across the push boundaries, zeros in front of the stream
        band = model(C_, delta(63), 0)
        stream = np.concatenate([np.zeros((C_, 63, 2), dtype=np.int8)] + hops, axis=1)
        pos = 0
        for q in hops:
            M = q.shape[1]
            assert np.array_equal(band.push(q), wb.ping_blocks(stream[:, pos:pos + M])), model.__name__
            pos += M
    # a shorter filter is zero-padded
    assert np.array_equal(wb.PingBand(C_, [[1, 0]], 0).push(hops[0]), wb.ping_blocks(hops[0]))


# ---- extremes ----

def test_extremes():
    for model in (wb.PingBand, bc.HostPingBand):
        band = model(2, np.full((64, 2), -128, dtype=np.int8), 0)
        assert not band.push(np.zeros((2, wb.FIRST_OUT, 2), dtype=np.int8)).any()
        # hops and taps all -128: every product is (-128 - 128j)^2 = 32768j, so z[n] = min(n + 1, 64) . 32768j from a zero tail and
        # 64 . 32768j = 2^21 j behind it
        full = np.full((2, wb.HOP_OUT, 2), -128, dtype=np.int8)
        band.reset()
        assert np.all(band.push(full) == (1 << 22) - 1) and np.all(band.push(full) == (1 << 22) - 1)
        first = [sum((min(n + 1, 64) * 32768) ** 2 for n in range(96 * b, 96 * b + 96)) for b in range(27)]
        steady = 96 * (1 << 42)
        assert first[1] == steady and steady < 1 << 50
        for shift in (18, 26, 27, 40):
            band = model(2, np.full((64, 2), -128, dtype=np.int8), shift)
            got = [band.push(full), band.push(full)]
            want = [[min(v >> shift, (1 << 22) - 1) for v in first], [min(steady >> shift, (1 << 22) - 1)] * 27]
            for g, w in zip(got, want):
                assert [int(v) for v in g[0]] == w and [int(v) for v in g[1]] == w, (model.__name__, shift)
        assert steady >> 26 > (1 << 22) - 1 > steady >> 27 and first[0] >> 26 < (1 << 22) - 1     # both sides of the clamp are met


# ---- the tail ----

def test_the_tail():
    rng = np.random.default_rng(13)
    taps = rng.integers(-128, 128, size=(64, 2)).astype(np.int8)
    C_ = 2
    q0, q1 = random_hops(rng, C_, True), random_hops(rng, C_, False)
    for model in (wb.PingBand, bc.HostPingBand):
        whole = model(C_, taps, 24).push(np.concatenate([q0, q1], axis=1))
        band = model(C_, taps, 24)
        assert not band.tail.any()
        parts = np.concatenate([band.push(q0), band.push(q1)], axis=1)
        assert np.array_equal(parts, whole) and whole.max() < (1 << 22) - 1
        assert np.array_equal(band.tail, q1[:, -63:, :])
        # reset() zeroes it: the next push is a stream's first
        band.reset()
        assert not band.tail.any()
        assert np.array_equal(band.push(q1), model(C_, taps, 24).push(q1))
        assert not np.array_equal(band.push(q1)[:, 0], model(C_, taps, 24).push(q1)[:, 0])     # ... and with a tail it is not


def test_pings_takes_energies():
    rng = np.random.default_rng(17)
    q = random_hops(rng, 2, False)
    E = wb.ping_blocks(q)
    a, b = wb.Pings(2), wb.Pings(2)
    assert a.push(q, 100.0).tobytes() == b.push(None, 100.0, energies=E).tobytes() and np.array_equal(b.energies, E)


# ---- sensitivity, deterministic ----

@pytest.fixture(scope="module")
def sens():
    hops = pc.scene_model_hops(bc.SENS_SNR, bc.SENS_SEED)
    taps, shift = wb.ping_band_taps()
    return hops, pc.model_run(hops), bc.banded_run(hops, taps, shift)


def test_the_band_sees_what_the_whole_channel_does_not(sens):
    hops, (_, up_e, ev_e), (rec_f, up_f, ev_f, _) = sens
    n = up_f.shape[1]
    for c, start, frames in pc.SCENE_PINGS:
        inside, far = pc.scene_blocks(c, n)
        assert inside.sum() >= frames * pc.FRAME // wb.PING_BLOCK - 2
        print(f"ch={c}: band {int(up_f[c][inside].sum())} of {int(inside.sum())} blocks inside up, whole channel {int(up_e[c][inside].sum())}")
        assert np.all(up_f[c][inside]), f"band: ch={c} blocks {np.flatnonzero(inside & ~up_f[c])} inside the ping are not up"
        assert not np.any(up_f[c][far]), f"band: ch={c} blocks {np.flatnonzero(far & up_f[c])} away from the ping are up"
    for c in pc.SCENE_NOISE_CHANNELS:
        assert not up_f[c].any(), f"band: noise channel {c} has blocks {np.flatnonzero(up_f[c])} up"
    assert sorted(e["channel"] for e in ev_f if e["blocks"] >= 9) == sorted(c for c, _, _ in pc.SCENE_PINGS)
    # the whole-channel detector at 2.0 has no event of a frame's length on either ping channel
    ping_channels = [c for c, _, _ in pc.SCENE_PINGS]
    assert not [e for e in ev_e if e["channel"] in ping_channels and e["blocks"] >= 9], ev_e


def test_the_capture_follows_the_band():
    hops = pc.scene_model_hops(bc.CAPTURE_SNR, bc.SENS_SEED)
    rec_e, up_e, _ = pc.model_run(hops)
    rec_f, up_f, _, _ = bc.banded_run(hops, *wb.ping_band_taps())
    assert not up_e.any(), "the whole-channel detector is meant to see nothing here"
    kept = {}
    for name, records in (("band", rec_f), ("plain", rec_e)):
        cap = wb.Capture(len(pc.SCENE_OFFSETS))
        units = []
        for i, r in enumerate(records):
            u, total = cap.push(r, first=i == 0)
            assert total == len(u)
            units += [(int(c), int(k)) for c, k in zip(u["channel"], u["hop"])]
        kept[name] = set(units)
    assert not kept["plain"]
    for c, start, frames in pc.SCENE_PINGS:
        ping_hops = set(range((start + pc.DELAY + pc.EDGE) // wb.HOP_OUT, (start + frames * pc.FRAME - 1) // wb.HOP_OUT + 1))
        assert len(ping_hops) >= 2 and {(c, k) for k in ping_hops} <= kept["band"], f"ch={c}: hops {ping_hops} of the ping, kept {sorted(kept['band'])}"
    assert {c for c, _ in kept["band"]} == {c for c, _, _ in pc.SCENE_PINGS}, "a noise channel is kept"
