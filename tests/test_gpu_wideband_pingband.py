"""-m gpu: the ping band of the wideband contract (include/msk144hip.h, csrc/pingband.hip) against its Python models, byte for byte and
with no tolerance: after every push wideband.PingBand is fed dump_wideband_hop of every channel, wideband.Pings those energies and
wideband_levels()["gain"], and wideband_ping_blocks() and wideband_pings() equal what they give (wideband_pingband_check.assert_push).

1. Shapes: the three of wideband_levels_check.py, a 1-channel and a 5-channel handle, cu8 and cs16, the default band and one with
   random int8 taps: one first push (54 blocks, two staged rows) and three later ones (27 blocks) of noise with two tone bursts.
2. Identity on the device: b[0] = 1 with shift 0 gives the records and energies of a handle without the band; b[63] = 1 gives the E
   of the hops delayed by 63 samples, across the push boundaries.
3. Extremes through the channeliser: cs16 zeros; a gain at which every component clips, with taps of +-127 and shift 0: the clamp.
4. AGC: a step restarts the history and leaves the tail as it is.
5. Read-only: two handles, the same stream, the band on one: hops, clip counts, levels, waterfall rows and decoded records are equal.
6. Switching: every EINVAL case; `set` in mid-stream gives history 0 and a zero tail; (h, NULL) returns to E; msk144_set_wideband
   switches it off; msk144_set_wideband_pings(h, NULL) leaves it configured; the same stream pushed twice gives the same bytes.
7. The program: --wideband-pings=FILE --wideband-pings-band on the sensitivity scene of wideband_pingband_check.py writes exactly the
   events of the models on the device's own hops, prints the decode lines of a run without either option and names the band.
"""
import numpy as np
import pytest

import wideband_gpu as wg
import wideband_levels_check as lc
import wideband_options as wo
import wideband_pingband_check as bc
import wideband_pings_check as pc
from msk144cudecoder_amd import wideband as wb
from wideband_options import EINVAL, code_of, shape_of

pytestmark = pytest.mark.gpu

CLAMP = (1 << 22) - 1


def random_band():
    taps = np.random.default_rng(31).integers(-128, 128, size=(64, 2)).astype(np.int8)
    taps[[3, 40], 1] = -128     # the tap that (br, -bi) cannot hold
    taps[[8, 63], 0] = -128
    return taps, 18


BANDS = {"default": wb.ping_band_taps, "random": random_band}


def delta(k, re=1, im=0):
    t = np.zeros((64, 2), dtype=np.int8)
    t[k] = (re, im)
    return t


@pytest.fixture(scope="module")
def handles(hip):
    """Two handles per channel count, made on first use and kept for the module."""
    with wo.handle_cache(wo.decode_pair(hip)) as get:
        yield get


# ---- 1. shapes ----

@pytest.mark.parametrize("which", list(BANDS))
@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
@pytest.mark.parametrize("name", wo.SHAPE_NAMES)
def test_shapes_against_the_models(handles, name, fmt, which):
    shape = shape_of(name)
    rate, offsets = shape["rate"], shape["offsets"]
    taps, shift = BANDS[which]()
    d, _ = handles(len(offsets))
    d.set_wideband(rate, offsets, fmt, taps_per_phase=shape["K"], gain=pc.burst_gain(rate))
    d.set_wideband_pings(ratio_q4=wb.PING_BAND_RATIO_Q4)
    d.set_wideband_ping_band(taps=taps, shift=shift)
    band, det = wb.PingBand(len(offsets), taps, shift), wb.Pings(len(offsets), ratio_q4=wb.PING_BAND_RATIO_Q4)
    up = 0
    for i, part in enumerate(pc.burst_parts(rate, tuple(int(f) for f in offsets), fmt)):
        d.push_wideband(i % 2, part, first=i == 0)
        rec, Ef, _ = bc.assert_push(d, band, det, f"{name} {fmt} {which} push {i}")
        assert list(rec["blocks"]) == [54 if i == 0 else 27] * len(offsets) and list(rec["history"]) == [i] * len(offsets)
        assert Ef.any() and Ef.max() <= CLAMP
        up += sum(bin(int(m)).count("1") for m in rec["up_mask"])
    d.synchronize()
    print(f"{name} {fmt} {which}: {up} blocks up")
    # the default band is centred on the channel, where the tone bursts sit: they are seen
    assert which != "default" or up > 0


# ---- 2. identity on the device ----

def test_delta_taps_are_the_whole_channel_detector(handles):
    shape = lc.SHAPES["rat"]
    rate, offsets = shape["rate"], shape["offsets"]
    a, b = handles(len(offsets))
    parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), "cu8")
    for d in (a, b):
        d.set_wideband(rate, offsets, "cu8", taps_per_phase=shape["K"], gain=pc.burst_gain(rate))
        d.set_wideband_pings()
    a.set_wideband_ping_band(taps=delta(0), shift=0)
    det = wb.Pings(len(offsets))
    for i, part in enumerate(parts):
        for d in (a, b):
            d.push_wideband(i % 2, part, first=i == 0)
        pc.assert_push(b, det, f"no band, push {i}")
        assert a.wideband_pings().tobytes() == b.wideband_pings().tobytes() and np.array_equal(a.wideband_ping_blocks(), b.wideband_ping_blocks()), f"push {i}"
    # b[0] = j turns every sample: E again; b[63] = 1 delays the stream by 63 samples
    for taps in (delta(0, 0, 1), delta(63)):
        a.set_wideband_ping_band(taps=taps, shift=0)
        band, det = wb.PingBand(len(offsets), taps, 0), wb.Pings(len(offsets))
        stream = [np.zeros((len(offsets), 63, 2), dtype=np.int8)]
        for i, part in enumerate(parts):
            a.push_wideband(i % 2, part, first=i == 0)
            _, Ef, hops = bc.assert_push(a, band, det, f"delta push {i}")
            stream.append(hops)
            if taps[0].any():
                assert np.array_equal(Ef, wb.ping_blocks(hops))
            else:
                whole = np.concatenate(stream, axis=1)
                M = hops.shape[1]
                assert np.array_equal(Ef, wb.ping_blocks(whole[:, whole.shape[1] - M - 63:whole.shape[1] - 63])), f"delayed E, push {i}"
    a.synchronize()
    b.synchronize()


# ---- 3. extremes through the channeliser ----

def test_all_zero_and_all_clipped_hops(handles):
    d, _ = handles(len(pc.SCENE_OFFSETS))
    sizes = wb.push_sizes_for_rate(2, pc.SCENE_RATE)
    taps, shift = wb.ping_band_taps()
    d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16")
    d.set_wideband_pings()
    d.set_wideband_ping_band()
    band, det = wb.PingBand(d.channels, taps, shift), wb.Pings(d.channels)
    for i, n in enumerate(sizes):
        d.push_wideband(i % 2, np.zeros(n, dtype=np.int16), first=i == 0)
        rec, Ef, _ = bc.assert_push(d, band, det, f"zeros push {i}")
        assert not Ef.any() and not rec["up_mask"].any() and list(rec["reference"]) == [96] * d.channels
    # every component clipped, taps of +-127, shift 0: far over the clamp
    rng = np.random.default_rng(8)
    taps = (127 * (2 * rng.integers(0, 2, size=(64, 2)) - 1)).astype(np.int8)
    d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16", gain=1e9)
    d.set_wideband_pings()
    d.set_wideband_ping_band(taps=taps, shift=0)
    band, det = wb.PingBand(d.channels, taps, 0), wb.Pings(d.channels)
    for i, n in enumerate(sizes):
        d.push_wideband(i % 2, rng.integers(-3000, 3000, size=n).astype(np.int16), first=i == 0)
        rec, Ef, hops = bc.assert_push(d, band, det, f"clipped push {i}")
        assert np.abs(hops.astype(np.int32)).min() >= 127, "not every component is clipped"
        assert Ef.min() == CLAMP and list(rec["peak"]) == [CLAMP] * d.channels and list(rec["peak_block"]) == [0] * d.channels and not rec["up_mask"].any()
    d.synchronize()


# ---- 4. AGC ----

def test_an_agc_step_restarts_the_history_and_keeps_the_tail(handles):
    d, _ = handles(len(pc.SCENE_OFFSETS))
    parts, gain = wo.loud_push_stream(5)               # a loud tone on channel 1 through the whole of push 2
    taps, shift = wb.ping_band_taps()
    d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16", gain=gain)
    d.set_wideband_agc()
    d.set_wideband_pings()
    d.set_wideband_ping_band()
    band, det = wb.PingBand(d.channels, taps, shift), wb.Pings(d.channels)
    hist, exps = [], []
    for i, part in enumerate(parts):
        tail = band.tail.copy()
        d.push_wideband(i % 2, part, first=i == 0)
        rec, Ef, hops = bc.assert_push(d, band, det, f"AGC push {i}")
        hist.append([int(v) for v in rec["history"]])
        exps.append([int(v) for v in d.wideband_levels()["exponent"]])
        if i == 3:
            # the push behind the step: a filter that had cleared its tail would give another first block
            cleared = wb.PingBand(d.channels, taps, shift).push(hops)
            assert tail[1].any() and cleared[1, 0] != Ef[1, 0]
    d.synchronize()
    print("exponents", exps, "history", hist)
    assert exps[2][1] == 0 and exps[3][1] == -1 and hist[2][1] == 2 and hist[3][1] == 0
    quiet = [c for c in range(d.channels) if all(e[c] == 0 for e in exps)]
    assert quiet and all([h[c] for h in hist] == list(range(5)) for c in quiet)
    d.set_wideband_agc(None)


# ---- 5. read-only ----

def test_it_changes_nothing(handles):
    shape = lc.SHAPES["rat"]
    rate, offsets, K = shape["rate"], shape["offsets"], shape["K"]
    a, b = handles(len(offsets))
    parts, planted, fmt, gain = wo.rat_scene()
    for d in (a, b):
        d.set_wideband(rate, offsets, fmt, taps_per_phase=K, gain=gain)
        d.set_wideband_pings()
        d.set_wideband_waterfall()
    a.set_wideband_ping_band()
    seen = wo.leaves_unchanged(a, b, parts, reads=(lambda d: d.wideband_waterfall(17),), decode=True)
    assert not np.array_equal(a.wideband_ping_blocks(), b.wideband_ping_blocks())     # the band was on
    assert all(s["reads"][0].any() for s in seen)
    assert sum(len(s["records"]) for s in seen) > 0 and planted     # the scene decodes to something
    for d in (a, b):
        d.set_wideband_waterfall(None)


# ---- 6. switching ----

def test_order_and_refusals(hip, handles):
    a, _ = handles(len(pc.SCENE_OFFSETS))
    rate, offsets = pc.SCENE_RATE, pc.SCENE_OFFSETS
    parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), "cs16")
    gain = pc.burst_gain(rate)
    taps, shift = wb.ping_band_taps()
    C_ = len(offsets)
    wo.refuses_outside_wideband_mode(hip, [hip.HipDecoder.set_wideband_ping_band, lambda f: f.set_wideband_ping_band(None)])
    a.set_wideband(rate, offsets, "cs16", gain=gain)
    for bad in (-1, 41, 1 << 20, -(1 << 31)):
        assert code_of(hip, lambda: a.set_wideband_ping_band(taps=taps, shift=bad)) == EINVAL, bad
    for good in (0, 40):
        a.set_wideband_ping_band(taps=np.full((64, 2), -128, dtype=np.int8), shift=good)
    a.set_wideband_ping_band(None)

    # valid with the detector off, and acts only once it is on: the tail has not moved with the first push, and is zero anyway
    a.set_wideband_ping_band()
    a.push_wideband(0, parts[0], first=True)
    wo.unreadable(hip, [a.wideband_pings])
    a.set_wideband_pings(ratio_q4=wb.PING_BAND_RATIO_Q4)
    band, det = wb.PingBand(C_, taps, shift), wb.Pings(C_, ratio_q4=wb.PING_BAND_RATIO_Q4)
    for i in (1, 2):
        a.push_wideband(i % 2, parts[i], first=False)
        rec, _, _ = bc.assert_push(a, band, det, f"detector set in mid-stream, push {i}")
        assert list(rec["history"]) == [i - 1] * C_
    # `set` in mid-stream: history 0 and a zero tail on the next push
    assert band.tail.any()
    a.set_wideband_ping_band(1000, 1000)
    band, det = wb.PingBand(C_, *wb.ping_band_taps(1000, 1000)), wb.Pings(C_, ratio_q4=wb.PING_BAND_RATIO_Q4)
    a.push_wideband(1, parts[3], first=False)
    rec, _, _ = bc.assert_push(a, band, det, "band set in mid-stream")
    assert list(rec["history"]) == [0] * C_
    # msk144_set_wideband_pings(h, NULL) leaves it configured; the detector's return restarts both
    a.set_wideband_pings(None)
    a.push_wideband(0, parts[1], first=False)
    wo.unreadable(hip, [a.wideband_pings])
    a.set_wideband_pings(ratio_q4=wb.PING_BAND_RATIO_Q4)
    band.reset()
    det.reset()
    a.push_wideband(1, parts[2], first=False)
    rec, _, _ = bc.assert_push(a, band, det, "detector off and on again")
    assert list(rec["history"]) == [0] * C_
    # (h, NULL): E again from the next push, with history 0
    a.set_wideband_ping_band(None)
    det = wb.Pings(C_, ratio_q4=wb.PING_BAND_RATIO_Q4)
    a.push_wideband(0, parts[3], first=False)
    rec, _ = pc.assert_push(a, det, "band off")
    assert list(rec["history"]) == [0] * C_

    # the same stream pushed twice gives the same bytes
    a.set_wideband_ping_band()
    again = wo.same_bytes_twice(a, parts, lambda d: (d.wideband_pings(), d.wideband_ping_blocks()))
    assert [int(r["history"][0]) for r, _ in again] == [0, 1, 2, 3]

    # msk144_set_wideband switches it off
    a.set_wideband(rate, offsets, "cs16", gain=gain)
    a.set_wideband_pings()
    det = wb.Pings(C_)
    a.push_wideband(0, parts[0], first=True)
    pc.assert_push(a, det, "after msk144_set_wideband")
    a.synchronize()


# ---- 7. the program ----

def test_the_program_writes_the_events_of_the_models(hip, tmp_path):
    parts = pc.scene_parts(bc.SENS_SNR, bc.SENS_SEED)
    data = np.concatenate(parts).tobytes()
    path = str(tmp_path / "pings.txt")
    args = [f"--wideband-rate={pc.SCENE_RATE}", "--wideband-format=cs16", "--channel-offsets=" + ",".join(str(int(f)) for f in pc.SCENE_OFFSETS)] + wg.SCENE_DECODE_ARGS
    plain, _ = wg.run_program(args, data)
    lines, err = wg.run_program(args + [f"--wideband-pings={path}", "--wideband-pings-band"], data)
    print(len(plain), "decode lines")
    assert lines == plain, "the decode lines differ with the options"
    with hip.HipDecoder(channels=len(pc.SCENE_OFFSETS), **wg.DECODE_CFG) as d:
        d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16")
        hops, scales = [], []
        for i, part in enumerate(parts):
            d.push_wideband(i % 2, part, first=i == 0)
            hops.append(wg.dump_hops(d, range(d.channels)))
            scales.append(d.wideband_levels()["gain"])
    taps, shift = wb.ping_band_taps()
    band, det, tracker = wb.PingBand(len(pc.SCENE_OFFSETS), taps, shift), wb.Pings(len(pc.SCENE_OFFSETS), ratio_q4=wb.PING_BAND_RATIO_Q4), wb.PingEvents()
    events = []
    for q, s in zip(hops, scales):
        rec = det.push(None, s, energies=band.push(q))
        events += tracker.push(rec, det.energies)
    events += tracker.close()
    with open(path) as f:
        got = [pc.parse_line(l) for l in f.read().splitlines()]
    print("events", events)
    assert len(got) == len(events) >= 2
    for g, e in zip(got, events):
        assert (int(g["ch"]), int(g["offset"]), int(g["blocks"]), int(g["peak"]), int(g["ref"])) == (e["channel"], int(pc.SCENE_OFFSETS[e["channel"]]), e["blocks"], e["peak"], e["reference"])
        assert g["start"] == "%.3f" % (e["start"] * 0.008) and g["dur"] == "%.3f" % (e["blocks"] * 0.008)
    channels = sorted({e["channel"] for e in events})
    assert (f"msk144hipdecoder: wideband pings: {len(events)} events on {len(channels)} of {len(pc.SCENE_OFFSETS)} channels, {tracker.up_blocks} of {tracker.total_blocks} blocks up, "
            f"band 0 +-1500 Hz shift {shift}") in err
