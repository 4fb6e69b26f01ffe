"""-m gpu: the ping detector of the wideband contract (include/msk144hip.h) against its Python model, wideband.Pings, byte for byte and
with no tolerance: after every push the model is fed dump_wideband_hop of every channel and wideband_levels()["gain"], and
wideband_pings() and every wideband_ping_blocks(c) equal what it gives (wideband_pings_check.assert_push).

1. Shapes: the three of wideband_levels_check.py (240 ksps x 130 channels; 24 125 sps x 33 channels, Q = 96; 8 Msps x 70 channels
   over ten bands with padded slots), a 1-channel and a 5-channel handle, cu8 and cs16: one first push (54 lanes) and three later
   ones (27 lanes) of noise with two tone bursts; 130, 33, 70, 1 and 5 channels fill no whole workgroup of four waves.
2. Extremes through the channeliser: cs16 zeros give all-zero hops; a gain at which every component clips.
3. AGC: a loud burst forces a step down, and the push after the step reports history 0.
4. Read-only: two handles, the same stream, the detector on one: hops, clip counts, levels and decoded records are identical.
5. Switching: every EINVAL / ESTATE case of the contract; `set` in mid-stream takes effect at the next push with history 0;
   msk144_set_wideband switches the detector off; the same stream pushed twice gives the same bytes.
6. The program: msk144hipdecoder --wideband-pings=FILE on the scene of wideband_pings_check.py writes exactly the events of the
   Python model, and its decode lines are those of a run without the option.
"""
import numpy as np
import pytest

import wideband_gpu as wg
import wideband_levels_check as lc
import wideband_options as wo
import wideband_pings_check as pc
from msk144cudecoder_amd import wideband as wb
from wideband_options import EINVAL, ESTATE, code_of, shape_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles(hip):
    """Two handles per channel count, made on first use and kept for the module."""
    with wo.handle_cache(wo.decode_pair(hip)) as get:
        yield get


# ---- 1. shapes ----

@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
@pytest.mark.parametrize("name", wo.SHAPE_NAMES)
def test_shapes_against_the_model(handles, name, fmt):
    shape = shape_of(name)
    rate, offsets = shape["rate"], shape["offsets"]
    d, _ = handles(len(offsets))
    d.set_wideband(rate, offsets, fmt, taps_per_phase=shape["K"], gain=pc.burst_gain(rate))
    d.set_wideband_pings()
    det, events = wb.Pings(len(offsets)), wb.PingEvents()
    seen, up = [], 0
    for i, part in enumerate(pc.burst_parts(rate, tuple(int(f) for f in offsets), fmt)):
        d.push_wideband(i % 2, part, first=i == 0)
        rec, E = pc.assert_push(d, det, f"{name} {fmt} push {i}")
        assert list(rec["blocks"]) == [54 if i == 0 else 27] * len(offsets) and list(rec["history"]) == [i] * len(offsets)
        seen += events.push(rec, E)
        up += sum(bin(int(m)).count("1") for m in rec["up_mask"])
    seen += events.close()
    d.synchronize()
    # the bursts are seen where they were put: each burst's own channel has an event that covers most of it
    print(f"{name} {fmt}: {up} blocks up, {len(seen)} events")
    for frac, m0, m1 in pc.BURSTS:
        c = int(frac * (len(offsets) - 1))
        mine = [e for e in seen if e["channel"] == c and e["start"] <= m0 // 96 + 2 and e["start"] + e["blocks"] >= m1 // 96 - 2]
        assert mine, f"{name} {fmt}: no event over the burst at samples {m0}..{m1} of ch={c}: {[e for e in seen if e['channel'] == c]}"


# ---- 2. extremes through the channeliser ----

def test_all_zero_and_all_clipped_hops(handles):
    d, _ = handles(len(pc.SCENE_OFFSETS))
    sizes = wb.push_sizes_for_rate(2, pc.SCENE_RATE)
    # cs16 zeros are exact zeros behind the filter
    d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16")
    d.set_wideband_pings()
    det = wb.Pings(d.channels)
    for i, n in enumerate(sizes):
        d.push_wideband(i % 2, np.zeros(n, dtype=np.int16), first=i == 0)
        rec, E = pc.assert_push(d, det, f"zeros push {i}")
        assert not E.any() and not rec["up_mask"].any() and not rec["peak"].any() and not rec["peak_block"].any()
        assert list(rec["reference"]) == [96] * d.channels and list(rec["quiet"]) == [0] * d.channels
    # a gain at which every component clips: |I| and |Q| are 127 or 128 everywhere, E close to the largest value
    rng = np.random.default_rng(8)
    d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16", gain=1e9)
    d.set_wideband_pings()
    det = wb.Pings(d.channels)
    for i, n in enumerate(sizes):
        d.push_wideband(i % 2, rng.integers(-3000, 3000, size=n).astype(np.int16), first=i == 0)
        hops = wg.dump_hops(d, range(d.channels)).astype(np.int32)
        assert np.abs(hops).min() >= 127, "not every component is clipped"
        rec, E = pc.assert_push(d, det, f"clipped push {i}")
        assert E.min() >= 96 * 2 * 127 * 127 and E.max() <= 96 * 2 * 128 * 128 and not rec["up_mask"].any()
    d.synchronize()


# ---- 3. AGC ----

def test_an_agc_step_restarts_the_history(handles):
    d, _ = handles(len(pc.SCENE_OFFSETS))
    parts, gain = wo.loud_push_stream(6)               # a loud tone on channel 1 through the whole of push 2
    d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16", gain=gain)
    d.set_wideband_agc()
    d.set_wideband_pings()
    det = wb.Pings(d.channels)
    hist, exps = [], []
    for i, part in enumerate(parts):
        d.push_wideband(i % 2, part, first=i == 0)
        rec, _ = pc.assert_push(d, det, f"AGC push {i}")
        hist.append([int(v) for v in rec["history"]])
        exps.append([int(v) for v in d.wideband_levels()["exponent"]])
    d.synchronize()
    print("exponents", exps, "history", hist)
    # channel 1 steps down behind push 2: push 3 is quantised with another scale and reports history 0; the step back up after
    # `hold` quiet pushes is not inside these six pushes or restarts it once more - the model decides, the device equals it
    assert exps[2][1] == 0 and exps[3][1] == -1 and hist[2][1] == 2 and hist[3][1] == 0 and hist[4][1] <= 1
    # a channel that never stepped counts on
    quiet = [c for c in range(d.channels) if all(e[c] == 0 for e in exps)]
    assert quiet and all([h[c] for h in hist] == list(range(6)) for c in quiet)
    d.set_wideband_agc(None)


# ---- 4. read-only ----

@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_it_changes_nothing(handles, name):
    shape = lc.SHAPES[name]
    rate, offsets, K = shape["rate"], shape["offsets"], shape["K"]
    a, b = handles(len(offsets))
    if name == "rat":
        parts, planted, fmt, gain = wo.rat_scene()
    else:
        fmt, gain = "cs16", pc.burst_gain(rate)
        parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), fmt)[:2]
    for d in (a, b):
        d.set_wideband(rate, offsets, fmt, taps_per_phase=K, gain=gain)
    a.set_wideband_pings()
    seen = wo.leaves_unchanged(a, b, parts, decode=name == "rat")
    assert list(a.wideband_pings()["blocks"]) == [27] * len(offsets)
    if name == "rat":
        assert sum(len(s["records"]) for s in seen) > 0 and planted     # the scene decodes to something


# ---- 5. switching ----

def test_order_and_refusals(hip, handles):
    a, _ = handles(len(pc.SCENE_OFFSETS))
    rate, offsets = pc.SCENE_RATE, pc.SCENE_OFFSETS
    parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), "cs16")
    gain = pc.burst_gain(rate)
    H = hip.HipDecoder
    wo.refuses_outside_wideband_mode(hip, [H.set_wideband_pings, lambda f: f.set_wideband_pings(None), H.wideband_pings, lambda f: f.wideband_ping_blocks(0)])
    a.set_wideband(rate, offsets, "cs16", gain=gain)
    for bad in (dict(ratio_q4=15), dict(ratio_q4=65536), dict(ratio_q4=-32), dict(memory=-1), dict(memory=17), dict(min_ref=0), dict(min_ref=(1 << 22) + 1), dict(min_ref=-96)):
        assert code_of(hip, lambda: a.set_wideband_pings(**bad)) == EINVAL, bad
    for good in (dict(ratio_q4=16), dict(ratio_q4=65535), dict(memory=0), dict(memory=16), dict(min_ref=1), dict(min_ref=1 << 22)):
        a.set_wideband_pings(**good)
    a.set_wideband_pings(None)
    wo.unreadable(hip, [a.wideband_pings, a.wideband_ping_blocks])                      # before any push
    a.push_wideband(0, parts[0], first=True)
    wo.unreadable(hip, [a.wideband_pings, lambda: a.wideband_ping_blocks(0)])           # ... and after one made with the detector off

    # `set` in mid-stream: the next push has records, with history 0; a channel out of range is refused
    a.set_wideband_pings(ratio_q4=24, memory=3)
    assert code_of(hip, a.wideband_pings) == ESTATE
    det = wb.Pings(a.channels, ratio_q4=24, memory=3)
    for i in (1, 2, 3):
        a.push_wideband(i % 2, parts[i], first=False)
        rec, _ = pc.assert_push(a, det, f"set in mid-stream, push {i}")
        assert list(rec["history"]) == [i - 1] * a.channels
    assert code_of(hip, lambda: a.wideband_ping_blocks(a.channels)) == EINVAL and code_of(hip, lambda: a.wideband_ping_blocks(-2)) == EINVAL
    # ... and once more: the history restarts, the last push's records stay readable until the next push
    before = a.wideband_pings()
    a.set_wideband_pings()
    assert a.wideband_pings().tobytes() == before.tobytes()
    det = wb.Pings(a.channels)
    a.push_wideband(0, parts[3], first=False)
    rec, _ = pc.assert_push(a, det, "set again")
    assert list(rec["history"]) == [0] * a.channels

    # the same stream pushed twice gives the same bytes: a first push clears the history
    again = wo.same_bytes_twice(a, parts, lambda d: (d.wideband_pings(), d.wideband_ping_blocks()))
    assert [int(r["history"][0]) for r, _ in again] == [0, 1, 2, 3]

    # switched off: from the next push on there is nothing to read; msk144_set_wideband switches it off as well
    a.set_wideband_pings(None)
    a.push_wideband(0, parts[1], first=False)
    wo.unreadable(hip, [a.wideband_pings])
    a.set_wideband_pings()
    a.set_wideband(rate, offsets, "cs16", gain=gain)
    a.push_wideband(0, parts[0], first=True)
    wo.unreadable(hip, [a.wideband_pings])
    a.synchronize()


# ---- 6. the program ----

def test_the_program_writes_the_events_of_the_model(hip, tmp_path):
    parts = pc.scene_parts()
    data = np.concatenate(parts).tobytes()
    path = str(tmp_path / "pings.txt")
    args = [f"--wideband-rate={pc.SCENE_RATE}", "--wideband-format=cs16", "--channel-offsets=" + ",".join(str(int(f)) for f in pc.SCENE_OFFSETS)] + wg.SCENE_DECODE_ARGS
    plain, _ = wg.run_program(args, data)
    lines, err = wg.run_program(args + [f"--wideband-pings={path}"], data)
    print(len(plain), "decode lines")
    assert lines == plain, "the decode lines differ with the option"
    # the model on the device's own hops
    with hip.HipDecoder(channels=len(pc.SCENE_OFFSETS), **wg.DECODE_CFG) as d:
        d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16")
        hops, scales = [], []
        for i, part in enumerate(parts):
            d.push_wideband(i % 2, part, first=i == 0)
            hops.append(wg.dump_hops(d, range(d.channels)))
            scales.append(d.wideband_levels()["gain"])
    det, tracker, events = wb.Pings(len(pc.SCENE_OFFSETS)), wb.PingEvents(), []
    records = []
    for q, s in zip(hops, scales):
        records.append(det.push(q, s))
        events += tracker.push(records[-1], det.energies)
    events += tracker.close()
    pc.assert_scene(pc.up_matrix(records), events, "device hops")
    with open(path) as f:
        got = [pc.parse_line(l) for l in f.read().splitlines()]
    print("events", events)
    assert len(got) == len(events) >= 2
    for g, e in zip(got, events):
        assert (int(g["ch"]), int(g["offset"]), int(g["blocks"]), int(g["peak"]), int(g["ref"])) == (e["channel"], int(pc.SCENE_OFFSETS[e["channel"]]), e["blocks"], e["peak"], e["reference"])
        assert g["start"] == "%.3f" % (e["start"] * 0.008) and g["dur"] == "%.3f" % (e["blocks"] * 0.008)
        assert abs(float(g["peak_db"]) - 10.0 * np.log10(e["peak"] / e["reference"])) <= 0.1
    channels = sorted({e["channel"] for e in events})
    assert f"msk144hipdecoder: wideband pings: {len(events)} events on {len(channels)} of {len(pc.SCENE_OFFSETS)} channels, {tracker.up_blocks} of {tracker.total_blocks} blocks up" in err
