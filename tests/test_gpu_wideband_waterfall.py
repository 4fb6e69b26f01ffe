"""-m gpu: the per-channel waterfall of the wideband contract (include/msk144hip.h) against its float64 model, wideband.Waterfall: after
every push the model is fed dump_wideband_hop of every channel, so the channeliser's tolerance never enters, and every row is held
to the contract's bound with u = MSK144_WATERFALL_U (wideband_waterfall_check.py; the u each case needed is printed).

1. Shapes: the three of wideband_levels_check.py (240 ksps x 130 channels; 24 125 sps x 33 channels; 8 Msps x 70 channels over ten
   bands with padded slots), a 1-channel and a 5-channel handle, cu8 and cs16, on the burst stream of wideband_pings_check.py: one
   first push (54 rows, both staging halves) and three later ones (27 rows), under the Hann, an all-ones and a seeded random window;
   the sums are the sequential double sum of the device's own rows, exactly.
2. Extremes through the channeliser: cs16 zeros give rows and sums of exactly 0.0; a gain at which every component clips stays
   within the bound and finite.
3. Axis: a wideband tone at f_c + 1375 Hz reads j = 59 and one at f_c - 2500 Hz j = 28, on the device's own rows.
4. Read-only: two handles, the same stream, the waterfall on one: hops, clip counts, levels, ping records and block energies, the
   input spectrum and decoded records are identical.
5. Switching: every EINVAL / ESTATE case of the contract; `set` in mid-stream takes effect at the next push; msk144_set_wideband
   switches it off; the same stream pushed twice gives the same bytes.
6. The program: msk144hipdecoder --wideband-pings=F1 --wideband-waterfall=F2 on the scene of wideband_pings_check.py writes the
   lines and frequencies wideband.waterfall_line and wideband.PingSpectra make of a Python handle's rows, and its decode lines and
   its ping lines up to the added field are those of a run without the option.
"""
import numpy as np
import pytest

import wideband_gpu as wg
import wideband_levels_check as lc
import wideband_options as wo
import wideband_pings_check as pc
import wideband_waterfall_check as wc
from msk144cudecoder_amd import wideband as wb
from wideband_check import split_pushes
from wideband_options import EINVAL, ESTATE, code_of, shape_of

pytestmark = pytest.mark.gpu

WINDOWS = {"hann": "hann", "ones": np.ones(96), "random": wc.random_window(2)}


@pytest.fixture(scope="module")
def handles(hip):
    """Two handles per channel count, made on first use and kept for the module."""
    with wo.handle_cache(wo.decode_pair(hip)) as get:
        yield get


def model_of(window):
    return wb.Waterfall(None if isinstance(window, str) else window)


# ---- 1. shapes ----

@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
@pytest.mark.parametrize("name", wo.SHAPE_NAMES)
def test_shapes_against_the_model(handles, name, fmt):
    shape = shape_of(name)
    rate, offsets = shape["rate"], shape["offsets"]
    d, _ = handles(len(offsets))
    d.set_wideband(rate, offsets, fmt, taps_per_phase=shape["K"], gain=pc.burst_gain(rate))
    parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), fmt)
    worst = 0.0
    for wname, window in WINDOWS.items():
        d.set_wideband_waterfall(window)
        model = model_of(window)
        for i, part in enumerate(parts):
            d.push_wideband(i % 2, part, first=i == 0)
            rows, need = wc.assert_push(d, model, wc.U, f"{name} {fmt} {wname} push {i}")
            assert rows.shape == (len(offsets), 54 if i == 0 else 27, 96) and rows.any()
            worst = max(worst, need)
    d.synchronize()
    print(f"{name} {fmt}: needed_u = {worst:.3e}")


# ---- 2. extremes through the channeliser ----

def test_all_zero_and_all_clipped_hops(handles):
    d, _ = handles(len(pc.SCENE_OFFSETS))
    sizes = wb.push_sizes_for_rate(2, pc.SCENE_RATE)
    # cs16 zeros are exact zeros behind the filter
    d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16")
    d.set_wideband_waterfall()
    for i, n in enumerate(sizes):
        d.push_wideband(i % 2, np.zeros(n, dtype=np.int16), first=i == 0)
        rows, sums = d.wideband_waterfall(), d.wideband_waterfall_sums()
        assert rows.shape == (d.channels, 54 if i == 0 else 27, 96)
        assert not rows.any() and not sums.any() and not np.signbit(rows).any() and not np.signbit(sums).any()
    # a gain at which every component clips: |I| and |Q| are 127 or 128 everywhere, the largest magnitudes the contract allows
    rng = np.random.default_rng(8)
    worst = 0.0
    for wname, window in WINDOWS.items():
        d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16", gain=1e9)
        d.set_wideband_waterfall(window)
        model = model_of(window)
        for i, n in enumerate(sizes):
            d.push_wideband(i % 2, rng.integers(-3000, 3000, size=n).astype(np.int16), first=i == 0)
            hops = wg.dump_hops(d, range(d.channels)).astype(np.int32)
            assert np.abs(hops).min() >= 127, "not every component is clipped"
            rows, need = wc.assert_push(d, model, wc.U, f"clipped {wname} push {i}")
            assert np.all(np.isfinite(rows)) and np.all(np.isfinite(d.wideband_waterfall_sums()))
            worst = max(worst, need)
    d.synchronize()
    print(f"clipped: needed_u = {worst:.3e}")


# ---- 3. the frequency axis ----

def test_a_tone_reads_its_slot(handles):
    rate, offsets = pc.SCENE_RATE, pc.SCENE_OFFSETS
    d, _ = handles(len(offsets))
    gain = pc.burst_gain(rate)
    n = np.arange(sum(wb.push_sizes_for_rate(3, rate)) // 2, dtype=np.int64)
    rng = np.random.default_rng(31)
    x = (rng.standard_normal(2 * len(n), dtype=np.float32) * np.float32(0.002)).view(np.complex64)
    planted = {1: (1375, 59), 3: (-2500, 28)}
    for c, (df, _) in planted.items():
        f = int(offsets[c]) + df
        x += (60.0 / (128.0 * gain) * np.exp(2j * np.pi * (np.mod(f * n, rate).astype(np.float64) / rate))).astype(np.complex64)
    raw = wb.write_samples(x, "cs16")
    d.set_wideband(rate, offsets, "cs16", gain=gain)
    d.set_wideband_waterfall()
    for i, part in enumerate(split_pushes(raw, rate, 3)):
        d.push_wideband(i % 2, part, first=i == 0)
        rows = d.wideband_waterfall()
        for c, (df, j) in planted.items():
            assert wb.waterfall_hz(j) == df
            # the tone runs through the whole stream; the stream's first block holds the filter's start
            got = list(np.argmax(rows[c], axis=1))[1 if i == 0 else 0:]
            assert got == [j] * len(got), f"push {i} ch={c}: {got}"
    d.synchronize()


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
        d.set_wideband_pings()
        d.set_wideband_spectrum(256)
    a.set_wideband_waterfall()
    H = type(a)
    seen = wo.leaves_unchanged(a, b, parts, reads=(H.wideband_pings, H.wideband_ping_blocks, H.wideband_spectrum), decode=name == "rat")
    assert a.wideband_waterfall().shape == (len(offsets), 27, 96) and a.wideband_waterfall().any()
    if name == "rat":
        assert sum(len(s["records"]) for s in seen) > 0 and planted     # the scene decodes to something
    for d in (a, b):
        d.set_wideband_pings(None)
        d.set_wideband_spectrum(None)


# ---- 5. switching ----

def test_order_and_refusals(hip, handles):
    a, _ = handles(len(pc.SCENE_OFFSETS))
    rate, offsets = pc.SCENE_RATE, pc.SCENE_OFFSETS
    parts = pc.burst_parts(rate, tuple(int(f) for f in offsets), "cs16")
    gain = pc.burst_gain(rate)
    H = hip.HipDecoder
    wo.refuses_outside_wideband_mode(hip, [H.set_wideband_waterfall, lambda f: f.set_wideband_waterfall(None), H.wideband_waterfall, lambda f: f.wideband_waterfall(0),
                                           H.wideband_waterfall_sums])
    a.set_wideband(rate, offsets, "cs16", gain=gain)
    for bad in (np.nan, np.inf, -np.inf):
        w = np.ones(96)
        w[95] = bad
        assert code_of(hip, lambda: a.set_wideband_waterfall(w)) == EINVAL, bad
    a.set_wideband_waterfall(-np.ones(96))                                              # real and finite is all a window must be
    a.set_wideband_waterfall(None)
    wo.unreadable(hip, [a.wideband_waterfall, a.wideband_waterfall_sums])               # before any push
    a.push_wideband(0, parts[0], first=True)
    wo.unreadable(hip, [a.wideband_waterfall, lambda: a.wideband_waterfall(0), a.wideband_waterfall_sums])     # ... and after one made with the waterfall off

    # `set` in mid-stream: the next push has rows; a channel out of range is refused
    a.set_wideband_waterfall(WINDOWS["random"])
    assert code_of(hip, a.wideband_waterfall) == ESTATE
    model = model_of(WINDOWS["random"])
    for i in (1, 2):
        a.push_wideband(i % 2, parts[i], first=False)
        rows, _ = wc.assert_push(a, model, wc.U, f"set in mid-stream, push {i}")
        assert rows.shape == (a.channels, 27, 96)
    assert code_of(hip, lambda: a.wideband_waterfall(a.channels)) == EINVAL and code_of(hip, lambda: a.wideband_waterfall(-2)) == EINVAL
    # ... and once more with another window: the last push's rows stay readable until the next push, which takes the new window
    before = a.wideband_waterfall()
    a.set_wideband_waterfall()
    assert a.wideband_waterfall().tobytes() == before.tobytes()
    a.push_wideband(1, parts[3], first=False)
    wc.assert_push(a, model_of("hann"), wc.U, "set again")

    # the same stream pushed twice gives the same bytes; a hop after a first push leaves no row of the first push behind
    again = wo.same_bytes_twice(a, parts, lambda d: (d.wideband_waterfall(), d.wideband_waterfall_sums(), d.wideband_waterfall(2)))
    assert [r.shape[1] for r, _, _ in again] == [54, 27, 27, 27]

    # switched off: from the next push on there is nothing to read; msk144_set_wideband switches it off as well
    a.set_wideband_waterfall(None)
    a.push_wideband(0, parts[1], first=False)
    wo.unreadable(hip, [a.wideband_waterfall])
    a.set_wideband_waterfall()
    a.set_wideband(rate, offsets, "cs16", gain=gain)
    a.push_wideband(0, parts[0], first=True)
    wo.unreadable(hip, [a.wideband_waterfall, a.wideband_waterfall_sums])
    a.synchronize()


# ---- 6. the program ----

def test_the_program_writes_the_lines_of_the_model(hip, tmp_path):
    parts = pc.scene_parts()
    data = np.concatenate(parts).tobytes()
    pings, wf, plain = str(tmp_path / "pings.txt"), str(tmp_path / "wf.txt"), str(tmp_path / "plain.txt")
    args = [f"--wideband-rate={pc.SCENE_RATE}", "--wideband-format=cs16", "--channel-offsets=" + ",".join(str(int(f)) for f in pc.SCENE_OFFSETS)] + wg.SCENE_DECODE_ARGS
    before, _ = wg.run_program(args + [f"--wideband-pings={plain}"], data)
    lines, err = wg.run_program(args + [f"--wideband-pings={pings}", f"--wideband-waterfall={wf}"], data)
    assert lines == before, "the decode lines differ with the option"
    # a Python handle pushed the same stream: the bytes are the same by the determinism contract
    with hip.HipDecoder(channels=len(pc.SCENE_OFFSETS), **wg.DECODE_CFG) as d:
        d.set_wideband(pc.SCENE_RATE, pc.SCENE_OFFSETS, "cs16")
        d.set_wideband_pings()
        d.set_wideband_waterfall()
        spectra, events, want, freqs, base = wb.PingSpectra(d.channels), wb.PingEvents(), [], [], 0
        full = wb.waterfall_full()
        for i, part in enumerate(parts):
            d.push_wideband(i % 2, part, first=i == 0)
            rec, rows = d.wideband_pings(), d.wideband_waterfall()
            events.push(rec, d.wideband_ping_blocks())
            freqs += spectra.push(rec, rows)
            for c in range(d.channels):
                for b in range(rows.shape[1]):
                    if (int(rec["up_mask"][c]) >> b) & 1:
                        want.append(wb.waterfall_line(c, int(pc.SCENE_OFFSETS[c]), base + b, rows[c][b], full))
            base += rows.shape[1]
        freqs += spectra.close()
    with open(wf) as f:
        got = f.read().splitlines()
    assert got == want and len(want) == events.up_blocks >= 60
    with open(plain) as f:
        plain_lines = f.read().splitlines()
    with open(pings) as f:
        ping_lines = f.read().splitlines()
    print("frequencies", freqs)
    assert len(plain_lines) == len(freqs) >= 2
    assert ping_lines == [f"{l} freq={f}" for l, f in zip(plain_lines, freqs)]
    # the carriers of the scene's pings lie within +-150 Hz of their channel's offset and MSK144's main lobe reaches 1500 Hz to either
    # side of the carrier: the strongest bin of a long event lies inside it (a plausibility check; the comparison above is the exact one)
    long_ones = [int(l.rsplit(" freq=", 1)[1]) for l in ping_lines if int(pc.parse_line(l.rsplit(" freq=", 1)[0])["blocks"]) >= 9]
    assert len(long_ones) == 2 and all(abs(f) <= 1500 for f in long_ones)
    assert f"msk144hipdecoder: wideband waterfall: {len(want)} rows written; " in err
