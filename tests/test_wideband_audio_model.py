"""The audio of the wideband contract (include/msk144hip.h) on the CPU: the Python model against the host rule, what the default
design does to a tone, and the refusals.

1. wideband.Audio equals msk144host_wideband_audio_push (csrc/wideband.h audio_push) exactly, over a first push, two later ones and a
   restart on two hops: random int8 hops with random taps and phasors; a stream of all -128 with all taps (-128, -128) and all
   phasors (-32768, -32768), at shift 1 - every sample clamps - and at shift 40; the default design on a tone.
2. The default design, measured on the integer model with a tone of amplitude 50 through four hops: a tone inside the band comes
   out at tone + df within 3.5 dB of 256 x 50 - 3.01 dB for the rint of the shift plus the pass-band ripple - and a tone 700 Hz or
   more outside the band edge at least 35 dB below 256 x 50.  Seen here: +0.7 .. +2.4 dB inside the band, 36.1 dB at worst outside
   (the design (-1000, 1250, 1500) with a tone at -5750 Hz; the int8 taps set the floor).  All of this is CPU simulation; no GPU
   measurement stands behind the default half-width, the level 256 or the rejection.
3. The argument rules of the design and of check_audio.
"""
import numpy as np
import pytest

import wideband_audio_check as ac
from msk144cudecoder_amd import wideband as wb

HOP = ac.HOP
DESIGNS = [(0, 1250, 1500), (1500, 1250, 1500), (-1000, 1250, 1500), (0, 3000, 3000)]


def pushes_of(x):
    """(rows, restart) of a stream x [C][5 x 2592][2]: a first push, two later ones, and a restart on the two hops the ring then holds."""
    return [(x[:, :2 * HOP], True), (x[:, 2 * HOP:3 * HOP], False), (x[:, 3 * HOP:4 * HOP], False), (x[:, 3 * HOP:5 * HOP], True)]


def assert_model_is_the_host_rule(channels, taps, phasor, shift, x, what):
    model, host = wb.Audio(channels, taps, phasor, shift), ac.HostAudio(channels, taps, phasor, shift)
    seen = []
    for i, (rows, restart) in enumerate(pushes_of(x)):
        y, c = model.push(rows, restart)
        hy, hc = host.push(rows, restart)
        assert y.dtype == np.int16 and y.shape == rows.shape[:2] and c.shape == (channels, rows.shape[1] // HOP)
        assert np.array_equal(y, hy), f"{what} push {i}: {np.count_nonzero(y != hy)} samples differ"
        assert np.array_equal(c, hc), f"{what} push {i}: clamp counts {c.tolist()} and {hc.tolist()}"
        assert np.array_equal(model.tail, host.tails), f"{what} push {i}: the tails differ"
        seen.append((y, c))
    return seen


# ---- 1. model against host rule ----

@pytest.mark.parametrize("shift", [1, 7, 16, 40])
def test_random_hops_taps_and_phasors(shift):
    rng = np.random.default_rng(100 + shift)
    x = rng.integers(-128, 128, size=(3, 5 * HOP, 2)).astype(np.int8)
    taps = rng.integers(-128, 128, size=(64, 2)).astype(np.int8)
    phasor = rng.integers(-32768, 32768, size=(96, 2)).astype(np.int16)
    seen = assert_model_is_the_host_rule(3, taps, phasor, shift, x, f"random shift {shift}")
    if shift == 16:
        # no trivial case: some samples clamp, most do not
        n = sum(int(c.sum()) for _, c in seen)
        assert 0 < n < 3 * 6 * HOP // 2


def test_the_extreme_set():
    """Re z = 0 and Im z = 2^21 behind the tail, so a = 2^36: the largest |a| the contract allows for but a factor of two."""
    x = np.full((1, 5 * HOP, 2), -128, dtype=np.int8)
    seen = assert_model_is_the_host_rule(1, ac.EXTREME_TAPS, ac.EXTREME_PHASOR, 1, x, "extreme shift 1")
    for y, c in seen:
        assert (c == HOP).all() and (y == 32767).all()                   # every sample clamps, from the first of a zero tail on
    seen = assert_model_is_the_host_rule(1, ac.EXTREME_TAPS, ac.EXTREME_PHASOR, 40, x, "extreme shift 40")
    for y, c in seen:
        assert (c == 0).all() and (y == 0).all()                         # (2^36 + 2^39) >> 40 = 0


def test_a_design_case():
    design = wb.audio_design(0, 1250, 1500)
    x = np.concatenate([ac.tone_hops(300, 50, 5), ac.tone_hops(-700, 127, 5)])
    seen = assert_model_is_the_host_rule(2, *design, x, "design")
    assert all(np.abs(y).max() > 5000 for y, _ in seen)


def test_the_restart_push_is_a_first_push_on_the_window():
    """What the library does at the first push after `set`: the two hops of the ring window from an all-zero tail."""
    rng = np.random.default_rng(7)
    x = rng.integers(-128, 128, size=(2, 5 * HOP, 2)).astype(np.int8)
    design = wb.audio_design()
    a, b = wb.Audio(2, *design), wb.Audio(2, *design)
    for rows, restart in pushes_of(x)[:3]:
        a.push(rows, restart)
    y, c = a.push(x[:, 3 * HOP:5 * HOP], restart=True)
    fy, fc = b.push(x[:, 3 * HOP:5 * HOP], restart=True)
    assert np.array_equal(y, fy) and np.array_equal(c, fc)
    # ... and a continued push differs from it in the first 63 samples only
    cont = wb.Audio(2, *design)
    cont.push(x[:, :3 * HOP], restart=True)
    cy, _ = cont.push(x[:, 3 * HOP:5 * HOP])
    assert np.array_equal(cy[:, 63:], y[:, 63:]) and not np.array_equal(cy[:, :63], y[:, :63])


def test_the_wav_file_rule():
    a = np.array([[0, 1, -1], [32767, -32768, 258]], dtype=np.int16)
    b = wb.wav_bytes(a)
    assert len(b) == 44 + 12 and b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and b[36:40] == b"data"
    le = lambda at, n: int.from_bytes(b[at:at + n], "little")
    assert (le(4, 4), le(16, 4), le(20, 2), le(22, 2), le(24, 4), le(28, 4), le(32, 2), le(34, 2), le(40, 4)) == (36 + 12, 16, 1, 1, 12000, 24000, 2, 16, 12)
    assert b[44:] == a.astype("<i2").tobytes()
    import ctypes as C
    head = C.create_string_buffer(44)
    wb._host_lib().msk144host_wideband_wav_header(C.c_uint32(6), head)
    assert head.raw == b[:44] == wb.wav_header(6)


# ---- 2. the default design ----

@pytest.mark.parametrize("design", DESIGNS)
def test_a_tone_inside_the_band_comes_out_at_the_tone_with_the_level(design):
    centre, halfwidth, tone = design
    params = wb.audio_design(*design)
    worst = [np.inf, -np.inf]
    for df in (0, 300, -300, 1000, -1000):
        y = ac.model_audio(params, ac.tone_hops(centre + df, 50, 4))[HOP:]          # three hops behind the start
        f, _ = ac.strongest_line(y)
        assert abs(f - (tone + df)) <= wb.OUT_RATE / len(y), f"{design} df {df}: the strongest line lies at {f} Hz"
        db = 20 * np.log10(ac.tone_amplitude(y, tone + df) / (ac.LEVEL * 50))
        print(f"{design} df {df:+5d}: {db:+.2f} dB")
        worst = [min(worst[0], db), max(worst[1], db)]
        assert abs(db) <= 3.5, f"{design} df {df}: {db:+.2f} dB from 256 x 50"
    print(f"{design}: {worst[0]:+.2f} .. {worst[1]:+.2f} dB")


@pytest.mark.parametrize("design", DESIGNS)
def test_a_tone_outside_the_band_is_rejected(design):
    centre, halfwidth, tone = design
    params = wb.audio_design(*design)
    cases = [centre + s * (halfwidth + out) for s in (1, -1) for out in (700, 1000, 2000, 3500)]
    cases = [f for f in cases if abs(f) <= 6000]
    assert len(cases) >= 2
    for f_in in cases:
        y = ac.model_audio(params, ac.tone_hops(f_in, 50, 4))[HOP:]
        f, amp = ac.strongest_line(y)
        db = 20 * np.log10(max(amp, 1e-9) / (ac.LEVEL * 50))
        print(f"{design} tone at {f_in:+5d} Hz: {db:.1f} dB, strongest line at {f:.0f} Hz")
        assert db <= -35.0, f"{design}: a tone at {f_in} Hz comes out {db:.1f} dB from 256 x 50"


def test_the_design_is_the_ping_bands_taps_and_the_stated_table():
    for centre, halfwidth, tone in DESIGNS + [(250, 500, 625), (-3000, 3000, 3000)]:
        taps, phasor, shift = wb.audio_design(centre, halfwidth, tone)
        ptaps, pshift = wb.ping_band_taps(centre, halfwidth)
        assert np.array_equal(taps, ptaps)
        t = 2 * np.pi * (tone - centre) * np.arange(96) / 12000
        assert np.abs(phasor[:, 0] - 16384 * np.cos(t)).max() <= 0.5 + 1e-6 and np.abs(phasor[:, 1] - 16384 * np.sin(t)).max() <= 0.5 + 1e-6
        k = np.arange(64)
        B = np.abs(np.sum((taps[:, 0] + 1j * taps[:, 1]) * np.exp(-2j * np.pi * centre * k / 12000)))
        assert shift == int(np.rint(np.log2(B) + 6)) and abs(2 * shift - 12 - pshift) <= 1


# ---- 3. refusals ----

@pytest.mark.parametrize("args, text", [
    ((0, 499, 1500), "half-width"), ((0, 3001, 3000), "half-width"), ((4751, 1250, 1501), "|centre|"), ((-4751, 1250, 1499), "|centre|"),
    ((0, 1250, 1249), "tone"), ((0, 1250, 4751), "tone"), ((0, 1250, 1501), "125"), ((100, 1250, 1500), "125"), ((0, 3000, 2999), "tone"),
])
def test_design_refusals(args, text):
    with pytest.raises(ValueError, match=text.replace("|", r"\|")):
        wb.audio_design(*args)


def test_design_accepts_the_edges():
    for args in [(0, 500, 500), (0, 500, 5500), (4750, 1250, 1250), (-4750, 1250, 4750), (0, 3000, 3000), (125, 1250, 1500), (-3000, 3000, 3000)]:
        taps, phasor, shift = wb.audio_design(*args)
        assert 1 <= shift <= 40 and ac.host_check(shift) == ""


def test_check_audio_and_the_model_refuse_the_same_shifts():
    design = wb.audio_design()
    for shift in (1, 2, 39, 40):
        assert ac.host_check(shift) == ""
        wb.Audio(1, design[0], design[1], shift)
    for shift in (0, -1, 41, 1 << 20):
        assert "1..40" in ac.host_check(shift)
        with pytest.raises(ValueError, match="1..40"):
            wb.Audio(1, design[0], design[1], shift)
    with pytest.raises(ValueError):
        wb.Audio(1, design[0], np.zeros((95, 2)), 5)
    with pytest.raises(ValueError):
        wb.Audio(1, design[0], np.full((96, 2), 40000), 5)
    with pytest.raises(ValueError):
        wb.Audio(1, design[0], design[1], 5).push(np.zeros((1, 96, 2), dtype=np.int8))
