"""What the tests of the wideband per-channel levels, gains and the stepped AGC share (CPU: test_wideband_levels_model.py, GPU:
test_gpu_wideband_levels.py): the three shapes, the tone scenes, the float64 model of a scene run under the Python Agc, and the
settled-state check that both the model and the device are held to.

Shapes (chosen for the kernel's edges, not for a workload):
  int    240 ksps (D = 20), K = 16, C = 130: two workgroups, the second with two channels; waves of 32.  Channels share offsets.
  rat    24 125 sps (P/Q = 193/96: 96 branches add into every channel's counter), C = 33.
  bank   8 Msps, C = 70 over ten bands of seven channels: every band's wave has 25 padding slots.

Tone scenes.  cs16 tones at the channel offsets (multiples of 125 Hz, so the tones repeat every Fs/125 samples and every later
push sees the same tone input), amplitudes spread over SPREAD_DB from the band centre (strongest) to its edges, faint white noise
(NOISE_LSB of a cs16 step per rail, added before rounding), and - where the rate leaves room - channels with no tone at the band
edges, as far from the strongest tones as the band allows.  At 24 125 sps the whole band is 12 kHz wide: every channel sees most
tones and none is silent; silence_then_tones covers silence and the way down there.

Silent channels carry a base gain SILENT_BASE times lower than the others.  cs16 rounds the tone sum to steps of 2^-15, which
leaves every 12 kHz channel of a 240 ksps stream a floor of about 2e-6 rms (0.29 steps x sqrt(12/240)), some 1e-5 at its peaks;
the gain that lifts the tone 60 dB below a 0.25 full-scale one to 8 LSB rms is 128 g 2^e = 8 sqrt(2) / 2.5e-4 = 45000, and
45000 x 1e-5 is about half an LSB.  No single base gain shows both a settled -60 dB tone and an all-zero empty channel in int8;
per-channel base gains are the means the contract gives for just that.

AGC parameters of the scenes: the defaults except hold = 1 and +-8 steps, so that 12 pushes are enough to walk the 60 dB of the
scene and then stay put for at least two pushes.  Base gains differ by channel (BASE_PATTERN), so that channels that share an offset
still take different trajectories.  Where the base gain puts the strongest tones far above full scale the ladder is walked downwards
as well; at 24 125 sps, where a channel holds many tones and its envelope is not constant, every channel starts below the window
(settling from below lands in [8, 16) LSB rms, peaks below 127 for any number of tones that matters).

Settled state (settled_state): from push SETTLED_FROM on no exponent moves; every non-silent channel is inside the window with no
clipped component; silent channels sit at max_exp with all-zero output.  For a single tone this is what the rule predicts: a
constant envelope of at most 32 LSB rms per component peaks at 45 LSB.
"""
from __future__ import annotations

import functools
from typing import Dict, List

import numpy as np

import wideband_check as wc
from msk144cudecoder_amd import wideband as wb

N_PUSHES = 12
SETTLED_FROM = 10                 # pushes 10 and 11 must repeat push 9's exponents
SPREAD_DB = 60.0
NOISE_LSB = 0.12                  # per rail, in cs16 steps
AGC = dict(lo_sq=64, hi_sq=1024, clip_ppm=1000, hold=1, min_exp=-8, max_exp=8)
BASE_PATTERN = (1.0, 2.0, 0.5, 1.0)   # base gain of channel c = g0 x BASE_PATTERN[c % 4]
SILENT_BASE = 2.0 ** -6               # ... times this for a channel without a tone


def _int_shape():
    grid = np.arange(-112000, 112001, 16000)                       # 15 offsets 16 kHz apart within +-(Fs/2 - 6000) = +-114000
    offsets = grid[np.arange(130) % len(grid)]
    return dict(name="int", rate=240000, K=16, offsets=offsets.astype(np.int32), silent_above=100000, a_max=0.25, g0=8.0, stats_gain=128.0)


def _rat_shape():
    offsets = -6000 + 375 * np.arange(33)                           # +-(Fs/2 - 6000) = +-6062
    return dict(name="rat", rate=24125, K=16, offsets=offsets.astype(np.int32), silent_above=None, a_max=0.15, g0=2.0 ** -6, stats_gain=64.0)


def _bank_shape():
    bands = [-31, -20, -9, -2, -1, 0, 1, 7, 18, 30]                 # band width Fs/64 = 125 kHz
    offsets = np.array([k * 125000 + f for k in bands for f in range(-48000, 48001, 16000)])
    return dict(name="bank", rate=8000000, K=16, offsets=offsets.astype(np.int32), silent_above=3500000, a_max=0.08, g0=32.0, stats_gain=512.0)


# g0: the base gain of the AGC scenes; stats_gain: the one gain of the statistics test, at which the strong tones clip heavily
SHAPES: Dict[str, dict] = {s["name"]: s for s in (_int_shape(), _rat_shape(), _bank_shape())}


def base_gains(shape: dict) -> np.ndarray:
    C = len(shape["offsets"])
    g = shape["g0"] * np.asarray(BASE_PATTERN)[np.arange(C) % len(BASE_PATTERN)]
    return np.where(silent_channels(shape), g * SILENT_BASE, g).astype(np.float32)


def silent_channels(shape: dict) -> np.ndarray:
    if shape["silent_above"] is None:
        return np.zeros(len(shape["offsets"]), dtype=bool)
    return np.abs(shape["offsets"]) > shape["silent_above"]


def tone_amplitudes(shape: dict):
    """(distinct tone frequencies, amplitudes): the one nearest the band centre the strongest, SPREAD_DB down to the outermost."""
    f = np.unique(shape["offsets"][~silent_channels(shape)])
    f = f[np.lexsort((f, np.abs(f)))]
    a = shape["a_max"] * 10.0 ** (-SPREAD_DB * np.arange(len(f)) / (len(f) - 1) / 20.0)
    return f, a


@functools.lru_cache(maxsize=None)
def tone_scene(name: str, n_pushes: int = N_PUSHES) -> np.ndarray:
    """Raw cs16 components of the scene, n_pushes pushes long.  Never saturates (asserted)."""
    shape = SHAPES[name]
    rate = shape["rate"]
    P, Q = wb.rate_ratio(rate)
    n = (wb.FIRST_OUT + (n_pushes - 1) * wb.HOP_OUT) * P // Q
    period = rate // 125
    assert n % period == 0
    rng = np.random.default_rng([rate, 60])
    f, a = tone_amplitudes(shape)
    t = np.arange(period, dtype=np.int64)
    x = np.zeros(period, dtype=np.complex128)
    for fk, ak in zip(f, a):
        ph = np.mod(int(fk) * t, rate).astype(np.float64) * (2.0 * np.pi / rate) + rng.uniform(0, 2 * np.pi)
        x += ak * np.exp(1j * ph)
    assert np.abs(x.real).max() < 0.99 and np.abs(x.imag).max() < 0.99
    one = np.empty(2 * period, dtype=np.float32)
    one[0::2], one[1::2] = x.real * 32768.0, x.imag * 32768.0
    v = np.tile(one, n // period)
    v += rng.standard_normal(v.size, dtype=np.float32) * np.float32(NOISE_LSB)
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def scene_parts(name: str, n_pushes: int = N_PUSHES) -> List[np.ndarray]:
    return wc.split_pushes(tone_scene(name, n_pushes), SHAPES[name]["rate"], n_pushes)


def make_model(shape: dict, gain=100.0, offsets=None):
    off = shape["offsets"] if offsets is None else offsets
    cls = wb.TwoStage if wb.is_bank_rate(shape["rate"]) else wb.Channeliser
    return cls(shape["rate"], off, K=shape["K"], gain=gain)


@functools.lru_cache(maxsize=None)
def model_outputs(name: str, n_pushes: int = N_PUSHES) -> tuple:
    """The float64 model's unquantised outputs y [C][M] of every push of the scene (the gains do not enter)."""
    m = make_model(SHAPES[name])
    m.reset()
    return tuple(m.filter(wb.read_samples(part, "cs16")) for part in scene_parts(name, n_pushes))


def model_agc_run(name: str, n_pushes: int = N_PUSHES, **agc):
    """The scene through the model and the Python Agc: (levels of every push, exponents used for every push, hops of the last push)."""
    shape = SHAPES[name]
    a = wb.Agc(len(shape["offsets"]), base_gains(shape), **dict(AGC, **agc))
    lv, used, q = [], [], None
    for y in model_outputs(name, n_pushes):
        used.append(list(a.e))
        q, clipped = wb.quantise(y, a.gains(), per_channel=True)
        lv.append(wb.levels(q, clipped))
        a.step(lv[-1])
    return lv, used, q


# Silence, then the tones, at the rational rate, where the scene itself has no silent channel and nothing steps down: SILENCE_PUSHES
# pushes of digital silence (every one of the 96 branches adds nothing to any counter; every channel climbs to max_exp with all-zero
# output and stays there), then the scene's later pushes, whose tones arrive at 2^8 times the base gain, too loud on every channel and clipped on some, and walk the ladder down.
SILENCE_PUSHES = 10
SILENCE_TONE_PUSHES = 8


def silence_then_tones(name: str = "rat") -> List[np.ndarray]:
    parts = scene_parts(name)
    zeros = [np.zeros_like(parts[0])] + [np.zeros_like(parts[1])] * (SILENCE_PUSHES - 1)
    return zeros + parts[1:1 + SILENCE_TONE_PUSHES]


def silence_then_tones_checks(levels, exponents, hops_of_silence, what: str, agc: dict = AGC):
    """What the model shows (test_wideband_levels_model.py) and the device is held to."""
    e = np.asarray(exponents)
    for i in range(SILENCE_PUSHES):
        assert not levels[i]["sum_sq"].any() and not levels[i]["clipped"].any(), f"{what}: silence counted at push {i}"
        assert np.all(e[i] == min(i, agc["max_exp"])), f"{what}: push {i} of the silence"
        assert not np.asarray(hops_of_silence[i]).any()
    assert levels[SILENCE_PUSHES]["clipped"].max() > 1000, f"{what}: the tones' onset at max_exp clips on no channel"
    assert np.all(e[SILENCE_PUSHES + 1] == agc["max_exp"] - 1) and np.all(np.diff(e[SILENCE_PUSHES:], axis=0) <= 0)
    assert np.any(e[-1] < agc["max_exp"] - 1) and np.array_equal(e[-1], e[-2]), f"{what}: not settled after the way down"
    last = levels[-1]
    assert not last["clipped"].any() and np.all(last["sum_sq"] <= agc["hi_sq"] * 2 * last["samples"]) and np.all(last["sum_sq"] >= agc["lo_sq"] * 2 * last["samples"])


def model_silence_run(name: str = "rat"):
    """silence_then_tones through the model and the Python Agc: (levels, exponents used, hops) of every push."""
    shape = SHAPES[name]
    m = make_model(shape)
    a = wb.Agc(len(shape["offsets"]), base_gains(shape), **AGC)
    lv, used, hops = [], [], []
    for i, part in enumerate(silence_then_tones(name)):
        if i == 0:
            m.reset()
        used.append(list(a.e))
        q, clipped = wb.quantise(m.filter(wb.read_samples(part, "cs16")), a.gains(), per_channel=True)
        lv.append(wb.levels(q, clipped))
        hops.append(q)
        a.step(lv[-1])
    return lv, used, hops


def settled_state(shape: dict, levels, exponents, last_hops, what: str, agc: dict = AGC):
    """levels[i], exponents[i]: records and exponents used of push i; last_hops: int8 [C][M][2] of the last push."""
    silent = silent_channels(shape)
    e = np.asarray(exponents)
    for i in range(SETTLED_FROM, len(e)):
        moved = np.flatnonzero(e[i] != e[SETTLED_FROM - 1])
        assert moved.size == 0, f"{what}: channels {moved[:8]} still step at push {i}"
    for i in range(SETTLED_FROM - 1, len(e)):
        lv = levels[i]
        two_n = 2 * lv["samples"][~silent]
        S = lv["sum_sq"][~silent]
        out = np.flatnonzero((S < agc["lo_sq"] * two_n) | (S > agc["hi_sq"] * two_n))
        assert out.size == 0, f"{what} push {i}: non-silent channels {np.flatnonzero(~silent)[out][:8]} outside the window"
        assert not lv["clipped"][~silent].any(), f"{what} push {i}: clipped components on settled channels"
        assert not lv["sum_sq"][silent].any() and not lv["clipped"][silent].any(), f"{what} push {i}: a silent channel is not silent"
    assert np.all(e[-1][silent] == agc["max_exp"]), f"{what}: silent channels below max_exp"
    assert not np.asarray(last_hops)[silent].any(), f"{what}: silent channels with non-zero output"


# ---- the faint decode scene ----

# 240 ksps cs16: eight channels 28 kHz apart, each with a neighbour 12 kHz above it; +10 dB pings on five of the eight, after
# DECODE_LEAD hops of noise alone in which the default AGC (hold 4) walks up from 0.2 LSB rms at gain 100 to its window: six steps
# of 6 dB, 24 pushes.  cs16, not cu8: a cu8 sample is at least 1/256 of full scale away from zero, which behind a decimation by 20 and
# gain 100 is 11 LSB rms; no cu8 stream leaves a fraction of an LSB at that gain.
DECODE_RATE = 240000
DECODE_OFFSETS = np.array([-98000 + 28000 * i for i in range(8)] + [-98000 + 28000 * i + 12000 for i in range(8)], dtype=np.int32)
DECODE_PINGS = [0, 2, 3, 5, 7]
DECODE_LEAD = 26
DECODE_PUSHES = DECODE_LEAD + 8
DECODE_FIXED_LSB = 0.2            # channel rms per component at gain 100


def decode_scene(seed: int = 240, with_starts: bool = False):
    """(raw cs16 components, {channel: planted 77-bit message}) - wideband_gpu.plant_scene with the pings behind the lead-in and
    the noise at DECODE_FIXED_LSB.  with_starts: also {channel: output sample at which its ping starts}.

    The scene was chosen on the CPU: test_wideband_levels_model.py runs it through the float64 model under the default Agc and has
    the oracle (oracle/oracle_cli.py) decode every planted message from the model's hops."""
    import pack77
    from msk144cudecoder_amd import synth
    rng = np.random.default_rng(seed)
    sigma = DECODE_FIXED_LSB / (128.0 * 100.0 * float(np.linalg.norm(wb.default_taps_for_rate(DECODE_RATE))))
    lead = wb.FIRST_OUT + (DECODE_LEAD - 1) * wb.HOP_OUT
    n_out = wb.FIRST_OUT + (DECODE_PUSHES - 1) * wb.HOP_OUT
    planted, pings = {}, []
    for k, c in enumerate(DECODE_PINGS):
        msg = pack77.pack_standard("CQ", "K%d%sZ" % (k % 10, "ABCDEFGHIJKLMNOPQRSTUVWXY"[k]), "FN42")
        start = lead + 1500 + (k * 2311) % (n_out - lead - 6 * 864 - 3000)
        pings.append((int(DECODE_OFFSETS[c]), synth.Ping(msg, start, 5, float(rng.uniform(-150, 150)), 10.0, float(rng.uniform(0, 6)))))
        planted[c] = bytes(np.asarray(msg, dtype=np.uint8))
    raw = wb.synth_wideband(n_out, DECODE_RATE, pings, sigma, rng, "cs16")
    if with_starts:
        return raw, planted, {c: p.start for c, (_, p) in zip(DECODE_PINGS, pings)}
    return raw, planted
