"""-m gpu: the audio of the wideband contract (include/msk144hip.h) against its integer model, wideband.Audio, with no tolerance.
After every push the model is fed the device's own dump_wideband_hop rows; every unit's audio row and clamp count must equal the
model's for that (channel, hop): zero samples differ.  Rate 240000 throughout, the smallest shape of the wideband tests.

1. Exactness over a first push and three later ones: 1 and 33 channels with the default design - the capture lists at most 16
   channels, so with 33 the 16 listed ones are spread over the range and the detector at a low ratio adds units on the others -
   257 channels with channels 0, 255 and 256 listed and max_units = 4, so that units are dropped and the plan's walk has a second
   chunk; and the extreme tap and phasor sets at shift 1 and 40 on a scene loud enough to clip the int8 stage.
2. Pre-roll: a unit emitted one push late has the audio of the older hop, from the other row of the audio ring.
3. Switch-on in mid-stream: the first push after `set` gives the model restarted on (older hop, newest hop) from a zero tail.
4. States and refusals.
5. It changes nothing: hops, levels, clip counts, ping records and energies, capture units and bytes and decoded records are
   byte-identical with the audio on and off; the same stream twice gives the same bytes.
6. Round trip: the audio rows of a channel with a +10 dB ping, fed to an audio handle (read_mode 1) at centre 1500, decode to the
   payload the wideband handle decoded.
"""
import numpy as np
import pytest

import wideband_audio_check as ac
import wideband_capture_check as cc
import wideband_check as wc
import wideband_gpu as wg
import wideband_options as wo
import wideband_pings_check as pc
from msk144cudecoder_amd import wideband as wb
from wideband_options import EINVAL, ESTATE, code_of

pytestmark = pytest.mark.gpu

RATE = 240000
HOP = wb.HOP_OUT
RATIO_Q4 = 22           # 1.375 x the reference: white noise alone puts a block up now and then


@pytest.fixture(scope="module")
def handles(hip):
    with wo.handle_cache(wo.decode_pair(hip)) as get:
        yield get


def grid_offsets(C):
    grid = np.arange(-112000, 112001, 16000)
    return grid[np.arange(C) % len(grid)].astype(np.int32)


class Follow:
    """The model beside a handle: fed the handle's own hops after every push, it keeps the audio and the clamp count of every
    (hop, channel), and the hops themselves."""

    def __init__(self, d, params, hop=None):
        self.d, self.model, self.audio, self.clamped, self.hops = d, wb.Audio(d.channels, *params), {}, {}, {}
        self.newest = hop          # the newest hop of the stream so far; None: no push yet

    def take(self, first, restart_on=None):
        """After a push: restart_on = the older hop's rows [C][2592][2] when the library restarts in mid-stream."""
        q = wg.dump_hops(self.d, range(self.d.channels))
        if first:
            self.newest, k0, rows = 1, 0, q
        else:
            self.newest += 1
            k0, rows = (self.newest - 1, np.concatenate([restart_on, q], axis=1)) if restart_on is not None else (self.newest, q)
        y, c = self.model.push(rows, restart=first or restart_on is not None)
        for j in range(rows.shape[1] // HOP):
            self.audio[k0 + j], self.clamped[k0 + j], self.hops[k0 + j] = y[:, j * HOP:(j + 1) * HOP], c[:, j], rows[:, j * HOP:(j + 1) * HOP]

    def assert_units(self, what):
        """The capture's units of the last push and their audio: every row is the model's.  Returns (units, clamped, total)."""
        units, data, total = self.d.wideband_capture()
        audio, clamped = self.d.wideband_capture_audio()
        assert audio.shape == (len(units), HOP) and audio.dtype == np.int16 and clamped.shape == (len(units),)
        for u, row, n, iq in zip(units, audio, clamped, data):
            c, k = int(u["channel"]), int(u["hop"])
            assert np.array_equal(iq, self.hops[k][c]), f"{what}: the I/Q of ch={c} hop={k} is not the hop's"
            diff = np.count_nonzero(row != self.audio[k][c])
            assert diff == 0, f"{what}: {diff} audio samples of ch={c} hop={k} differ from the model"
            assert int(n) == int(self.clamped[k][c]), f"{what}: ch={c} hop={k} clamped {n}, the model {self.clamped[k][c]}"
        return units, clamped, total


def run(d, parts, params, what):
    """Push parts with capture and audio set by the caller; hold every push to the model.  Returns [(units, clamped, total)]."""
    f, out = Follow(d, params), []
    for i, part in enumerate(parts):
        d.push_wideband(i % 2, part, first=i == 0)
        f.take(i == 0)
        out.append(f.assert_units(f"{what} push {i}"))
    d.synchronize()
    return out


def all_off(d):
    d.set_wideband_audio(None)
    d.set_wideband_capture(None)
    d.set_wideband_pings(None)


# ---- 1. exactness ----

@pytest.mark.parametrize("C", [1, 33])
def test_the_default_design_against_the_model(handles, C):
    offsets = grid_offsets(C)
    d, _ = handles(C)
    listed = sorted({int(round(f * (C - 1))) for f in np.linspace(0.0, 1.0, 16)})
    d.set_wideband(RATE, offsets, "cs16", gain=pc.burst_gain(RATE))
    d.set_wideband_pings(ratio_q4=RATIO_Q4)
    d.set_wideband_capture(1, 1, 2 * C, listed)
    params = wb.audio_design(0, 1250, 1500)
    d.set_wideband_audio()
    out = run(d, pc.burst_parts(RATE, tuple(int(f) for f in offsets), "cs16"), params, f"{C} channels")
    print(f"{C} channels: units per push {[t for _, _, t in out]}, clamped {[int(c.sum()) for _, c, _ in out]}")
    assert len(out) == 4 and out[0][2] >= 2 * len(listed) and all(t >= len(listed) for _, _, t in out)
    assert all(len(u) == t for u, _, t in out)
    if C > 16:
        assert len({int(c) for u, _, _ in out for c in u["channel"]}) > len(listed), "the detector added no channel"
    all_off(d)


def test_257_channels_with_dropped_units(handles):
    C = 257
    offsets = grid_offsets(C)
    d, _ = handles(C)
    d.set_wideband(RATE, offsets, "cs16", gain=pc.burst_gain(RATE))
    d.set_wideband_capture(0, 0, 4, [0, 255, 256])
    d.set_wideband_audio(250, 1000, 1500)
    out = run(d, pc.burst_parts(RATE, tuple(int(f) for f in offsets), "cs16"), wb.audio_design(250, 1000, 1500), "257 channels")
    assert [(len(u), t) for u, _, t in out] == [(4, 6), (3, 3), (3, 3), (3, 3)]                   # two of the first push's units dropped
    assert [(int(u["channel"]), int(u["hop"])) for u in out[0][0]] == [(0, 0), (0, 1), (255, 0), (255, 1)]
    assert [(int(u["channel"]), int(u["hop"])) for u in out[3][0]] == [(0, 4), (255, 4), (256, 4)]
    all_off(d)


@pytest.mark.parametrize("shift", [1, 40])
def test_the_extreme_set_on_a_clipping_scene(handles, shift):
    C = 33
    offsets = grid_offsets(C)
    d, _ = handles(C)
    listed = list(range(0, 33, 3)) + [32]
    d.set_wideband(RATE, offsets, "cs16", gain=200.0 * pc.burst_gain(RATE))                       # noise at some 3000 LSB: nearly every component clips
    d.set_wideband_capture(0, 0, 2 * C, listed)
    d.set_wideband_audio(taps=ac.EXTREME_TAPS, phasor=ac.EXTREME_PHASOR, shift=shift)
    f, counts = Follow(d, (ac.EXTREME_TAPS, ac.EXTREME_PHASOR, shift)), []
    for i, part in enumerate(pc.burst_parts(RATE, tuple(int(x) for x in offsets), "cs16")):
        d.push_wideband(i % 2, part, first=i == 0)
        f.take(i == 0)
        q = f.hops[f.newest]
        assert np.mean((q == 127) | (q == -128)) > 0.9, "the scene does not clip the int8 stage"
        _, clamped, _ = f.assert_units(f"extreme shift {shift} push {i}")
        counts += [int(n) for n in clamped]
    d.synchronize()
    print(f"shift {shift}: clamped per unit {min(counts)} .. {max(counts)}")
    if shift == 1:
        assert min(counts) > HOP // 2
    else:
        assert max(counts) == 0
    all_off(d)


# ---- 2. pre-roll ----

def test_the_pre_roll_unit_has_the_older_hops_audio(handles):
    d, _ = handles(len(cc.SCENE_OFFSETS))
    d.set_wideband(cc.SCENE_RATE, cc.SCENE_OFFSETS, "cs16", gain=cc.SCENE_GAIN)
    d.set_wideband_pings()
    d.set_wideband_capture(1, 1, None, [])
    d.set_wideband_audio()
    out = run(d, cc.scene_parts(), wb.audio_design(), "pre-roll")
    pre = [(i, int(u["channel"]), int(u["hop"])) for i, (units, _, _) in enumerate(out) for u in units if u["flags"] & wb.CAPTURE_PRE]
    print("pre-roll units (push, channel, hop):", pre)
    # a pre-roll unit of a later push: hop i of push i, which the push before wrote to the other row of the ring
    assert any(i >= 1 and k == i for i, _, k in pre), "no pre-roll unit in a later push"
    all_off(d)


# ---- 3. switch-on in mid-stream ----

def test_switch_on_in_mid_stream(handles):
    d, _ = handles(len(cc.SCENE_OFFSETS))
    parts = cc.scene_parts()
    d.set_wideband(cc.SCENE_RATE, cc.SCENE_OFFSETS, "cs16", gain=cc.SCENE_GAIN)
    d.set_wideband_pings()
    older = None
    for i in range(2):
        d.push_wideband(i % 2, parts[i], first=i == 0)
        older = wg.dump_hops(d, range(d.channels))                # after push 1: hop 2
    # before the push that carries hop 3, where channel 3's event starts: hop 2 is its pre-roll, emitted with hop 3
    d.set_wideband_capture(cc.SCENE_PRE, cc.SCENE_POST, None, cc.SCENE_LISTED)
    d.set_wideband_audio()
    f = Follow(d, wb.audio_design(), hop=2)
    d.push_wideband(0, parts[2], first=False)
    f.take(False, restart_on=older)
    units, _, _ = f.assert_units("switch-on")
    seen = [(int(u["channel"]), int(u["hop"])) for u in units]
    print("units of the switch-on push:", seen)
    assert (3, 2) in seen and (3, 3) in seen, "the push does not emit both hops of a window"
    # the next push continues the tail
    d.push_wideband(1, parts[3], first=False)
    f.take(False)
    assert len(f.assert_units("behind the switch-on")[0]) > 0
    d.synchronize()
    all_off(d)


# ---- 4. states and refusals ----

def test_states_and_refusals(hip, handles):
    H = hip.HipDecoder
    wo.refuses_outside_wideband_mode(hip, [H.set_wideband_audio, lambda f: f.set_wideband_audio(None), H.wideband_capture_audio])
    a, _ = handles(len(cc.SCENE_OFFSETS))
    parts = cc.scene_parts()
    a.set_wideband(cc.SCENE_RATE, cc.SCENE_OFFSETS, "cs16", gain=cc.SCENE_GAIN)
    taps, phasor, _ = wb.audio_design()
    for shift in (0, -1, 41):
        assert code_of(hip, lambda: a.set_wideband_audio(taps=taps, phasor=phasor, shift=shift)) == EINVAL
    a.set_wideband_capture(0, 0, None, [2])
    a.set_wideband_audio()
    wo.unreadable(hip, [a.wideband_capture_audio])                                        # before any push
    a.push_wideband(0, parts[0], first=True)
    audio, clamped = a.wideband_capture_audio()
    assert audio.shape == (2, HOP) and audio.any()
    # a refused `set` changes nothing
    assert code_of(hip, lambda: a.set_wideband_audio(taps=taps, phasor=phasor, shift=41)) == EINVAL
    again = a.wideband_capture_audio()
    assert again[0].tobytes() == audio.tobytes() and again[1].tobytes() == clamped.tobytes()
    # after msk144_set_wideband_capture: wherever msk144_wideband_capture answers MSK144_ESTATE
    a.set_wideband_capture(0, 0, None, [2])
    wo.unreadable(hip, [a.wideband_capture, a.wideband_capture_audio])
    a.push_wideband(1, parts[1], first=False)
    assert a.wideband_capture_audio()[0].shape == (1, HOP)
    # the last push was made with the audio off: the units are there, their audio is not
    a.set_wideband_audio(None)
    a.push_wideband(0, parts[2], first=False)
    assert len(a.wideband_capture()[0]) == 1
    wo.unreadable(hip, [a.wideband_capture_audio])
    # the audio on and the capture off: the ring is written, there is nothing to read
    a.set_wideband_audio()
    a.set_wideband_capture(None)
    a.push_wideband(1, parts[3], first=False)
    wo.unreadable(hip, [a.wideband_capture_audio])
    # a larger max_units with the audio on: the dense rows follow it
    a.set_wideband_capture(0, 0, 64, list(range(a.channels)))
    a.push_wideband(0, parts[4], first=False)
    assert a.wideband_capture_audio()[0].shape == (a.channels, HOP)
    a.synchronize()
    all_off(a)


# ---- 5. it changes nothing ----

def test_it_changes_nothing(handles):
    parts, planted, fmt, gain = wo.rat_scene()
    shape = wo.shape_of("rat")
    a, b = handles(len(shape["offsets"]))
    listed = [3, 17, 30]
    for d in (a, b):
        d.set_wideband(shape["rate"], shape["offsets"], fmt, taps_per_phase=shape["K"], gain=gain)
        d.set_wideband_pings(ratio_q4=RATIO_Q4)
        d.set_wideband_capture(1, 1, None, listed)
    a.set_wideband_audio()
    H = type(a)
    seen = wo.leaves_unchanged(a, b, parts, reads=(H.wideband_pings, H.wideband_ping_blocks, H.wideband_capture), decode=True)
    assert a.wideband_capture_audio()[0].any()
    assert sum(len(s["records"]) for s in seen) > 0 and planted
    assert all(len(s["reads"][2][0]) >= len(listed) for s in seen)
    for d in (a, b):
        all_off(d)


def test_the_same_stream_twice_gives_the_same_bytes(handles):
    d, _ = handles(len(cc.SCENE_OFFSETS))
    d.set_wideband(cc.SCENE_RATE, cc.SCENE_OFFSETS, "cs16", gain=cc.SCENE_GAIN)
    d.set_wideband_pings()
    d.set_wideband_capture(cc.SCENE_PRE, cc.SCENE_POST, None, cc.SCENE_LISTED)
    d.set_wideband_audio()
    wo.same_bytes_twice(d, cc.scene_parts(), lambda h: h.wideband_capture_audio()[0])
    d.synchronize()
    all_off(d)


# ---- 6. round trip ----

ROUND_TRIP_PUSHES = 6
ROUND_TRIP_CHANNEL = 1
ROUND_TRIP_SEED = 2025


def test_round_trip_through_the_audio_front_end(hip, handles):
    """One +10 dB ping (wideband_gpu.plant_scene: five frames from output sample 1500 of channel 1, six pushes, seed 2025) on a
    listed channel; the channel's audio rows, hop after hop, go to an audio handle (read_mode 1, centre 1500, width 500) as windows
    of two hops, and the payload the wideband handle decoded on that channel must be among the audio handle's.  Checked on the CPU
    (simulation, no GPU): the float64 channeliser model's int8 hops of this scene through wideband.Audio with the default design,
    window by window through the reference decoder's audio front end and decode (oracle.Oracle, centre 1500, width 500, step 1,
    depth 6), decode the planted payload in the windows that hold the ping."""
    offsets = pc.SCENE_OFFSETS
    n_out = wb.FIRST_OUT + (ROUND_TRIP_PUSHES - 1) * HOP
    raw, planted = wg.plant_scene(n_out, RATE, offsets, [ROUND_TRIP_CHANNEL], np.random.default_rng(ROUND_TRIP_SEED))
    parts = wc.split_pushes(raw, RATE, ROUND_TRIP_PUSHES)
    d, _ = handles(len(offsets))
    d.set_wideband(RATE, offsets, "cu8", gain=16.0)
    d.set_wideband_capture(0, 0, None, [ROUND_TRIP_CHANNEL])
    d.set_wideband_audio()
    rows, recs, clamped = [], [], 0
    for i, part in enumerate(parts):
        d.push_wideband(i % 2, part, first=i == 0)
        recs.append(wg._decode(d, i % 2))
        audio, n = d.wideband_capture_audio()
        rows += list(audio)
        clamped += int(n.sum())
    all_off(d)
    live = wg.messages_by_channel(recs).get(ROUND_TRIP_CHANNEL, set())
    assert planted[ROUND_TRIP_CHANNEL] in live, "the wideband handle did not decode the planted ping"
    stream = np.concatenate(rows)
    assert stream.shape == (n_out,) and clamped == 0
    got = set()
    with hip.HipDecoder(channels=1, **dict(wg.DECODE_CFG, center=1500.0, read_mode=1)) as audio_handle:
        for k in range(len(rows) - 1):
            audio_handle.submit_audio(stream[k * HOP:k * HOP + 2 * HOP])
            audio_handle.decode()
            audio_handle.synchronize()
            got |= {bytes(np.unpackbits(r["message"])[:77]) for r in audio_handle.results()}
    print(f"live {len(live)} message(s), audio {len(got)}")
    assert live <= got, "a payload the wideband handle decoded is not among the audio handle's"
