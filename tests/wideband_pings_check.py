"""What the tests of the wideband ping detector share (CPU: test_wideband_pings_model.py, test_wideband_pings_cli.py; GPU:
test_gpu_wideband_pings.py): the ctypes view of the C++ rule and tracker in libmsk144host.so, the planted scene, the burst streams
of the shape tests, and the comparison of a device push with the Python model.

The scene.  240 ksps cs16, five channels 48 kHz apart, noise at about SCENE_LSB = 20 LSB rms per component behind gain 100, and two
+10 dB pings: five frames on channel 1 that end 22 blocks into the second push (that push's lower quartile is then a ping block:
only the memory keeps the ping visible), and three frames on channel 3 that start 200 samples before the boundary between the third
and the fourth push.  Channels 0, 2 and 4 carry noise alone.  The seed was fixed after the float64 model alone met the conditions
test_wideband_pings_model.py asserts; the default ratio 2.0 leaves white noise some 3 dB of margin (include/msk144hip.h).

A ping that starts at output sample s and lasts n samples shows in the channel from s + DELAY on, DELAY = 8 samples being the
channel filter's group delay (320 taps at 240 ksps, decimation 20); the filter's transition smears each edge over another 8.
"inside" below is [s + 16, s + n], "near" is [s, s + n + 16].
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import List

import numpy as np

import pack77
import wideband_check as wc
from msk144cudecoder_amd import synth
from msk144cudecoder_amd import wideband as wb

EVENT_DTYPE = np.dtype([("channel", "<i4"), ("_pad", "<i4"), ("start", "<i8"), ("blocks", "<i8"), ("peak", "<i4"), ("reference", "<i4")])
assert EVENT_DTYPE.itemsize == 32


@functools.lru_cache(maxsize=None)
def host():
    L = C.CDLL(wb.HOST_LIB)
    vp, i32 = C.c_void_p, C.c_int32
    L.msk144host_wideband_ping_check.argtypes, L.msk144host_wideband_ping_check.restype = [vp, C.c_char_p, C.c_int], C.c_int
    L.msk144host_wideband_ping_rank.argtypes, L.msk144host_wideband_ping_rank.restype = [C.c_int], C.c_int
    L.msk144host_wideband_ping_up.argtypes, L.msk144host_wideband_ping_up.restype = [i32, i32, i32], C.c_int
    L.msk144host_wideband_ping_new.argtypes, L.msk144host_wideband_ping_new.restype = [C.c_int, vp], vp
    L.msk144host_wideband_ping_free.argtypes, L.msk144host_wideband_ping_free.restype = [vp], None
    L.msk144host_wideband_ping_push.argtypes, L.msk144host_wideband_ping_push.restype = [vp, C.c_int, vp, vp, C.c_int, vp], None
    L.msk144host_wideband_ping_tracker_new.argtypes, L.msk144host_wideband_ping_tracker_new.restype = [C.c_int, C.c_int], vp
    L.msk144host_wideband_ping_tracker_free.argtypes, L.msk144host_wideband_ping_tracker_free.restype = [vp], None
    L.msk144host_wideband_ping_tracker_push.argtypes, L.msk144host_wideband_ping_tracker_push.restype = [vp, vp, vp, vp, C.c_int], C.c_int
    L.msk144host_wideband_ping_tracker_close.argtypes, L.msk144host_wideband_ping_tracker_close.restype = [vp, vp, C.c_int], C.c_int
    L.msk144host_wideband_ping_tracker_counts.argtypes, L.msk144host_wideband_ping_tracker_counts.restype = [vp, vp], None
    L.msk144host_wideband_ping_line.argtypes, L.msk144host_wideband_ping_line.restype = [vp, i32, C.c_char_p, C.c_int], None
    L.msk144host_wideband_pings_parse.argtypes, L.msk144host_wideband_pings_parse.restype = [C.c_char_p, vp], C.c_int
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_check(**params) -> str:
    """'' when msk144_set_wideband_pings takes the parameters (the defaults where not given), else the refusal text."""
    p = np.array([dict(wb.PINGS_DEFAULTS, **params)[k] for k in ("ratio_q4", "memory", "min_ref")], dtype=np.int32)
    why = C.create_string_buffer(256)
    return "" if host().msk144host_wideband_ping_check(_p(p), why, len(why)) == 0 else why.value.decode()


def host_parse(arg: str):
    """(ratio_q4, min_blocks, memory, len(FILE)) as the program parses --wideband-pings=arg, None when it refuses it."""
    out = np.zeros(4, dtype=np.int32)
    return tuple(int(v) for v in out) if host().msk144host_wideband_pings_parse(arg.encode(), _p(out)) == 0 else None


def padded(energies) -> np.ndarray:
    """int32 [channel][54] from E [channel][nb]."""
    e = np.asarray(energies)
    out = np.zeros((e.shape[0], wb.PING_MAX_BLOCKS), dtype=np.int32)
    out[:, :e.shape[1]] = e
    return out


class HostPings:
    """The C++ rule (csrc/wideband.h ping_record, the functions the kernel runs) with the interface of wideband.Pings, fed E."""

    def __init__(self, channels: int, **params):
        p = np.array([dict(wb.PINGS_DEFAULTS, **params)[k] for k in ("ratio_q4", "memory", "min_ref")], dtype=np.int32)
        self.channels = channels
        self.m = host().msk144host_wideband_ping_new(channels, _p(p))
        assert self.m, "parameters refused"
        self.restart = True

    def reset(self):
        self.restart = True

    def push_energies(self, energies, scales) -> np.ndarray:
        e = padded(energies)
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scales, dtype=np.float32), (self.channels,)))
        out = np.zeros(self.channels, dtype=wb.PING_DTYPE)
        host().msk144host_wideband_ping_push(self.m, 1 if self.restart else 0, _p(sc), _p(e), np.asarray(energies).shape[1], _p(out))
        self.restart = False
        return out

    def __del__(self):
        if getattr(self, "m", None):
            host().msk144host_wideband_ping_free(self.m)
            self.m = None


def _events(a, n) -> List[dict]:
    return [dict(channel=int(r["channel"]), start=int(r["start"]), blocks=int(r["blocks"]), peak=int(r["peak"]), reference=int(r["reference"])) for r in a[:n]]


class HostTracker:
    """The C++ event tracker (csrc/wideband.h PingTracker, the one the program runs) with the interface of wideband.PingEvents."""
    CAP = 4096

    def __init__(self, channels: int, min_blocks: int = wb.PING_MIN_BLOCKS):
        self.t = host().msk144host_wideband_ping_tracker_new(channels, min_blocks)
        assert self.t, "parameters refused"

    def push(self, records, energies) -> List[dict]:
        out = np.zeros(self.CAP, dtype=EVENT_DTYPE)
        rec = np.ascontiguousarray(records)
        e = padded(energies)
        n = host().msk144host_wideband_ping_tracker_push(self.t, _p(rec), _p(e), _p(out), self.CAP)
        assert n <= self.CAP
        return _events(out, n)

    def close(self) -> List[dict]:
        out = np.zeros(self.CAP, dtype=EVENT_DTYPE)
        n = host().msk144host_wideband_ping_tracker_close(self.t, _p(out), self.CAP)
        assert n <= self.CAP
        return _events(out, n)

    def counts(self):
        """(events, up blocks, total blocks)"""
        out = np.zeros(3, dtype=np.int64)
        host().msk144host_wideband_ping_tracker_counts(self.t, _p(out))
        return tuple(int(v) for v in out)

    def __del__(self):
        if getattr(self, "t", None):
            host().msk144host_wideband_ping_tracker_free(self.t)
            self.t = None


def host_line(event: dict, offset_hz: int) -> str:
    e = np.zeros(1, dtype=EVENT_DTYPE)
    for k in ("channel", "start", "blocks", "peak", "reference"):
        e[k] = event[k]
    buf = C.create_string_buffer(256)
    host().msk144host_wideband_ping_line(_p(e), int(offset_hz), buf, len(buf))
    return buf.value.decode()


def parse_line(line: str) -> dict:
    """The fields of one line of the event log, the numbers as numbers."""
    head, *fields = line.split()
    assert head == "ping", line
    d = dict(f.split("=", 1) for f in fields)
    assert list(d) == ["ch", "offset", "start", "dur", "blocks", "peak", "ref", "peak_db"], line
    return d


# ---- the scene ----

SCENE_RATE = 240000
SCENE_OFFSETS = np.array([-96000, -48000, 0, 48000, 96000], dtype=np.int32)
SCENE_PUSHES = 5
SCENE_GAIN = 100.0
SCENE_LSB = 20.0
SCENE_SEED = 7
DELAY, EDGE = 8, 8
FRAME = 864
# (channel, first output sample, frames)
SCENE_PINGS = ((1, wb.FIRST_OUT + 22 * wb.PING_BLOCK - 5 * FRAME - 24, 5), (3, wb.FIRST_OUT + 2 * wb.HOP_OUT - 200, 3))
SCENE_NOISE_CHANNELS = (0, 2, 4)


@functools.lru_cache(maxsize=None)
def scene(snr_db: float = 10.0, seed: int = SCENE_SEED) -> np.ndarray:
    """Raw cs16 components of the scene, SCENE_PUSHES pushes long."""
    rng = np.random.default_rng(seed)
    sigma = SCENE_LSB / (128.0 * SCENE_GAIN * float(np.linalg.norm(wb.default_taps_for_rate(SCENE_RATE))))
    n_out = wb.FIRST_OUT + (SCENE_PUSHES - 1) * wb.HOP_OUT
    pings = []
    for k, (c, start, frames) in enumerate(SCENE_PINGS):
        msg = pack77.pack_standard("CQ", "K%dAZ" % k, "FN42")
        pings.append((int(SCENE_OFFSETS[c]), synth.Ping(msg, start, frames, float(rng.uniform(-150, 150)), snr_db, float(rng.uniform(0, 6)))))
    return wb.synth_wideband(n_out, SCENE_RATE, pings, sigma, rng, "cs16")


def scene_parts(snr_db: float = 10.0, seed: int = SCENE_SEED) -> List[np.ndarray]:
    return wc.split_pushes(scene(snr_db, seed), SCENE_RATE, SCENE_PUSHES)


@functools.lru_cache(maxsize=None)
def scene_model_hops(snr_db: float = 10.0, seed: int = SCENE_SEED) -> tuple:
    """int8 hops [C][M][2] of every push of the scene through the float64 channeliser model."""
    m = wb.Channeliser(SCENE_RATE, SCENE_OFFSETS, gain=SCENE_GAIN)
    return tuple(m.push(wb.read_samples(part, "cs16"), first=i == 0)[0] for i, part in enumerate(scene_parts(snr_db, seed)))


def model_run(hops, scales=SCENE_GAIN, min_blocks: int = wb.PING_MIN_BLOCKS, **params):
    """(records of every push, up [channel][all blocks] bool, events) of a stream of pushes through wideband.Pings and PingEvents."""
    det = wb.Pings(hops[0].shape[0], **params)
    ev = wb.PingEvents(min_blocks)
    records, events = [], []
    for q in hops:
        records.append(det.push(q, scales))
        events += ev.push(records[-1], det.energies)
    events += ev.close()
    return records, up_matrix(records), events


def up_matrix(records) -> np.ndarray:
    rows = []
    for r in records:
        nb = int(r["blocks"][0])
        rows.append(np.array([[(int(m) >> b) & 1 for b in range(nb)] for m in r["up_mask"]], dtype=bool))
    return np.concatenate(rows, axis=1)


def scene_blocks(channel: int, n_blocks: int):
    """(inside, far) bool [n_blocks] for the channel: blocks wholly inside one of its pings, and blocks more than one block away
    from every one of them."""
    lo = np.arange(n_blocks) * wb.PING_BLOCK
    hi = lo + wb.PING_BLOCK
    inside = np.zeros(n_blocks, dtype=bool)
    far = np.ones(n_blocks, dtype=bool)
    for c, start, frames in SCENE_PINGS:
        if c != channel:
            continue
        end = start + frames * FRAME
        inside |= (lo >= start + DELAY + EDGE) & (hi <= end)
        far &= (hi + wb.PING_BLOCK <= start) | (lo - wb.PING_BLOCK >= end + DELAY + EDGE)
    return inside, far


def assert_scene(up, events, what: str):
    """The four conditions of the scene, on up [channel][blocks] and the events."""
    n = up.shape[1]
    for c, start, frames in SCENE_PINGS:
        inside, far = scene_blocks(c, n)
        assert inside.sum() >= frames * FRAME // wb.PING_BLOCK - 2
        assert np.all(up[c][inside]), f"{what}: ch={c} blocks {np.flatnonzero(inside & ~up[c])} inside the ping are not up"
        assert not np.any(up[c][far]), f"{what}: ch={c} blocks {np.flatnonzero(far & up[c])} away from the ping are up"
    for c in SCENE_NOISE_CHANNELS:
        assert not up[c].any(), f"{what}: noise channel {c} has blocks {np.flatnonzero(up[c])} up"
    # the ping across the push boundary is one event
    c, start, frames = SCENE_PINGS[1]
    boundary = (wb.FIRST_OUT + 2 * wb.HOP_OUT) // wb.PING_BLOCK
    assert start < boundary * wb.PING_BLOCK < start + frames * FRAME
    mine = [e for e in events if e["channel"] == c]
    assert len(mine) == 1 and mine[0]["start"] < boundary < mine[0]["start"] + mine[0]["blocks"], f"{what}: {mine}"
    assert [e["channel"] for e in events if e["blocks"] >= 9] == [SCENE_PINGS[0][0], c]


# ---- burst streams of the shape tests ----

BURST_LSB = 15.0          # noise per component in the channels, roughly
BURST_TONE_LSB = 60.0     # amplitude of a burst in its channel
BURST_SIGMA = 0.02        # noise per rail at the input, of full scale: 2.6 cu8 steps
# (which channel by fraction of the channel list, first and last output sample): one burst across the first push's halves and the
# boundary behind it, one inside the third push
BURSTS = ((0.3, 2000, 6000), (0.8, 8100, 9100))
BURST_PUSHES = 4


def burst_gain(rate: int) -> float:
    """The gain that puts BURST_SIGMA of white input noise at about BURST_LSB per component in a 12 kHz channel."""
    return float(np.float32(BURST_LSB / (128.0 * BURST_SIGMA * np.sqrt(12000.0 / rate))))


@functools.lru_cache(maxsize=None)
def _burst_signal(rate: int, offsets: tuple, seed: int) -> np.ndarray:
    P, Q = wb.rate_ratio(rate)
    N = (wb.FIRST_OUT + (BURST_PUSHES - 1) * wb.HOP_OUT) * P // Q
    rng = np.random.default_rng([seed, rate])
    x = (rng.standard_normal(2 * N, dtype=np.float32) * np.float32(BURST_SIGMA)).view(np.complex64)
    amp = BURST_TONE_LSB / (128.0 * burst_gain(rate))
    for frac, m0, m1 in BURSTS:
        f = int(offsets[int(frac * (len(offsets) - 1))])
        n = np.arange(m0 * P // Q, m1 * P // Q, dtype=np.int64)
        x[n] += (amp * np.exp(2j * np.pi * (np.mod(f * n, rate).astype(np.float64) / rate))).astype(np.complex64)
    return x


@functools.lru_cache(maxsize=None)
def burst_parts(rate: int, offsets: tuple, fmt: str, seed: int = 3) -> tuple:
    """Raw pushes (a first push and three later ones) of white noise with the two tone bursts of BURSTS at channel offsets."""
    return tuple(wc.split_pushes(wb.write_samples(_burst_signal(rate, offsets, seed), fmt), rate, BURST_PUSHES))


# ---- a device push against the model ----

def assert_push(d, det: wb.Pings, what: str):
    """The last push of handle d equals the model fed d's own hops and scales, byte for byte: records and every channel's E.
    Returns (records, energies)."""
    hops = np.stack([d.dump_wideband_hop(c) for c in range(d.channels)])
    want = det.push(hops, d.wideband_levels()["gain"])
    got = d.wideband_pings()
    for name in wb.PING_DTYPE.names:
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, f"{what}: {name} differs on channels {bad[:8]}: got {got[name][bad[:8]]}, want {want[name][bad[:8]]}"
    assert got.tobytes() == want.tobytes(), what
    every = d.wideband_ping_blocks()
    assert every.dtype == np.int32 and np.array_equal(every, det.energies), f"{what}: block energies"
    for c in range(d.channels):
        assert np.array_equal(d.wideband_ping_blocks(c), det.energies[c]), f"{what}: block energies of ch={c}"
    return got, every
