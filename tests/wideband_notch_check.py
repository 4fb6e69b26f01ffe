"""What the tests of the notch share (CPU: test_wideband_notch_model.py, test_wideband_notch_cli.py; GPU: test_gpu_wideband_notch.py): the ctypes view of the C++
design, checks, response, filter, option parser and planner in libmsk144host.so (csrc/wideband.h, host/wideband_cli.h), tables of taps,
and the comparison of a device push with wideband.Notch.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import wideband_check as wc
from msk144cudecoder_amd import wideband as wb


@functools.lru_cache(maxsize=None)
def host():
    L = C.CDLL(wb.HOST_LIB)
    vp, i32 = C.c_void_p, C.c_int32
    L.msk144host_wideband_notch_design.argtypes, L.msk144host_wideband_notch_design.restype = [vp, i32, i32, vp, vp, C.c_char_p, C.c_int], C.c_int
    L.msk144host_wideband_notch_check.argtypes, L.msk144host_wideband_notch_check.restype = [i32, C.c_char_p, C.c_int], C.c_int
    L.msk144host_wideband_notch_response.argtypes, L.msk144host_wideband_notch_response.restype = [vp, i32, C.c_double], C.c_double
    L.msk144host_wideband_notch_filter.argtypes, L.msk144host_wideband_notch_filter.restype = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp], C.c_int
    L.msk144host_wideband_notch_parse.argtypes, L.msk144host_wideband_notch_parse.restype = [C.c_char_p, vp, C.c_int, vp], C.c_int
    L.msk144host_wideband_notch_planner_new.argtypes, L.msk144host_wideband_notch_planner_new.restype = [C.c_int, C.c_double, i32, i32, i32], vp
    L.msk144host_wideband_notch_planner_free.argtypes, L.msk144host_wideband_notch_planner_free.restype = [vp], None
    L.msk144host_wideband_notch_planner_push.argtypes, L.msk144host_wideband_notch_planner_push.restype = [vp, vp, vp, vp, vp, C.c_int], C.c_int
    L.msk144host_wideband_notch_line.argtypes, L.msk144host_wideband_notch_line.restype = [i32, i32, C.c_double, i32, C.c_int64, C.c_char_p, C.c_int], None
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_design(freqs, halfwidth_hz: int = 100):
    """(taps int8 [64][2], shift) of the C++ design, or the refusal text."""
    f = np.asarray(freqs, dtype=np.int32).reshape(-1)
    taps, shift, why = np.zeros((64, 2), dtype=np.int8), np.zeros(1, dtype=np.int32), C.create_string_buffer(256)
    rc = host().msk144host_wideband_notch_design(_p(f), len(f), halfwidth_hz, _p(taps), _p(shift), why, len(why))
    return (taps, int(shift[0])) if rc == 0 else why.value.decode()


def host_check(shift: int) -> str:
    why = C.create_string_buffer(256)
    return "" if host().msk144host_wideband_notch_check(shift, why, len(why)) == 0 else why.value.decode()


def response_db(taps, shift: int, f_hz) -> np.ndarray:
    """10 log10 |H(f)|^2 of the stage (csrc/wideband.h notch_response) at every f_hz."""
    t = np.ascontiguousarray(taps, dtype=np.int8)
    return np.array([10.0 * np.log10(max(host().msk144host_wideband_notch_response(_p(t), shift, float(f)), 1e-300)) for f in np.atleast_1d(f_hz)])


class HostNotch:
    """The C++ filter (csrc/wideband.h notch_filter) over channels, every channel with an entry: taps [channels][64][2], shifts."""

    def __init__(self, taps, shifts):
        self.taps = np.ascontiguousarray(taps, dtype=np.int8)
        self.shifts = np.ascontiguousarray(shifts, dtype=np.int32)
        self.channels = len(self.shifts)
        self.tail = np.zeros((self.channels, 63, 2), dtype=np.int8)

    def push(self, q):
        q = np.ascontiguousarray(q, dtype=np.int8)
        y, clipped = np.zeros_like(q), np.zeros(self.channels, dtype=np.int32)
        assert host().msk144host_wideband_notch_filter(_p(self.taps), _p(self.shifts), self.channels, _p(q), q.shape[1], _p(self.tail), _p(y), _p(clipped)) == 0
        return y, clipped.astype(np.int64)


def host_parse(arg: str):
    """None when the program refuses --wideband-notch=arg; else dict(auto, halfwidth, db, period, persist, table {channel: [Hz, ...]})."""
    out, db = np.zeros(4 + 4 * 64, dtype=np.int32), np.zeros(1, dtype=np.float64)
    n = host().msk144host_wideband_notch_parse(arg.encode(), _p(out), len(out), _p(db))
    if n < 0:
        return None
    table = {int(out[4 + 4 * i]): [int(v) for v in out[6 + 4 * i:6 + 4 * i + int(out[5 + 4 * i])]] for i in range(n)}
    return dict(auto=bool(out[0]), halfwidth=int(out[1]), db=float(db[0]), period=int(out[2]), persist=int(out[3]), table=table)


class HostPlanner:
    """The C++ planner (csrc/wideband.h NotchPlanner) with the interface of wideband.NotchPlanner."""

    def __init__(self, channels: int, db: float = 10.0, period: int = 23, persist: int = 2, halfwidth_hz: int = 100):
        self.channels = channels
        self.p = host().msk144host_wideband_notch_planner_new(channels, db, period, persist, halfwidth_hz)
        assert self.p

    def __del__(self):
        if getattr(self, "p", None):
            host().msk144host_wideband_notch_planner_free(self.p)

    def push(self, sums) -> list:
        s = np.ascontiguousarray(sums, dtype=np.float64)
        ch, hz, ex = np.zeros(self.channels, dtype=np.int32), np.zeros(self.channels, dtype=np.int32), np.zeros(self.channels, dtype=np.float64)
        n = host().msk144host_wideband_notch_planner_push(self.p, _p(s), _p(ch), _p(hz), _p(ex), self.channels)
        return [(int(ch[i]), int(hz[i]), float(ex[i])) for i in range(n)]


def host_line(channel: int, hz: int, excess_db: float, offset_hz: int, hop: int) -> str:
    buf = C.create_string_buffer(256)
    host().msk144host_wideband_notch_line(channel, hz, excess_db, offset_hz, hop, buf, len(buf))
    return buf.value.decode()


def random_taps(seed: int) -> np.ndarray:
    """Random int8 taps [64][2] with -128 in both components: the tap that a packing (br, -bi) cannot hold."""
    taps = np.random.default_rng([91, seed]).integers(-128, 128, size=(64, 2)).astype(np.int8)
    taps[[3, 40], 1] = -128
    taps[[8, 63], 0] = -128
    return taps


def delta(k, re=1, im=0) -> np.ndarray:
    t = np.zeros((64, 2), dtype=np.int8)
    t[k] = (re, im)
    return t


def assert_push(a, b, model: wb.Notch, what: str):
    """The last push of handle a (the notch on) equals the model fed handle b's hops (the same stream, no notch), byte for byte, and
    a's stats equal the model's table and counts.  Returns (a's hops, b's hops, clipped)."""
    raw = np.stack([b.dump_wideband_hop(c) for c in range(b.channels)])
    want, clipped = model.push(raw)
    got = np.stack([a.dump_wideband_hop(c) for c in range(a.channels)])
    bad = np.argwhere(got != want)
    assert got.dtype == np.int8 and bad.size == 0, f"{what}: {len(bad)} components differ, first at (channel, sample, rail) {bad[:4].tolist()}: got {[int(got[tuple(i)]) for i in bad[:4]]}, want {[int(want[tuple(i)]) for i in bad[:4]]}"
    if model.table:
        st = a.wideband_notch_stats()
        assert list(st["on"]) == [1 if c in model.table else 0 for c in range(a.channels)], what
        assert list(st["clipped"]) == [int(v) for v in clipped], f"{what}: clipped {list(st['clipped'])}, want {list(clipped)}"
    return got, raw, clipped


# ---- the decode scene: pings under two carriers per channel ----

# 240 ksps cs16, eight channels 28 kHz apart, three pushes.  Every channel carries one +6 dB ping of 5 frames near its offset, noise of
# about SCENE_NOISE_LSB per rail at the quantiser, and two steady tones of about SCENE_TONE_LSB each, 1000 Hz apart and inside
# +-1200 Hz: the carriers of the CPU simulation behind the stage.  The decoder searches +-100 Hz in steps of 2 Hz.
SCENE_RATE = 240000
SCENE_OFFSETS = np.array([-98000 + 28000 * i for i in range(8)], dtype=np.int32)
SCENE_PUSHES = 3
SCENE_GAIN = 100.0
SCENE_NOISE_LSB = 8.0
SCENE_TONE_LSB = 50.0
SCENE_SNR = 6.0
SCENE_SEED = 1
SCENE_CFG = dict(center=0.0, width=200.0, step=2.0, depth=6, nbadsync_threshold=1)
SCENE_DECODE_ARGS = ["--search-width=200", "--search-step=2", "--scan-depth=6", "--nbadsync-threshold=1", "--print-bits"]


@functools.lru_cache(maxsize=None)
def decode_scene(seed: int = SCENE_SEED):
    """(raw cs16 components of the three pushes in one array, {channel: planted 77-bit message}, {channel: [Hz, Hz]} the notch table).
    The tones sit within +-40 Hz of the table's frequencies, as a carrier found at 125 Hz resolution would."""
    import pack77
    from msk144cudecoder_amd import synth
    rng = np.random.default_rng([77, seed])
    n_out = wb.FIRST_OUT + (SCENE_PUSHES - 1) * wb.HOP_OUT
    unit = 128.0 * SCENE_GAIN
    sigma = SCENE_NOISE_LSB / (unit * float(np.linalg.norm(wb.default_taps_for_rate(SCENE_RATE))))
    planted, pings, table, tones = {}, [], {}, []
    for c, f_c in enumerate(SCENE_OFFSETS):
        msg = pack77.pack_standard("CQ", "K%d%sZ" % (c, "ABCDEFGH"[c]), "FN42")
        start = 700 + int(rng.integers(0, n_out - 5 * 864 - 1400))
        pings.append((int(f_c), synth.Ping(msg, start, 5, float(rng.uniform(-60, 60)), SCENE_SNR, float(rng.uniform(0, 6)))))
        planted[c] = bytes(np.asarray(msg, dtype=np.uint8))
        f1 = int(rng.integers(-1200, 201))
        table[c] = [f1, f1 + 1000]
        tones += [(int(f_c) + f + float(rng.uniform(-40, 40)), float(rng.uniform(0, 2 * np.pi))) for f in table[c]]
    x = wb.read_samples(wb.synth_wideband(n_out, SCENE_RATE, pings, sigma, rng, "cs16"), "cs16")
    n = np.arange(len(x), dtype=np.float64)
    for f, ph in tones:
        x = x + (SCENE_TONE_LSB / unit) * np.exp(1j * (2.0 * np.pi * f * n / SCENE_RATE + ph))
    raw = wb.write_samples(x, "cs16")
    raw.setflags(write=False)
    return raw, planted, table


def scene_parts(seed: int = SCENE_SEED):
    return wc.split_pushes(decode_scene(seed)[0], SCENE_RATE, SCENE_PUSHES)


def scene_model_hops(seed: int = SCENE_SEED, notched: bool = True):
    """int8 [channel][10368][2]: the scene through wideband.Channeliser and, with `notched`, wideband.Notch with the scene's table."""
    m = wb.Channeliser(SCENE_RATE, SCENE_OFFSETS, gain=SCENE_GAIN)
    notch = wb.Notch(len(SCENE_OFFSETS), decode_scene(seed)[2] if notched else None)
    hops = []
    for i, part in enumerate(scene_parts(seed)):
        q, _ = m.push(wb.read_samples(part, "cs16"), first=i == 0)
        hops.append(notch.push(q)[0])
    return np.concatenate(hops, axis=1)


def oracle_decodes(hops, seed: int = SCENE_SEED):
    """The channels whose planted message the oracle decodes from hops [channel][M][2] on that channel."""
    from oracle import oracle_cli
    planted = decode_scene(seed)[1]
    got = []
    for c, msg in planted.items():
        pay = set()
        oracle_cli.decode_stream(hops[c].reshape(-1), SCENE_CFG, read_mode=2, payloads=pay)
        if "".join(str(int(b)) for b in msg) in pay:
            got.append(c)
    return got
