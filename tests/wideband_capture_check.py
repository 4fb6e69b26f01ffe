"""What the tests of the wideband capture share (CPU: test_wideband_capture_model.py, test_wideband_capture_cli.py; GPU:
test_gpu_wideband_capture.py): the ctypes view of the C++ rule and file rule in libmsk144host.so, the brute-force evaluation of the
contract's W and P, the list of cases a scene must contain, and the planned scene.

Brute force.  From an activity matrix a[channel][hop] the definitions of include/msk144hip.h are evaluated as written - W(k) by
looking back over post hops, P(k) by looking one hop ahead - with no state carried from hop to hop; hop k is then placed in the push
that carries it (W) or the next one (P).  wideband.Capture and the C++ rule are state machines and are held to this.

The planned scene.  240 ksps cs16, eight channels 24 kHz apart, noise at about SCENE_LSB = 10 LSB rms per component behind gain
100, nine hops (eight pushes), pre = 1, post = 2, channel 6 listed.  Activity is planted as bursts of MSK144 frames (constant
envelope) at +20 dB from the wideband synthesiser, each two frames (1728 samples) long from sample 192 of its hop, so that with the
channel filter's 16 samples of delay and smear it ends 656 samples before the hop does; the event across a push boundary is one
burst of three frames from sample 1500 of hop 3.  PLAN lists the active hops per channel:
  channel 0   hop 0             a start in hop 0; its tail (hops 1, 2) expires at hop 3
  channel 1   hop 1             a start in hop 1: hop 0 is its pre-roll, in the same first push
  channel 2   hop 5             a start in a later hop: hop 4 is its pre-roll, from the push before
  channel 3   hops 3 and 4      one event across the boundary between two later pushes
  channel 4   hop 2             a tail that expires (hops 3, 4; hop 5 is not kept)
  channel 5   hops 2 and 4      hop 3 is tail, hop 4 a re-trigger inside the tail
  channel 6   none, listed      every hop is kept
  channel 7   none              nothing is kept
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

HOP_BLOCKS = wb.CAPTURE_HOP_BLOCKS


@functools.lru_cache(maxsize=None)
def host():
    L = C.CDLL(wb.HOST_LIB)
    vp, i32 = C.c_void_p, C.c_int32
    L.msk144host_wideband_capture_parse.argtypes, L.msk144host_wideband_capture_parse.restype = [C.c_char_p, vp], C.c_int
    L.msk144host_wideband_capture_default_max_units.argtypes, L.msk144host_wideband_capture_default_max_units.restype = [C.c_int], C.c_int
    L.msk144host_wideband_capture_new.argtypes, L.msk144host_wideband_capture_new.restype = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int], vp
    L.msk144host_wideband_capture_free.argtypes, L.msk144host_wideband_capture_free.restype = [vp], None
    L.msk144host_wideband_capture_restart.argtypes, L.msk144host_wideband_capture_restart.restype = [vp], None
    L.msk144host_wideband_capture_set_hop.argtypes, L.msk144host_wideband_capture_set_hop.restype = [vp, C.c_int64], None
    L.msk144host_wideband_capture_push.argtypes, L.msk144host_wideband_capture_push.restype = [vp, vp, C.c_int, vp, C.c_int, vp], C.c_int
    L.msk144host_wideband_capture_segments_new.argtypes, L.msk144host_wideband_capture_segments_new.restype = [C.c_char_p, vp, C.c_int], vp
    L.msk144host_wideband_capture_segments_free.argtypes, L.msk144host_wideband_capture_segments_free.restype = [vp], None
    L.msk144host_wideband_capture_segments_push.argtypes, L.msk144host_wideband_capture_segments_push.restype = [vp, vp, vp, C.c_int], C.c_int
    L.msk144host_wideband_capture_segments_close.argtypes, L.msk144host_wideband_capture_segments_close.restype = [vp], C.c_int
    L.msk144host_wideband_capture_segments_locate.argtypes, L.msk144host_wideband_capture_segments_locate.restype = [vp, C.c_int, C.c_int64, C.c_char_p], None
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_parse(arg: str):
    """The fields of --wideband-capture=arg as the program parses it, None when it refuses it."""
    out = np.zeros(24, dtype=np.int32)
    if host().msk144host_wideband_capture_parse(arg.encode(), _p(out)) != 0:
        return None
    return dict(by_pings=bool(out[0]), post=int(out[1]), pre=int(out[2]), dir_len=int(out[3]), channels=[int(v) for v in out[5:5 + out[4]]])


def host_default_max_units(channels: int) -> int:
    return int(host().msk144host_wideband_capture_default_max_units(channels))


class HostCapture:
    """The C++ rule (csrc/wideband.h Capture: capture_step, the function the plan kernel runs) with the interface of wideband.Capture."""

    def __init__(self, channels: int, pre: int = 1, post: int = 1, max_units=None, listed=()):
        self.max_units = wb.capture_default_max_units(channels) if max_units is None else int(max_units)
        l = np.array(list(listed), dtype=np.int32)
        self.m = host().msk144host_wideband_capture_new(channels, pre, post, self.max_units, _p(l), len(l))

    def restart(self):
        host().msk144host_wideband_capture_restart(self.m)

    def set_hop(self, hop: int):
        host().msk144host_wideband_capture_set_hop(self.m, hop)

    def push(self, records, first: bool):
        out = np.zeros(max(self.max_units, 1), dtype=wb.CAPTURE_DTYPE)
        count = C.c_int32()
        rec = None if records is None else np.ascontiguousarray(records)
        total = host().msk144host_wideband_capture_push(self.m, None if rec is None else _p(rec), 1 if first else 0, _p(out), len(out), C.byref(count))
        return out[:count.value].copy(), int(total)

    def __del__(self):
        if getattr(self, "m", None):
            host().msk144host_wideband_capture_free(self.m)
            self.m = None


class HostSegments:
    """The C++ file rule (csrc/wideband.h CaptureSegments, the one the program runs) with the interface of wideband.CaptureSegments."""

    def __init__(self, directory: str, offsets_hz):
        o = np.array(list(offsets_hz), dtype=np.int32)
        self.s = host().msk144host_wideband_capture_segments_new(str(directory).encode(), _p(o), len(o))

    def push(self, units, data):
        u = np.ascontiguousarray(units)
        d = np.ascontiguousarray(data, dtype=np.int8)
        assert host().msk144host_wideband_capture_segments_push(self.s, _p(u), _p(d), len(u)) == 0

    def close(self):
        assert host().msk144host_wideband_capture_segments_close(self.s) == 0

    def locate(self, channel: int, block: int) -> str:
        buf = C.create_string_buffer(96)
        host().msk144host_wideband_capture_segments_locate(self.s, channel, block, buf)
        return buf.value.decode()

    def __del__(self):
        if getattr(self, "s", None):
            host().msk144host_wideband_capture_segments_free(self.s)
            self.s = None


# ---- activity, records, brute force ----

def records_of(active, first: bool, rng=None) -> np.ndarray:
    """PING_DTYPE [channel] of one push whose hops have the activity active[channel][1 or 2]: an active hop gets one up block (a
    random one of its 27 with rng, else its block 26 or 0 by channel parity), an inactive hop none."""
    a = np.asarray(active, dtype=bool)
    rec = np.zeros(a.shape[0], dtype=wb.PING_DTYPE)
    rec["blocks"] = HOP_BLOCKS * a.shape[1]
    assert a.shape[1] == (2 if first else 1)
    for c in range(a.shape[0]):
        mask = 0
        for i in range(a.shape[1]):
            if a[c, i]:
                mask |= 1 << (HOP_BLOCKS * i + (int(rng.integers(HOP_BLOCKS)) if rng is not None else (26 if c % 2 else 0)))
        rec["up_mask"][c] = mask
    return rec


def push_records(activity, rng=None) -> List[np.ndarray]:
    """The records of every push of a stream with activity[channel][hop] (hops 0 and 1 in the first push)."""
    a = np.asarray(activity, dtype=bool)
    return [records_of(a[:, :2], True, rng)] + [records_of(a[:, k:k + 1], False, rng) for k in range(2, a.shape[1])]


def activity_of(records) -> np.ndarray:
    """bool [channel][hop] from the records of every push of a stream."""
    hop = (1 << HOP_BLOCKS) - 1
    cols = []
    for i, r in enumerate(records):
        m = r["up_mask"].astype(np.uint64)
        cols.append((m & np.uint64(hop)) != 0)
        if i == 0:
            cols.append(((m >> np.uint64(HOP_BLOCKS)) & np.uint64(hop)) != 0)
    return np.stack(cols, axis=1)


def W(a, k, post, listed) -> bool:
    return bool(listed or any(a[j] for j in range(max(0, k - post), k + 1)))


def P(a, k, pre, post, listed) -> bool:
    return bool(pre == 1 and not W(a, k, post, listed) and k + 1 < len(a) and a[k + 1])


def brute(activity, pre: int, post: int, listed=(), max_units=None, on=None):
    """[(units, total)] per push from the definitions.  on[hop]: the detector was on in the push that carried the hop (default: all)."""
    a = np.array(activity, dtype=bool)
    if on is not None:
        a &= np.asarray(on, dtype=bool)[None, :]
    C_, K = a.shape
    max_units = wb.capture_default_max_units(C_) if max_units is None else max_units
    carried = lambda k: max(k - 1, 0)           # the push that carries hop k
    pushes = [[] for _ in range(K - 1)]
    for c in range(C_):
        L = c in listed
        for k in range(K):
            if W(a[c], k, post, L):
                tail = not a[c, k] and any(a[c, j] for j in range(max(0, k - post), k))
                pushes[carried(k)].append((c, (wb.CAPTURE_ACTIVE if a[c, k] else 0) | (wb.CAPTURE_LISTED if L else 0) | (wb.CAPTURE_TAIL if tail else 0), k))
            elif P(a[c], k, pre, post, L):
                pushes[carried(k + 1)].append((c, wb.CAPTURE_PRE, k))
    out = []
    for u in pushes:
        u.sort(key=lambda x: (x[0], x[2]))
        out.append((np.array(u[:max_units], dtype=wb.CAPTURE_DTYPE), len(u)))
    return out


def assert_units(got, want, what: str):
    (gu, gt), (wu, wt) = got, want
    assert gt == wt, f"{what}: total {gt}, want {wt}"
    assert gu.dtype == wb.CAPTURE_DTYPE and len(gu) == len(wu), f"{what}: {len(gu)} units, want {len(wu)}"
    for name in wb.CAPTURE_DTYPE.names:
        bad = np.flatnonzero(gu[name] != wu[name])
        assert bad.size == 0, f"{what}: {name} differs at units {bad[:8]}: got {gu[name][bad[:8]]}, want {wu[name][bad[:8]]}"
    assert gu.tobytes() == wu.tobytes(), what


# ---- the cases a scene must contain ----

CASES = ("a start in hop 0", "a start in hop 1", "a later start with pre-roll from the push before", "an event across a push boundary", "a tail that expires",
         "a re-trigger inside a tail", "a silent listed channel")


def cases(up, pre: int, post: int, listed=()) -> set:
    """Which of CASES the up matrix [channel][27 x hops] of a stream holds under (pre, post, listed)."""
    up = np.asarray(up, dtype=bool)
    a = up.reshape(up.shape[0], -1, HOP_BLOCKS).any(axis=2)
    found = set()
    for c in range(a.shape[0]):
        L, K = c in listed, a.shape[1]
        if L and not a[c].any():
            found.add(CASES[6])
        if a[c, 0]:
            found.add(CASES[0])
        if not L and pre and a[c, 1] and not a[c, 0]:
            found.add(CASES[1])
        for k in range(2, K):
            if not L and pre and a[c, k] and not W(a[c], k - 1, post, L):
                found.add(CASES[2])
            if up[c, HOP_BLOCKS * k - 1] and up[c, HOP_BLOCKS * k]:
                found.add(CASES[3])
        for k in range(1, K):
            if not L and W(a[c], k - 1, post, L) and not W(a[c], k, post, L):
                found.add(CASES[4])
            if a[c, k] and not a[c, k - 1] and W(a[c], k - 1, post, False):
                found.add(CASES[5])
    return found


# ---- the planned scene ----

SCENE_RATE = 240000
SCENE_OFFSETS = (-84000 + 24000 * np.arange(8)).astype(np.int32)
SCENE_HOPS = 9
SCENE_PUSHES = SCENE_HOPS - 1
SCENE_GAIN = 100.0
SCENE_LSB = 10.0
SCENE_SNR_DB = 20.0
SCENE_SEED = 11
SCENE_PRE, SCENE_POST, SCENE_LISTED = 1, 2, (6,)
PLAN = {0: (0,), 1: (1,), 2: (5,), 3: (3, 4), 4: (2,), 5: (2, 4), 6: (), 7: ()}
# (channel, first output sample, frames)
SCENE_BURSTS = tuple((c, wb.HOP_OUT * k + 192, 2) for c, hops in PLAN.items() if c != 3 for k in hops) + ((3, wb.HOP_OUT * 3 + 1500, 3),)


def planned_activity() -> np.ndarray:
    a = np.zeros((len(SCENE_OFFSETS), SCENE_HOPS), dtype=bool)
    for c, hops in PLAN.items():
        a[c, list(hops)] = True
    return a


@functools.lru_cache(maxsize=None)
def scene_parts() -> tuple:
    """Raw cs16 pushes of the planned scene."""
    rng = np.random.default_rng(SCENE_SEED)
    sigma = SCENE_LSB / (128.0 * SCENE_GAIN * float(np.linalg.norm(wb.default_taps_for_rate(SCENE_RATE))))
    pings = []
    for k, (c, start, frames) in enumerate(SCENE_BURSTS):
        msg = pack77.pack_standard("CQ", "K%dAZ" % (k % 10), "FN42")
        pings.append((int(SCENE_OFFSETS[c]), synth.Ping(msg, start, frames, float(rng.uniform(-150, 150)), SCENE_SNR_DB, float(rng.uniform(0, 6)))))
    raw = wb.synth_wideband(wb.FIRST_OUT + (SCENE_PUSHES - 1) * wb.HOP_OUT, SCENE_RATE, pings, sigma, rng, "cs16")
    return tuple(wc.split_pushes(raw, SCENE_RATE, SCENE_PUSHES))


def up_matrix(records) -> np.ndarray:
    rows = []
    for r in records:
        nb = int(r["blocks"][0])
        rows.append(np.array([[(int(m) >> b) & 1 for b in range(nb)] for m in r["up_mask"]], dtype=bool))
    return np.concatenate(rows, axis=1)
