"""What the tests of the wideband gate share (CPU: test_wideband_gate_model.py, test_wideband_gate_cli.py, test_wideband_gate_decode.py;
GPU: test_gpu_wideband_gate.py): the ctypes view of the C++ rule and option parser in libmsk144host.so (csrc/wideband.h Gate,
host/wideband_cli.h), random ping records, the brute-force evaluation of the contract's sentence, and the decode scene.

Brute force.  From the records of a stream the activity a[channel][hop] is the contract's "at least min_up of the hop's 27 blocks
up".  The window of push p (p = 0 is the first push) has hop p + 1 as its newest; it is decoded iff the channel is an always channel
or some hop within newest - hold .. newest is active - with no state carried from push to push.  wideband.Gate and the C++ rule are
state machines and are held to this.

The decode scene.  192 ksps cs16, channels 24 kHz apart (12 kHz when there are sixteen), noise at about SCENE_LSB = 10 LSB rms per
component behind gain 100, +10 dB pings of standard messages (no hashed calls) in three channels at different hops - one of them
across a hop boundary - and one quiet channel that is always decoded.  `python tests/wideband_gate_check.py --report` measures, on
the CPU, what the gate lets in on noise alone and what it keeps of the ungated decodes at falling SNR.
"""
from __future__ import annotations

import ctypes as C
import functools
import re
import sys

import numpy as np

HOP_BLOCKS = 27


def _wb():
    from msk144cudecoder_amd import wideband as wb
    return wb


@functools.lru_cache(maxsize=None)
def host():
    L = C.CDLL(_wb().HOST_LIB)
    vp = C.c_void_p
    L.msk144host_wideband_gate_parse.argtypes, L.msk144host_wideband_gate_parse.restype = [C.c_char_p, vp, C.c_int], C.c_int
    L.msk144host_wideband_gate_new.argtypes, L.msk144host_wideband_gate_new.restype = [C.c_int, C.c_int, C.c_int, C.c_int, vp], vp
    L.msk144host_wideband_gate_free.argtypes, L.msk144host_wideband_gate_free.restype = [vp], None
    L.msk144host_wideband_gate_restart.argtypes, L.msk144host_wideband_gate_restart.restype = [vp], None
    L.msk144host_wideband_gate_push.argtypes, L.msk144host_wideband_gate_push.restype = [vp, vp, C.c_int, vp, C.c_int, vp], C.c_int
    L.msk144host_wideband_gate_check.argtypes, L.msk144host_wideband_gate_check.restype = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p], None
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_parse(arg):
    """The fields of --wideband-gate[=arg] as the program parses it (None: the bare option); None when it refuses it."""
    out = np.zeros(4 + 4096, dtype=np.int32)
    if host().msk144host_wideband_gate_parse(None if arg is None else arg.encode(), _p(out), len(out)) != 0:
        return None
    return dict(hold=int(out[0]), min_up=int(out[1]), max_channels=int(out[2]), always=[int(v) for v in out[4:4 + out[3]]])


def host_check(channels: int, hold: int = 1, min_up: int = 1, max_channels: int = 0) -> str:
    """The text msk144_set_wideband_gate refuses the parameters with (csrc/wideband.h check_gate); empty: it takes them."""
    buf = C.create_string_buffer(128)
    host().msk144host_wideband_gate_check(channels, hold, min_up, max_channels, buf)
    return buf.value.decode()


class HostGate:
    """The C++ rule (csrc/wideband.h Gate: gate_step, the function the plan kernel runs) with the interface of wideband.Gate."""

    def __init__(self, channels: int, hold: int = 1, min_up: int = 1, max_channels=None, always=()):
        self.channels = channels
        flags = np.zeros(channels, dtype=np.uint8)
        flags[[c for c in always if 0 <= c < channels]] = 1
        bad = any(not 0 <= c < channels for c in always)
        self.m = None if bad else host().msk144host_wideband_gate_new(channels, hold, min_up, 0 if max_channels is None else max_channels, _p(flags))

    def restart(self):
        host().msk144host_wideband_gate_restart(self.m)

    def push(self, records, first: bool):
        out = np.zeros(self.channels, dtype=np.int32)
        count = C.c_int32()
        rec = None if records is None else np.ascontiguousarray(records)
        total = host().msk144host_wideband_gate_push(self.m, None if rec is None else _p(rec), 1 if first else 0, _p(out), len(out), C.byref(count))
        return out[:count.value].copy(), int(total)

    def __del__(self):
        if getattr(self, "m", None):
            host().msk144host_wideband_gate_free(self.m)
            self.m = None


# ---- records, activity, brute force ----

def random_records(rng, channels: int, pushes: int, density: float):
    """PING_DTYPE [channel] per push (the first carries two hops): a hop is busy with probability `density`, and a busy hop has
    1, 2, 3, 4, 26 or 27 of its blocks up, at random places - so that min_up = 3 and 27 split the busy hops."""
    wb = _wb()
    out = []
    for p in range(pushes):
        hops = 2 if p == 0 else 1
        rec = np.zeros(channels, dtype=wb.PING_DTYPE)
        rec["blocks"] = HOP_BLOCKS * hops
        for c in range(channels):
            mask = 0
            for i in range(hops):
                if rng.random() < density:
                    n = int(rng.choice([1, 2, 3, 4, 26, 27]))
                    for b in rng.choice(HOP_BLOCKS, size=n, replace=False):
                        mask |= 1 << (HOP_BLOCKS * i + int(b))
            rec["up_mask"][c] = mask
        out.append(rec)
    return out


def hop_activity(records, min_up: int = 1) -> np.ndarray:
    """bool [channel][hop] from the records of every push of a stream (None: the detector was off in that push)."""
    cols = []
    channels = next(len(r) for r in records if r is not None)
    for i, r in enumerate(records):
        for h in range(2 if i == 0 else 1):
            if r is None:
                cols.append(np.zeros(channels, dtype=bool))
            else:
                cols.append(np.array([bin((int(m) >> (HOP_BLOCKS * h)) & ((1 << HOP_BLOCKS) - 1)).count("1") >= min_up for m in r["up_mask"]]))
    return np.stack(cols, axis=1)


def brute(activity, hold: int, always=(), max_channels=None, since_push: int = 0):
    """[(list, total)] per push from the contract's sentence.  since_push: activity in hops carried by earlier pushes counts as none
    (the gate was set, or restarted, ahead of that push)."""
    a = np.asarray(activity, dtype=bool)
    channels, hops = a.shape
    cap = channels if not max_channels else max_channels
    oldest = 0 if since_push == 0 else since_push + 1          # the first hop that counts
    out = []
    for p in range(hops - 1):
        newest = p + 1
        chosen = [c for c in range(channels) if c in always or a[c, max(oldest, newest - hold):newest + 1].any()]
        out.append((np.array(chosen[:cap], dtype=np.int32), len(chosen)))
    return out


def assert_list(got, want, what: str):
    (gl, gt), (wl, wt) = got, want
    assert gt == wt, f"{what}: total {gt}, want {wt}"
    assert np.asarray(gl).dtype == np.int32 and list(gl) == list(wl), f"{what}: list {list(gl)}, want {list(wl)}"


# ---- the decode scene ----

SCENE_RATE = 192000
SCENE_GAIN = 100.0
SCENE_LSB = 10.0
SCENE_SNR_DB = 10.0
SCENE_SEED = 3
SCENE_ALWAYS = (2,)
SCENE_PING_CHANNELS = (1, 4, 6)
SCENE_CFG = dict(center=0.0, width=100.0, step=2.0, depth=6, nbadsync_threshold=1)
SCENE_DECODE_ARGS = ["--search-width=100", "--search-step=2", "--scan-depth=6", "--nbadsync-threshold=1"]
CALLS = ("K1ABC", "W9XYZ", "N0GTE")


def scene_offsets(channels: int) -> np.ndarray:
    step = 24000 if channels <= 8 else 12000
    return (-step * (channels - 1) // 2 // 1000 * 1000 + step * np.arange(channels)).astype(np.int32)


def scene_bursts(hops: int):
    """(channel, first output sample, frames): a ping inside one hop, one across a hop boundary, one inside a later hop."""
    wb = _wb()
    h = [hops // 4, hops // 2, hops - 3]
    return ((SCENE_PING_CHANNELS[0], wb.HOP_OUT * h[0] + 300, 2), (SCENE_PING_CHANNELS[1], wb.HOP_OUT * (h[1] + 1) - 1300, 3), (SCENE_PING_CHANNELS[2], wb.HOP_OUT * h[2] + 400, 2))


@functools.lru_cache(maxsize=None)
def scene_parts(channels: int = 8, hops: int = 12, snr_db: float = SCENE_SNR_DB, seed: int = SCENE_SEED) -> tuple:
    """Raw cs16 pushes of the scene: hops - 1 of them."""
    import pack77
    import wideband_check as wc
    from msk144cudecoder_amd import synth
    wb = _wb()
    rng = np.random.default_rng([41, seed])
    offsets = scene_offsets(channels)
    sigma = SCENE_LSB / (128.0 * SCENE_GAIN * float(np.linalg.norm(wb.default_taps_for_rate(SCENE_RATE))))
    pings = []
    for k, (c, start, frames) in enumerate(scene_bursts(hops)):
        msg = pack77.pack_standard("CQ", CALLS[k], "FN42")
        pings.append((int(offsets[c]), synth.Ping(msg, start, frames, float(rng.uniform(-8, 8)), snr_db, float(rng.uniform(0, 6)))))
    pushes = hops - 1
    raw = wb.synth_wideband(wb.FIRST_OUT + (pushes - 1) * wb.HOP_OUT, SCENE_RATE, pings, sigma, rng, "cs16")
    return tuple(wc.split_pushes(raw, SCENE_RATE, pushes))


def scene_model(channels: int = 8, hops: int = 12, snr_db: float = SCENE_SNR_DB, seed: int = SCENE_SEED, pings=None, band=None):
    """(int8 hops [channel][M][2] of the whole stream, the ping records of every push) through wideband.Channeliser and wideband.Pings
    (pings: its parameters; band: (centre, halfwidth) of wideband.PingBand ahead of it)."""
    wb = _wb()
    m = wb.Channeliser(SCENE_RATE, scene_offsets(channels), gain=SCENE_GAIN)
    det = wb.Pings(channels, **(pings or {}))
    pb = wb.PingBand(channels, *wb.ping_band_taps(*band)) if band else None
    hop_list, records = [], []
    for i, part in enumerate(scene_parts(channels, hops, snr_db, seed)):
        q = m.push(wb.read_samples(part, "cs16"), first=i == 0)[0]
        hop_list.append(q)
        records.append(det.push(q, SCENE_GAIN, energies=pb.push(q)) if pb else det.push(q, SCENE_GAIN))
    return np.concatenate(hop_list, axis=1), records


class OracleWindows:
    """The oracle decoder and the program's host layer over the windows of one channel's int8 stream: accepted(k) the accepted
    candidates of window k (decoded once, whoever asks), lines(decoded) the output lines per window of a run that decodes the windows
    in `decoded` (None: all) and hands every other window to the host layer with no candidates - its SNR tracker sees every window."""

    def __init__(self, stream, cfg=None):
        from oracle import oracle as orc
        from oracle import oracle_cli
        self.orc, self.cli = orc, oracle_cli
        self.o = orc.Oracle(threads=8, **(cfg or SCENE_CFG))
        self.cd = [self.o.frontend_iq(w) for w in oracle_cli.windows_of(np.ascontiguousarray(stream).reshape(-1), 2)]
        self._acc = {}

    def accepted(self, k: int):
        if k not in self._acc:
            items, _ = self.o.decode_window(self.cd[k])
            self._acc[k] = items[items["is_message_present"] == 1]
        return self._acc[k]

    def lines(self, decoded=None):
        H = C.CDLL(self.cli.HOST_SO)
        H.msk144host_table_new.restype = C.c_void_p
        H.msk144host_table_free.argtypes = [C.c_void_p]
        H.msk144host_postprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
        table, snr, out = H.msk144host_table_new(), self.orc.Snr(), []
        for k, cd in enumerate(self.cd):
            s = snr.process(cd)
            acc = self.accepted(k) if decoded is None or k in decoded else []
            arr = (self.cli.Accepted * max(len(acc), 1))()
            for a, it in zip(arr, acc):
                a.f0, a.num_avg, a.nbadsync, a.pattern_idx = float(it["f0"]), int(it["num_avg"]), int(it["nbadsync"]), int(it["pattern_idx"])
                a.bits[:] = [int(b) for b in it["message"]]
            buf = C.create_string_buffer(65536)
            n = H.msk144host_postprocess(table, arr, len(acc), s, 1, buf, len(buf))
            out.append([re.sub(r"date=\d{14}", "date=X", l) for l in buf.value.decode().split("\n")] if n else [])
        H.msk144host_table_free(table)
        return out


def gate_lists(records, hold: int = 1, min_up: int = 1, always=SCENE_ALWAYS, max_channels=None):
    """[(list, total)] of wideband.Gate over the records of a stream."""
    g = _wb().Gate(len(records[0]), hold, min_up, max_channels, always)
    return [g.push(r, i == 0) for i, r in enumerate(records)]


# ---- --report: what the gate lets in on noise, and what it keeps of the ungated decodes (CPU simulation) ----

def report(pushes: int = 40, channels: int = 8):
    wb = _wb()
    print("windows gated in on noise alone (hold 1), share of channel windows; %d channels x %d pushes per cell" % (channels, pushes))
    for band in (None, (0, 1500)):
        for ratio in (2.0, 1.5, 1.3):
            for min_up in (1, 3):
                rng = np.random.default_rng([5, int(ratio * 100), min_up])
                det = wb.Pings(channels, ratio_q4=int(round(16 * ratio)))
                pb = wb.PingBand(channels, *wb.ping_band_taps(*band)) if band else None
                gate = wb.Gate(channels, 1, min_up)
                got = 0
                for i in range(pushes):
                    n = wb.FIRST_OUT if i == 0 else wb.HOP_OUT
                    q = np.clip(np.rint(rng.normal(0.0, SCENE_LSB, size=(channels, n, 2))), -128, 127).astype(np.int8)
                    rec = det.push(q, SCENE_GAIN, energies=pb.push(q)) if pb else det.push(q, SCENE_GAIN)
                    got += gate.push(rec, i == 0)[1]
                print(f"  {'in-band' if band else 'whole channel'} ratio {ratio} min_up {min_up}: {got} of {channels * pushes} ({100.0 * got / (channels * pushes):.1f} %)")
    print("ungated decoded windows of the ping channels kept by the gate (hold 1, min_up 1), 8 channels x 11 pushes, seeds 1..4")
    for name, kw in (("default detector (ratio 2)", {}), ("--wideband-pings-band (+-1500 Hz, ratio 3.25)", dict(pings=dict(ratio_q4=52), band=(0, 1500)))):
        for snr in (6.0, 3.0, 0.0, -3.0):
            kept = have = 0
            for seed in (1, 2, 3, 4):
                hops, records = scene_model(8, 12, snr, seed, **kw)
                lists = gate_lists(records, always=())
                for c in SCENE_PING_CHANNELS:
                    ow = OracleWindows(hops[c])
                    for k in range(len(records)):
                        if len(ow.accepted(k)):
                            have += 1
                            kept += c in lists[k][0]
            print(f"  {name} at {snr:+.0f} dB: {kept} of {have} decoded windows kept")


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if "--report" in sys.argv:
        report()
