"""What the tests of the ping band share (CPU: test_wideband_pingband_model.py, test_wideband_pingband_cli.py; GPU:
test_gpu_wideband_pingband.py): the ctypes view of the C++ filter and design in libmsk144host.so, the sensitivity scene, a run of
the models with the band ahead of the rule, and the comparison of a device push with them.

The sensitivity scene is the scene of wideband_pings_check.py, seed and all, at SENS_SNR = +6 dB instead of +10 dB.  The SNR was fixed
after the float64 model alone met the conditions test_wideband_pingband_model.py asserts: with the default band (0 +- 1500 Hz) at its
default ratio 3.25 every block wholly inside each ping is up (the lowest Ef / R among them is 3.44) and nothing else is (the highest
Ef / R elsewhere is 2.08), while the whole-channel detector at its default ratio 2.0 has 38 scattered blocks up and no event longer
than 4 blocks.

The capture follows single up blocks, not events, and the model has no SNR at which the band sees every block of these pings while
the whole-channel detector sees none at all (at +5.5 dB it still has 13 blocks up, at +5 dB the band misses blocks).  So the capture
test takes the same scene at CAPTURE_SNR = +3 dB: there the whole-channel detector has no block up on any channel and keeps nothing,
and the band, with 38 % of the inside blocks up, has at least one in every hop of either ping and keeps them all.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import wideband_pings_check as pc
from msk144cudecoder_amd import wideband as wb

SENS_SNR = 6.0
CAPTURE_SNR = 3.0
SENS_SEED = pc.SCENE_SEED


@functools.lru_cache(maxsize=None)
def host():
    L = C.CDLL(wb.HOST_LIB)
    vp, i32 = C.c_void_p, C.c_int32
    L.msk144host_wideband_ping_band_design.argtypes, L.msk144host_wideband_ping_band_design.restype = [i32, i32, vp, vp, C.c_char_p, C.c_int], C.c_int
    L.msk144host_wideband_ping_band_check.argtypes, L.msk144host_wideband_ping_band_check.restype = [i32, C.c_char_p, C.c_int], C.c_int
    L.msk144host_wideband_ping_band_energies.argtypes, L.msk144host_wideband_ping_band_energies.restype = [vp, i32, C.c_int, vp, C.c_int, vp, vp], C.c_int
    L.msk144host_wideband_ping_band_parse.argtypes, L.msk144host_wideband_ping_band_parse.restype = [C.c_char_p, i32, vp], C.c_int
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_design(centre_hz: int, halfwidth_hz: int):
    """(taps int8 [64][2], shift) of the C++ design, or the refusal text."""
    taps, shift, why = np.zeros((64, 2), dtype=np.int8), np.zeros(1, dtype=np.int32), C.create_string_buffer(256)
    rc = host().msk144host_wideband_ping_band_design(centre_hz, halfwidth_hz, _p(taps), _p(shift), why, len(why))
    return (taps, int(shift[0])) if rc == 0 else why.value.decode()


def host_check(shift: int) -> str:
    why = C.create_string_buffer(256)
    return "" if host().msk144host_wideband_ping_band_check(shift, why, len(why)) == 0 else why.value.decode()


def host_parse(arg: str, centre_default: int = 0):
    """(halfwidth, centre) as the program parses --wideband-pings-band=arg, None when it refuses it."""
    out = np.zeros(2, dtype=np.int32)
    return tuple(int(v) for v in out) if host().msk144host_wideband_ping_band_parse(arg.encode(), centre_default, _p(out)) == 0 else None


class HostPingBand:
    """The C++ filter (csrc/wideband.h ping_band_energies) with the interface of wideband.PingBand."""

    def __init__(self, channels: int, taps, shift: int):
        self.taps = np.zeros((64, 2), dtype=np.int8)
        t = np.asarray(taps, dtype=np.int8)
        self.taps[:len(t)] = t
        self.shift, self.channels = int(shift), int(channels)
        self.reset()

    def reset(self):
        self.tail = np.zeros((self.channels, 63, 2), dtype=np.int8)

    def push(self, q) -> np.ndarray:
        q = np.ascontiguousarray(q, dtype=np.int8)
        M = q.shape[1]
        out = np.zeros((self.channels, M // wb.PING_BLOCK), dtype=np.int32)
        assert host().msk144host_wideband_ping_band_energies(_p(self.taps), self.shift, self.channels, _p(q), M, _p(self.tail), _p(out)) == 0
        return out.astype(np.int64)


def response_db(taps, f_hz) -> np.ndarray:
    """10 log10 |B(f)|^2 of integer taps [64][2], B(f) = sum b[k] e^{-j 2 pi f k / 12000}."""
    b = taps[:, 0].astype(np.float64) + 1j * taps[:, 1].astype(np.float64)
    k = np.arange(len(b))
    B = np.exp(-2j * np.pi * np.outer(np.atleast_1d(f_hz).astype(np.float64), k) / wb.OUT_RATE) @ b
    return 10.0 * np.log10(np.maximum(np.abs(B) ** 2, 1e-300))


def banded_run(hops, taps, shift, scales=pc.SCENE_GAIN, min_blocks: int = wb.PING_MIN_BLOCKS, **params):
    """As wideband_pings_check.model_run with the band ahead of the rule: (records, up [channel][all blocks], events, Ef per push).
    The ratio defaults to the band's."""
    params.setdefault("ratio_q4", wb.PING_BAND_RATIO_Q4)
    band = wb.PingBand(hops[0].shape[0], taps, shift)
    det = wb.Pings(hops[0].shape[0], **params)
    ev = wb.PingEvents(min_blocks)
    records, events, energies = [], [], []
    for q in hops:
        energies.append(band.push(q))
        records.append(det.push(None, scales, energies=energies[-1]))
        events += ev.push(records[-1], det.energies)
    events += ev.close()
    return records, pc.up_matrix(records), events, energies


def assert_push(d, band: wb.PingBand, det: wb.Pings, what: str):
    """The last push of handle d, made with the band on, equals the models fed d's own hops and scales, byte for byte: every channel's
    Ef against PingBand, the records against Pings on those energies.  Returns (records, energies, hops)."""
    hops = np.stack([d.dump_wideband_hop(c) for c in range(d.channels)])
    Ef = band.push(hops)
    want = det.push(None, d.wideband_levels()["gain"], energies=Ef)
    every = d.wideband_ping_blocks()
    bad = np.argwhere(every != Ef)
    assert every.dtype == np.int32 and bad.size == 0, f"{what}: Ef differs at (channel, block) {bad[:6].tolist()}: got {[int(every[c, b]) for c, b in bad[:6]]}, want {[int(Ef[c, b]) for c, b in bad[:6]]}"
    got = d.wideband_pings()
    for name in wb.PING_DTYPE.names:
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, f"{what}: {name} differs on channels {bad[:8]}: got {got[name][bad[:8]]}, want {want[name][bad[:8]]}"
    assert got.tobytes() == want.tobytes(), what
    for c in (0, d.channels - 1):
        assert np.array_equal(d.wideband_ping_blocks(c), Ef[c]), f"{what}: block energies of ch={c}"
    return got, every, hops
