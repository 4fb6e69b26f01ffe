"""Audio input at 24 to 192 kHz: the integer model of the resampler in front of the hop ring (include/msk144hip.h, "Audio input at
24 to 192 kHz").

`Resampler` is the contract in int64 numpy - what csrc/resample.hip computes on the device and msk144ir::Resampler on the host - as
wideband.PingBand is for its filter.  The default taps and the configuration rules come from libmsk144host.so (csrc/input_rate.h),
the same integers and the same checks the library and the program use.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Sequence, Tuple

import numpy as np

from .wideband import HOST_LIB, rate_ratio

OUT_RATE = 12000
FIRST_OUT = 5184
HOP_OUT = 2592
MIN_RATE, MAX_RATE = 24000, 192000
DEFAULT_SHIFT = 14
DEFAULT_TAPS_PER_PHASE = 16
BRANCH_SUM_MAX = 65535

_host = None


def _host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise FileNotFoundError(f"{HOST_LIB} not found: build it with `make -C msk144cudecoder_amd/host`")
        L = C.CDLL(HOST_LIB)
        L.msk144host_input_rate_taps.argtypes = [C.c_int64, C.c_int, C.c_void_p]
        L.msk144host_input_rate_taps.restype = C.c_int
        L.msk144host_input_rate_check.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
        L.msk144host_input_rate_check.restype = C.c_int
        L.msk144host_input_rate_new.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int]
        L.msk144host_input_rate_new.restype = C.c_void_p
        L.msk144host_input_rate_push.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.msk144host_input_rate_push.restype = C.c_int
        L.msk144host_input_rate_free.argtypes = [C.c_void_p]
        L.msk144host_input_rate_free.restype = None
        _host = L
    return _host


def row_samples(rate_hz: int) -> int:
    """Input samples of a later hop, 2592 P/Q; a first hop is twice that."""
    P, Q = rate_ratio(rate_hz)
    return HOP_OUT // Q * P


def default_taps(rate_hz: int, K: int = DEFAULT_TAPS_PER_PHASE) -> np.ndarray:
    """h[k] = rint(2^14 d[k]) with d the channel filter's design at rate_hz (K*P taps summing to Q), int16, for shift 14: exactly
    what the program hands to the library."""
    L = _host_lib()
    n = L.msk144host_input_rate_taps(int(rate_hz), int(K), None)
    if n < 0:
        raise ValueError(f"no default resampler taps for rate {rate_hz} Hz, K={K} (a multiple of 125 Hz in {MIN_RATE}..{MAX_RATE} except 12000, K 1..64)")
    out = np.zeros(n, dtype=np.int16)
    L.msk144host_input_rate_taps(int(rate_hz), int(K), out.ctypes.data_as(C.c_void_p))
    return out


def check_config(rate_hz: int, taps, shift: int = DEFAULT_SHIFT) -> str:
    """The contract's configuration rules as libmsk144host.so applies them (csrc/input_rate.h check_config, shared with the library
    and the program): '' when valid, else the refusal text."""
    t = np.asarray(taps)
    if t.ndim != 1 or t.size == 0 or not np.issubdtype(t.dtype, np.integer) or np.any(t < -32768) or np.any(t > 32767):
        return "taps must be a non-empty row of int16 values"
    t = np.ascontiguousarray(t, dtype=np.int16)
    why = C.create_string_buffer(256)
    rc = _host_lib().msk144host_input_rate_check(int(rate_hz), int(shift), len(t), t.ctypes.data_as(C.c_void_p), why, len(why))
    return "" if rc == 0 else why.value.decode()


class Resampler:
    """Every stream of a handle: push(rows, streams, is_first) is one msk144_push_rate_hops.

    rows[j] holds the input samples of position j: 2 x 2592 P/Q for a first hop (the first-half row, then the hop row), else
    2592 P/Q.  Returns (hops, clamped): hops[j] the 5184 or 2592 int16 output samples, clamped[j] how many of them were clamped.
    All arithmetic in int64."""

    def __init__(self, channels: int, rate_hz: int, taps=None, shift: int = DEFAULT_SHIFT):
        if taps is None:
            taps = default_taps(rate_hz)
        why = check_config(rate_hz, taps, shift)
        if why:
            raise ValueError(why)
        self.channels = int(channels)
        self.rate_hz = int(rate_hz)
        self.P, self.Q = rate_ratio(rate_hz)
        self.h = np.asarray(taps, dtype=np.int64)
        self.L = len(self.h)
        self.shift = int(shift)
        self.H = -(-self.L // self.Q) - 1
        self.row = row_samples(rate_hz)
        self.hist = np.zeros((self.channels, self.H), dtype=np.int64)
        self.started = np.zeros(self.channels, dtype=bool)
        # the outputs of a first hop by branch: a later hop is the first 2592 of them (Q divides 2592)
        m = np.arange(FIRST_OUT, dtype=np.int64)
        self._n = m * self.P // self.Q
        self._r = m * self.P % self.Q

    def _one(self, stream: int, x: np.ndarray, first: bool) -> Tuple[np.ndarray, int]:
        M = FIRST_OUT if first else HOP_OUT
        if x.shape != ((2 if first else 1) * self.row,):
            raise ValueError(f"a {'first' if first else 'later'} hop carries {(2 if first else 1) * self.row} samples, got {x.shape}")
        if first:
            self.hist[stream] = 0
        elif not self.started[stream]:
            raise RuntimeError(f"stream {stream}: a later hop before a first one")
        self.started[stream] = True
        xx = np.concatenate([self.hist[stream], x.astype(np.int64)])
        acc = np.zeros(M, dtype=np.int64)
        n, r = self._n[:M], self._r[:M]
        for b in range(self.Q):
            g = self.h[b::self.Q]
            if g.size == 0:
                continue
            sel = np.nonzero(r == b)[0]
            idx = self.H + n[sel][:, None] - np.arange(g.size, dtype=np.int64)[None, :]
            acc[sel] = (xx[idx] * g[None, :]).sum(axis=1)
        assert np.all(np.abs(acc) <= 2**31 - 32768)
        y = (acc + (1 << (self.shift - 1))) >> self.shift
        clamped = int(np.count_nonzero((y > 32767) | (y < -32768)))
        if self.H:
            self.hist[stream] = xx[-self.H:]
        return np.clip(y, -32768, 32767).astype(np.int16), clamped

    def push(self, rows: Sequence[np.ndarray], streams: Sequence[int], is_first: Sequence[int]) -> Tuple[List[np.ndarray], np.ndarray]:
        s = [int(v) for v in streams]
        if len(rows) != len(s) or len(is_first) != len(s) or any(v < 0 or v >= self.channels for v in s) or any(b <= a for a, b in zip(s, s[1:])):
            raise ValueError("streams must be ascending stream numbers below channels, one row and one is_first each")
        for j, st in enumerate(s):
            if not is_first[j] and not self.started[st]:
                raise RuntimeError(f"stream {st}: a later hop before a first one")
        out, clamped = [], np.zeros(len(s), dtype=np.int32)
        for j, st in enumerate(s):
            y, c = self._one(st, np.asarray(rows[j]).reshape(-1), bool(is_first[j]))
            out.append(y)
            clamped[j] = c
        return out, clamped


class HostResampler:
    """The same through libmsk144host.so's C++ (msk144ir::Resampler): what the CPU tests pin against `Resampler` bit for bit."""

    def __init__(self, channels: int, rate_hz: int, taps, shift: int = DEFAULT_SHIFT):
        self._taps = np.ascontiguousarray(taps, dtype=np.int16)
        self.row = row_samples(rate_hz)
        self._p = _host_lib().msk144host_input_rate_new(int(channels), int(rate_hz), self._taps.ctypes.data_as(C.c_void_p), len(self._taps), int(shift))
        if not self._p:
            raise ValueError(check_config(rate_hz, taps, shift) or "bad channel count")

    def push_one(self, stream: int, x: np.ndarray, first: bool) -> Tuple[np.ndarray, int]:
        x = np.ascontiguousarray(x, dtype=np.int16)
        if x.shape != ((2 if first else 1) * self.row,):
            raise ValueError("wrong hop length")
        y = np.zeros(FIRST_OUT if first else HOP_OUT, dtype=np.int16)
        c = _host_lib().msk144host_input_rate_push(self._p, int(stream), x.ctypes.data_as(C.c_void_p), 1 if first else 0, y.ctypes.data_as(C.c_void_p))
        if c < 0:
            raise RuntimeError(f"stream {stream}: a later hop before a first one")
        return y, c

    def close(self):
        if self._p:
            _host_lib().msk144host_input_rate_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
