"""Wideband channeliser: float64 numpy model of the contract in include/msk144hip.h, sample-format readers and writers, and a
wideband scene synthesiser.

The model is the yardstick the device channeliser (csrc/channelise.hip) is tested against: the same prototype taps (the default
design comes from libmsk144host.so, csrc/wideband.h), the same integer phase reduction, the same int8 quantisation - only in
float64 where the device computes in f32.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

from . import synth

_PKG = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(_PKG, "libmsk144host.so")

OUT_RATE = 12000
FIRST_OUT = 5184   # output samples per channel of a first push
HOP_OUT = 2592     # ... of every later push
FORMATS = ("cu8", "cs8", "cs16")
MAX_RATE = 6144000          # the single-stage channeliser's top rate
BANDS = 64                  # the two-stage bank above it: 64 bands, decimation 32, rates multiples of 8000 up to 61.44 Msps
BANK_DECIMATION = 32
MAX_BANK_RATE = 61440000
_RAW_DTYPE = {"cu8": np.uint8, "cs8": np.int8, "cs16": np.int16}

_host = None


def _host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise FileNotFoundError(f"{HOST_LIB} not found: build it with `make -C msk144cudecoder_amd/host`")
        L = C.CDLL(HOST_LIB)
        L.msk144host_wideband_taps_rate.argtypes = [C.c_int64, C.c_int, C.c_void_p]
        L.msk144host_wideband_taps_rate.restype = C.c_int
        L.msk144host_wideband_check.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
        L.msk144host_wideband_check.restype = C.c_int
        L.msk144host_wideband_bank_taps.argtypes = [C.c_int64, C.c_int, C.c_void_p]
        L.msk144host_wideband_bank_taps.restype = C.c_int
        L.msk144host_wideband_ping_band_design.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
        L.msk144host_wideband_ping_band_design.restype = C.c_int
        L.msk144host_wideband_notch_design.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
        L.msk144host_wideband_notch_design.restype = C.c_int
        L.msk144host_wideband_audio_design.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
        L.msk144host_wideband_audio_design.restype = C.c_int
        _host = L
    return _host


def default_taps(D: int, K: int = 16) -> np.ndarray:
    """The default prototype at the integer rate D x 12000 Hz (K*D taps summing to 1)."""
    return default_taps_for_rate(OUT_RATE * int(D), K)


def rate_ratio(rate_hz: int) -> Tuple[int, int]:
    """Fs / 12000 = P/Q in lowest terms; Q = 1 for an integer decimation D = P."""
    g = math.gcd(int(rate_hz), OUT_RATE)
    return int(rate_hz) // g, OUT_RATE // g


def default_taps_for_rate(rate_hz: int, K: int = 16) -> np.ndarray:
    """The default prototype for any rate Fs = 12000 P/Q, exactly what the program hands to the library: K*P taps at 12000 P Hz
    summing to Q (each polyphase branch about unit DC gain)."""
    L = _host_lib()
    n = L.msk144host_wideband_taps_rate(int(rate_hz), int(K), None)
    if n < 0:
        raise ValueError(f"no default filter for rate {rate_hz} Hz, K={K} (a multiple of 125 Hz in 24000..6144000, K 1..64)")
    h = np.empty(n, dtype=np.float64)
    L.msk144host_wideband_taps_rate(int(rate_hz), int(K), h.ctypes.data_as(C.c_void_p))
    return h


def is_bank_rate(rate_hz: int) -> bool:
    """A rate the two-stage bank takes: a multiple of 8000 Hz above 6.144 Msps up to 61.44 Msps."""
    return MAX_RATE < int(rate_hz) <= MAX_BANK_RATE and int(rate_hz) % 8000 == 0


def stage2_rate(rate_hz: int) -> int:
    """The channeliser's rate: rate_hz, or the sub-band rate rate_hz/32 behind the bank."""
    return int(rate_hz) // BANK_DECIMATION if is_bank_rate(rate_hz) else int(rate_hz)


def bank_band(rate_hz: int, offsets_hz) -> np.ndarray:
    """k_c = floor((64 f_c + Fs/2) / Fs) in integers: -32..32 (band 32 is band -32)."""
    f = np.asarray(offsets_hz, dtype=np.int64)
    return np.floor_divide(BANDS * f + int(rate_hz) // 2, int(rate_hz))


def bank_residual(rate_hz: int, offsets_hz) -> np.ndarray:
    """d_c = f_c - k_c Fs/64, an integer with |d_c| <= Fs/128."""
    return np.asarray(offsets_hz, dtype=np.int64) - bank_band(rate_hz, offsets_hz) * (int(rate_hz) // BANDS)


def default_bank_taps(rate_hz: int, K1: int = 8) -> np.ndarray:
    """The default analysis-bank prototype (64 K1 taps at Fs, summing to 1), exactly what the library uses."""
    L = _host_lib()
    n = L.msk144host_wideband_bank_taps(int(rate_hz), int(K1), None)
    if n < 0:
        raise ValueError(f"no default bank for rate {rate_hz} Hz, K1={K1} (a multiple of 8000 Hz above 6144000 up to 61440000, K1 1..16)")
    h = np.empty(n, dtype=np.float64)
    L.msk144host_wideband_bank_taps(int(rate_hz), int(K1), h.ctypes.data_as(C.c_void_p))
    return h


def check_config(rate_hz: int, fmt: str, K: int, gain: float, offsets_hz: Sequence[int]) -> str:
    """The contract's configuration rules as libmsk144host.so applies them (csrc/wideband.h check_config, shared with the library
    and the program): '' when valid, else the refusal text."""
    off = np.ascontiguousarray(offsets_hz, dtype=np.int32)
    why = C.create_string_buffer(256)
    rc = _host_lib().msk144host_wideband_check(int(rate_hz), FORMATS.index(fmt), int(K), float(gain), off.ctypes.data_as(C.c_void_p), len(off), why, len(why))
    return "" if rc == 0 else why.value.decode()


# ---- sample formats ----

def read_samples(raw, fmt: str) -> np.ndarray:
    """Interleaved I,Q components (bytes or array) -> complex128: cu8 (u - 127.5)/128, cs8 s/128, cs16 s/32768."""
    a = np.frombuffer(raw, dtype=_RAW_DTYPE[fmt]) if isinstance(raw, (bytes, bytearray, memoryview)) else np.asarray(raw, dtype=_RAW_DTYPE[fmt])
    a = a.astype(np.float64).reshape(-1, 2)
    if fmt == "cu8":
        a = (a - 127.5) / 128.0
    elif fmt == "cs8":
        a = a / 128.0
    else:
        a = a / 32768.0
    return a[:, 0] + 1j * a[:, 1]


def write_samples(x: np.ndarray, fmt: str) -> np.ndarray:
    """complex -> interleaved raw components in `fmt` (rounded and clipped), the inverse of read_samples."""
    x = np.asarray(x)
    v = np.empty(2 * len(x), dtype=np.float64)
    v[0::2], v[1::2] = x.real, x.imag
    if fmt == "cu8":
        return np.clip(np.rint(v * 128.0 + 127.5), 0, 255).astype(np.uint8)
    if fmt == "cs8":
        return np.clip(np.rint(v * 128.0), -128, 127).astype(np.int8)
    return np.clip(np.rint(v * 32768.0), -32768, 32767).astype(np.int16)


# ---- the channeliser model ----

def tap_matrix(rate_hz: int, offsets_hz: Sequence[int], taps: np.ndarray) -> np.ndarray:
    """G[c][k] = h[k] e^{+j2pi ((f_c k) mod Fs)/Fs}, phases reduced in integers."""
    fs = int(rate_hz)
    k = np.arange(len(taps), dtype=np.int64)
    f = np.mod(np.asarray(offsets_hz, dtype=np.int64), fs)
    ph = np.mod(f[:, None] * k[None, :], fs).astype(np.float64) * (2.0 * np.pi / fs)
    return taps[None, :] * np.exp(1j * ph)


def output_rotation(offsets_hz: Sequence[int], m: np.ndarray) -> np.ndarray:
    """e^{-j2pi ((f_c m) mod 12000)/12000}, [channel][sample]."""
    f = np.mod(np.asarray(offsets_hz, dtype=np.int64), OUT_RATE)
    mm = np.mod(np.asarray(m, dtype=np.int64), OUT_RATE)
    return np.exp(-2j * np.pi * (np.mod(f[:, None] * mm[None, :], OUT_RATE).astype(np.float64) / OUT_RATE))


def quantise(y: np.ndarray, gain=100.0, per_channel: bool = False):
    """complex [..] -> (int8 [..][2] I/Q, clipped components): q = clamp(rint(128 gain y), -128, 127).  gain: one number, or one per
    channel for y [channel][M].  per_channel: the clipped components of each channel (int64 [channel]) instead of their total."""
    g = np.asarray(gain, dtype=np.float64)
    if g.ndim:
        g = g.reshape(-1, 1, 1)
    v = np.stack([y.real, y.imag], axis=-1) * (128.0 * g)
    r = np.rint(v)
    over = (r < -128) | (r > 127)
    clipped = np.count_nonzero(over, axis=(1, 2)).astype(np.int64) if per_channel else int(np.count_nonzero(over))
    return np.clip(r, -128, 127).astype(np.int8), clipped


# msk144_wideband_level (include/msk144hip.h); HipDecoder.wideband_levels() returns the same records
LEVEL_DTYPE = np.dtype([("samples", "<i8"), ("sum_sq", "<i8"), ("clipped", "<i8"), ("gain", "<f4"), ("exponent", "<i4")])
assert LEVEL_DTYPE.itemsize == 32


def levels(q: np.ndarray, clipped=None) -> np.ndarray:
    """The statistics msk144_wideband_levels reports, from the int8 hops q [channel][M][2] of one push: samples = M and sum_sq = the
    sum of I*I + Q*Q over the stored values, exactly; clipped = the caller's per-channel counts (quantise(..., per_channel=True);
    the hops alone do not tell a stored 127 from a clipped one), 0 when not given.  gain and exponent are left 0."""
    q = np.asarray(q)
    out = np.zeros(q.shape[0], dtype=LEVEL_DTYPE)
    out["samples"] = q.shape[1]
    out["sum_sq"] = np.sum(q.astype(np.int64) ** 2, axis=(1, 2))
    if clipped is not None:
        out["clipped"] = clipped
    return out


# the defaults of msk144_wideband_agc (csrc/wideband.h AgcParams); hipdecoder.AGC_DEFAULTS is this dict
AGC_DEFAULTS = dict(lo_sq=64, hi_sq=1024, clip_ppm=1000, hold=4, min_exp=-20, max_exp=20)


class Agc:
    """The stepped AGC of the contract (include/msk144hip.h) in Python integers: per channel an exponent e and a count of quiet
    pushes; gains() is what the next push is quantised with, step() moves the state by one push's statistics."""

    def __init__(self, channels: int, gains=100.0, **params):
        p = dict(AGC_DEFAULTS)
        unknown = set(params) - set(p)
        if unknown:
            raise TypeError(f"unknown AGC parameters {sorted(unknown)}")
        p.update({k: int(v) for k, v in params.items()})
        if p["lo_sq"] < 0 or p["hi_sq"] <= 4 * p["lo_sq"]:
            raise ValueError("hi_sq must exceed 4 x lo_sq >= 0: one 6 dB step multiplies the power by 4")
        if p["clip_ppm"] < 0:
            raise ValueError("clip_ppm must not be negative")
        if p["hold"] < 1:
            raise ValueError("hold must be at least 1 push")
        if p["min_exp"] > p["max_exp"] or p["min_exp"] < -126 or p["max_exp"] > 126:
            raise ValueError("min_exp <= max_exp, both within -126..126")
        self.p = p
        self.base = np.broadcast_to(np.asarray(gains, dtype=np.float32), (channels,)).astype(np.float32)
        with np.errstate(over="ignore"):
            top = np.ldexp(np.float32(128.0) * self.base, p["max_exp"])
        if not (np.all(self.base > 0) and np.all(np.isfinite(top))):
            raise ValueError("every gain must be positive with 128 x gain x 2^max_exp finite in f32")
        self.reset()

    def reset(self):
        """A first push: exponent 0, no quiet push counted."""
        self.e = [0] * len(self.base)
        self.quiet = [0] * len(self.base)

    def gains(self) -> np.ndarray:
        """float64 [channel]: base gain x 2^e, exactly the f32 value the device scales with (a 6 dB ladder is exact)."""
        return np.ldexp(self.base.astype(np.float64), np.asarray(self.e, dtype=np.int64))

    def step(self, lv):
        """lv: records with samples, sum_sq, clipped per channel (levels(), or HipDecoder.wideband_levels()) of the push just made."""
        p = self.p
        for c in range(len(self.e)):
            n, S, k = int(lv["samples"][c]), int(lv["sum_sq"][c]), int(lv["clipped"][c])
            if k * 1000000 > p["clip_ppm"] * 2 * n or S > p["hi_sq"] * 2 * n:
                self.e[c] = max(self.e[c] - 1, p["min_exp"])
                self.quiet[c] = 0
            elif S < p["lo_sq"] * 2 * n:
                self.quiet[c] += 1
                if self.quiet[c] >= p["hold"]:
                    self.e[c] = min(self.e[c] + 1, p["max_exp"])
                    self.quiet[c] = 0
            else:
                self.quiet[c] = 0


# the defaults of msk144_wideband_blanker (csrc/wideband.h BlankerParams): design parameters, not measurements
BLANKER_DEFAULTS = dict(threshold_q4=256, pre=2, post=8)
_CS16_UNIT = {"cu8": 128, "cs8": 256, "cs16": 1}


def blanker_components(raw, fmt: str) -> np.ndarray:
    """int64 [n][2]: the integer components the blanker measures power in - cu8 c = 2u - 255, cs8 and cs16 c = s."""
    a = np.frombuffer(raw, dtype=_RAW_DTYPE[fmt]) if isinstance(raw, (bytes, bytearray, memoryview)) else np.asarray(raw, dtype=_RAW_DTYPE[fmt])
    c = a.astype(np.int64).reshape(-1, 2)
    return 2 * c - 255 if fmt == "cu8" else c


def as_cs16(raw, fmt: str) -> np.ndarray:
    """Raw components of fmt as the cs16 components that read as the same numbers: cu8 (2u - 255) x 128, cs8 s x 256.  What the
    device keeps of a blanked stream."""
    return (blanker_components(raw, fmt) * _CS16_UNIT[fmt]).astype(np.int16).reshape(-1)


class Blanker:
    """The impulse-noise blanker of the contract (include/msk144hip.h), push by push: every decision in integers (the powers in
    int64, exact; their sum, the mean and the threshold in Python integers).  It holds what the last hit of a push still owes to the
    next one, and the totals since reset()."""

    def __init__(self, fmt: str, **params):
        if fmt not in FORMATS:
            raise ValueError(f"format must be one of {FORMATS}")
        p = dict(BLANKER_DEFAULTS)
        unknown = set(params) - set(p)
        if unknown:
            raise TypeError(f"unknown blanker parameters {sorted(unknown)}")
        p.update({k: int(v) for k, v in params.items()})
        if not 16 <= p["threshold_q4"] <= 65535:
            raise ValueError("threshold_q4 must lie within 16..65535")
        if not (0 <= p["pre"] <= 4096 and 0 <= p["post"] <= 4096):
            raise ValueError("pre and post must lie within 0..4096 samples")
        self.fmt, self.p = fmt, p
        self.reset()

    def reset(self):
        """A first push follows: nothing owed, totals at 0."""
        self.carry = 0
        self.total = dict(total_samples=0, total_hits=0, total_blanked=0)

    def push(self, raw):
        """(the push as cs16 components, I,Q interleaved, blanked samples 0; the statistics msk144_wideband_blanker_stats reports)."""
        c = blanker_components(raw, self.fmt)
        N = len(c)
        power = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]
        S = int(power.sum(dtype=np.int64))   # at most 2^56: exact in int64
        T = ((S // N) * self.p["threshold_q4"]) >> 4
        hits = np.flatnonzero(power > T)
        edge = np.zeros(N + 1, dtype=np.int64)
        np.add.at(edge, np.maximum(hits - self.p["pre"], 0), 1)
        np.add.at(edge, np.minimum(hits + self.p["post"], N - 1) + 1, -1)
        blanked = np.cumsum(edge[:N]) > 0
        blanked[:min(self.carry, N)] = True
        self.carry = max(0, int(hits[-1]) + self.p["post"] - (N - 1)) if len(hits) else 0
        out = as_cs16(raw, self.fmt).reshape(-1, 2)
        out[blanked] = 0
        nb = int(np.count_nonzero(blanked))
        self.total["total_samples"] += N
        self.total["total_hits"] += len(hits)
        self.total["total_blanked"] += nb
        st = dict(samples=N, sum_power=S, threshold=T, hits=len(hits), blanked=nb, carry_out=self.carry, **self.total)
        return out.reshape(-1), st


# ---- the power spectrum of the input stream (msk144_set_wideband_spectrum) ----

SPECTRUM_MIN_BINS, SPECTRUM_MAX_BINS, SPECTRUM_DEFAULT_BINS = 256, 8192, 1024
SPECTRUM_FLOOR_DBFS = -200.0


def spectrum_window(bins: int) -> np.ndarray:
    """The default window of the contract, periodic Hann: w[i] = 0.5 - 0.5 cos(2 pi i / B), float64 (the library's own is
    msk144host_wideband_spectrum_window)."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(bins), dtype=np.float64) / int(bins))


def spectrum_dbfs(power, segments: int, window) -> np.ndarray:
    """10 log10(P / (S (sum w)^2)), floored at -200: a full-scale complex tone on a bin centre reads 0 dBFS."""
    full = float(segments) * float(np.sum(np.asarray(window, dtype=np.float64))) ** 2
    p = np.asarray(power, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10.0 * np.log10(p / full) if full > 0.0 else np.full(p.shape, SPECTRUM_FLOOR_DBFS)
    return np.maximum(np.nan_to_num(db, nan=SPECTRUM_FLOOR_DBFS, neginf=SPECTRUM_FLOOR_DBFS), SPECTRUM_FLOOR_DBFS)


class Spectrum:
    """The power spectrum of the contract (include/msk144hip.h), push by push and in float64 throughout: S = floor(N / B) segments of
    the push's own samples, not overlapped, P[k] = sum_s |FFT(w x_s)[k]|^2, returned in ascending frequency (power[j] is bin
    (j - B/2) mod B).  The window is the f32 the device stores, as float64.  fmt is the format the samples arrive in: a raw format, or
    "cs16" for the output of the Blanker model.  Nothing is carried from push to push."""

    def __init__(self, fmt: str, bins: int = SPECTRUM_DEFAULT_BINS, window=None):
        if fmt not in FORMATS:
            raise ValueError(f"format must be one of {FORMATS}")
        bins = int(bins)
        if not SPECTRUM_MIN_BINS <= bins <= SPECTRUM_MAX_BINS or bins & (bins - 1):
            raise ValueError("bins must be a power of two within 256..8192")
        w = spectrum_window(bins) if window is None else np.asarray(window, dtype=np.float64)
        if w.shape != (bins,) or not np.all(np.isfinite(w)):
            raise ValueError("the window must hold `bins` finite values")
        self.fmt, self.bins = fmt, bins
        self.window = w.astype(np.float32).astype(np.float64)

    def push(self, raw):
        """(power float64 [bins] in ascending frequency, segments) of one push's raw samples."""
        x = read_samples(raw, self.fmt)
        S = len(x) // self.bins
        if S < 1:
            raise ValueError("a push must hold at least one segment")
        X = np.fft.fft(x[:S * self.bins].reshape(S, self.bins) * self.window[None, :], axis=1)
        return np.fft.fftshift(np.sum(X.real ** 2 + X.imag ** 2, axis=0)), S


# ---- per-channel ping detection (msk144_set_wideband_pings) ----

# msk144_wideband_ping (include/msk144hip.h); HipDecoder.wideband_pings() returns the same records
PING_DTYPE = np.dtype([("up_mask", "<u8"), ("blocks", "<i4"), ("history", "<i4"), ("quiet", "<i4"), ("reference", "<i4"), ("peak", "<i4"), ("peak_block", "<i4")])
assert PING_DTYPE.itemsize == 32
PING_BLOCK = 96           # samples per block: 8 ms
PING_MAX_BLOCKS = 54      # blocks of a first push; a later push has 27
PING_MAX_MEMORY = 16
# the defaults of msk144_wideband_pings_params (csrc/wideband.h PingParams): design parameters, not measurements
PINGS_DEFAULTS = dict(ratio_q4=32, memory=8, min_ref=96)
PING_MIN_BLOCKS = 2       # the event rule's default


def ping_blocks(q) -> np.ndarray:
    """int64 [channel][nb]: E[b] = the sum of I*I + Q*Q over samples 96b .. 96b+95 of the int8 hops q [channel][M][2]."""
    q = np.asarray(q)
    C_, M = q.shape[0], q.shape[1]
    if M % PING_BLOCK or q.shape[2:] != (2,):
        raise ValueError("hops must be [channel][M][2] with M a multiple of 96")
    return np.sum(q.astype(np.int64).reshape(C_, M // PING_BLOCK, 2 * PING_BLOCK) ** 2, axis=2)


class Pings:
    """The ping detector of the contract (include/msk144hip.h) in Python integers, push by push: per channel the quiet levels of the
    pushes since its history last restarted, and the scale of its last push.  reset() stands for a first push and for
    msk144_set_wideband_pings: the next push restarts every history.  `energies` holds the last push's E, int64 [channel][nb]."""

    def __init__(self, channels: int, **params):
        p = dict(PINGS_DEFAULTS)
        unknown = set(params) - set(p)
        if unknown:
            raise TypeError(f"unknown ping parameters {sorted(unknown)}")
        p.update({k: int(v) for k, v in params.items()})
        if not 16 <= p["ratio_q4"] <= 65535:
            raise ValueError("ratio_q4 must lie within 16..65535")
        if not 0 <= p["memory"] <= PING_MAX_MEMORY:
            raise ValueError("memory must lie within 0..16 pushes")
        if not 1 <= p["min_ref"] <= 1 << 22:
            raise ValueError("min_ref must lie within 1..2^22")
        self.p, self.channels = p, int(channels)
        self.energies = None
        self.reset()

    def reset(self):
        self.quiet = [[] for _ in range(self.channels)]   # the q of the pushes since the restart, oldest first
        self.scale = [None] * self.channels

    def push(self, q, scales, energies=None) -> np.ndarray:
        """PING_DTYPE [channel] from the int8 hops q [channel][M][2] of one push and the f32 scale each channel was quantised with
        (wideband_levels()["gain"]); a scale other than the channel's last restarts its history.  `energies`: the rule runs on
        these [channel][nb] in place of the E of q (the in-band Ef of PingBand.push; q is then not read and may be None)."""
        E = ping_blocks(q) if energies is None else np.asarray(energies, dtype=np.int64)
        if E.shape[0] != self.channels:
            raise ValueError(f"{self.channels} channels, got {E.shape[0]}")
        sc = np.broadcast_to(np.asarray(scales, dtype=np.float32), (self.channels,))
        nb = E.shape[1]
        out = np.zeros(self.channels, dtype=PING_DTYPE)
        for c in range(self.channels):
            e = [int(v) for v in E[c]]
            if self.scale[c] is None or self.scale[c] != sc[c]:
                self.quiet[c] = []
            self.scale[c] = sc[c]
            quiet = sorted(e)[nb // 4]
            h = min(self.p["memory"], len(self.quiet[c]))
            R = max(min([quiet] + self.quiet[c][len(self.quiet[c]) - h:]), self.p["min_ref"])
            self.quiet[c] = (self.quiet[c] + [quiet])[-PING_MAX_MEMORY:]
            mask = 0
            for b in range(nb):
                if e[b] * 16 > R * self.p["ratio_q4"]:
                    mask |= 1 << b
            peak = max(e)
            out[c] = (mask, nb, h, quiet, R, peak, e.index(peak))
        self.energies = E
        return out


# ---- the ping band: an in-band filter ahead of the block energies (msk144_set_wideband_ping_band) ----

PING_BAND_TAPS = 64
PING_BAND_MAX_SHIFT = 40
PING_BAND_MAX_ENERGY = (1 << 22) - 1
PING_BAND_RATIO_Q4 = 52   # MSK144_PING_BAND_RATIO_Q4: the detector's default ratio with the default band on


def _fir_taps(taps, shape_error: str, value_error: str) -> np.ndarray:
    """int8 [64][2] from taps [k][2], 1 <= k <= 64, zero-padded; the two refusals are the caller's texts."""
    t = np.asarray(taps)
    if t.ndim != 2 or t.shape[1] != 2 or not 1 <= t.shape[0] <= PING_BAND_TAPS:
        raise ValueError(shape_error)
    if np.any(t != t.astype(np.int8)):
        raise ValueError(value_error)
    full = np.zeros((PING_BAND_TAPS, 2), dtype=np.int8)
    full[:t.shape[0]] = t
    return full


def _fir_push(tail, q, taps) -> Tuple[np.ndarray, np.ndarray]:
    """The 64-tap FIR behind the ping band and the notch (csrc/wideband.h fir_push): int8 tail [..][63][2], int8 hops q [..][M][2] and
    taps [64][2] give the joined stream s [..][63 + M][2], so that x[m - k] is s[..., 63 + m - k, :], and z [..][M][2],
    z[m] = sum b[k] x[m - k], both int64.  The next tail is s[..., M:, :]."""
    s = np.concatenate([tail, np.asarray(q).astype(np.int8)], axis=-2).astype(np.int64)
    M, T = s.shape[-2] - (PING_BAND_TAPS - 1), PING_BAND_TAPS - 1
    z = np.zeros(s.shape[:-2] + (M, 2), dtype=np.int64)
    for k in range(PING_BAND_TAPS):
        br, bi = int(taps[k, 0]), int(taps[k, 1])
        if br == 0 and bi == 0:
            continue
        a, b = s[..., T - k:T - k + M, 0], s[..., T - k:T - k + M, 1]
        z[..., 0] += br * a - bi * b
        z[..., 1] += br * b + bi * a
    return s, z


def ping_band_taps(centre_hz: int = 0, halfwidth_hz: int = 1500) -> Tuple[np.ndarray, int]:
    """The default design of the contract, from libmsk144host.so (csrc/wideband.h ping_band_design), exactly what the program hands
    to the library: (int8 [64][2] taps (br, bi), shift)."""
    taps = np.zeros((PING_BAND_TAPS, 2), dtype=np.int8)
    shift = C.c_int32(0)
    why = C.create_string_buffer(256)
    if _host_lib().msk144host_wideband_ping_band_design(int(centre_hz), int(halfwidth_hz), taps.ctypes.data_as(C.c_void_p), C.byref(shift), why, len(why)) != 0:
        raise ValueError(why.value.decode())
    return taps, int(shift.value)


class PingBand:
    """The ping band of the contract (include/msk144hip.h) in int64 numpy, push by push: z[n] = sum b[k] x[n - k] on the stored int8
    values, Ef[b] = min((sum over the block of |z|^2) >> shift, 2^22 - 1), and per channel the 63 stored samples before the next
    push.  reset() stands for every push at which the library restarts the ping history (a first push, the first push after
    msk144_set_wideband_pings or msk144_set_wideband_ping_band): the tail is all zero there.  A change of scale does not reset."""

    def __init__(self, channels: int, taps, shift: int):
        self.taps = _fir_taps(taps, "taps must be [k][2] with 1 <= k <= 64", "taps must be int8 values")
        if not 0 <= int(shift) <= PING_BAND_MAX_SHIFT:
            raise ValueError("shift must lie within 0..40")
        self.shift, self.channels = int(shift), int(channels)
        self.reset()

    def reset(self):
        self.tail = np.zeros((self.channels, PING_BAND_TAPS - 1, 2), dtype=np.int8)

    def push(self, q) -> np.ndarray:
        """int64 [channel][nb]: Ef of the int8 hops q [channel][M][2] of one push, M a multiple of 96; the tail moves on."""
        q = np.asarray(q)
        if q.ndim != 3 or q.shape[0] != self.channels or q.shape[1] % PING_BLOCK or q.shape[2] != 2:
            raise ValueError(f"hops must be [{self.channels}][M][2] with M a multiple of 96")
        M = q.shape[1]
        s, z = _fir_push(self.tail, q, self.taps)
        S = np.sum(np.sum(z * z, axis=2).reshape(self.channels, M // PING_BLOCK, PING_BLOCK), axis=2)   # < 2^50
        self.tail = s[:, M:, :].astype(np.int8)
        return np.minimum(S >> self.shift, PING_BAND_MAX_ENERGY)


# ---- each captured hop as 12 kHz audio (msk144_set_wideband_audio, msk144_wideband_capture_audio) ----

AUDIO_PHASORS = 96
AUDIO_MIN_SHIFT, AUDIO_MAX_SHIFT = 1, 40
AUDIO_HALFWIDTH_HZ = 1250     # the defaults are design parameters, not measurements
AUDIO_TONE_HZ = 1500
WAV_HEADER_BYTES = 44


def audio_design(centre_hz: int = 0, halfwidth_hz: int = AUDIO_HALFWIDTH_HZ, tone_hz: int = AUDIO_TONE_HZ) -> Tuple[np.ndarray, np.ndarray, int]:
    """The default design of the contract, from libmsk144host.so (csrc/wideband.h audio_design), exactly what the program hands to
    the library: (int8 [64][2] taps (br, bi), int16 [96][2] phasors (pr, pi), shift)."""
    taps = np.zeros((PING_BAND_TAPS, 2), dtype=np.int8)
    phasor = np.zeros((AUDIO_PHASORS, 2), dtype=np.int16)
    shift = C.c_int32(0)
    why = C.create_string_buffer(256)
    if _host_lib().msk144host_wideband_audio_design(int(centre_hz), int(halfwidth_hz), int(tone_hz), taps.ctypes.data_as(C.c_void_p), phasor.ctypes.data_as(C.c_void_p), C.byref(shift), why,
                                          len(why)) != 0:
        raise ValueError(why.value.decode())
    return taps, phasor, int(shift.value)


def _audio_phasor(phasor) -> np.ndarray:
    """int16 [96][2] from phasor [96][2]."""
    w = np.asarray(phasor)
    if w.shape != (AUDIO_PHASORS, 2) or np.any(w != w.astype(np.int16)):
        raise ValueError("phasor must be int16 [96][2]")
    return w.astype(np.int16)


class Audio:
    """The audio of the contract (include/msk144hip.h) in int64 numpy, push by push: z[n] = sum b[k] x[n - k] on the stored int8
    values, a[n] = Re z pr[n mod 96] - Im z pi[n mod 96], y[n] = clamp((a + 2^(shift - 1)) >> shift) to int16, and per channel the 63
    stored samples before the next push.  restart stands for every push at which the library starts from an all-zero tail: a first
    push, and the first push after msk144_set_wideband_audio, whose rows are then the two hops of the ring window, older first."""

    def __init__(self, channels: int, taps, phasor, shift: int):
        self.taps = _fir_taps(taps, "taps must be [k][2] with 1 <= k <= 64", "taps must be int8 values")
        self.phasor = _audio_phasor(phasor).astype(np.int64)
        if not AUDIO_MIN_SHIFT <= int(shift) <= AUDIO_MAX_SHIFT:
            raise ValueError("audio shift must lie within 1..40")
        self.shift, self.channels = int(shift), int(channels)
        self.tail = np.zeros((self.channels, PING_BAND_TAPS - 1, 2), dtype=np.int8)

    def push(self, rows, restart: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """(int16 [channel][M], int64 [channel][M / 2592]): the audio of the int8 hops rows [channel][M][2] of one push, M a multiple
        of 2592 that starts on a hop, and the samples of each hop that the clamp changed; the tail moves on."""
        q = np.asarray(rows)
        if q.ndim != 3 or q.shape[0] != self.channels or q.shape[1] % HOP_OUT or q.shape[2] != 2:
            raise ValueError(f"hops must be [{self.channels}][M][2] with M a multiple of 2592")
        if restart:
            self.tail = np.zeros_like(self.tail)
        M = q.shape[1]
        s, z = _fir_push(self.tail, q, self.taps)
        w = self.phasor[np.arange(M) % AUDIO_PHASORS]
        a = z[..., 0] * w[:, 0] - z[..., 1] * w[:, 1]                # |a| <= 2^37
        v = (a + (1 << (self.shift - 1))) >> self.shift              # numpy's >> on int64 is arithmetic: floor
        y = np.clip(v, -32768, 32767)
        self.tail = s[:, M:, :].astype(np.int8)
        return y.astype(np.int16), np.sum((y != v).reshape(self.channels, M // HOP_OUT, HOP_OUT), axis=2)


def wav_header(samples: int) -> bytes:
    """The 44-byte RIFF/WAVE header of --wideband-audio's files: PCM format 1, one channel, 12000 Hz, 16 bits."""
    import struct
    data = 2 * int(samples)
    return struct.pack("<4sI8sIHHIIHH4sI", b"RIFF", data + WAV_HEADER_BYTES - 8, b"WAVEfmt ", 16, 1, 1, OUT_RATE, 2 * OUT_RATE, 2, 16, b"data", data)


def wav_bytes(audio) -> bytes:
    """The file rule of --wideband-audio: the header, then the int16 samples of audio (any shape, row after row), little-endian."""
    a = np.ascontiguousarray(audio, dtype="<i2").reshape(-1)
    return wav_header(a.size) + a.tobytes()


# ---- the notch: steady carriers taken out of a channel's stored samples (msk144_set_wideband_notch) ----

NOTCH_TAPS = 64
NOTCH_DELAY = 31        # MSK144_NOTCH_DELAY: the output is the input delayed by 31 samples, minus the estimate of the carriers
NOTCH_MAX_SHIFT = 15
NOTCH_HALFWIDTH_HZ = 100


def notch_taps(freqs, halfwidth_hz: int = NOTCH_HALFWIDTH_HZ) -> Tuple[np.ndarray, int]:
    """The default design of the contract for 1 or 2 frequencies (Hz from the channel's offset), from libmsk144host.so
    (csrc/wideband.h notch_design): (int8 [64][2] taps (br, bi), shift)."""
    f = np.ascontiguousarray(np.atleast_1d(freqs), dtype=np.int32)
    if f.ndim != 1 or np.any(f != np.atleast_1d(freqs)):
        raise ValueError("notch frequencies must be integers")
    taps = np.zeros((NOTCH_TAPS, 2), dtype=np.int8)
    shift = C.c_int32(0)
    why = C.create_string_buffer(256)
    if _host_lib().msk144host_wideband_notch_design(f.ctypes.data_as(C.c_void_p), len(f), int(halfwidth_hz), taps.ctypes.data_as(C.c_void_p), C.byref(shift), why, len(why)) != 0:
        raise ValueError(why.value.decode())
    return taps, int(shift.value)


def notch_entry(entry) -> Tuple[np.ndarray, int]:
    """One entry of a notch table as (int8 [64][2] taps, shift): a list of frequencies takes the default design, (taps, shift) is
    checked and zero-padded."""
    if isinstance(entry, tuple) and len(entry) == 2 and np.ndim(entry[0]) == 2:
        shift, why = int(entry[1]), "taps must be int8 [k][2] with 1 <= k <= 64"
        return _fir_taps(entry[0], why, why), shift
    return notch_taps(list(entry))


class Notch:
    """The notch of the contract (include/msk144hip.h) in int64 numpy, push by push: per channel of the table z[n] = sum b[k] x[n - k]
    on the stored int8 values, y[n] = sat8(((x[n - 31] << s) - z[n] + r) >> s), and the 63 raw stored samples before the next push.
    set(table) takes what HipDecoder.set_wideband_notch takes and, as the library, zeroes the tail of a channel whose entry is new or
    changed and keeps that of an unchanged one; reset() stands for a first push: every tail is zero."""

    def __init__(self, channels: int, table=None):
        self.channels = int(channels)
        self.table = {}
        self.reset()
        self.set(table)

    def reset(self):
        self.tail = np.zeros((self.channels, NOTCH_TAPS - 1, 2), dtype=np.int8)

    def set(self, table):
        new = {}
        for c, entry in (table or {}).items():
            c = int(c)
            if not 0 <= c < self.channels or c in new:
                raise ValueError(f"channel {c} is out of range or listed twice")
            t, s = notch_entry(entry)
            if not 0 <= s <= NOTCH_MAX_SHIFT:
                raise ValueError("shift must lie within 0..15")
            new[c] = (t, s)
            old = self.table.get(c)
            if old is None or old[1] != s or not np.array_equal(old[0], t):
                self.tail[c] = 0
        self.table = new

    def push(self, q):
        """(int8 [channel][M][2] the notched hops, int64 [channel] clamped components) from the int8 hops q [channel][M][2] of one
        push; the channels not in the table pass unchanged; the tails of those in it move on."""
        q = np.asarray(q)
        if q.ndim != 3 or q.shape[0] != self.channels or q.shape[2] != 2:
            raise ValueError(f"hops must be [{self.channels}][M][2]")
        M, T = q.shape[1], NOTCH_TAPS - 1
        out = q.astype(np.int8).copy()
        clipped = np.zeros(self.channels, dtype=np.int64)
        for c, (taps, s) in self.table.items():
            x, z = _fir_push(self.tail[c], q[c], taps)
            v = ((x[T - NOTCH_DELAY:T - NOTCH_DELAY + M] << s) - z + ((1 << (s - 1)) if s else 0)) >> s
            y = np.clip(v, -128, 127)
            clipped[c] = int(np.count_nonzero(y != v))
            out[c] = y.astype(np.int8)
            self.tail[c] = x[M:].astype(np.int8)
        return out, clipped


NOTCH_PLAN_DEFAULTS = dict(db=10.0, period=23, persist=2)   # msk144wb::NotchPlan: design parameters, not measurements
NOTCH_PLAN_GUARD_BINS = 3


def notch_design_refused(freqs, halfwidth_hz: int) -> bool:
    """The rules of the default design (csrc/wideband.h check_notch_design)."""
    f = [int(v) for v in freqs]
    return (not 1 <= len(f) <= 2 or not 50 <= halfwidth_hz <= 500 or any(abs(v) + halfwidth_hz > OUT_RATE // 2 for v in f)
            or (len(f) == 2 and abs(f[0] - f[1]) < 1000))


class NotchPlanner:
    """The host rule of msk144hipdecoder --wideband-notch=auto (csrc/wideband.h NotchPlanner), operation for operation: fed every
    push's waterfall sums [channel][96], it adds them over `period` pushes; at the end of a period the highest bin j of a channel
    that is not within 3 bins of one of its notches is hot when it lies at least `db` over the period's median bin; the same bin, +-1,
    hot in `persist` consecutive periods adds a notch at rint(125 (j - 48 + d)) Hz, d the vertex of the parabola through 10 log10 of
    bins j - 1, j, j + 1 clamped to +-0.5, if the channel has fewer than 2 and the spacing rule holds.  Notches are only ever added."""

    def __init__(self, channels: int, db: float = 10.0, period: int = 23, persist: int = 2, halfwidth_hz: int = NOTCH_HALFWIDTH_HZ):
        if not 1.0 <= db <= 100.0 or not 1 <= period <= 100000 or not 1 <= persist <= 1000:
            raise ValueError("db must lie within 1..100, period within 1..100000, persist within 1..1000")
        self.channels, self.db, self.period, self.persist, self.halfwidth = int(channels), float(db), int(period), int(persist), int(halfwidth_hz)
        self.acc = np.zeros((self.channels, WATERFALL_BINS), dtype=np.float64)
        self.pushes = 0
        self.notches = [[] for _ in range(self.channels)]
        self.state = [(-1, 0)] * self.channels     # (the hot bin of the last period, the periods in a row it has been hot)

    @staticmethod
    def vertex(a, j: int) -> float:
        if j <= 0 or j >= WATERFALL_BINS - 1 or not a[j - 1] > 0.0 or not a[j + 1] > 0.0 or not a[j] > 0.0:
            return 0.0
        lm, l0, lp = (10.0 * math.log10(float(a[i])) for i in (j - 1, j, j + 1))
        den = lm - 2.0 * l0 + lp
        if not den < 0.0:
            return 0.0
        return min(max(0.5 * (lm - lp) / den, -0.5), 0.5)

    def push(self, sums) -> list:
        """[(channel, hz, excess_db)] added by this push, by channel."""
        s = np.asarray(sums, dtype=np.float64).reshape(self.channels, WATERFALL_BINS)
        self.acc += s
        self.pushes += 1
        if self.pushes < self.period:
            return []
        self.pushes = 0
        out = []
        for c in range(self.channels):
            a = self.acc[c]
            j = -1
            for i in range(WATERFALL_BINS):
                if any(abs(i - (round(f / 125.0) + WATERFALL_BINS // 2)) <= NOTCH_PLAN_GUARD_BINS for f in self.notches[c]):
                    continue
                if j < 0 or a[i] > a[j]:
                    j = i
            median = float(np.sort(a)[WATERFALL_BINS // 2])
            excess = 10.0 * math.log10(float(a[j]) / median) if j >= 0 and median > 0.0 and a[j] > 0.0 else 0.0
            if not (j >= 0 and median > 0.0 and excess >= self.db):
                self.state[c] = (-1, 0)
                continue
            last, run = self.state[c]
            run = run + 1 if last >= 0 and abs(j - last) <= 1 else 1
            self.state[c] = (j, run)
            if run < self.persist or len(self.notches[c]) >= 2:
                continue
            nxt = self.notches[c] + [int(round(125.0 * (j - WATERFALL_BINS // 2 + self.vertex(a, j))))]
            if notch_design_refused(nxt, self.halfwidth):
                continue
            self.notches[c] = nxt
            self.state[c] = (-1, 0)
            out.append((c, nxt[-1], excess))
        self.acc[:] = 0.0
        return out


class PingEvents:
    """The event rule of the contract: with g = (blocks of all earlier pushes) + b an event is a maximal run of consecutive up blocks
    of a channel.  A run that reaches a push's last block stays open into the next push; close() - the end of the stream - closes
    every open run.  An event is reported when it closes, if it has at least min_blocks blocks, as a dict with channel, start and
    blocks (in blocks of 8 ms), peak (the largest E of the run, at its lowest g on a tie) and reference (the R of the push that block
    lay in): by push, then by channel, then by start."""

    def __init__(self, min_blocks: int = PING_MIN_BLOCKS):
        if not 1 <= int(min_blocks) <= 64:
            raise ValueError("min_blocks must lie within 1..64")
        self.min_blocks = int(min_blocks)
        self.base = 0
        self.open = {}
        self.up_blocks = self.total_blocks = 0

    def _finish(self, c, out):
        run = self.open.pop(c, None)
        if run is not None and run["blocks"] >= self.min_blocks:
            out.append(run)

    def push(self, records, energies) -> list:
        """records: PING_DTYPE [channel] of one push; energies: its E [channel][nb] (Pings.energies, or
        HipDecoder.wideband_ping_blocks()).  Returns the events that closed in this push."""
        out = []
        nb = 0
        for c in range(len(records)):
            mask, nb, R = int(records["up_mask"][c]), int(records["blocks"][c]), int(records["reference"][c])
            for b in range(nb):
                if (mask >> b) & 1:
                    e = int(energies[c][b])
                    run = self.open.get(c)
                    if run is None:
                        self.open[c] = dict(channel=c, start=self.base + b, blocks=1, peak=e, reference=R)
                    else:
                        run["blocks"] += 1
                        if e > run["peak"]:
                            run["peak"], run["reference"] = e, R
                    self.up_blocks += 1
                else:
                    self._finish(c, out)
            self.total_blocks += nb
        self.base += nb
        return out

    def close(self) -> list:
        out = []
        for c in sorted(self.open):
            self._finish(c, out)
        return out


def ping_event_line(event: dict, offset_hz: int) -> str:
    """One line of the event log of msk144hipdecoder --wideband-pings=FILE; start and dur are block counts x 0.008 s."""
    s, d = event["start"] * 8, event["blocks"] * 8
    return (f"ping ch={event['channel']} offset={int(offset_hz)} start={s // 1000}.{s % 1000:03d} dur={d // 1000}.{d % 1000:03d} blocks={event['blocks']} "
            f"peak={event['peak']} ref={event['reference']} peak_db={10.0 * math.log10(event['peak'] / event['reference']):.1f}")


# ---- per-channel waterfall (msk144_set_wideband_waterfall) ----

WATERFALL_BINS = PING_BLOCK          # one 96-point transform per block of the ping detector: 125 Hz per bin
WATERFALL_ROWS = PING_MAX_BLOCKS
WATERFALL_FLOOR = 1e-10              # -100 dB under a tone of 1 LSB on a bin centre
WATERFALL_CARRIER_DB = 10.0          # the carrier rule of the program's summary: a design parameter


def waterfall_window() -> np.ndarray:
    """The default window of the contract, periodic Hann: w[i] = 0.5 - 0.5 cos(2 pi i / 96), float64 (the library's own is
    msk144host_wideband_waterfall_window)."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WATERFALL_BINS, dtype=np.float64) / WATERFALL_BINS)


def waterfall_full(window=None) -> float:
    """(sum w)^2 over the f32 window the device holds: what a tone of 1 LSB on a bin centre reads, 0 dB of the program's output."""
    w = waterfall_window() if window is None else np.asarray(window, dtype=np.float64)
    s = 0.0
    for v in w.astype(np.float32):
        s += float(v)
    return s * s


def waterfall_hz(j: int) -> int:
    """(j - 48) x 125 Hz: slot j of a row from the channel's offset."""
    return (int(j) - WATERFALL_BINS // 2) * (12000 // WATERFALL_BINS)


def waterfall_db(power, full: float) -> np.ndarray:
    """10 log10(max(P / (sum w)^2, 1e-10)), value by value with math.log10 as the program does."""
    p = np.asarray(power, dtype=np.float64)
    out = np.empty(p.shape, dtype=np.float64)
    flat = out.reshape(-1)
    for n, v in enumerate(p.reshape(-1)):
        r = float(v) / full
        flat[n] = 10.0 * math.log10(r) if r > WATERFALL_FLOOR else 10.0 * math.log10(WATERFALL_FLOOR)
    return out


def waterfall_line(channel: int, offset_hz: int, block: int, row, full: float) -> str:
    """One line of msk144hipdecoder --wideband-waterfall=FILE: row [96] of global block g, t = 0.008 g, two decimals per bin."""
    ms = int(block) * 8
    db = ",".join("0.00" if s == "-0.00" else s for s in ("%.2f" % v for v in waterfall_db(row, full)))
    return f"wf ch={int(channel)} offset={int(offset_hz)} block={int(block)} t={ms // 1000}.{ms % 1000:03d} db={db}"


class Waterfall:
    """The waterfall of the contract (include/msk144hip.h) in float64, fed hops: P_b[k] = |sum_i w[i] x[96b + i] e^{-j2pi ik/96}|^2 of
    the int8 hops x = I + jQ, by a direct product with the exact 96 x 96 matrix (the angle reduced mod 96 in integers), returned in
    ascending frequency: rows[c][b][j] is bin (j - 48) mod 96.  The window is the f32 the device stores, as float64.  Nothing is
    carried from push to push."""

    def __init__(self, window=None):
        w = waterfall_window() if window is None else np.asarray(window, dtype=np.float64)
        if w.shape != (WATERFALL_BINS,) or not np.all(np.isfinite(w)):
            raise ValueError("the window must hold 96 finite values")
        self.window = w.astype(np.float32).astype(np.float64)
        i = np.arange(WATERFALL_BINS, dtype=np.int64)
        k = (i - WATERFALL_BINS // 2) % WATERFALL_BINS
        self.matrix = self.window[:, None] * np.exp(-2j * np.pi * ((i[:, None] * k[None, :]) % WATERFALL_BINS) / WATERFALL_BINS)   # [i][j]

    def push(self, q) -> np.ndarray:
        """float64 [channel][nb][96] from the int8 hops q [channel][M][2] of one push."""
        q = np.asarray(q)
        if q.ndim != 3 or q.shape[1] % WATERFALL_BINS or q.shape[2] != 2:
            raise ValueError("hops must be [channel][M][2] with M a multiple of 96")
        x = q[..., 0].astype(np.float64) + 1j * q[..., 1].astype(np.float64)
        X = x.reshape(q.shape[0], -1, WATERFALL_BINS) @ self.matrix
        return X.real ** 2 + X.imag ** 2


def waterfall_sums(rows) -> np.ndarray:
    """float64 [channel][96]: the f32 rows [channel][nb][96] added one after another in double, b ascending."""
    r = np.asarray(rows, dtype=np.float32)
    out = np.zeros((r.shape[0], r.shape[2]), dtype=np.float64)
    for b in range(r.shape[1]):
        out += r[:, b, :].astype(np.float64)
    return out


class PingSpectra:
    """The frequency of a ping event (csrc/wideband.h PingSpectra, the rule the program runs): one float64 accumulator [96] per channel;
    blocks are taken in stream order, a block that is up adds its row, a block that is not up clears it.  push and close return one
    frequency in Hz - (j* - 48) x 125, j* the lowest j at the maximum - per event PingEvents reports from the same records (runs of
    at least min_blocks blocks), in its order."""

    def __init__(self, channels: int, min_blocks: int = PING_MIN_BLOCKS):
        self.min_blocks = int(min_blocks)
        self.acc = np.zeros((int(channels), WATERFALL_BINS), dtype=np.float64)
        self.blocks = [0] * int(channels)

    def _finish(self, c, out):
        if self.blocks[c] >= self.min_blocks:
            out.append(waterfall_hz(int(np.argmax(self.acc[c]))))
        self.acc[c] = 0.0
        self.blocks[c] = 0

    def push(self, records, rows) -> list:
        """records: PING_DTYPE [channel] of one push; rows: its waterfall [channel][nb][96] (HipDecoder.wideband_waterfall())."""
        out = []
        for c in range(len(records)):
            mask, nb = int(records["up_mask"][c]), int(records["blocks"][c])
            for b in range(nb):
                if (mask >> b) & 1:
                    self.acc[c] += np.asarray(rows[c][b], dtype=np.float32).astype(np.float64)
                    self.blocks[c] += 1
                else:
                    self._finish(c, out)
        return out

    def close(self) -> list:
        out = []
        for c in range(len(self.blocks)):
            self._finish(c, out)
        return out


# ---- the hop rule that the capture and the gate share (csrc/wideband.h: hop_up_bits, since_next) ----

HOP_BLOCKS = HOP_OUT // PING_BLOCK   # 27
SINCE_QUIET = 17                     # a channel's `since`, the hops since its last active one, saturates here


def hop_masks(records, c: int, first: bool) -> list:
    """The 27 up bits of each hop that a push brings channel c, oldest hop first: hops 0 and 1 of a first push, else the newest
    alone.  records: PING_DTYPE [channel], or None: the detector was off, no block is up."""
    mask = 0 if records is None else int(records["up_mask"][c])
    hop_mask = (1 << HOP_BLOCKS) - 1
    return [mask & hop_mask, (mask >> HOP_BLOCKS) & hop_mask] if first else [mask & hop_mask]


def since_next(since: int, active: bool) -> int:
    return 0 if active else min(since + 1, SINCE_QUIET)


# ---- per-ping capture of a channel's hops (msk144_set_wideband_capture) ----

# msk144_wideband_capture_unit (include/msk144hip.h); HipDecoder.wideband_capture() returns the same records
CAPTURE_DTYPE = np.dtype([("channel", "<i4"), ("flags", "<i4"), ("hop", "<i8")])
assert CAPTURE_DTYPE.itemsize == 16
CAPTURE_UNIT_BYTES = 2 * HOP_OUT     # one hop of one channel: 2592 int8 I/Q pairs
CAPTURE_HOP_BLOCKS = HOP_BLOCKS
CAPTURE_MAX_POST = 16
CAPTURE_MAX_UNITS = 16384
CAPTURE_MAX_LISTED = 16
CAPTURE_ACTIVE, CAPTURE_LISTED, CAPTURE_PRE, CAPTURE_TAIL = 1, 2, 4, 8   # the bits of `flags`
# the defaults of msk144_wideband_capture_params (csrc/wideband.h CaptureParams): design parameters, not measurements
CAPTURE_DEFAULTS = dict(pre=1, post=1)


def capture_default_max_units(channels: int) -> int:
    """What the program and HipDecoder.set_wideband_capture take: min(2 x channels, 512)."""
    return min(2 * int(channels), 512)


class Capture:
    """The capture rule of the contract (include/msk144hip.h) in Python integers, push by push.  Per channel: the hops since the last
    active one (SINCE_QUIET: none that counts) and whether the newest hop was emitted.  push() takes the ping records of one push
    (PING_DTYPE [channel], or None: the detector was off) and returns (units, total): the stored units as CAPTURE_DTYPE, by channel
    then by hop, and the number of units the push had.  restart() stands for msk144_set_wideband_capture in mid-stream: the state is
    cleared, the hop count stays.  `hop` is the newest hop of the last push; a model that joins a stream in mid-stream sets it."""

    def __init__(self, channels: int, pre: int = 1, post: int = 1, max_units=None, listed=()):
        max_units = capture_default_max_units(channels) if max_units is None else int(max_units)
        listed = [int(c) for c in listed]
        if pre not in (0, 1):
            raise ValueError("pre must be 0 or 1")
        if not 0 <= int(post) <= CAPTURE_MAX_POST:
            raise ValueError("post must lie within 0..16 hops")
        if not 1 <= max_units <= CAPTURE_MAX_UNITS:
            raise ValueError("max_units must lie within 1..16384")
        if len(listed) > CAPTURE_MAX_LISTED or len(set(listed)) != len(listed) or any(not 0 <= c < channels for c in listed):
            raise ValueError("up to 16 different listed channels within the channels")
        self.channels, self.pre, self.post, self.max_units, self.listed = int(channels), int(pre), int(post), max_units, frozenset(listed)
        self.hop = 0
        self.restart()

    def restart(self):
        self.since = [SINCE_QUIET] * self.channels
        self.emitted = [False] * self.channels

    def push(self, records, first: bool):
        if first:
            self.restart()
        self.hop = 1 if first else self.hop + 1
        units = []
        for c in range(self.channels):
            listed = c in self.listed
            masks = hop_masks(records, c, first)
            for k, active in enumerate(masks, start=self.hop + 1 - len(masks)):   # hops 0 and 1 of a first push, else the newest
                self.since[c] = since_next(self.since[c], active != 0)
                near = self.since[c] <= self.post
                if k > 0 and self.pre and active and not self.emitted[c]:
                    units.append((c, CAPTURE_PRE, k - 1))
                if listed or near:
                    units.append((c, (CAPTURE_ACTIVE if active else 0) | (CAPTURE_LISTED if listed else 0) | (CAPTURE_TAIL if near and not active else 0), k))
                self.emitted[c] = listed or near
        return np.array(units[:self.max_units], dtype=CAPTURE_DTYPE), len(units)


# ---- the gate: only the channels with activity are decoded (msk144_set_wideband_gate) ----

GATE_MAX_HOLD = 16
GATE_QUIET = SINCE_QUIET
GATE_HOP_BLOCKS = HOP_BLOCKS
assert CAPTURE_MAX_POST < SINCE_QUIET and GATE_MAX_HOLD < SINCE_QUIET
# the defaults of msk144_wideband_gate_params (csrc/wideband.h GateParams): design parameters, not measurements
GATE_DEFAULTS = dict(hold=1, min_up=1)


class Gate:
    """The gate rule of the contract (include/msk144hip.h) in Python integers, push by push.  Per channel `since`: the hops since
    the last active one, saturating at SINCE_QUIET.  push() takes the ping records of one push (PING_DTYPE [channel], or None: the
    detector was off) and returns (list, total): the channels whose window the push decodes as int32, ascending, at most
    max_channels of them, and the number that qualified.  restart() stands for msk144_set_wideband_gate in mid-stream."""

    def __init__(self, channels: int, hold: int = 1, min_up: int = 1, max_channels=None, always=()):
        channels = int(channels)
        max_channels = channels if not max_channels else int(max_channels)
        always = [int(c) for c in always]
        if not 0 <= int(hold) <= GATE_MAX_HOLD:
            raise ValueError("hold must lie within 0..16 hops")
        if not 1 <= int(min_up) <= GATE_HOP_BLOCKS:
            raise ValueError("min_up must lie within 1..27 blocks")
        if not 1 <= max_channels <= channels:
            raise ValueError("max_channels must lie within 1..channels")
        if any(not 0 <= c < channels for c in always):
            raise ValueError("an always channel is out of range")
        self.channels, self.hold, self.min_up, self.max_channels, self.always = channels, int(hold), int(min_up), max_channels, frozenset(always)
        self.restart()

    def restart(self):
        self.since = [GATE_QUIET] * self.channels

    def push(self, records, first: bool):
        if first:
            self.restart()
        chosen = []
        for c in range(self.channels):
            for bits in hop_masks(records, c, first):
                self.since[c] = since_next(self.since[c], bin(bits).count("1") >= self.min_up)
            if c in self.always or self.since[c] <= self.hold:
                chosen.append(c)
        return np.array(chosen[:self.max_channels], dtype=np.int32), len(chosen)


def capture_segment_name(channel: int, hop: int) -> str:
    return f"ch{int(channel)}_hop{int(hop)}.cs8"


def capture_log_line(channel: int, offset_hz: int, hop: int, hops: int) -> str:
    """One line of DIR/capture.log of msk144hipdecoder --wideband-capture=DIR; t = 0.216 x hop."""
    ms = int(hop) * 216
    return f"capture ch={int(channel)} offset={int(offset_hz)} hop={int(hop)} t={ms // 1000}.{ms % 1000:03d} hops={int(hops)} file={capture_segment_name(channel, hop)}"


class CaptureSegments:
    """The file rule of --wideband-capture=DIR (csrc/wideband.h CaptureSegments): a channel's unit continues the channel's open segment
    iff its hop is the segment's last hop + 1, otherwise the open segment ends and DIR/ch<c>_hop<k0>.cs8 begins.  Every write is
    open-append-close.  A segment that ends - when the channel's next unit does not continue it, or at close() - appends one line to
    DIR/capture.log.  The last four ended segments of a channel and its open one are remembered for locate().  A segment's first
    write truncates a file of that name and the log is only appended to: the program starts capture.log afresh with every run."""

    REMEMBERED = 4

    def __init__(self, directory: str, offsets_hz: Sequence[int]):
        self.dir, self.offsets = str(directory), [int(f) for f in offsets_hz]
        self.open = {}   # channel -> [k0, hops]
        self.past = {}   # channel -> the last ended (k0, hops), oldest first
        self.segments = self.hops = 0

    @property
    def bytes(self) -> int:
        return self.hops * CAPTURE_UNIT_BYTES

    def _finish(self, c):
        k0, n = self.open.pop(c)
        with open(os.path.join(self.dir, "capture.log"), "a") as f:
            f.write(capture_log_line(c, self.offsets[c], k0, n) + "\n")
        self.past[c] = (self.past.get(c, []) + [(k0, n)])[-self.REMEMBERED:]

    def push(self, units, data):
        """units: CAPTURE_DTYPE [count] of one push; data: their int8 rows, [count][2592][2] or [count][5184]."""
        data = np.ascontiguousarray(data, dtype=np.int8).reshape(len(units), CAPTURE_UNIT_BYTES)
        for u in range(len(units)):
            c, k = int(units["channel"][u]), int(units["hop"][u])
            if c in self.open and k != sum(self.open[c]):
                self._finish(c)
            if c not in self.open:
                self.open[c] = [k, 0]
                self.segments += 1
            with open(os.path.join(self.dir, capture_segment_name(c, self.open[c][0])), "ab" if self.open[c][1] else "wb") as f:
                f.write(data[u].tobytes())
            self.open[c][1] += 1
            self.hops += 1

    def close(self):
        for c in sorted(self.open):
            self._finish(c)

    def locate(self, channel: int, block: int) -> str:
        """What a ping line gains for an event of `channel` that starts at global block `block`: ' file=<name> at=<sample offset of
        that block in the file>', or ' file=-' when the hop it lies in is in none of the remembered segments."""
        k = int(block) // CAPTURE_HOP_BLOCKS
        spans = ([tuple(self.open[channel])] if channel in self.open else []) + self.past.get(channel, [])
        for k0, n in spans:
            if k0 <= k < k0 + n:
                return f" file={capture_segment_name(channel, k0)} at={(k - k0) * HOP_OUT + int(block) % CAPTURE_HOP_BLOCKS * PING_BLOCK}"
        return " file=-"


class Channeliser:
    """The contract, push by push: keeps the history input samples and the output index m like the device does.

    Any rate Fs = 12000 P/Q runs the polyphase form, branch by branch: outputs m = mr + Q a read x[n0 + a P - k] with the taps
    h[r + kQ], r = mr P mod Q, n0 = floor(mr P/Q).  Fs = D x 12000 is Q = 1: the one branch (0, 0, all taps), D = P."""

    def __init__(self, rate_hz: int, offsets_hz: Sequence[int], taps: Optional[np.ndarray] = None, K: int = 16, gain=100.0):
        """gain: one number or one per channel; it may be replaced between pushes (self.gain)."""
        if rate_hz <= 0 or rate_hz % 125:
            raise ValueError("rate must be a positive multiple of 125 Hz")
        self.P, self.Q = rate_ratio(rate_hz)
        if self.Q == 1:
            self.D = self.P
        self.rate = int(rate_hz)
        self.offsets = np.asarray(offsets_hz, dtype=np.int64)
        self.taps = default_taps_for_rate(rate_hz, K) if taps is None else np.asarray(taps, dtype=np.float64)
        self.L = len(self.taps)
        self.gain = gain
        # branch taps by output residue mr: (r, n0, G_r [channel][K_r])
        self.branches = []
        for mr in range(self.Q):
            r, n0 = mr * self.P % self.Q, mr * self.P // self.Q
            self.branches.append((r, n0, tap_matrix(rate_hz, self.offsets, self.taps[r::self.Q])))
        self.reset()

    @property
    def n_hist(self) -> int:
        """Input samples kept between pushes: ceil(L/Q) - 1 (L - 1 for Q = 1)."""
        return -(-self.L // self.Q) - 1

    def reset(self):
        self.hist = np.zeros(self.n_hist, dtype=np.complex128)
        self.m = 0

    def filter(self, x: np.ndarray) -> np.ndarray:
        """complex y [channel][M] of the next len(x) Q/P output samples (history and m advance)."""
        x = np.asarray(x, dtype=np.complex128)
        P, Q, H = self.P, self.Q, self.n_hist
        if len(x) % P:
            raise ValueError("a push carries a whole number of output samples per branch (a multiple of Q outputs)")
        M = len(x) * Q // P
        A = M // Q
        xp = np.concatenate([self.hist, x])
        y = np.empty((len(self.offsets), M), dtype=np.complex128)
        for mr, (r, n0, G) in enumerate(self.branches):
            k = np.arange(G.shape[1])
            GT = G.T
            for a0 in range(0, A, 256):
                a = np.arange(a0, min(A, a0 + 256))
                idx = (H + n0 + a * P)[:, None] - k[None, :]
                X = np.where(idx >= 0, xp[np.maximum(idx, 0)], 0)      # x[n0 + aP - k]; before the stream: 0
                y[:, mr + Q * a] = (X @ GT).T
        m = self.m + np.arange(M, dtype=np.int64)
        n = (m * P) // Q                                                 # n_m, from the first sample of the stream
        f = np.mod(self.offsets, self.rate)
        ph = np.mod(f[:, None] * np.mod(n, self.rate)[None, :], self.rate).astype(np.float64) / self.rate
        y *= np.exp(-2j * np.pi * ph)
        self.hist = xp[len(xp) - H:].copy() if H > 0 else self.hist
        self.m += M
        return y

    def push(self, x: np.ndarray, first: bool = False) -> Tuple[np.ndarray, int]:
        """(int8 [channel][M][2], clipped components) of one push; first=True restarts the stream."""
        if first:
            self.reset()
        return quantise(self.filter(x), self.gain)


class AnalysisBank:
    """Stage 1 of the two-stage contract, push by push, in polyphase form (16 MACs per input sample at K1 = 8, the DFT only for the
    requested bands):
        s_k[n] = (-1)^{k n} sum_{p<64} e^{+j2pi (k p mod 64)/64} u_p[n],   u_p[n] = sum_q h1[p + 64 q] x[32 n - p - 64 q]
    which is the contract's sum over l = p + 64 q.  Keeps the last L1 - 1 input samples and the frame index n."""

    CHUNK = 1 << 15   # frames per numpy block

    def __init__(self, h1: np.ndarray, bands: Sequence[int]):
        self.h1 = np.asarray(h1, dtype=np.float64)
        self.L1 = len(self.h1)
        if self.L1 % BANDS:
            raise ValueError("the bank filter has 64 K1 taps")
        self.K1 = self.L1 // BANDS
        self.bands = np.mod(np.asarray(bands, dtype=np.int64), BANDS)
        p = np.arange(BANDS)
        self.W = np.exp(2j * np.pi * np.mod(p[:, None] * self.bands[None, :], BANDS) / BANDS)   # [p][band]
        self.reset()

    def reset(self):
        self.hist = np.zeros(self.L1 - 1, dtype=np.complex128)
        self.n = 0

    def polyphase(self, x: np.ndarray) -> np.ndarray:
        """u [frames][64] of the next len(x)/32 frames (history and n are not advanced)."""
        xp = np.concatenate([self.hist, np.asarray(x, dtype=np.complex128)])
        F = len(x) // BANK_DECIMATION
        u = np.empty((F, BANDS), dtype=np.complex128)
        p = np.arange(BANDS)
        for f0 in range(0, F, self.CHUNK):
            f = np.arange(f0, min(F, f0 + self.CHUNK))
            base = (self.L1 - 1) + BANK_DECIMATION * f[:, None] - p[None, :]
            acc = np.zeros((len(f), BANDS), dtype=np.complex128)
            for q in range(self.K1):
                acc += self.h1[p + BANDS * q][None, :] * xp[base - BANDS * q]
            u[f0:f0 + len(f)] = acc
        return u

    def advance(self, x: np.ndarray):
        xp = np.concatenate([self.hist, np.asarray(x, dtype=np.complex128)])
        self.hist = xp[len(xp) - (self.L1 - 1):].copy()
        self.n += len(x) // BANK_DECIMATION

    def push(self, x: np.ndarray) -> np.ndarray:
        """complex s [band][frames] of the next len(x)/32 frames, for self.bands in order (history and n advance)."""
        if len(x) % BANK_DECIMATION:
            raise ValueError("a push carries whole 32-sample frames")
        u = self.polyphase(x)
        n = self.n + np.arange(u.shape[0], dtype=np.int64)
        s = (u @ self.W).T * np.where((self.bands[:, None] * n[None, :]) % 2 == 1, -1.0, 1.0)
        self.advance(x)
        return s


class TwoStage:
    """The two-stage contract above 6.144 Msps, push by push: AnalysisBank over the stream, then the existing Channeliser at Fs/32
    on each occupied band with the residual offsets of its channels.  filter(x) -> y [channel][M] in channel order."""

    def __init__(self, rate_hz: int, offsets_hz: Sequence[int], taps: Optional[np.ndarray] = None, K: int = 16, gain=100.0,
                 bank_taps: Optional[np.ndarray] = None):
        """gain: one number or one per channel, as for Channeliser."""
        if not is_bank_rate(rate_hz):
            raise ValueError("the two-stage bank takes multiples of 8000 Hz above 6144000 up to 61440000")
        self.rate = int(rate_hz)
        self.rate2 = self.rate // BANK_DECIMATION
        self.offsets = np.asarray(offsets_hz, dtype=np.int64)
        self.h1 = default_bank_taps(rate_hz) if bank_taps is None else np.asarray(bank_taps, dtype=np.float64)
        k = np.mod(bank_band(rate_hz, self.offsets), BANDS)
        self.bands = sorted(set(int(b) for b in k))
        self.members = [np.flatnonzero(k == b) for b in self.bands]
        resid = bank_residual(rate_hz, self.offsets)
        self.stage1 = AnalysisBank(self.h1, self.bands)
        self.stage2 = [Channeliser(self.rate2, resid[m], taps=taps, K=K, gain=gain) for m in self.members]
        self.taps = self.stage2[0].taps
        self.gain = gain

    def reset(self):
        self.stage1.reset()
        for ch in self.stage2:
            ch.reset()

    def filter(self, x: np.ndarray) -> np.ndarray:
        s = self.stage1.push(x)
        M = s.shape[1] * self.stage2[0].Q // self.stage2[0].P
        y = np.empty((len(self.offsets), M), dtype=np.complex128)
        for j, (m, ch) in enumerate(zip(self.members, self.stage2)):
            y[m] = ch.filter(s[j])
        self.last_subbands = s
        return y

    def push(self, x: np.ndarray, first: bool = False) -> Tuple[np.ndarray, int]:
        if first:
            self.reset()
        return quantise(self.filter(x), self.gain)


def naive_channel(x: np.ndarray, rate_hz: int, offset_hz: int, taps: np.ndarray) -> np.ndarray:
    """Mix by e^{-j2pi f_c n/Fs}, filter with h, keep every D-th sample: y[m] = (h * (x e^{-j2pi f_c n/Fs}))[mD]."""
    D = rate_hz // OUT_RATE
    n = np.arange(len(x), dtype=np.int64)
    mixed = x * np.exp(-2j * np.pi * np.mod(offset_hz * n, rate_hz).astype(np.float64) / rate_hz)
    return np.convolve(mixed, taps)[:len(x)][::D]


def naive_resampled_channel(x: np.ndarray, rate_hz: int, offset_hz: int, taps: np.ndarray) -> np.ndarray:
    """Mix by e^{-j2pi f_c n/Fs}, upsample by Q (zero-stuff), filter with h at Q Fs, keep every P-th sample:
    y[m] = (h * u)[mP] with u[nQ] = x[n] e^{-j2pi f_c n/Fs} and zeros between.  The filter is evaluated only at the kept samples."""
    P, Q = rate_ratio(rate_hz)
    n = np.arange(len(x), dtype=np.int64)
    mixed = x * np.exp(-2j * np.pi * np.mod(offset_hz * n, rate_hz).astype(np.float64) / rate_hz)
    u = np.zeros(len(x) * Q, dtype=np.complex128)
    u[::Q] = mixed
    M = len(x) * Q // P
    idx = (np.arange(M, dtype=np.int64) * P)[:, None] - np.arange(len(taps))[None, :]
    U = np.where(idx >= 0, u[np.maximum(idx, 0)], 0)
    return U @ taps


# ---- scene synthesis ----

def _upsample(bb: np.ndarray, D: int) -> np.ndarray:
    """Band-limited interpolation by D (spectrum zero-padded): a 12 kHz baseband at D*12000 Hz with no images."""
    n = len(bb)
    S = np.fft.fft(bb)
    P = np.zeros(n * D, dtype=np.complex128)
    h = n // 2
    P[:h] = S[:h]
    P[-(n - h):] = S[h:]
    return np.fft.ifft(P) * D


def _resample(bb: np.ndarray, N: int) -> np.ndarray:
    """Band-limited resampling of a 12 kHz baseband to N samples (spectrum zero-padded from len(bb) to N bins)."""
    n = len(bb)
    S = np.fft.fft(bb)
    R = np.zeros(N, dtype=np.complex128)
    h = n // 2
    R[:h] = S[:h]
    R[-(n - h):] = S[h:]
    return np.fft.ifft(R) * (N / n)


def _synth_wideband_rational(n_out, rate_hz, pings, noise_sigma, rng, fmt):
    P, Q = rate_ratio(rate_hz)
    if n_out % Q:
        raise ValueError(f"n_out must be a multiple of Q = {Q} at {rate_hz} Hz")
    N = n_out * P // Q
    x = rng.normal(0.0, noise_sigma, N) + 1j * rng.normal(0.0, noise_sigma, N) if noise_sigma > 0 else np.zeros(N, dtype=np.complex128)
    ref = noise_sigma if noise_sigma > 0 else 1.0
    n = np.arange(N)
    for f_c, p in pings:
        bb = synth._ping_baseband(p)
        amp = np.sqrt(2.0 * ref ** 2 * (2500.0 / rate_hz) * 10.0 ** (p.snr_db / 10.0))
        full = np.zeros(n_out, dtype=np.complex128)
        m1 = min(n_out, p.start + len(bb))
        if m1 <= p.start:
            continue
        full[p.start:m1] = bb[:m1 - p.start]
        carrier = np.exp(1j * (2 * np.pi * (f_c + p.freq_hz) * n / rate_hz + p.phase))
        x += amp * _resample(full, N) * carrier
    return write_samples(x, fmt)


def _synth_wideband_bank(n_out, rate_hz, pings, noise_sigma, rng, fmt):
    """As _synth_wideband_rational, but each ping is FFT-resampled over its own span only (plus a margin), so that a scene at tens of
    Msps costs what its pings cost; a span starts at a multiple of Q output samples."""
    P, Q = rate_ratio(rate_hz)
    if n_out % Q:
        raise ValueError(f"n_out must be a multiple of Q = {Q} at {rate_hz} Hz")
    N = n_out * P // Q
    x = rng.normal(0.0, noise_sigma, N) + 1j * rng.normal(0.0, noise_sigma, N) if noise_sigma > 0 else np.zeros(N, dtype=np.complex128)
    ref = noise_sigma if noise_sigma > 0 else 1.0
    margin = 96 * Q
    for f_c, p in pings:
        bb = synth._ping_baseband(p)
        amp = np.sqrt(2.0 * ref ** 2 * (2500.0 / rate_hz) * 10.0 ** (p.snr_db / 10.0))
        m0 = max(0, (p.start - margin) // Q * Q)
        m1 = min(n_out, -(-(p.start + len(bb) + margin) // Q) * Q)
        if min(n_out, p.start + len(bb)) <= p.start:
            continue
        seg = np.zeros(m1 - m0, dtype=np.complex128)
        k1 = min(n_out, p.start + len(bb))
        seg[p.start - m0:k1 - m0] = bb[:k1 - p.start]
        n0, n1 = m0 * P // Q, m1 * P // Q
        n = np.arange(n0, n1)
        carrier = np.exp(1j * (2 * np.pi * (f_c + p.freq_hz) * n / rate_hz + p.phase))
        x[n0:n1] += amp * _resample(seg, n1 - n0) * carrier
    return write_samples(x, fmt)


def synth_wideband(n_out: int, rate_hz: int, pings: Iterable[Tuple[int, synth.Ping]], noise_sigma: float, rng: np.random.Generator,
                   fmt: str = "cu8") -> np.ndarray:
    """Raw interleaved components of a wideband scene n_out output samples long (n_out * P/Q wideband samples; n_out * D for an
    integer rate, otherwise n_out must be a multiple of Q and each ping is FFT-resampled over the whole scene).

    pings: (channel offset f_c in Hz, synth.Ping) pairs; the Ping's start is in 12 kHz samples and its freq_hz is the frequency
    inside the channel, so the carrier lands at f_c + freq_hz.  noise_sigma: per rail, in full-scale units (1 = the format's full
    scale).  SNR in 2500 Hz as in synth.synth_iq: 10log10(A^2 / (2 sigma^2 2500 / Fs))."""
    if is_bank_rate(rate_hz):
        return _synth_wideband_bank(n_out, rate_hz, pings, noise_sigma, rng, fmt)
    if rate_ratio(rate_hz)[1] > 1:
        return _synth_wideband_rational(n_out, rate_hz, pings, noise_sigma, rng, fmt)
    D = rate_hz // OUT_RATE
    N = n_out * D
    x = rng.normal(0.0, noise_sigma, N) + 1j * rng.normal(0.0, noise_sigma, N) if noise_sigma > 0 else np.zeros(N, dtype=np.complex128)
    ref = noise_sigma if noise_sigma > 0 else 1.0
    for f_c, p in pings:
        bb = synth._ping_baseband(p)
        amp = np.sqrt(2.0 * ref ** 2 * (2500.0 / rate_hz) * 10.0 ** (p.snr_db / 10.0))
        up = _upsample(bb, D)
        n0 = p.start * D
        n1 = min(N, n0 + len(up))
        if n1 <= n0:
            continue
        n = np.arange(n0, n1)
        carrier = np.exp(1j * (2 * np.pi * (f_c + p.freq_hz) * n / rate_hz + p.phase))
        x[n0:n1] += amp * up[:n1 - n0] * carrier
    return write_samples(x, fmt)


def push_sizes(n_pushes: int, D: int):
    """Raw component counts of a first push followed by n_pushes-1 later ones, at the integer rate D x 12000 Hz."""
    return push_sizes_for_rate(n_pushes, OUT_RATE * D)


def push_sizes_for_rate(n_pushes: int, rate_hz: int):
    """The same for any rate: 2 x 5184 P/Q components, then 2 x 2592 P/Q."""
    P, Q = rate_ratio(rate_hz)
    return [2 * FIRST_OUT * P // Q] + [2 * HOP_OUT * P // Q] * (n_pushes - 1)
