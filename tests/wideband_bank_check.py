"""Checks of the two-stage wideband bank (csrc/bank.hip, then csrc/channelise.hip at Fs/32) shared by the CPU and GPU test files.

- BankReference: the float64 two-stage model (wideband.TwoStage) plus, per output, the magnitude sums that bound the device's f32
  rounding in both stages.
- The two-stage near-tie tolerance (derivation below), which BankReference.push returns for tests/wideband_check.py's check_hops.
- Slip: the same model with one deliberate error in stage 1 or in the band rule, for the sensitivity tests.
- CASES: the configurations the GPU tests run, so that the CPU tests check the very cases the device is held to.

Tolerance.  Stage 1 forms, per frame n and band, u_p = sum_q h1 x (K1 products and sums per component) and the 64-term complex sum
against f32 twiddles, from exact inputs and f32-rounded taps: K1 + 64 groups of roundings, plus a few for the taps, the twiddles and
the sign, each of relative size at most u = 2^-24 against a partial sum bounded by T1[n] = sum_l |h1_l| |x[32n - l]|.  As in
wideband_check.delta, independent roundings add as a square root, so one component of the device's s_k[n] is within
    e1[n] = F sqrt(K1 + 72) u T1[n]
of the float64 value (F = 16, the factor of wideband_check).  Stage 2 is linear: the stage-1 errors reach an output as
sum_k G_k e1[n_m - k], bounded by F sqrt(K1 + 72) u TC with TC = sum_k |h_k| T1[n_m - k] (the stage-2 magnitude model run on T1),
and stage 2 adds its own rounding, F sqrt(N + 8) u T2 with T2 = sum_k |h_k| |s[n_m - k]| (wideband_check.delta on the sub-band
stream).  With the output scale 128 gain:
    delta = F u 128 gain (sqrt(N + 8) T2 + sqrt(K1 + 72) TC).
Not fitted to measured device output.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np

import wideband_check as wc
from msk144cudecoder_amd import wideband as wb

STAGE1_EXTRA = 72     # roundings of stage 1 besides its K1 products: the 64-term DFT and 8 more


def stage1_delta(T1: np.ndarray, K1: int) -> np.ndarray:
    """Bound on |Re| and |Im| of (device s_k[n] - float64 s_k[n]) for one frame."""
    return wc.DELTA_FACTOR * math.sqrt(K1 + STAGE1_EXTRA) * wc.U32 * T1


class BankReference:
    """The two-stage model with what the near-tie rule needs, push by push.

    push(x, first) -> (y [C][M], d [C][M]): d = delta() above for every output component."""

    def __init__(self, rate_hz: int, offsets_hz: Sequence[int], taps=None, K: int = 16, gain: float = 100.0, bank_taps=None):
        self.model = wb.TwoStage(rate_hz, offsets_hz, taps=taps, K=K, gain=gain, bank_taps=bank_taps)
        m = self.model
        self.gain = gain
        self.K1 = m.stage1.K1
        self.mag1 = wb.AnalysisBank(np.abs(m.h1), [0])
        self.mag2 = [wb.Channeliser(m.rate2, [0], taps=np.abs(m.taps), gain=gain) for _ in m.bands]
        self.magc = wb.Channeliser(m.rate2, [0], taps=np.abs(m.taps), gain=gain)
        P, Q = m.stage2[0].P, m.stage2[0].Q
        self.branch_taps = np.array([len(m.taps[(mr * P) % Q::Q]) for mr in range(Q)], dtype=np.int64)

    def reset(self):
        self.model.reset()
        self.mag1.reset()
        self.magc.reset()
        for c in self.mag2:
            c.reset()

    def push(self, x: np.ndarray, first: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        if first:
            self.reset()
        m = self.model
        m0 = m.stage2[0].m
        y = m.filter(x)
        T1 = self.mag1.push(np.abs(x))[0].real
        TC = self.magc.filter(T1)[0].real
        N = self.branch_taps[(m0 + np.arange(y.shape[1])) % len(self.branch_taps)]
        g = wc.f32(self.gain)
        d = np.empty(y.shape)
        for j, members in enumerate(m.members):
            T2 = self.mag2[j].filter(np.abs(m.last_subbands[j]))[0].real
            d[members] = wc.DELTA_FACTOR * wc.U32 * 128.0 * g * (np.sqrt(N + 8.0) * T2 + math.sqrt(self.K1 + STAGE1_EXTRA) * TC)
        self.T1 = T1
        return y, d


# ---- deliberate slips ----

class _SlipBank(wb.AnalysisBank):
    def __init__(self, h1, bands, kind):
        self.kind = kind
        super().__init__(h1[::-1] if kind == "reversed_h1" else h1, bands)
        if kind == "twiddle_sign":
            self.W = np.conj(self.W)

    def push(self, x):
        if self.kind != "no_sign":
            return super().push(x)
        s = (self.polyphase(x) @ self.W).T
        self.advance(x)
        return s

    def advance(self, x):
        if self.kind != "history_frame":
            return super().advance(x)
        xp = np.concatenate([self.hist, np.asarray(x, dtype=np.complex128)])       # keeps the history one frame too early
        self.hist = xp[len(xp) - (self.L1 - 1) - wb.BANK_DECIMATION:len(xp) - wb.BANK_DECIMATION].copy()
        self.n += len(x) // wb.BANK_DECIMATION


SLIPS = ("no_sign", "band_rounding", "reversed_h1", "history_frame", "twiddle_sign")


def slipped_model(kind: str, rate_hz: int, offsets_hz, taps, K, gain, bank_taps) -> wb.TwoStage:
    """wb.TwoStage with one slip: no (-1)^{kn}; k = floor(64 f / Fs) (truncated, not rounded); h1 reversed; the bank history one
    frame off; the DFT twiddle's sign flipped."""
    m = wb.TwoStage(rate_hz, offsets_hz, taps=taps, K=K, gain=gain, bank_taps=bank_taps)
    if kind == "band_rounding":
        f = np.asarray(offsets_hz, dtype=np.int64)
        k = np.floor_divide(wb.BANDS * f, int(rate_hz))
        resid = f - k * (int(rate_hz) // wb.BANDS)
        kb = np.mod(k, wb.BANDS)
        m.bands = sorted(set(int(b) for b in kb))
        m.members = [np.flatnonzero(kb == b) for b in m.bands]
        m.stage2 = [wb.Channeliser(m.rate2, resid[mm], taps=taps, K=K, gain=gain) for mm in m.members]
        m.stage1 = wb.AnalysisBank(m.h1, m.bands)
    elif kind in SLIPS:
        m.stage1 = _SlipBank(m.h1, m.bands, kind)
    else:
        raise ValueError(kind)
    return m


# ---- the cases the GPU tests run ----

SIGMA = 0.1
K2 = 4           # channel taps per phase at Fs/32 in the random-tap cases: N of about 100-170 taps per output
K1 = 8

# (rate, format, pushes): every bank rate the issue names, every format
CASES = [(8000000, "cu8", 3), (10000000, "cs8", 3), (20000000, "cs16", 3), (61440000, "cu8", 2)]


def offsets_for(rate_hz: int, rng: np.random.Generator) -> np.ndarray:
    """Channels in several bands: 0, +-(Fs/2 - 6000), both sides of the band boundaries (2k+1) Fs/128 for k = 0, 1, -2, the largest
    residual offsets, two channels of one band 12 kHz apart, and random offsets."""
    lim = rate_hz // 2 - 6000
    b = -(-rate_hz // 128)          # the first integer at or above Fs/128: band 1 starts there
    b3 = -(-3 * rate_hz // 128)
    fixed = [0, lim, -lim, b, b - 1, b3, b3 - 1, -b3 + 1, -b3, 12000, -12000 + 1, b // 2]
    rest = rng.integers(-lim, lim + 1, size=8)
    return np.array([f for f in fixed if abs(f) <= lim] + list(rest), dtype=np.int32)


def case(rate_hz: int, fmt: str, n_pushes: int, seed: int = 0):
    """(offsets, channel taps, bank taps, gain, raw) of one random-tap case: non-symmetric random taps for both stages, white input."""
    rng = np.random.default_rng([rate_hz, n_pushes, seed])
    P2, Q2 = wb.rate_ratio(wb.stage2_rate(rate_hz))
    taps = wc.random_taps(K2 * P2, rng)
    bank_taps = wc.random_taps(wb.BANDS * K1, rng)
    gain = wc.gain_for(taps, Q2, SIGMA * float(np.linalg.norm(bank_taps)))
    return offsets_for(rate_hz, rng), taps, bank_taps, gain, wc.raw_input(rate_hz, n_pushes, fmt, rng, SIGMA)
