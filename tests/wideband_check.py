"""Checks of the wideband channeliser (csrc/channelise.hip) shared by the CPU and GPU test files.

- Reference: the float64 model (msk144cudecoder_amd/wideband.py, Channeliser) plus, per output, the magnitude sum and the tap
  count that bound the device's f32 rounding error.
- check_hops: the near-tie rule - every int8 component equals clamp(rint(v), -128, 127) unless v lies within delta of a half-integer.
- impulse_expected: exact closed forms of the output for a single unit tap, independent of Channeliser.
- sample_channels, random_taps, gain_for, offsets_for, raw_input, split_pushes: configurations.
- The configurations the GPU tests run (INT_GRID, RAT_GRID, impulse tap lists, ...) live here so that the CPU sensitivity tests
  check the very cases the device is held to.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from msk144cudecoder_amd import wideband as wb

U32 = 2.0 ** -24            # unit roundoff of f32
DELTA_FACTOR = 16.0


def f32(x: float) -> float:
    """The value the C ABI carries for a float parameter (msk144_wideband_params.gain)."""
    return float(np.float32(x))


# ---- the reference ----

class Reference:
    """The float64 model of the contract with what the near-tie rule needs beside y, push by push.

    push(x, first) -> (y [C][M] complex, d [M]): d = delta(T, N, f32(gain)), the near-tie tolerance of every output, with
      T[m] = sum_k |h_k| |x[n_m - k]| over the taps of output m's branch - the same model run once more with |h| and |x| (channel
             independent: |G[c][k]| = |h_k|), which bounds |Re| and |Im| of every product sum the device forms for output m;
      N[m] = the number of taps in output m's branch (L for Q = 1, K_r = len(h[r::Q]) otherwise)."""

    def __init__(self, rate_hz: int, offsets_hz: Sequence[int], taps: Optional[np.ndarray] = None, K: int = 16, gain: float = 100.0):
        self.model = wb.Channeliser(rate_hz, offsets_hz, taps=taps, K=K, gain=gain)
        self.mag = wb.Channeliser(rate_hz, [0], taps=np.abs(self.model.taps), gain=gain)
        self.gain = gain
        P, Q = self.model.P, self.model.Q
        self.branch_taps = np.array([len(self.model.taps[(mr * P) % Q::Q]) for mr in range(Q)], dtype=np.int64)

    def push(self, x: np.ndarray, first: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        if first:
            self.model.reset()
            self.mag.reset()
        m0 = self.model.m
        y = self.model.filter(x)
        T = self.mag.filter(np.abs(x))[0].real
        N = self.branch_taps[(m0 + np.arange(y.shape[1])) % len(self.branch_taps)]
        return y, delta(T, N, f32(self.gain))


def delta(T: np.ndarray, N: np.ndarray, gain: float) -> np.ndarray:
    """delta = 16 sqrt(N + 8) 2^-24 128 gain T, the bound on |v_device - v| for one output component.

    The device forms v = 128 gain Re/Im(e^{-j phi} sum_k G_k x_k) in f32 from exact inputs (every format's samples are exact in
    f32): each G_k is rounded once to f32, every product and every accumulation step of the 2N-term real sum (N complex taps, two
    real products each; |Re G_k Re x_k| + |Im G_k Im x_k| <= |h_k| |x_k|) is rounded once, then the rotation entry, its two
    products and difference, and the scale 128 gain are rounded: N + 8 groups of roundings, each of relative size at most 2^-24
    against a partial sum bounded by T.  Rounding errors of independent data are unbiased and uncorrelated, so their sum grows as
    sqrt(N + 8) 2^-24 T (standard deviation below that); the factor 16 leaves the bound far above any random excursion while
    staying well below one LSB.  Not fitted to measured device output.  With random taps T grows as sqrt(N) times the output rms,
    so delta grows as N: about 0.002 LSB at N = 32, 0.04 at 2560, 0.3 at 10923 (K = 64 at 2.048 Msps), where most components
    count as near-ties; the sensitivity tests therefore use shapes with N of a few hundred to a few thousand."""
    return DELTA_FACTOR * np.sqrt(N + 8.0) * U32 * (128.0 * gain) * T


def check_hops(got: np.ndarray, y: np.ndarray, d: np.ndarray, gain: float, clip_got: Optional[int] = None) -> Dict:
    """The near-tie rule for one push.  got: int8 [C][M][2] device hops; y: model [C][M]; d: the tolerance per output, [M] or
    [C][M], from Reference.push or BankReference.push; gain: the configured gain (compared at its f32 value, as the ABI carries
    it); clip_got: the device's wideband_clip_count, or None.

    Every component must equal clamp(rint(v), -128, 127), v = 128 gain y, unless v lies within d (see delta(), and
    wideband_bank_check.py for two stages) of a half-integer, where either neighbour is accepted.  The clip count must equal the
    model's, give or take the near-ties on the 127.5 / -128.5 clip edges.  Returns a report; report['ok'] says whether the push
    passes."""
    v = np.stack([y.real, y.imag], axis=-1) * (128.0 * f32(gain))             # [C][M][2]
    d = np.broadcast_to(np.asarray(d)[..., None], v.shape)
    r = np.rint(v)
    want = np.clip(r, -128, 127)
    fl = np.floor(v)
    near = np.abs(v - fl - 0.5) < d
    q = got.astype(np.float64)
    alt = near & ((q == np.clip(fl, -128, 127)) | (q == np.clip(fl + 1, -128, 127)))
    bad = (q != want) & ~alt
    edge = near & ((np.abs(v - 127.5) < d) | (np.abs(v + 128.5) < d))
    clip_model = int(np.count_nonzero((r < -128) | (r > 127)))
    inside = (v > -128.5) & (v < 127.5) & (d > 0)                              # d = 0: y is exactly 0 (T = 0)
    excess = (np.abs(q - v) - 0.5)[inside] / d[inside] if np.any(inside) else np.zeros(1)
    rep = dict(components=int(v.size), near_ties=int(np.count_nonzero(near)), edge_ties=int(np.count_nonzero(edge)),
               mismatches=int(np.count_nonzero(bad)), max_excess_over_delta=float(excess.max()), max_delta_lsb=float(d.max()),
               clip_model=clip_model, clip_device=clip_got)
    rep["clip_ok"] = clip_got is None or abs(int(clip_got) - clip_model) <= rep["edge_ties"]
    rep["ok"] = rep["mismatches"] == 0 and rep["clip_ok"]
    if rep["mismatches"]:
        i = np.argwhere(bad)[0]
        rep["first_mismatch"] = dict(channel=int(i[0]), sample=int(i[1]), component=int(i[2]), got=int(q[tuple(i)]), v=float(v[tuple(i)]),
                                     delta=float(d[tuple(i)]))
    return rep


def assert_hops(got, y, d, gain, clip_got=None, what="") -> Dict:
    rep = check_hops(got, y, d, gain, clip_got)
    assert rep["mismatches"] == 0, f"{what}: {rep['mismatches']} components off the near-tie rule, first {rep.get('first_mismatch')}"
    assert rep["clip_ok"], f"{what}: clip count {clip_got}, model {rep['clip_model']} (+-{rep['edge_ties']} edge ties)"
    return rep


class Tally:
    """Sums check_hops reports over pushes and configurations, for parity_report."""

    def __init__(self):
        self.r = dict(pushes=0, components=0, near_ties=0, edge_ties=0, max_excess_over_delta=-math.inf, max_delta_lsb=0.0)

    def add(self, rep: Dict) -> Dict:
        self.r["pushes"] += 1
        for k in ("components", "near_ties", "edge_ties"):
            self.r[k] += rep[k]
        self.r["max_excess_over_delta"] = max(self.r["max_excess_over_delta"], rep["max_excess_over_delta"])
        self.r["max_delta_lsb"] = max(self.r["max_delta_lsb"], rep["max_delta_lsb"])
        return rep

    def report(self) -> Dict:
        return dict(self.r)


def old_check(got: np.ndarray, want: np.ndarray) -> Tuple[int, float]:
    """The check the suite had before the near-tie rule: (max |dq|, fraction of exact components); it passed at <= 1 and >= 0.999."""
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    return int(d.max()), float(np.count_nonzero(d == 0)) / d.size


def old_check_passes(got, want) -> bool:
    mx, exact = old_check(got, want)
    return mx <= 1 and exact >= 0.999


# ---- impulse closed forms ----

def unit_taps(L: int, j: int) -> np.ndarray:
    h = np.zeros(L)
    h[j] = 1.0
    return h


def impulse_expected(raw: np.ndarray, rate_hz: int, j: int, m0: int, M: int) -> np.ndarray:
    """int8 [M][2] of outputs m0 .. m0+M-1 for the taps e_j, offset 0, cs8 and gain 1 (q = the input component itself):
    Q = 1: raw[m D - j]; otherwise raw[(m P - j) / Q] when Q divides m P - j >= 0; 0 before the stream start.
    raw: the cs8 components of the whole stream from its first sample."""
    P, Q = wb.rate_ratio(rate_hz)
    s = np.asarray(raw, dtype=np.int8).reshape(-1, 2)
    t = (m0 + np.arange(M, dtype=np.int64)) * P - j
    ok = (t >= 0) & (t % Q == 0)
    out = np.zeros((M, 2), dtype=np.int8)
    out[ok] = s[t[ok] // Q]
    return out


def branch_impulse_taps(rate_hz: int, K: int, branches: Sequence[int]) -> List[int]:
    """Tap positions j that exercise the rational kernel's per-branch bookkeeping, for each output residue mr in branches: the
    branch's first and last tap, the last tap of phase 0 and of the last long phase (p < s_full, Kq taps) and of the first short
    phase (Kq - 1 taps), and the
    first and last tap of phase 32 when the branch has more than 32 phases (the second LDS phase chunk).  j = r + kQ, k = p + P q."""
    P, Q = wb.rate_ratio(rate_hz)
    L = K * P
    js = set()
    for mr in branches:
        r = mr * P % Q
        Kr = (L - r + Q - 1) // Q
        Kq = (Kr + P - 1) // P
        s_full = Kr - (Kq - 1) * P
        phases = min(P, Kr)
        ks = [0, Kr - 1, P * (Kq - 1), (s_full - 1) + P * (Kq - 1)]
        if s_full < phases and Kq >= 2:
            ks.append(s_full + P * (Kq - 2))
        if phases > 32:
            ks += [32, 32 + P * ((Kq if 32 < s_full else Kq - 1) - 1)]
        js.update(r + k * Q for k in ks)
    return sorted(js)


# ---- configurations ----

def sample_channels(C: int, rng: np.random.Generator, n_random: int = 32) -> np.ndarray:
    """Channels to evaluate the model on when C is large (channels are independent): every c with c % 32 in {0, 31} - the edges of
    each wave's 32 channels and of each workgroup's 128 - plus n_random others."""
    edge = [c for c in range(C) if c % 32 in (0, 31)]
    rest = np.setdiff1d(np.arange(C), edge)
    pick = rng.choice(rest, size=min(n_random, len(rest)), replace=False) if len(rest) else []
    return np.unique(np.concatenate([edge, pick]).astype(np.int64))


def random_taps(L: int, rng: np.random.Generator) -> np.ndarray:
    """Non-symmetric random taps N(0, 1)/sqrt(L): every tap matters, and none is small."""
    return rng.normal(size=L) / math.sqrt(L)


def gain_for(taps: np.ndarray, Q: int, sigma: float) -> float:
    """A gain (exact in f32) that puts the output at about 30 LSB rms per component for white input of sigma per rail: each branch
    h[r::Q] carries about |h|^2 / Q of the energy.  Gaussian output at 30 LSB rms clips in about 2e-5 of components (< 0.1 %)."""
    rms = sigma * float(np.linalg.norm(taps)) / math.sqrt(Q)
    return f32(30.0 / (128.0 * rms))


def offsets_for(rate_hz: int, C: int, rng: np.random.Generator) -> np.ndarray:
    """C offsets: 0, +-(Fs/2 - 6000), then points off every grid (random integers within the limit)."""
    lim = rate_hz // 2 - 6000
    fixed = [0, lim, -lim, 1, -(lim - 1), 6001, -12007]
    fixed = [f for f in fixed if abs(f) <= lim][:C]
    rest = rng.integers(-lim, lim + 1, size=max(0, C - len(fixed)))
    return np.array(fixed + list(rest), dtype=np.int32)


SIGMA = 0.1      # input level per rail, in full-scale units


def raw_input(rate_hz: int, n_pushes: int, fmt: str, rng: np.random.Generator, sigma: float = SIGMA) -> np.ndarray:
    """Gaussian white input of sigma per rail for n_pushes pushes, as raw components of fmt."""
    P, Q = wb.rate_ratio(rate_hz)
    n = (wb.FIRST_OUT + (n_pushes - 1) * wb.HOP_OUT) * P // Q
    return wb.write_samples(sigma * (rng.normal(size=n) + 1j * rng.normal(size=n)), fmt)


def random_cs8(rate_hz: int, n_pushes: int, rng: np.random.Generator) -> np.ndarray:
    """Uniform cs8 components over the whole range -128 .. 127, for the impulse references."""
    P, Q = wb.rate_ratio(rate_hz)
    n = (wb.FIRST_OUT + (n_pushes - 1) * wb.HOP_OUT) * P // Q
    return rng.integers(-128, 128, size=2 * n).astype(np.int8)


def split_pushes(raw: np.ndarray, rate_hz: int, n_pushes: int) -> List[np.ndarray]:
    out, pos = [], 0
    for n in wb.push_sizes_for_rate(n_pushes, rate_hz):
        out.append(raw[pos:pos + n])
        pos += n
    return out


def push_m0(i: int) -> int:
    """Output index of the first sample of push i of a stream (push 0 the first push)."""
    return 0 if i == 0 else wb.FIRST_OUT + (i - 1) * wb.HOP_OUT


# ---- the cases the GPU tests run ----

# random taps over the shape grid: (rate, K, format); C = 33
INT_GRID = [(2, 1, "cu8"), (2, 64, "cs8"), (3, 16, "cs16"), (31, 7, "cu8"), (33, 16, "cs8"), (80, 1, "cs16"), (160, 64, "cu8"), (512, 16, "cs8")]
INT_GRID = [(D * 12000, K, fmt) for D, K, fmt in INT_GRID]
RAT_GRID = [(30000, 16, "cs16"), (24125, 16, "cu8"), (250000, 1, "cs8"), (2048000, 64, "cs16"), (6143875, 16, "cu8")]
GRID_CHANNELS = 33
GRID_PUSHES = 3

# impulses, exact: integer (D, K) and tap positions; rational rates with K = 16 and branch residues
INT_IMPULSE = [(2, 16), (33, 16), (80, 3), (512, 4)]
RAT_IMPULSE = {30000: [0, 1], 24125: [0, 1, 47, 95], 2048000: [0, 1, 2]}
IMPULSE_K_RATIONAL = 16
IMPULSE_CHANNELS = 33
IMPULSE_PUSHES = 3


def int_impulse_taps(D: int, K: int) -> List[int]:
    L = K * D
    return sorted({j for j in (0, 1, D - 1, D, 31, 32, D * (K - 1), L - 1) if 0 <= j < L})


def impulse_cases() -> List[Tuple[int, int, int]]:
    """(rate, K, j) of every exact impulse test."""
    cases = [(D * 12000, K, j) for D, K in INT_IMPULSE for j in int_impulse_taps(D, K)]
    for rate, mrs in RAT_IMPULSE.items():
        cases += [(rate, IMPULSE_K_RATIONAL, j) for j in branch_impulse_taps(rate, IMPULSE_K_RATIONAL, mrs)]
    return cases


def grid_case(rate_hz: int, K: int, fmt: str, C: int = GRID_CHANNELS, n_pushes: int = GRID_PUSHES, seed: int = 0):
    """The random-tap configuration of one grid or tiling test: (offsets, taps, gain, raw), all from one seed."""
    rng = np.random.default_rng([rate_hz, K, C, seed])
    P, Q = wb.rate_ratio(rate_hz)
    taps = random_taps(K * P, rng)
    return offsets_for(rate_hz, C, rng), taps, gain_for(taps, Q, SIGMA), raw_input(rate_hz, n_pushes, fmt, rng)
