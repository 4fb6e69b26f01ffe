"""What tests/test_scan_winners_model.py (CPU) and tests/test_gpu_scan_winners.py (GPU) share: the numpy model of scan_kernel's
reduction from |S|^2 to one (position, value) per 256-position slice, and two families of windows on which the winner of a slice
sits at a run of its own.

The kernel's fold keeps a running MAXIMUM per run of eleven positions and no position (csrc/scan.hip, phases 3 to 4a): the first
lane of an octet of runs at the octet's maximum parks (maximum, run); the first strict maximum over a slice's three octets names the
winning run; that run is walked once more with strict > from 0 for the position.  slice_winners is that reduction, step by step.

  R  24 windows, six bursts of falling amplitude one frame apart: window k has its strongest burst in slice (5 k + 3) mod 21 at
     run min(k, 23)'s start plus 5 k mod 11, so every run of a slice and every position of a run holds a winner somewhere, and
     every pattern's frame set folds a sum of its own
  N  noise: every slice has a winner at an arbitrary run"""
from __future__ import annotations

import collections

import numpy as np

import scan_windows as sw

RUN = 11
RUNS_PER_SLICE = 24
OCTETS_PER_SLICE = 3

R_WINDOWS = 24
R_DEPTHS = (8, 6, 3, 1)
R_AMP = (1.0, 0.93, 0.87, 0.81, 0.76, 0.71)          # no two patterns fold equal sums
R_MIN_DECIDED = 28                                   # of the 40 groups of a window
PERIODIC_PATTERNS = (5, 6)                           # 111111 and 100100: the same frames at pos and at pos + 864 / pos + 2592
N_SEEDS = (9101, 9103, 9105)
N_CFG = sw.C_CFG[17]
N_PATTERNS = (0, 1, 2, 3, 4, 7)                      # the periodic patterns are never decided on noise
N_MIN_DECIDED = 41                                   # of the 102 groups of those patterns


def run_start(run: int) -> int:
    """First position of run `run` (24 per slice; the last restarts at 245 and overlaps the one before)."""
    sl, k = divmod(run, RUNS_PER_SLICE)
    return sw.SLICE * sl + min(RUN * k, sw.SLICE - RUN)


def slice_winners(v):
    """(pos int64 [21], value float32 [21]) of a surface v float32 [5376] (|S|^2 or xb: the order is the same), by the kernel's steps."""
    v = np.asarray(v, dtype=np.float32)
    assert v.shape == (sw.POSITIONS,)
    zero = np.float32(0.0)
    run_max = np.empty(sw.SLICES * RUNS_PER_SLICE, dtype=np.float32)
    for r in range(len(run_max)):
        best = zero
        for x in v[run_start(r):run_start(r) + RUN]:
            best = max(best, x)                       # a running maximum from 0; no position kept
        run_max[r] = best
    pos = np.zeros(sw.SLICES, dtype=np.int64)
    val = np.zeros(sw.SLICES, dtype=np.float32)
    for sl in range(sw.SLICES):
        bv, brun = None, None
        for o in range(OCTETS_PER_SLICE):
            lanes = range(RUNS_PER_SLICE * sl + 8 * o, RUNS_PER_SLICE * sl + 8 * o + 8)
            omax = max(run_max[r] for r in lanes)
            first = next(r for r in lanes if run_max[r] >= omax)          # the first lane of the octet at its maximum
            if bv is None or omax > bv:                                    # the first strict maximum over the octets, in position order
                bv, brun = omax, first
        best, idx = zero, 0
        for i, x in enumerate(v[run_start(brun):run_start(brun) + RUN]):  # the winning run once more: strict >, from 0, index 0 when nothing is greater
            if x > best:
                best, idx = x, i
        pos[sl], val[sl] = run_start(brun) + idx, best
    return pos, val


def lowest_argmax(v):
    v = np.asarray(v, dtype=np.float32).reshape(sw.SLICES, sw.SLICE)
    first = v.argmax(axis=1)
    return sw.SLICE * np.arange(sw.SLICES) + first, v[np.arange(sw.SLICES), first]


def r_start(k: int) -> int:
    sl = (5 * k + 3) % sw.SLICES
    return sw.SLICE * sl + min(RUN * k, sw.SLICE - RUN) + (5 * k) % RUN


def r_window(k: int) -> np.ndarray:
    x = np.zeros(sw.N, dtype=np.complex128)
    for m, amp in enumerate(R_AMP):
        sw._add_burst(x, (r_start(k) + sw.FRAME * m) % sw.N, amp, True)
    return x.astype(np.complex64)


def n_window(seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (rng.normal(size=sw.N) + 1j * rng.normal(size=sw.N)).astype(np.complex64)


def nonfinite_windows():
    """Family E's windows: the finite burst, the same with one NaN and with one Inf sample, and the all-zero window."""
    cd = sw.burst_window(2600)
    nan = cd.copy()
    nan[3000] = np.complex64(complex(np.nan, 0.0))
    inf = cd.copy()
    inf[3000] = np.complex64(complex(np.inf, 0.0))
    return [cd, nan, inf, np.zeros(sw.N, dtype=np.complex64)]


_CENSUS = {}


def census_of(orc, key, cfg, cd):
    """group_census at depth 8, once per window: a shallower scan sees the first patterns of the same surfaces."""
    if key not in _CENSUS:
        _CENSUS[key] = sw.group_census(orc.Oracle(depth=8, threads=8, **cfg), cd)
    return _CENSUS[key]


Geometry = collections.namedtuple("Geometry", "F D")


def gpu_scan(hip, cfg, depth, windows):
    """(candidate dumps [channels], the handle's geometry) of the windows (complex64 [channels][5184]) scanned by one handle."""
    from msk144cudecoder_amd.hipdecoder import STAGE_SCAN
    windows = np.ascontiguousarray(windows, dtype=np.complex64).reshape(-1, sw.N)
    n = len(windows)
    with hip.HipDecoder(depth=depth, channels=n, llr_block_channels=n, **cfg) as d:
        d.submit_analytic(windows)
        d.decode(STAGE_SCAN)
        return [d.dump_candidates(c) for c in range(n)], Geometry(d.F, d.D)


def scan_bytes(items):
    """The dump's bytes with the LLR rows blanked: no stage that writes them has run."""
    a = items.copy()
    a["softbits_wo_sync"] = 0
    return a.tobytes()
