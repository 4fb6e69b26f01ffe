"""Analytic windows with exact ties for scan_kernel alone (tests/test_scan_windows_model.py on the CPU, tests/test_gpu_scan_windows.py
on the GPU), the host model of the scan's arg-max and slot rule, and the census that says where the oracle leaves no comparison open.

On noise-plus-ping windows a tie never occurs, so what csrc/scan.hip promises about ties - strict > in the fold, the first lane of an
octet, the first octet of a slice, the lowest slot of the arg-min, replacement on strict > only - is decided there by the seed.  Here
every window is complex64 [5184], built with plain numpy from fixed seeds, and the ties are the point:

  A  antiperiodic_window(d): x[n] = (-1)^(n // d) u[n % d] scanned at a 0 Hz hypothesis (A_CFG: F = 1, phasor exactly (1, 0)).  Negation is
     exact in every operation, so xb(pos + d) == xb(pos) bit for bit in the oracle and in the kernel alike: every slice holds its maximum
     at every d-th position, every octet, every slice and all eight slots tie, and only the tie rules decide the positions
  B  burst_window(s): one sync word (plus a short asymmetric tail, which breaks the mirror symmetry |R(tau)| = |R(-tau)| of its
     sidelobes) at ring sample s on an exactly zero background, at B_FREQ.  The only exact ties left are structural - the same C[s] seen
     at s - 336 and at s - 864 m, and the ring twins pos + 5184 - and s walks the edges of the fold: runs, octets, slices, the ring end
     multi_burst_window(): eight bursts of falling amplitude in slices 0..7 and three stronger ones later - the fast path that fills
     slots 0..7 at once, then replacements in a known order
  C  channel_burst_window(c): the burst of channel c at s = 37 + 53 c, whose strongest position names the channel

slot_rule is the ten-line model of the reference's rule, census decides per (frequency, pattern) group whether the oracle's surface
leaves anything to a tolerance, compare_exact holds the kernel to equality where it does not."""
from __future__ import annotations

import numpy as np

import numpy_model
import parity

N = 5184
POSITIONS = 5376
SLICE = 256
SLICES = 21
FRAME = 864
SECOND_SYNC = 336
SLOTS = 8
DEPTHS = tuple(range(1, 9))

# ---- family A ----
A_CFG = dict(center=0.0, width=0.0, step=2.0)       # F = 1 and frequency(0) == 0: the mixer's phasor is exactly (1, 0)
A_PERIODS = (2, 3, 6, 8, 9)                         # 864 / d is even for each: every frame of a fold adds the same values
# seeds chosen so that the d values of a period differ by >= 4 * TOL_XB_REL of the largest (tests/test_scan_windows_model.py holds them to it)
A_SEEDS = {2: 102, 3: 103, 6: 106, 8: 108, 9: 109}

# ---- family B ----
B_CFG = dict(center=1500.0, width=8.0, step=2.0)    # F = 5: five tiles on a grid of eight, three workgroups leave at once
B_FREQ = 1500.0
B_BLOCK = 2                                         # frequency(B_BLOCK) == B_FREQ
B_STARTS = (0, 3, 10, 11, 41, 87, 88, 100, 175, 176, 244, 245, 252, 253, 255, 256, 400, 1279, 1280, 2600, 4799, 5119, 5120, 5142, 5143, 5183)
B_DEPTH_STARTS = (245, 255, 5143, 5183)             # these also at depths 1..7
TAIL = 0.37 * np.exp(0.8j)                          # times cb42[:9], behind the sync word
TAIL_TAPS = 9
MULTI_FIRST = tuple(256 * k + 100 + 3 * k for k in range(8))                 # slices 0..7
MULTI_FIRST_AMPLITUDES = tuple(1.0 / 1.07 ** k for k in range(8))            # falling, ratio 1.07
MULTI_LATER = (256 * 10 + 131, 256 * 13 + 57, 256 * 16 + 201)
MULTI_LATER_AMPLITUDES = (1.5, 2.4, 1.9)

# ---- family C ----
C_SHAPES = ((1, 1), (7, 1), (8, 1), (9, 1), (3, 5), (13, 5), (64, 17))      # (channels, F)
C_CFG = {1: dict(center=1500.0, width=0.0, step=2.0), 5: B_CFG, 17: dict(center=1500.0, width=32.0, step=2.0)}

# ---- family D ----
D_STARTS = (11, 255, 5143)
D_EXPONENTS = (-50, -20, 20, 40)


def antiperiodic_window(d: int, seed: int = None) -> np.ndarray:
    rng = np.random.default_rng(A_SEEDS[d] if seed is None else seed)
    u = (rng.normal(size=d) + 1j * rng.normal(size=d)).astype(np.complex64)
    n = np.arange(N)
    assert N % (2 * d) == 0 and FRAME % (2 * d) == 0        # the ring closes on a whole number of sign pairs, and so does every frame
    return (np.where((n // d) % 2 == 1, -1.0, 1.0).astype(np.float32) * u[n % d]).astype(np.complex64)


def _add_burst(x, s, amp, tail):
    """amp * cb42 at ring samples s .. s + 41 (and the tail behind it) on the carrier e^{+j 2 pi B_FREQ n / 12000}, phase seeded by s."""
    cb = numpy_model.cb42()
    taps = np.concatenate([cb, TAIL * cb[:TAIL_TAPS]]) if tail else cb
    phase = np.random.default_rng(7000 + s).uniform(0.0, 2.0 * np.pi)
    n = (s + np.arange(len(taps))) % N
    x[n] += amp * taps * np.exp(1j * (2.0 * np.pi * B_FREQ * n / 12000.0 + phase))


def burst_window(s: int, amp: float = 1.0, tail: bool = True) -> np.ndarray:
    x = np.zeros(N, dtype=np.complex128)
    _add_burst(x, s, amp, tail)
    return x.astype(np.complex64)


def multi_burst_window() -> np.ndarray:
    x = np.zeros(N, dtype=np.complex128)
    for s, a in zip(MULTI_FIRST + MULTI_LATER, MULTI_FIRST_AMPLITUDES + MULTI_LATER_AMPLITUDES):
        _add_burst(x, s, a, True)
    return x.astype(np.complex64)


def channel_start(c: int) -> int:
    return 37 + 53 * c


def channel_burst_window(c: int) -> np.ndarray:
    return burst_window(channel_start(c))


def peak_positions(s: int):
    """The scanned positions at which a pattern-0 fold sees the sync word at ring sample s whole: s and its ghost s - 336, with ring twins."""
    ring = {s % N, (s - SECOND_SYNC) % N}
    return sorted(p for p in range(POSITIONS) if p % N in ring)


# ------------------------------------------------------------------------------------------------
# the rule, the census, the comparison
# ------------------------------------------------------------------------------------------------
def slot_rule(xb5376):
    """(pos uint32 [8], xb float32 [8]) of one (frequency, pattern) surface: per 256-position slice the lowest position of the maximum,
    then the 8-slot rule in slice order - the arg-min slot (lowest slot on ties) is replaced only on strict >, slots start at (0, 0.0)."""
    xb = np.asarray(xb5376, dtype=np.float32)
    assert xb.shape == (POSITIONS,)
    pos = np.zeros(SLOTS, dtype=np.uint32)
    val = np.zeros(SLOTS, dtype=np.float32)
    for s in range(SLICES):
        j = int(np.argmax(xb[SLICE * s:SLICE * (s + 1)]))     # first maximum: the lowest position
        w = int(np.argmin(val))                               # first minimum: the lowest slot
        if xb[SLICE * s + j] > val[w]:
            val[w], pos[w] = xb[SLICE * s + j], SLICE * s + j
    return pos, val


def _structural(pa: int, pb: int, period) -> bool:
    """Two positions fold the same values bit for bit: the same sync word seen from the first or the second sync position of a frame
    and from any frame (ring distance a + 864 j, a in {-336, 0, 336}; ring twins are distance 0) - or, on an anti-periodic window,
    a whole number of periods apart."""
    dist = (pa - pb) % N
    return any((dist - a) % FRAME == 0 for a in (-SECOND_SYNC, 0, SECOND_SYNC)) or (period is not None and dist % period == 0)


def census(xb5376, period: int = None) -> bool:
    """True when the surface leaves no comparison open (the group is DECIDED): with scale = max xb and the threshold of
    parity._near_tie_sets, 4 * TOL_XB_REL * scale,
      (a) in every slice with a positive maximum, the maximum leads every other position of the slice by the threshold;
      (b) any two positive slice maxima are that far apart, or bitwise equal at a structural distance (_structural).
    period = d (family A only) names the window's exact anti-period: positions a multiple of d from the slice's first maximum that equal it
    bit for bit are the same value, in the kernel as in the oracle, and do not open (a) - there the lowest-position rule decides, which is
    what the family is for.  A bitwise tie at any other distance, and any non-finite value, leaves the group undecided."""
    xb = np.ascontiguousarray(xb5376, dtype=np.float32)
    assert xb.shape == (POSITIONS,)
    if not np.isfinite(xb).all():
        return False
    scale = float(xb.max())
    thr = 4.0 * parity.TOL_XB_REL * scale
    val = xb.astype(np.float64).reshape(SLICES, SLICE)
    bits = xb.view(np.uint32).reshape(SLICES, SLICE)
    first = val.argmax(axis=1)
    top = val[np.arange(SLICES), first]
    offs = np.arange(SLICE)
    for s in np.nonzero(top > 0.0)[0]:
        open_ = top[s] - val[s] < thr
        open_[first[s]] = False
        if period is not None:
            open_ &= ~((bits[s] == bits[s, first[s]]) & ((offs - first[s]) % period == 0))
        if open_.any():
            return False
    live = [int(s) for s in np.nonzero(top > 0.0)[0]]
    for i, s in enumerate(live):
        for t in live[i + 1:]:
            if abs(top[s] - top[t]) >= thr:
                continue
            if bits[s, first[s]] == bits[t, first[t]] and _structural(SLICE * s + int(first[s]), SLICE * t + int(first[t]), period):
                continue
            return False
    return True


def group_census(o, cd, period: int = None):
    """bool [F][D]: census of every (frequency, pattern) surface of the oracle for this window."""
    return np.array([[census(o.scan_xb(cd, b, p), period) for p in range(o.D)] for b in range(o.F)])


def compare_exact(o, cd, items_o, items_g, period: int = None, decided=None):
    """One window's groups, the kernel's (items_g) against the oracle's (items_o = o.scan(cd)).  In a decided group (census; `decided`
    takes a group_census already made, of at least o.D patterns) pos must be EQUAL slot by slot and xb within TOL_XB_REL of the group's
    largest; slots that are bitwise equal in the oracle's group are bitwise equal in the kernel's.  An undecided group goes through
    parity.compare_scan without its rate limit (these windows are degenerate by design; the model test caps the undecided share instead).
    Returns dict(groups, decided, undecided, exact, near_ties)."""
    n = len(items_o)
    assert len(items_g) == n == o.F * o.D * SLOTS
    rep = dict(groups=n // SLOTS, decided=0, undecided=0, exact=0, near_ties=0)
    for g0 in range(0, n, SLOTS):
        b, p = int(items_o["block_idx"][g0]), int(items_o["pattern_idx"][g0])
        assert (b, p) == (g0 // SLOTS // o.D, g0 // SLOTS % o.D)
        sel = slice(g0, g0 + SLOTS)
        po, pg = items_o["pos"][sel].astype(np.int64), items_g["pos"][sel].astype(np.int64)
        xo, xg = items_o["xb"][sel], items_g["xb"][sel]
        rep["exact"] += int(np.array_equal(po, pg))
        if decided[b][p] if decided is not None else census(o.scan_xb(cd, b, p), period):
            rep["decided"] += 1
            assert np.array_equal(po, pg), ("positions differ in a decided group", dict(block=b, pattern=p, oracle=po.tolist(), kernel=pg.tolist(),
                                                                                         oracle_xb=xo.tolist(), kernel_xb=xg.tolist()))
            scale = max(float(xo.max()), 1e-30)
            assert np.all(np.abs(xo.astype(np.float64) - xg.astype(np.float64)) <= parity.TOL_XB_REL * scale), (b, p, xo.tolist(), xg.tolist())
            tie_o = xo.view(np.uint32)[:, None] == xo.view(np.uint32)[None, :]
            tie_g = xg.view(np.uint32)[:, None] == xg.view(np.uint32)[None, :]
            assert not (tie_o & ~tie_g).any(), ("slots that tie bit for bit in the oracle do not in the kernel", dict(block=b, pattern=p, oracle_xb=xo.tolist(),
                                                                                                                    kernel_xb=xg.tolist()))
        else:
            rep["undecided"] += 1
            r = parity.compare_scan(o, cd, items_o[sel], items_g[sel], enforce_limits=False)
            rep["near_ties"] += r["near_ties"] + r["periodic_fallbacks"]
    return rep


def add_counts(total: dict, rep: dict) -> dict:
    for k, v in rep.items():
        total[k] = total.get(k, 0) + v
    return total
