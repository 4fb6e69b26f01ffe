"""Windows, position plans, a vectorised float64 model and a fitted comparison for softbits_kernel alone
(tests/test_softbits_positions_model.py on the CPU, tests/test_gpu_softbits_positions.py on the GPU).

The kernel is driven on a retained handle with seeded candidates - submit_analytic, load_candidates, decode(STAGE_SOFTBITS),
dump_candidates - so the positions are the plan's, not what a scan happens to find:

  A  one noise-plus-pings window in 672 channels at a 0 Hz hypothesis (scan_windows.A_CFG: F = 1, the mixer is exactly (1, 0)), the
     plan pos = 672 ((slot + pattern) mod 8) + tile: per pattern a bijection onto 0..5375, and every wave meets every residue mod 6,
     every base entry q and every pattern
  B  A's tiles 0..5 and 666..671 at depths 1..7: a candidate's arithmetic does not depend on D
  C  four shapes of (channels, frequencies) whose tile counts are no multiple of 8, each channel its own window, positions drawn
     from the structural edges of the plane (ring start and end, the wrap of the last frame, q = 719..723, the twins) and at random
  D  A's window times a power of two
  E  NaN and Inf samples beside a finite channel

The metric splits a row's distance from the float64 model into what a carrier angle explains, what a gain explains and the rest:
with e = G - L, least squares for e ~ delta Q + g L (Q = dL / d angle), then rho = max |rest| / max(1, |L|), alpha = |delta| / kappa
(kappa: the condition number of the 84-term phase sum) and gamma = |g|.  A wrong tap, fold, wrap entry or lane map lands in rho, a
wrong phase sum in alpha, a wrong normalisation in gamma.  The yardsticks are the float32 oracle's own worst rho, alpha and gamma
on the same candidates; the kernel is held to LIMIT_FACTOR times each."""
from __future__ import annotations

import collections
import concurrent.futures

import numpy as np

from msk144cudecoder_amd import synth
from msk144cudecoder_amd.protocol import PATTERN_MASK

import numpy_model
import scan_windows

N = 5184
POSITIONS = 5376
FRAME = 864
SLOTS = 8
RING_Q = N // 6
SYNC = np.r_[0:8, 56:64]                               # the softbits no LLR row carries
ROW = np.r_[8:56, 64:144]
S16 = np.concatenate([numpy_model.S8, numpy_model.S8])
LIMIT_FACTOR = 4.0                                     # kernel limit = 4 x the oracle's own worst (1-ulp rsq/rcp/sqrt for atan2f/sincosf, the divide and
                                                       # the sqrt; filter before fold; a 1.5e-7 mixer: each of the size of the oracle's own rounding)
MARGINAL_SHARE = 0.005                                 # candidates with a marginal sync softbit: at most this share of a family
SENTINEL = np.float32(-1.2345e33)                      # seeded into every LLR row; the stage must leave none
SEEDED_NBADSYNC = 99
SEEDED_XB = np.float32(1.0)

# ---- family A ----
A_CFG = scan_windows.A_CFG
A_SEED = 4301
A_TILES = 672                                          # 672 = 0 mod 6 and 8 * 672 = 5376
PINGS = ((700, 3, 1.2, 0.7), (3900, 2, 2.0, 2.1))      # (start, frames, amplitude, phase); the second is cut at the ring's end
TWINS = 192                                            # positions p0 < 192 have a ring twin p0 + 5184

# ---- family B ----
B_TILES = tuple(range(6)) + tuple(range(666, 672))
B_DEPTHS = tuple(range(1, 8))

# ---- family C ----
C_WIDE = dict(center=1500.0, width=20.0, step=2.0)     # F = 11
C_FINE = dict(center=1500.0, width=6.0, step=0.7)      # F = 9, an inexact step
C_SHAPES = ((1, C_WIDE), (3, C_WIDE), (13, scan_windows.B_CFG), (2, C_FINE))      # tiles: 11, 33, 65, 18
C_TILE_COUNTS = (11, 33, 65, 18)
C_SEED = 4310
C_CARRIER = 1502.0
C_SINGLE_13 = (0, 7, 8, 12)                            # channels of the 13-channel batch that are also run alone
STRUCTURAL = np.concatenate([np.arange(0, 12), np.arange(852, 876), np.arange(4314, 4344), np.arange(5172, 5196), np.arange(5364, 5376)])

# ---- family D ----
D_TILES = tuple(range(6))
D_EXPONENTS = (-40, -20, 20, 40)

# ---- family E ----
E_SAMPLE = 3000


# ------------------------------------------------------------------------------------------------
# windows
# ------------------------------------------------------------------------------------------------
def window(seed: int = A_SEED, carrier: float = 0.0) -> np.ndarray:
    """complex64 [5184]: unit complex Gaussian noise plus the two pings, each a fresh random message, on `carrier` Hz."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=N) + 1j * rng.normal(size=N)
    for start, frames, amp, phase in PINGS:
        bb = np.tile(synth.modulate_frame(synth.frame_bits(synth.encode_message(synth.random_message(rng)))), frames)
        n = np.arange(start, min(N, start + len(bb)))
        x[n] += amp * np.exp(1j * (2.0 * np.pi * carrier * n / 12000.0 + phase)) * bb[:len(n)]
    return x.astype(np.complex64)


def c_window(c: int) -> np.ndarray:
    return window(C_SEED + c, C_CARRIER)


def d_window(k: int) -> np.ndarray:
    return (window() * np.float32(2.0) ** k).astype(np.complex64)


def e_windows() -> np.ndarray:
    w = np.stack([window()] * 3)
    w[1, E_SAMPLE] = np.complex64(complex(np.nan, 0.0))
    w[2, E_SAMPLE] = np.complex64(complex(np.inf, 0.0))
    return w


# ------------------------------------------------------------------------------------------------
# plans: pos [channels][F * D * 8] in item order (item = (block * D + pattern) * 8 + slot)
# ------------------------------------------------------------------------------------------------
def plan_a(tiles=range(A_TILES), depth: int = 8) -> np.ndarray:
    t = np.asarray(list(tiles))[:, None, None]
    p = np.arange(depth)[None, :, None]
    s = np.arange(SLOTS)[None, None, :]
    pos = (A_TILES * ((s + p) % 8) + t) % POSITIONS
    return pos.reshape(len(t), depth * SLOTS).astype(np.uint32)


def c_rounds(tiles: int) -> int:
    """Handle runs of a shape: enough for every structural position to meet every pattern."""
    return -(-len(STRUCTURAL) // (tiles * SLOTS))


def plan_c(shape: int) -> np.ndarray:
    """pos [rounds][channels][F * 64] of shape C_SHAPES[shape]: per pattern the structural set and seeded random positions, laid over
    the (round, tile, slot) places of that pattern by a seeded permutation."""
    channels, tiles = C_SHAPES[shape][0], C_TILE_COUNTS[shape]
    F = tiles // channels
    rounds = c_rounds(tiles)
    rng = np.random.default_rng(4400 + shape)
    places = rounds * tiles * SLOTS
    pos = np.empty((rounds, tiles, 8, SLOTS), dtype=np.uint32)
    for p in range(8):
        pool = np.concatenate([STRUCTURAL, rng.integers(0, POSITIONS, size=places - len(STRUCTURAL))])
        pos[:, :, p, :] = rng.permutation(pool).reshape(rounds, tiles, SLOTS)
    return pos.reshape(rounds, channels, F * 8 * SLOTS)


def seed_items(dtype, pos_row) -> np.ndarray:
    """The candidates of one channel as loaded: the plan's pos, xb 1.0, nbadsync 99, every LLR the sentinel."""
    items = np.zeros(len(pos_row), dtype=dtype)
    items["pos"] = pos_row
    items["xb"] = SEEDED_XB
    items["nbadsync"] = SEEDED_NBADSYNC
    items["softbits_wo_sync"] = SENTINEL
    return items


# ------------------------------------------------------------------------------------------------
# the float64 model, vectorised over positions
# ------------------------------------------------------------------------------------------------
Model = collections.namedtuple("Model", "soft L Q perp rms kappa nbad")


def _model_chunk(ring, pos):
    m = len(pos)
    c3 = ring[(pos[:, None] + np.arange(FRAME)[None, :]) % N]
    cb = numpy_model.cb42()
    t = np.concatenate([c3[:, :42], c3[:, 336:378]], axis=1) * np.conj(np.concatenate([cb, cb]))[None, :]
    s = t.sum(axis=1)
    kappa = np.abs(t).sum(axis=1) / np.abs(s)
    c3 = c3 * np.exp(-1j * np.angle(s))[:, None]
    zi = (c3.reshape(m, 72, 12) * numpy_model.PP).sum(axis=2)                        # I bit 2 j + 1: samples 12 j .. 12 j + 11
    zq = (np.roll(c3, 6, axis=1).reshape(m, 72, 12) * numpy_model.PP).sum(axis=2)    # Q bit 2 j: samples 12 j - 6 .. 12 j + 5 of the frame ring
    soft = np.empty((m, 144))
    perp = np.empty((m, 144))
    soft[:, 1::2], soft[:, 0::2] = zi.real, zq.imag
    perp[:, 1::2], perp[:, 0::2] = -zi.imag, zq.real                                 # the same sums of i * c3
    sav = soft.mean(axis=1)
    s2av = (soft ** 2).mean(axis=1)
    scale = 2.0 / (np.sqrt(s2av - sav * sav) * 0.6 * 0.6)
    hard = np.where(soft < 0, -1, 1)
    nbad = (8 - (hard[:, 0:8] * numpy_model.S8).sum(axis=1)) // 2 + (8 - (hard[:, 56:64] * numpy_model.S8).sum(axis=1)) // 2
    return Model(soft, scale[:, None] * soft[:, ROW], scale[:, None] * perp[:, ROW], perp, np.sqrt(s2av), kappa, nbad)


def model(mixed, pattern: int, positions, chunk: int = 1344) -> Model:
    """numpy_model.softbits at many positions of one mixed window (complex128 [5184]) and one pattern.  Beside the softbits, the LLR row
    L and nbadsync: Q, the row of i * c3 at L's scale (dL / d carrier angle), perp (its 144 softbits), the softbits' rms and kappa =
    sum |t_k| / |sum t_k| over the 84 terms c3 conj(cb) of the two sync words."""
    mask = PATTERN_MASK[pattern]
    ring = sum(np.roll(mixed, -FRAME * m) for m in range(6) if mask[m])              # ring[n] = sum over the frames of x[(n + 864 m) mod 5184]
    pos = np.asarray(positions, dtype=np.int64) % N
    with np.errstate(all="ignore"):
        parts = [_model_chunk(ring, pos[i:i + chunk]) for i in range(0, len(pos), chunk)]
    return Model(*(np.concatenate(f) for f in zip(*parts)))


def take(m: Model, idx) -> Model:
    return Model(*(f[idx] for f in m))


def join(models) -> Model:
    return Model(*(np.concatenate(f) for f in zip(*models)))


_MIXED = {}


def mixed(key, cd, freq):
    """numpy_model.mix (float32 phase, as the kernel and the oracle form it), once per (window key, frequency)."""
    k = (key, float(freq))
    if k not in _MIXED:
        with np.errstate(all="ignore"):
            _MIXED[k] = numpy_model.mix(cd, np.float32(freq))
    return _MIXED[k]


def model_of_channel(key, cd, freqs, depth: int, pos_row) -> Model:
    """The model of one channel's candidates in item order; freqs: the F hypotheses as float32."""
    pos = np.asarray(pos_row).reshape(len(freqs), depth, SLOTS)
    return join([model(mixed(key, cd, f), p, pos[b, p]) for b, f in enumerate(freqs) for p in range(depth)])


_MODEL_A = {}


def model_a() -> Model:
    """All 43008 candidates of family A in the order [tile][pattern][slot].  At 0 Hz the mixed window is the window."""
    if "m" not in _MODEL_A:
        x = window().astype(np.complex128)
        plan = plan_a().reshape(A_TILES, 8, SLOTS)
        per_pattern = [model(x, p, plan[:, p, :].reshape(-1)) for p in range(8)]     # [tile * 8 + slot]
        order = np.empty((A_TILES, 8, SLOTS), dtype=np.int64)
        for p in range(8):
            order[:, p, :] = p * A_TILES * SLOTS + np.arange(A_TILES * SLOTS).reshape(A_TILES, SLOTS)
        _MODEL_A["m"] = take(join(per_pattern), order.reshape(-1))
    return _MODEL_A["m"]


def a_rows(tiles, depth: int = 8):
    """Indices into model_a() (and into the depth-8 run's flat candidates) of the candidates of `tiles` at patterns < depth."""
    idx = np.arange(A_TILES * 64).reshape(A_TILES, 8, SLOTS)
    return idx[list(tiles), :depth, :].reshape(-1)


# ------------------------------------------------------------------------------------------------
# the fit, the yardsticks, the comparison
# ------------------------------------------------------------------------------------------------
Fit = collections.namedtuple("Fit", "rho alpha gamma rest")


def fit(rows, m: Model) -> Fit:
    """Per candidate: least squares (delta, g) of e = rows - L on (Q, L); rho, alpha, gamma as in the module text; rest [n][128]."""
    L, Q = m.L, m.Q
    with np.errstate(all="ignore"):
        e = np.asarray(rows, dtype=np.float64) - L
        a, b, c = (Q * Q).sum(axis=1), (Q * L).sum(axis=1), (L * L).sum(axis=1)
        u, v = (Q * e).sum(axis=1), (L * e).sum(axis=1)
        det = a * c - b * b
        delta, g = (c * u - b * v) / det, (a * v - b * u) / det
        rest = e - delta[:, None] * Q - g[:, None] * L
        rho = (np.abs(rest) / np.maximum(1.0, np.abs(L))).max(axis=1)
        return Fit(rho, np.abs(delta) / m.kappa, np.abs(g), rest)


def worst(f: Fit, finite=None) -> dict:
    sel = slice(None) if finite is None else finite
    return dict(rho=float(f.rho[sel].max()), alpha=float(f.alpha[sel].max()), gamma=float(f.gamma[sel].max()))


def oracle_rows(o, cd, blocks, patterns, positions, threads: int = 16):
    """(rows float32 [n][128], nbadsync [n]) of Oracle.softbits_at at each (block, pattern, pos)."""
    def one(k):
        _, llr, nb = o.softbits_at(cd, int(blocks[k]), int(patterns[k]), int(positions[k]))
        return llr, nb
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:        # the library call releases the interpreter lock
        out = list(ex.map(one, range(len(positions)), chunksize=256))
    return np.stack([r for r, _ in out]), np.array([n for _, n in out])


def limits_of(yard: dict) -> dict:
    return {k: LIMIT_FACTOR * v for k, v in yard.items()}


def sync_bounds(m: Model, lim: dict):
    """(sure, marginal counts) per candidate: sync softbit u is marginal when |soft_u| <= alpha_limit kappa |perp_u| + rho_limit rms;
    sure counts the non-marginal ones that disagree with the sync word."""
    soft, perp = m.soft[:, SYNC], m.perp[:, SYNC]
    with np.errstate(all="ignore"):
        marginal = ~(np.abs(soft) > lim["alpha"] * m.kappa[:, None] * np.abs(perp) + lim["rho"] * m.rms[:, None])    # a NaN is marginal
    disagree = np.where(soft < 0, -1, 1) != S16[None, :]
    return (disagree & ~marginal).sum(axis=1), marginal.sum(axis=1)


def where(k: int, pos, items_per_tile: int, depth: int, rest=None) -> dict:
    """What names candidate k of a flat [tile][block][pattern][slot] order in a failure message."""
    p = int(pos[k]) % N
    d = dict(candidate=int(k), tile_or_channel=int(k // items_per_tile), pattern=int(k % (depth * SLOTS) // SLOTS), slot=int(k % SLOTS),
             pos=int(pos[k]), residue=p % 6, q=p // 6)
    if rest is not None:
        u = int(np.nanargmax(np.abs(rest[k])))
        d["softbit"] = int(ROW[u])
    return d


def compare(m: Model, yard: dict, rows, nbad, pos, items_per_tile: int, depth: int = 8) -> dict:
    """The kernel's rows and nbadsync of a family against its model under LIMIT_FACTOR times the oracle's yardsticks, and the nbadsync
    rule.  Returns the report; raises AssertionError naming the worst candidate (residue, q, pattern, slot, softbit)."""
    lim = limits_of(yard)
    f = fit(rows, m)
    kernel = worst(f)
    rep = dict(candidates=len(rows), oracle=yard, kernel=kernel, ratio={k: kernel[k] / yard[k] for k in yard}, limit_factor=LIMIT_FACTOR)
    for name, values in (("rho", f.rho), ("alpha", f.alpha), ("gamma", f.gamma)):
        over = np.nonzero(~(values <= lim[name]))[0]
        if len(over):
            k = int(over[np.nanargmax(np.where(np.isfinite(values[over]), values[over], np.inf))])
            by_residue = np.bincount(np.asarray(pos)[over] % N % 6, minlength=6).tolist()
            by_pattern = np.bincount(over % (depth * SLOTS) // SLOTS, minlength=8).tolist()
            by_slot = np.bincount(over % SLOTS, minlength=8).tolist()
            raise AssertionError((name + " beyond %g x the oracle's own" % LIMIT_FACTOR, dict(value=float(values[k]), limit=lim[name], over=len(over),
                                                                                            over_by_residue=by_residue, over_by_pattern=by_pattern,
                                                                                            over_by_slot=by_slot, worst=where(k, pos, items_per_tile, depth, f.rest)), rep))
    sure, marg = sync_bounds(m, lim)
    nbad = np.asarray(nbad)
    bad = np.nonzero((nbad < sure) | (nbad > sure + marg))[0]
    assert len(bad) == 0, ("nbadsync outside [sure, sure + marginal]", dict(count=len(bad), kernel=int(nbad[bad[0]]), sure=int(sure[bad[0]]),
                                                                             marginal=int(marg[bad[0]]), model=int(m.nbad[bad[0]]),
                                                                             first=where(int(bad[0]), pos, items_per_tile, depth)), rep)
    rep["nbadsync_marginal_candidates"] = int((marg > 0).sum())
    rep["nbadsync_equal_to_model"] = int((nbad == m.nbad).sum())
    return rep


def marginal_share(m: Model, yard: dict) -> float:
    _, marg = sync_bounds(m, limits_of(yard))
    return float((marg > 0).mean())
