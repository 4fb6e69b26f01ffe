"""The softbits kernel's filtered-plane decomposition (csrc/softbits.hip), checked in numpy against tests/numpy_model.py.

The kernel filters the mixed window once per tile, P[n] = sum_{s=1..11} pp[s] x[(n + s) mod 5184], and demodulates a candidate
at `pos` with frame mask M from F(g) = sum_{m in M} P[pos + 864 m + 6 g]: softbit u = 1..143 is Re(rot F(u-1)) for odd u and
Im(rot F(u-1)) for even u.  Five half-pulse sums per candidate come from the window itself: u2[0] and u1[143] (softbit 0 wraps
round the folded frame) and u1[6], u2[56], u1[62] (the half pulses at the sync words' edges, needed by the carrier phase).
P is stored residue-major, sub-ring r = pos mod 6 at r * STRIDE, entry ((pos - r) / 6 + 144 m) mod 864 + g, with a 142-entry
wrap pad.  CPU only: this pins the index algebra of the kernel, not its float arithmetic."""
import numpy as np
import pytest

from msk144cudecoder_amd import protocol as P
import numpy_model as M

N = 5184
FRAME = 864
RING = N // 6            # entries per sub-ring
PAD = 142                # wrap pad: groups 0..142 of a folded frame come from P
STRIDE = 1009            # softbits.hip kPlaneStride
PP = M.PP
S8 = M.S8


def _masks():
    # kPatternMask (msk_context.cuh:231-238), every pattern up to depth 8
    return [np.array(m) for m in P.PATTERN_MASK]


def _window(seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N) + 1j * rng.standard_normal(N)


def plane(x, dtype=np.float64):
    """P[n] in the kernel's order: u1 = x[n+1] pp1 + ... + x[n+5] pp5, u2 = x[n+6] + x[n+7] pp7 + ... ; P = u1 + u2."""
    n = np.arange(N)
    re, im = x.real.astype(dtype), x.imag.astype(dtype)
    pp = PP.astype(dtype)

    def half(taps, first_plain):
        t0 = taps[0]
        if first_plain:
            ar, ai = re[(n + t0) % N].copy(), im[(n + t0) % N].copy()
        else:
            ar, ai = re[(n + t0) % N] * pp[t0], im[(n + t0) % N] * pp[t0]
        for s in taps[1:]:
            ar = (re[(n + s) % N] * pp[s] + ar).astype(dtype)
            ai = (im[(n + s) % N] * pp[s] + ai).astype(dtype)
        return ar, ai

    u1r, u1i = half(list(range(1, 6)), False)
    u2r, u2i = half(list(range(6, 12)), True)
    return (u1r + u2r).astype(dtype) + 1j * (u1i + u2i).astype(dtype) if dtype == np.float64 else (u1r + u2r, u1i + u2i)


def residue_major(Pn):
    """The LDS image of the plane: sub-ring r holds P[6 k + r] at r * STRIDE + k, k < 864, and its first PAD entries again behind."""
    lds = np.full(6 * STRIDE, np.nan, dtype=Pn.dtype)
    k = np.arange(N) // 6
    r = np.arange(N) % 6
    lds[r * STRIDE + k] = Pn
    pad = k < PAD
    lds[r[pad] * STRIDE + k[pad] + RING] = Pn[pad]
    return lds


def fold(lds, mask, pos):
    """F(g), g = 0..142, read from the residue-major image as the kernel's lanes do."""
    q, r = pos // 6, pos % 6
    g = np.arange(PAD + 1)
    F = None
    for m in range(6):
        if not mask[m]:
            continue
        base = (q + 144 * m) % RING
        v = lds[r * STRIDE + base + g]
        F = v if F is None else F + v
    return F


def half_pulse(x, mask, pos, group, rising):
    """u2[group] (rising: taps pp[6..11] on samples 0..5 of the group) or u1[group] (taps pp[1..5] on samples 1..5), folded over mask."""
    t = np.arange(6)
    c = sum(x[(pos + FRAME * m + 6 * group + t) % N] for m in range(6) if mask[m])
    w = PP[6:] if rising else PP[:6]
    return (c[1:] * w[1:]).sum() + (c[0] * w[0] if rising else 0.0)


def plane_softbits(x, mask, pos, lds=None):
    if lds is None:
        lds = residue_major(plane(x))
    F = fold(lds, mask, pos)
    u2_0 = half_pulse(x, mask, pos, 0, True)
    u1_143 = half_pulse(x, mask, pos, 143, False)
    u1_6 = half_pulse(x, mask, pos, 6, False)
    u2_56 = half_pulse(x, mask, pos, 56, True)
    u1_62 = half_pulse(x, mask, pos, 62, False)
    s = (S8[1] * F[0] + S8[3] * F[2] + S8[5] * F[4] + S8[7] * u1_6 - 1j * (S8[0] * u2_0 + S8[2] * F[1] + S8[4] * F[3] + S8[6] * F[5])
         + S8[1] * F[56] + S8[3] * F[58] + S8[5] * F[60] + S8[7] * u1_62 - 1j * (S8[0] * u2_56 + S8[2] * F[57] + S8[4] * F[59] + S8[6] * F[61]))
    rot = np.conj(s) / abs(s)
    G = np.concatenate([[u1_143 + u2_0], F])  # G[u]: the complex sum softbit u projects
    v = rot * G
    u = np.arange(144)
    soft = np.where(u % 2 == 1, v.real, v.imag)
    return soft, s


def _positions():
    # ring wrap of every frame, softbit 0 / group 143 at the ring's end, both parities, all residues
    return [0, 1, 5, 6, 863, 864, 2591, 2592, 4319, 4320, 4325, 5000, 5177, 5178, 5183]


def _reference_phase_sum(x, mask, pos):
    n = np.arange(FRAME)
    c3 = sum(x[(pos + n + FRAME * m) % N] for m in range(6) if mask[m])
    cb = M.cb42()
    return (c3[:42] * np.conj(cb)).sum() + (c3[336:378] * np.conj(cb)).sum()


@pytest.mark.parametrize("p", range(8))
def test_plane_softbits_equal_model_float64(p):
    x = _window(100 + p)
    lds = residue_major(plane(x))
    mask = _masks()[p]
    for pos in _positions() + list(np.random.default_rng(p).integers(0, N, 16)):
        soft_ref, _, nbad_ref = M.softbits(x, mask, int(pos))
        soft, s = plane_softbits(x, mask, int(pos), lds)
        scale = np.abs(soft_ref).max()
        assert np.abs(soft - soft_ref).max() <= 1e-12 * scale, (p, pos)
        # the carrier-phase sum itself, side values included
        s_ref = _reference_phase_sum(x, mask, int(pos))
        assert abs(s - s_ref) <= 1e-12 * abs(s_ref), (p, pos)
        hard = np.where(soft < 0, -1, 1)
        nbad = int(((8 - (hard[0:8] * S8).sum()) // 2) + ((8 - (hard[56:64] * S8).sum()) // 2))
        assert nbad == nbad_ref


def test_layout_index_formula():
    """Every (residue, base, group) the lanes read is P[(pos + 864 m + 6 g) mod 5184], and the image fits the kernel's LDS buffer."""
    Pn = np.arange(N, dtype=np.float64)
    lds = residue_major(Pn)
    assert 6 * STRIDE <= N + (FRAME + 5) + 3          # softbits.hip: kGroup * kPlaneStride <= kWindowLds
    assert STRIDE >= RING + PAD
    for pos in range(N):
        q, r = pos // 6, pos % 6
        g = np.arange(PAD + 1)
        for m in range(6):
            base = (q + 144 * m) % RING
            got = lds[r * STRIDE + base + g]
            assert np.array_equal(got, Pn[(pos + FRAME * m + 6 * g) % N])


def test_side_values_are_the_wrap_and_sync_edges():
    """u1[g] + u2[g + 1] is the folded P at group g; softbit 0 and the sync-word edges are the only sums P cannot give."""
    x = _window(7)
    Pn = plane(x)
    for p, mask in enumerate(_masks()):
        for pos in (0, 5183, 4321):
            for g in (0, 5, 6, 55, 61, 62, 142):
                lhs = half_pulse(x, mask, pos, g, False) + half_pulse(x, mask, pos, g + 1, True)
                rhs = sum(Pn[(pos + FRAME * m + 6 * g) % N] for m in range(6) if mask[m])
                assert abs(lhs - rhs) <= 1e-12 * (1 + abs(rhs))
            # group 143 of the folded frame wraps into group 0 of the SAME frame, not of the next one
            wrap = half_pulse(x, mask, pos, 143, False) + half_pulse(x, mask, pos, 0, True)
            soft_ref = M.softbits(x, mask, pos)[0]
            soft, s = plane_softbits(x, mask, pos)
            assert abs(soft[0] - soft_ref[0]) <= 1e-12 * np.abs(soft_ref).max()
            assert abs((np.conj(s) / abs(s) * wrap).imag - soft_ref[0]) <= 1e-12 * np.abs(soft_ref).max()


def test_plane_float32_emulation_within_1e5():
    """The kernel's float32 arithmetic (plane in the kernel's tap order, fold in frame order, float32 rotation) stays within
    1e-5 of the float64 model, relative to the frame's largest softbit."""
    f32 = np.float32
    for p, mask in enumerate(_masks()):
        x = _window(200 + p)
        Pr, Pi = plane(x, np.float32)
        lr, li = residue_major(Pr), residue_major(Pi)
        x32 = x.real.astype(f32).astype(np.float64) + 1j * x.imag.astype(f32).astype(np.float64)
        for pos in (0, 863, 5183, 3000 + p):
            Fr, Fi = fold(lr, mask, pos), fold(li, mask, pos)
            F = Fr.astype(np.float64) + 1j * Fi.astype(np.float64)
            side = [half_pulse(x32, mask, pos, g, rising) for g, rising in ((0, True), (143, False), (6, False), (56, True), (62, False))]
            side = [complex(f32(v.real)) + 1j * complex(f32(v.imag)) for v in side]
            u2_0, u1_143, u1_6, u2_56, u1_62 = side
            s = (S8[1] * F[0] + S8[3] * F[2] + S8[5] * F[4] + S8[7] * u1_6 - 1j * (S8[0] * u2_0 + S8[2] * F[1] + S8[4] * F[3] + S8[6] * F[5])
                 + S8[1] * F[56] + S8[3] * F[58] + S8[5] * F[60] + S8[7] * u1_62 - 1j * (S8[0] * u2_56 + S8[2] * F[57] + S8[4] * F[59] + S8[6] * F[61]))
            s = complex(f32(s.real)) + 1j * complex(f32(s.imag))
            rot = np.conj(s) / abs(s)
            cr, ci = f32(rot.real), f32(rot.imag)
            G = np.concatenate([[u1_143 + u2_0], F])
            gr, gi = G.real.astype(f32), G.imag.astype(f32)
            u = np.arange(144)
            soft = np.where(u % 2 == 1, gr * cr - gi * ci, gr * ci + gi * cr).astype(np.float64)
            soft_ref = M.softbits(x, mask, pos)[0]
            assert np.abs(soft - soft_ref).max() <= 1e-5 * np.abs(soft_ref).max(), (p, pos)
