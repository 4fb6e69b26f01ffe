"""csrc/mix.h in float32, operation for operation: mix_phase (two plain multiplies and the Markstein division by the sample rate)
and sincos_reduced, with an FMA that rounds once.  Shared by tests/test_mix_table_model.py (CPU) and tests/test_gpu_mix_table.py,
which holds the handle's phasor table to it bit for bit.  The constants come from the sources, so the model follows the code."""
import os
import re
from fractions import Fraction

import numpy as np

from test_mix_sincos import constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msk144cudecoder_amd", "csrc")
F32 = np.float32
WINDOW = 5184
THREADS = 512  # the mixers' workgroup: sample n = tid + 512 i is formed as float(tid) + float(512 i)


def _round_exact(x: Fraction, lo: float, hi: float) -> np.float32:
    """x rounded to nearest-even among the adjacent float32 lo < hi that bracket it."""
    mid = (Fraction(lo) + Fraction(hi)) / 2
    if x != mid:
        return F32(hi if x > mid else lo)
    return F32(lo) if (np.array(lo, F32).view(np.uint32) & 1) == 0 else F32(hi)


def fma_exact(a, b, c) -> np.float32:
    """RN32(a b + c) of three float32 scalars in rational arithmetic: the reference every other FMA here is held to."""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = F32(float(x))  # float(Fraction) is correctly rounded to float64; one more rounding can only be off by one float32
    cands = sorted({float(np.nextafter(near, F32(-np.inf))), float(near), float(np.nextafter(near, F32(np.inf)))})
    for lo, hi in zip(cands, cands[1:]):
        if Fraction(lo) <= x <= Fraction(hi):
            return _round_exact(x, lo, hi)
    raise AssertionError("not bracketed")


def fma(a, b, c):
    """float32 fused multiply-add with ONE rounding.  The product of two float32 is exact in float64 and the float64 sum rounds once
    more before the cast, which can only differ from a single rounding when that sum sits exactly on a float32 midpoint (or the
    result is a float32 denormal): those elements are recomputed in rational arithmetic."""
    a, b, c = (np.atleast_1d(np.asarray(v, F32)).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    s = a * b + c
    r = s.astype(F32)
    tie = ((s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)) | ((np.abs(s) < 2.0 ** -126) & (s != 0))
    for i in np.nonzero(tie.ravel())[0]:
        r.ravel()[i] = fma_exact(a.ravel()[i], b.ravel()[i], c.ravel()[i])
    return r


def mul(a, b):
    """one float32 multiply: the exact float64 product, rounded once"""
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)).astype(F32)


def phase_constants():
    mix = open(os.path.join(CSRC, "mix.h")).read()
    two, pi = re.search(r"const float twopi = (\d+\.\d+)f \* (\d+\.\d+)f;", mix).groups()
    rate = re.search(r"constexpr float kSampleRate = (\d+\.\d+)f;", open(os.path.join(CSRC, "msk144_protocol.h")).read()).group(1)
    rate = F32(rate)
    return mul(F32(two), F32(pi)), rate, (F32(1.0) / rate).astype(F32)  # IEEE float32 division: correctly rounded, as the constexpr is


def mix_phase(nf, f0):
    """div_sample_rate(f32_mul(f32_mul(nf, twopi), f0))"""
    twopi, rate, r = phase_constants()
    x = mul(mul(nf, twopi), f0)
    q = mul(x, r)
    e = fma(-q, rate, x)
    return fma(e, r, q)


def sincos_reduced(phi):
    """(sn, cs) of sincos_reduced(phi)"""
    k_round, inv_pi, pi_hi, pi_lo, s, c = constants()
    phi = np.atleast_1d(np.asarray(phi, F32))
    kb = fma(phi, inv_pi, k_round)
    k = (kb - k_round).astype(F32)  # exact
    r = fma(-k, pi_hi, phi)
    r = fma(-k, pi_lo, r)
    z = mul(r, r)
    sp = fma(s[3], z, s[2])
    sp = fma(sp, z, s[1])
    sp = fma(sp, z, s[0])
    s_r = fma(mul(r, z), sp, r)
    cp = fma(c[4], z, c[3])
    cp = fma(cp, z, c[2])
    cp = fma(cp, z, c[1])
    cp = fma(cp, z, c[0])
    c_r = fma(cp, z, F32(1.0))
    flip = kb.view(np.uint32) << np.uint32(31)
    return (s_r.view(np.uint32) ^ flip).view(F32), (c_r.view(np.uint32) ^ flip).view(F32)


def table_row(freq_hz) -> np.ndarray:
    """Row of the phasor table for one hypothesis frequency (float32 Hz): float32 [5184][2] = (cs, sn), from the operands the
    fill kernel uses: nf = float(tid) + float(512 i), f0 = -1.0f * freq."""
    n = np.arange(WINDOW)
    nf = ((n % THREADS).astype(F32) + (n // THREADS * THREADS).astype(F32)).astype(F32)
    f0 = mul(F32(-1.0), F32(freq_hz))
    sn, cs = sincos_reduced(mix_phase(nf, f0))
    return np.stack([cs, sn], axis=1)
