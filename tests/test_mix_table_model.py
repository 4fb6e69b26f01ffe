"""CPU: the float32 model of the phasor table (tests/mix_table_model.py: mix_phase + sincos_reduced of csrc/mix.h with a
single-rounding FMA) and the tile map of the scan and softbits kernels (csrc/tile_map.h, compiled with the host compiler)."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mix_table_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the model's FMA ----

def test_fma_rounds_once_on_a_seeded_sample():
    """Random operands of the magnitudes the mix uses, against rational arithmetic element by element."""
    rng = np.random.default_rng(20)
    n = 4000
    a = (rng.uniform(-2.0, 2.0, n) * 2.0 ** rng.integers(-12, 14, n)).astype(F32)
    b = (rng.uniform(-2.0, 2.0, n) * 2.0 ** rng.integers(-12, 3, n)).astype(F32)
    c = (rng.uniform(-2.0, 2.0, n) * 2.0 ** rng.integers(-12, 14, n)).astype(F32)
    got = M.fma(a, b, c)
    want = np.array([M.fma_exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fma_where_the_float64_sum_sits_on_a_float32_midpoint():
    """(1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is the midpoint of the float32 pair lo = 1 + 2^-11 (even) and hi = lo + 2^-23.  With
    c = 2^-60 the float64 sum rounds to that midpoint and a second rounding to even gives lo; the single rounding is hi."""
    a = F32(1.0 + 2.0 ** -12)
    lo = F32(1.0 + 2.0 ** -11)
    hi = np.nextafter(lo, F32(2.0))
    tiny = F32(2.0 ** -60)
    assert Fraction(float(a)) ** 2 == (Fraction(float(lo)) + Fraction(float(hi))) / 2
    assert (np.float64(a) * np.float64(a) + np.float64(tiny)).astype(F32) == lo    # two roundings: what the model must not do
    assert M.fma(a, a, tiny)[0] == hi
    assert M.fma(a, a, -tiny)[0] == lo
    assert M.fma(a, a, F32(0.0))[0] == lo                                          # the exact tie goes to even
    assert M.fma(a, a, F32(2.0 ** -23))[0] == np.nextafter(hi, F32(2.0))           # ... also from an odd float32 upwards
    assert M.fma_exact(a, a, tiny) == hi and M.fma_exact(a, a, -tiny) == lo


# ---- the model against double precision, and its fixed points ----

def test_rows_match_double_precision_and_zero_frequency_is_one():
    """The float phase IS the argument (as for the reference's sincosf): sin and cos of it to the 2e-7 of tests/test_mix_sincos.py;
    against the ideal phase 2 pi n f / 12000 only to the float phase's own error, |phi| 2^-22.  f = 0: every entry is (1, +0)."""
    n = np.arange(M.WINDOW, dtype=np.float64)
    for f in (1250.0, 1500.25, 1750.0, -250.0, 250.0):
        row = M.table_row(F32(f))
        nf = n.astype(F32)
        phi = M.mix_phase(nf, M.mul(F32(-1.0), F32(f))).astype(np.float64)
        assert np.abs(row[:, 0] - np.cos(phi)).max() < 2.0e-7 and np.abs(row[:, 1] - np.sin(phi)).max() < 2.0e-7
        ideal = -2.0 * np.pi * n * f / 12000.0
        assert np.abs(phi - ideal).max() <= np.abs(ideal).max() * 2.0 ** -22
    zero = M.table_row(F32(0.0))
    assert np.array_equal(zero.view(np.uint32), np.tile(np.array([1.0, 0.0], F32).view(np.uint32), (M.WINDOW, 1)))
    assert np.array_equal(M.table_row(F32(1500.0))[0].view(np.uint32), np.array([1.0, 0.0], F32).view(np.uint32))   # sample 0


# ---- the tile map ----

TILE_MAIN = r"""
#include "tile_map.h"
#include <cstdio>
#include <cstdlib>
template<int G> static void dump(int nch, int F)
{
    const int total = nch * F;
    std::printf("%d %d %d %d\n", G, nch, F, msk144::tiles_per_xcd(total) * 8);
    for(int blk = 0; blk < msk144::tiles_per_xcd(total) * 8; blk++)
    {
        const int t = msk144::tile_index(blk, total);
        if(t < 0) { std::printf("%d -1 -1 -1\n", blk); continue; }
        const msk144::Tile tl = msk144::tile_of<G>(t, nch, F);
        std::printf("%d %d %d %d\n", blk, t, tl.ch_rel, tl.b);
    }
}
int main(int argc, char** argv)
{
    const int G = std::atoi(argv[1]), nch = std::atoi(argv[2]), F = std::atoi(argv[3]);
    switch(G)
    {
    case 1: dump<1>(nch, F); break;
    case 4: dump<4>(nch, F); break;
    case 8: dump<8>(nch, F); break;
    case 16: dump<16>(nch, F); break;
    case 0: dump<msk144::kTileGroup>(nch, F); break;
    default: return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def tile_prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_map")
    src, exe = os.path.join(d, "main.cpp"), os.path.join(d, "tile_map")
    open(src, "w").write(TILE_MAIN)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", M.CSRC, "-o", exe, src], check=True)

    def run(G, nch, F):
        out = subprocess.run([exe, str(G), str(nch), str(F)], check=True, capture_output=True, text=True).stdout.split("\n")
        head = [int(v) for v in out[0].split()]
        rows = np.array([[int(v) for v in l.split()] for l in out[1:] if l], dtype=np.int64)
        assert len(rows) == head[3] and np.array_equal(rows[:, 0], np.arange(head[3]))
        return head[0], rows
    return run


@pytest.mark.parametrize("G", [1, 4, 8, 16])
def test_tile_map_covers_every_tile_once_and_groups_share_a_row(tile_prog, G):
    for nch in sorted({1, max(G - 1, 1), G, G + 1, 2 * G + 3, 128}):
        for F in (1, 5, 17, 501):
            g, rows = tile_prog(G, nch, F)
            assert g == G
            total = nch * F
            live = rows[rows[:, 1] >= 0]
            # workgroup -> tile: one contiguous range per XCD (workgroups b and b + 8 share one), every tile once
            assert np.array_equal(np.sort(live[:, 1]), np.arange(total))
            per_xcd = (total + 7) // 8
            assert np.array_equal(live[:, 1], (live[:, 0] & 7) * per_xcd + (live[:, 0] >> 3))
            # tile -> (channel, frequency): every pair once
            by_tile = live[np.argsort(live[:, 1])]
            ch, b = by_tile[:, 2], by_tile[:, 3]
            assert ch.min() >= 0 and ch.max() < nch and b.min() >= 0 and b.max() < F
            assert len(set(zip(ch.tolist(), b.tolist()))) == total
            t = np.arange(total)
            if G == 1:
                assert np.array_equal(ch, t // F) and np.array_equal(b, t % F)       # the plain order
            # a group is G channels (the last one what is left), frequency outer and channel inner
            group = t // (G * F)
            assert np.array_equal(ch // G, group)
            for k in range((nch + G - 1) // G):
                sel = group == k
                gc = min(G, nch - k * G)
                assert sel.sum() == gc * F
                assert np.array_equal(b[sel], np.repeat(np.arange(F), gc))             # consecutive tiles share b, gc at a time
                assert np.array_equal(ch[sel], k * G + np.tile(np.arange(gc), F))


def test_the_build_uses_the_group_size_the_header_names(tile_prog):
    """kTileGroup, the product's G: whatever it is set to, the map with it is one of the tested ones."""
    g, _ = tile_prog(0, 3, 5)
    assert g in (1, 4, 8, 16)
