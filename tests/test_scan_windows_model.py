"""The windows of tests/scan_windows.py meet, with the oracle alone, what tests/test_gpu_scan_windows.py relies on: the host model of the
arg-max and slot rule is the oracle's rule bit for bit on every one of them, and the census leaves few groups - and none of those the
GPU test names - to a tolerance.  These are conditions on the inputs: seeds, amplitudes and the tail were chosen until they held, the
threshold is parity's."""
import numpy as np
import pytest

from msk144cudecoder_amd.protocol import PATTERN_MASK

import numpy_model
import parity
import scan_windows as sw

B_CASES = [(s, 8) for s in sw.B_STARTS] + [("multi", 8)] + [(s, depth) for s in sw.B_DEPTH_STARTS for depth in range(1, 8)]


class Surfaces:
    """All F x 8 surfaces of one window, their census and the slot rule applied to them."""

    def __init__(self, orc, cfg, cd, period=None):
        self.cfg, self.cd = cfg, cd
        o = orc.Oracle(depth=8, threads=8, **cfg)
        self.xb = [[o.scan_xb(cd, b, p) for p in range(8)] for b in range(o.F)]
        self.decided = np.array([[sw.census(x, period) for x in row] for row in self.xb])
        self.rule = [[sw.slot_rule(x) for x in row] for row in self.xb]

    def check_rule(self, orc, depth):
        """slot_rule(o.scan_xb) == o.scan, pos and xb, bit for bit, at this depth."""
        o = orc.Oracle(depth=depth, threads=8, **self.cfg)
        items = o.scan(self.cd)
        for b in range(o.F):
            for p in range(depth):
                g = items[(b * depth + p) * 8:][:8]
                pos, xb = self.rule[b][p]
                assert np.array_equal(g["pos"], pos) and np.array_equal(g["xb"].view(np.uint32), xb.view(np.uint32)), (b, p, g["pos"], pos, g["xb"], xb)


@pytest.fixture(scope="module")
def family_a(orc):
    return {d: Surfaces(orc, sw.A_CFG, sw.antiperiodic_window(d), d) for d in sw.A_PERIODS}


@pytest.fixture(scope="module")
def family_b(orc):
    out = {s: Surfaces(orc, sw.B_CFG, sw.burst_window(s)) for s in sw.B_STARTS}
    out["multi"] = Surfaces(orc, sw.B_CFG, sw.multi_burst_window())
    return out


def test_windows_are_seeded_and_shaped():
    for w in [sw.antiperiodic_window(d) for d in sw.A_PERIODS] + [sw.burst_window(s) for s in sw.B_STARTS] + [sw.multi_burst_window(), sw.channel_burst_window(63)]:
        assert w.dtype == np.complex64 and w.shape == (sw.N,) and np.isfinite(w).all()
    assert sw.antiperiodic_window(6).tobytes() == sw.antiperiodic_window(6).tobytes() and sw.burst_window(5183).tobytes() == sw.burst_window(5183).tobytes()
    x = sw.antiperiodic_window(9)
    assert np.array_equal(np.roll(x, -9), -x)                                            # anti-periodic on the ring, wrap included
    b = sw.burst_window(5183)
    assert np.count_nonzero(b) <= 42 + sw.TAIL_TAPS and b[5183] != 0 and b[49] != 0 and b[50] == 0    # the burst wraps the ring end
    # the edges the GPU test is about are among the starts
    for s in (0, 5183, 10, 11, 244, 245, 252, 253, 255, 256, 1279, 1280, 5119, 5120, 87, 88, 175, 176, 5142, 5143):
        assert s in sw.B_STARTS
    assert any(0 <= s - sw.SECOND_SYNC < 192 for s in sw.B_STARTS)                       # a ghost below 192: its ring twin sits in slice 20
    ratios = np.array(sw.MULTI_FIRST_AMPLITUDES[:-1]) / np.array(sw.MULTI_FIRST_AMPLITUDES[1:])
    assert (ratios >= 1.05).all() and min(sw.MULTI_LATER_AMPLITUDES) >= 1.05 * max(sw.MULTI_FIRST_AMPLITUDES)
    assert [s // sw.SLICE for s in sw.MULTI_FIRST] == list(range(8)) and min(sw.MULTI_LATER) >= 8 * sw.SLICE


def test_slot_rule_is_the_oracles_rule_family_a(orc, family_a):
    for d, sf in family_a.items():
        for depth in sw.DEPTHS:
            sf.check_rule(orc, depth)


def test_slot_rule_is_the_oracles_rule_family_b(orc, family_b):
    for key, depth in B_CASES:
        family_b[key].check_rule(orc, depth)


def test_slot_rule_is_the_oracles_rule_family_c_and_d(orc):
    """C: every channel's window at F = 1, the first thirteen at F = 5, three at F = 17.  D: the scaled windows."""
    for F, chans in ((1, range(64)), (5, range(13)), (17, (0, 31, 63))):
        for c in chans:
            Surfaces(orc, sw.C_CFG[F], sw.channel_burst_window(c)).check_rule(orc, 8)
    for s in sw.D_STARTS:
        for k in sw.D_EXPONENTS:
            Surfaces(orc, sw.B_CFG, (sw.burst_window(s) * np.float32(2.0) ** k).astype(np.complex64)).check_rule(orc, 8)


def test_family_a_is_periodic_and_fully_decided(orc, family_a):
    """Measured: 0 of 40 groups undecided (5 periods x 8 patterns); the smallest gap between two values of a period is 5.2e-4 of the
    largest (d = 8), the threshold 4e-4.  The arg-max residue of the float64 model is the oracle's."""
    o = orc.Oracle(depth=8, **sw.A_CFG)
    assert o.F == 1 and o.frequency(0) == 0.0
    for d, sf in family_a.items():
        for p in range(8):
            xb = sf.xb[0][p]
            assert np.array_equal(xb[d:].view(np.uint32), xb[:-d].view(np.uint32)), (d, p)           # exactly d-periodic over all 5376 positions
            v = np.sort(xb[:d].astype(np.float64))
            assert np.diff(v).min() >= 4 * parity.TOL_XB_REL * v[-1], (d, p, v)
            model = numpy_model.scan_xb(sf.cd.astype(np.complex128), PATTERN_MASK[p])
            assert int(np.argmax(model[:d])) == int(np.argmax(xb[:d])), (d, p)
            pos, val = sf.rule[0][p]
            assert len(set(val.view(np.uint32).tolist())) == 1 and val[0] > 0                        # all eight slots tie, and the fast path is taken
            assert np.array_equal(pos, [sw.SLICE * k + int(np.argmax(xb[sw.SLICE * k:sw.SLICE * k + d])) for k in range(8)])
        assert sf.decided.all(), (d, sf.decided)


def test_family_b_census_shares(family_b):
    """Measured on the 27 windows at depth 8: 31 of 1080 groups undecided (2.9 %; 21 of 1040 over the single bursts, 10 of 40 on the
    eight-plus-three window), none at the on-frequency hypothesis in patterns 0..2.  Over all the groups the GPU test compares, the
    depth sweeps included: 43 of 1640 (2.6 %)."""
    undecided = total = 0
    for key, depth in B_CASES:
        dec = family_b[key].decided[:, :depth]
        undecided += int((~dec).sum())
        total += dec.size
        assert dec[sw.B_BLOCK, :3].all(), (key, dec[sw.B_BLOCK])
    assert total == 1640 and undecided <= total // 10, (undecided, total)
    at8 = sum(int((~family_b[key].decided).sum()) for key, depth in B_CASES if depth == 8)
    assert at8 <= 1080 // 10, at8


def test_family_b_pattern_0_runs_the_serial_rule(family_b):
    """Fewer than eight slices see a single burst in pattern 0, and the slots at the largest value are the sync word's positions."""
    for s in sw.B_STARTS:
        pos, val = family_b[s].rule[sw.B_BLOCK][0]
        n_pos = int((val > 0).sum())
        assert 2 <= n_pos < 8 and np.all(val[n_pos:] == 0) and np.all(pos[n_pos:] == 0), (s, pos, val)
        assert sorted(pos[val.view(np.uint32) == val.max().view(np.uint32)].tolist()) == sw.peak_positions(s), (s, pos, val)
    pos, val = family_b["multi"].rule[sw.B_BLOCK][0]
    assert np.all(val > 0) and int((pos >= 8 * sw.SLICE).sum()) >= 3, (pos, val)                    # the fast path, then replacements
    first = family_b["multi"].xb[sw.B_BLOCK][0].reshape(sw.SLICES, sw.SLICE)[:8].max(axis=1)
    assert np.all(first > 0)


def test_family_d_stays_normal(orc):
    """|S|^2 of every stored maximum is a normal float at 2^-50 and finite at 2^40, so a power of two scales every stored value exactly."""
    o = orc.Oracle(depth=8, threads=8, **sw.B_CFG)
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    for s in sw.D_STARTS:
        xb = o.scan(sw.burst_window(s))["xb"].astype(np.float64)
        live = xb[xb > 0]
        assert (live * 2.0 ** min(sw.D_EXPONENTS)) .min() ** 2 > 4 * tiny and (live.max() * 2.0 ** max(sw.D_EXPONENTS)) ** 2 < huge / 4


def test_census_and_compare_exact_bite(orc, family_b):
    """The census opens on a near-tie and on a bitwise tie at a non-structural distance; compare_exact refuses a moved position and an
    xb beyond the tolerance in a decided group, and a split tie."""
    xb = np.zeros(sw.POSITIONS, dtype=np.float32)
    xb[100], xb[700] = 2.0, 1.0
    assert sw.census(xb)
    y = xb.copy(); y[101] = np.float32(2.0 * (1 - 3e-4))
    assert not sw.census(y)                                                                          # (a): a near-tie inside a slice
    y = xb.copy(); y[700] = np.float32(2.0 * (1 - 3e-4))
    assert not sw.census(y)                                                                          # (b): a near-tie between slices
    y = xb.copy(); y[700] = 2.0
    assert not sw.census(y)                                                                          # a bitwise tie 600 apart is not structural
    y = xb.copy(); y[100 + 864 - 336] = 2.0
    assert sw.census(y)                                                                              # ... at 864 - 336 it is
    y = xb.copy(); y[106] = 2.0
    assert not sw.census(y) and sw.census(y, period=6) and not sw.census(y, period=4)
    y = xb.copy(); y[5] = np.nan
    assert not sw.census(y)
    pos, val = sw.slot_rule(np.full(sw.POSITIONS, 3.0, dtype=np.float32))
    assert pos.tolist() == [256 * k for k in range(8)] and np.all(val == 3.0)                        # strict >: nothing is replaced on a tie

    s = 255
    sf = family_b[s]
    o = orc.Oracle(depth=8, threads=8, **sw.B_CFG)
    items = o.scan(sf.cd)
    rep = sw.compare_exact(o, sf.cd, items, items.copy(), decided=sf.decided)
    assert rep == dict(groups=40, decided=int(sf.decided.sum()), undecided=int((~sf.decided).sum()), exact=40, near_ties=0)
    g0 = (sw.B_BLOCK * 8 + 0) * 8
    bad = items.copy(); bad["pos"][g0] += 1
    with pytest.raises(AssertionError, match="positions differ"):
        sw.compare_exact(o, sf.cd, items, bad, decided=sf.decided)
    bad = items.copy(); bad["xb"][g0] *= np.float32(1 + 3e-4)
    with pytest.raises(AssertionError):
        sw.compare_exact(o, sf.cd, items, bad, decided=sf.decided)
    bad = items.copy(); bad["xb"][g0] = np.nextafter(bad["xb"][g0], np.float32(0))
    with pytest.raises(AssertionError, match="tie bit for bit"):
        sw.compare_exact(o, sf.cd, items, bad, decided=sf.decided)
