"""scan_kernel alone on the windows of tests/scan_windows.py: submit_analytic, decode(STAGE_SCAN), then the candidate dump.

  A  anti-periodic windows at a 0 Hz hypothesis, all eight depths: every run, octet, slice and slot ties bit for bit, so each position is
     the work of a tie rule - a >= for a > in the fold, the slice merge or the replacement, or a merge that prefers the higher lane,
     shows as a wrong position
  B  one sync word on a zero background at every structural edge of the fold (run, octet and slice boundaries, the overlapped last run,
     the ring end and its twins), the serial slot rule from the reset state, and a window that takes the fast path and then replaces
  C  the tile map and the channel map: every channel of a batch equals its single-channel run
  D  windows times a power of two: the same positions, xb scaled bit for bit
  E  NaN and Inf samples beside finite channels

Which rule a failure names: A's positions are 256 k + (residue of the period's maximum) - a position later in its run, octet or slice is
the fold, the octet store or the slice merge; a slot holding a later slice is the replacement; B's (0, 0.0) slots and slot order are
the arg-min; a missing peak at 253..255 or 5184.. is the last run or the wrap pad."""
import collections

import numpy as np
import pytest

from msk144cudecoder_amd.hipdecoder import STAGE_SCAN
from msk144cudecoder_amd.protocol import PATTERN_MASK

import numpy_model
import scan_windows as sw

pytestmark = pytest.mark.gpu

_COUNTS = {}


Geometry = collections.namedtuple("Geometry", "F D freq")


def gpu_scan(hip, cfg, depth, windows):
    """(candidate dumps [channels], the handle's geometry) of the windows (complex64 [channels][5184]) scanned by one handle."""
    windows = np.ascontiguousarray(windows, dtype=np.complex64).reshape(-1, sw.N)
    n = len(windows)
    with hip.HipDecoder(depth=depth, channels=n, llr_block_channels=n, **cfg) as d:
        d.submit_analytic(windows)
        d.decode(STAGE_SCAN)
        return [d.dump_candidates(c) for c in range(n)], Geometry(d.F, d.D, [np.float32(d.frequency(b)) for b in range(d.F)])


def scan_bytes(items):
    """The dump's bytes with the LLR rows blanked: no stage that writes them has run."""
    a = items.copy()
    a["softbits_wo_sync"] = 0
    return a.tobytes()


def group(items, depth, b, p):
    g0 = (b * depth + p) * sw.SLOTS
    return items[g0:g0 + sw.SLOTS]


def report(parity_report, family, rep):
    parity_report("scan_windows_" + family, dict(sw.add_counts(_COUNTS.setdefault(family, {}), rep)))


_CENSUS = {}


def census_of(orc, key, cfg, cd, period=None):
    """group_census at depth 8, once per window: a shallower scan sees the first patterns of the same surfaces."""
    if key not in _CENSUS:
        _CENSUS[key] = sw.group_census(orc.Oracle(depth=8, threads=8, **cfg), cd, period)
    return _CENSUS[key]


# ------------------------------------------------------------------------------------------------
# A. exact ties everywhere
# ------------------------------------------------------------------------------------------------
_A_EXPECTED = {}


def a_expected(d):
    """[8 patterns][8 slots]: 256 k + the lowest arg-max of the slice's first d positions, from the float64 model (the d values of a period
    are >= 4e-4 of the largest apart, tests/test_scan_windows_model.py: float64 and float32 agree on their order)."""
    if d not in _A_EXPECTED:
        cd = sw.antiperiodic_window(d).astype(np.complex128)      # 0 Hz: the mixed window is the window
        rows = []
        for p in range(8):
            xb = numpy_model.scan_xb(cd, PATTERN_MASK[p])
            rows.append([sw.SLICE * k + int(np.argmax(xb[sw.SLICE * k:sw.SLICE * k + d])) for k in range(sw.SLOTS)])
        _A_EXPECTED[d] = np.array(rows)
    return _A_EXPECTED[d]


@pytest.mark.parametrize("depth", sw.DEPTHS)
def test_a_antiperiodic_ties(orc, hip, parity_report, depth):
    wins = [sw.antiperiodic_window(d) for d in sw.A_PERIODS]
    dumps, dec = gpu_scan(hip, sw.A_CFG, depth, wins)                     # an audio handle takes centre 0 as any other
    assert (dec.F, dec.D) == (1, depth)
    o = orc.Oracle(depth=depth, threads=8, **sw.A_CFG)
    assert o.frequency(0) == 0.0
    for d, cd, items_g in zip(sw.A_PERIODS, wins, dumps):
        want = a_expected(d)
        for p in range(depth):
            g = group(items_g, depth, 0, p)
            assert np.all(g["xb"] > 0.0), (d, p, g["xb"])                                          # the fast path fills the slots
            assert len(set(g["xb"].view(np.uint32).tolist())) == 1, ("the eight slots do not tie bit for bit", d, p, g["xb"].tolist())
            assert np.array_equal(g["pos"], want[p]), ("slot k is not the lowest arg-max of slice k", dict(period=d, pattern=p, kernel=g["pos"].tolist(),
                                                                                                         expected=want[p].tolist()))
        rep = sw.compare_exact(o, cd, o.scan(cd), items_g, period=d, decided=census_of(orc, ("A", d), sw.A_CFG, cd, d))
        assert rep["undecided"] == 0 and rep["exact"] == rep["groups"] == depth, rep
        report(parity_report, "A", rep)


# ------------------------------------------------------------------------------------------------
# B. one peak at every structural edge
# ------------------------------------------------------------------------------------------------
B_CASES = [(s, 8) for s in sw.B_STARTS] + [(s, depth) for s in sw.B_DEPTH_STARTS for depth in range(1, 8)]


@pytest.mark.parametrize("s,depth", B_CASES)
def test_b_burst_at_edge(orc, hip, parity_report, s, depth):
    cd = sw.burst_window(s)
    (items_g,), dec = gpu_scan(hip, sw.B_CFG, depth, cd)
    assert (dec.F, dec.D) == (5, depth) and dec.freq[sw.B_BLOCK] == np.float32(sw.B_FREQ)
    # the on-frequency pattern-0 group, without the oracle: fewer than eight slices see the burst, so the serial rule runs from the reset
    # state - the positive slice maxima fill slots 0, 1, .. in slice order, the rest stay (0, 0.0) - and the slots at the largest value
    # are exactly the positions that fold the whole sync word, equal bit for bit
    g = group(items_g, depth, sw.B_BLOCK, 0)
    n_pos = int((g["xb"] > 0.0).sum())
    assert 2 <= n_pos < 8, g["xb"]
    assert np.all(g["xb"][:n_pos] > 0.0) and np.all(g["xb"][n_pos:] == 0.0) and np.all(g["pos"][n_pos:] == 0), ("slots beyond the positive slices are not (0, 0.0)",
                                                                                                                g["pos"].tolist(), g["xb"].tolist())
    assert np.all(np.diff(g["pos"][:n_pos].astype(np.int64) // sw.SLICE) > 0), ("slots are not filled in slice order", g["pos"].tolist())
    top = g["xb"].view(np.uint32) == g["xb"][int(np.argmax(g["xb"]))].view(np.uint32)
    assert sorted(g["pos"][top].tolist()) == sw.peak_positions(s), ("the largest slots are not the sync word's positions", g["pos"].tolist(), g["xb"].tolist(),
                                                                     sw.peak_positions(s))
    o = orc.Oracle(depth=depth, threads=8, **sw.B_CFG)
    rep = sw.compare_exact(o, cd, o.scan(cd), items_g, decided=census_of(orc, ("B", s), sw.B_CFG, cd))
    report(parity_report, "B", rep)


def test_b_fast_path_then_replacements(orc, hip, parity_report):
    """Eight bursts of falling amplitude in slices 0..7 fill the slots at once; three stronger ones (each seen twice more, at its ghost
    s - 336 and bit for bit the same) then replace the weakest slots in slice order."""
    cd = sw.multi_burst_window()
    (items_g,), dec = gpu_scan(hip, sw.B_CFG, 8, cd)
    o = orc.Oracle(depth=8, threads=8, **sw.B_CFG)
    decided = census_of(orc, ("B", "multi"), sw.B_CFG, cd)
    assert decided[sw.B_BLOCK, :3].all()
    g = group(items_g, 8, sw.B_BLOCK, 0)
    assert np.all(g["xb"] > 0.0) and int((g["pos"] >= 8 * sw.SLICE).sum()) >= 3, (g["pos"].tolist(), g["xb"].tolist())
    rep = sw.compare_exact(o, cd, o.scan(cd), items_g, decided=decided)
    report(parity_report, "B", rep)


# ------------------------------------------------------------------------------------------------
# C. tile map and channel map
# ------------------------------------------------------------------------------------------------
_SINGLE = {}


def single_channel_bytes(hip, F, channels):
    """scan_bytes of channel windows 0 .. channels - 1, each scanned alone by a one-channel handle with F hypotheses."""
    have = _SINGLE.setdefault(F, {})
    todo = [c for c in range(channels) if c not in have]
    if todo:
        with hip.HipDecoder(depth=8, channels=1, llr_block_channels=1, **sw.C_CFG[F]) as d1:
            assert d1.F == F
            for c in todo:
                d1.submit_analytic(sw.channel_burst_window(c))
                d1.decode(STAGE_SCAN)
                have[c] = scan_bytes(d1.dump_candidates(0))
    return have


@pytest.mark.parametrize("channels,F", sw.C_SHAPES)
def test_c_batch_equals_single(hip, parity_report, channels, F):
    wins = [sw.channel_burst_window(c) for c in range(channels)]
    dumps, dec = gpu_scan(hip, sw.C_CFG[F], 8, wins)
    assert dec.F == F
    single = single_channel_bytes(hip, F, channels)
    on = F // 2
    assert dec.freq[on] == np.float32(sw.B_FREQ)
    for c, items in enumerate(dumps):
        g = group(items, 8, on, 0)
        assert int(g["pos"][int(np.argmax(g["xb"]))]) % sw.N in {sw.channel_start(c), (sw.channel_start(c) - sw.SECOND_SYNC) % sw.N}, ("not this channel's burst", c, g["pos"].tolist())
        assert scan_bytes(items) == single[c], ("a channel of the batch differs from its single-channel run", dict(channel=c, channels=channels, F=F))
    report(parity_report, "C", dict(groups=channels * F * 8, identical_to_single_channel_run=channels * F * 8))


# ------------------------------------------------------------------------------------------------
# D. scale invariance
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", sw.D_STARTS)
def test_d_power_of_two_scale(hip, parity_report, s):
    cd = sw.burst_window(s)
    wins = [cd] + [(cd * np.float32(2.0) ** k).astype(np.complex64) for k in sw.D_EXPONENTS]
    dumps, _ = gpu_scan(hip, sw.B_CFG, 8, wins)
    base = dumps[0]
    for k, items in zip(sw.D_EXPONENTS, dumps[1:]):
        assert np.array_equal(items["pos"], base["pos"]), ("positions move under a power-of-two scale", s, k)
        want = base["xb"] * np.float32(2.0) ** k                     # exact: every product and sum scales, |S|^2 stays normal
        assert np.array_equal(items["xb"].view(np.uint32), want.view(np.uint32)), ("xb is not xb_0 * 2^k bit for bit", s, k)
    report(parity_report, "D", dict(groups=len(sw.D_EXPONENTS) * 5 * 8, scaled_bit_for_bit=len(sw.D_EXPONENTS) * 5 * 8))


# ------------------------------------------------------------------------------------------------
# E. non-finite samples beside finite channels
# ------------------------------------------------------------------------------------------------
def test_e_nonfinite_channels(orc, hip, parity_report):
    cd = sw.burst_window(2600)
    nan = cd.copy()
    nan[3000] = np.complex64(complex(np.nan, 0.0))
    inf = cd.copy()
    inf[3000] = np.complex64(complex(np.inf, 0.0))
    wins = [cd, nan, inf, np.zeros(sw.N, dtype=np.complex64)]
    dumps, _ = gpu_scan(hip, sw.B_CFG, 8, wins)                       # the call returns
    (alone,), _ = gpu_scan(hip, sw.B_CFG, 8, cd)
    assert scan_bytes(dumps[0]) == scan_bytes(alone)
    assert np.all(dumps[3]["pos"] == 0) and np.all(dumps[3]["xb"].view(np.uint32) == 0)
    for c, items in enumerate(dumps):
        assert np.all(items["pos"] < sw.POSITIONS), ("a position outside the scanned range: softbits indexes with it", c, int(items["pos"].max()))
    o = orc.Oracle(depth=8, threads=8, **sw.B_CFG)
    rep = {}
    for name, w, items in (("nan", nan, dumps[1]), ("inf", inf, dumps[2])):
        items_o = o.scan(w)
        rep[name] = dict(slots=len(items), same_pos=int((items_o["pos"] == items["pos"]).sum()),
                         same_xb_bits=int((items_o["xb"].view(np.uint32) == items["xb"].view(np.uint32)).sum()),
                         kernel_nonfinite_xb=int((~np.isfinite(items["xb"])).sum()), oracle_nonfinite_xb=int((~np.isfinite(items_o["xb"])).sum()))
    parity_report("scan_windows_E", rep)
