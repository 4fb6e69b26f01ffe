"""scan_kernel alone where the winners' pass has work at every run: submit_analytic, decode(STAGE_SCAN), then the candidate dump,
held to the oracle through scan_windows.compare_exact with a depth-8 census (tests/scan_winners.py builds the windows,
tests/test_scan_winners_model.py holds them to the census shares asserted here).

  R  six bursts of falling amplitude one frame apart, the strongest walking over every run of a slice, every position of a run
     and every slice in 24 windows of one handle: each pattern folds a sum of its own from its own frames, so a winners' pass that
     loads the wrong frames for a pattern, names the wrong run or walks it from the wrong start moves a position in a decided group
  N  noise: a winner at an arbitrary run of every slice, all eight depths; then the all-zero, NaN and Inf windows beside a finite one

A position later in its slice than the oracle's is the octet store or the slice merge taking a later run; one that is off by less
than eleven is the walk; a pattern >= 6 alone is its frame set (100100, 100110)."""
import numpy as np
import pytest

import scan_windows as sw
import scan_winners as wn

pytestmark = pytest.mark.gpu

_COUNTS = {}


def report(parity_report, family, rep):
    parity_report("scan_winners_" + family, dict(sw.add_counts(_COUNTS.setdefault(family, {}), rep)))


def exact_groups(decided):
    """The census with the periodic patterns (wn.PERIODIC_PATTERNS: 111111 and 100100) left to the near-tie rule, as they are in family N.
    Their surfaces repeat after 864 / 2592 positions and the oracle folds the frames of such a pattern in one order for all positions, so
    its slots a period apart tie bit for bit and the census calls the group decided; scan_kernel folds from the position's own frame
    on, the same sum in a rotated order, and its slots differ by an ulp or two where six non-zero frames meet (a single burst, family B,
    adds zeros and stays exact).  Measured on the kernels from before the winners' pass and on these alike: window 0, hypothesis 1,
    pattern 5: oracle xb 8 x 43.98389435, kernel 43.98390198, 43.98389435, 43.98390198, 43.98389435, 4 x 43.98389816 - equal positions,
    inside TOL_XB_REL, but compare_exact's bit-for-bit tie check does not hold for either.  The census shares asserted are those of
    the full census."""
    out = decided.copy()
    out[:, list(wn.PERIODIC_PATTERNS)] = False
    return out


@pytest.mark.parametrize("depth", wn.R_DEPTHS)
def test_r_every_run_holds_a_winner(orc, hip, parity_report, depth):
    wins = [wn.r_window(k) for k in range(wn.R_WINDOWS)]
    dumps, dec = wn.gpu_scan(hip, sw.B_CFG, depth, wins)
    assert dec == (5, depth)
    o = orc.Oracle(depth=depth, threads=8, **sw.B_CFG)
    for k, (cd, items_g) in enumerate(zip(wins, dumps)):
        decided = wn.census_of(orc, ("R", k), sw.B_CFG, cd)
        assert int(decided.sum()) >= wn.R_MIN_DECIDED, (k, int(decided.sum()))
        rep = sw.compare_exact(o, cd, o.scan(cd), items_g, decided=exact_groups(decided))      # decided: equal positions; the rest: the near-tie rule
        assert rep["decided"] == int(exact_groups(decided)[:, :depth].sum())
        report(parity_report, "R", rep)


@pytest.mark.parametrize("depth", sw.DEPTHS)
def test_n_noise_windows(orc, hip, parity_report, depth):
    wins = [wn.n_window(seed) for seed in wn.N_SEEDS]
    dumps, dec = wn.gpu_scan(hip, wn.N_CFG, depth, wins)
    assert dec == (17, depth)
    o = orc.Oracle(depth=depth, threads=8, **wn.N_CFG)
    for seed, cd, items_g in zip(wn.N_SEEDS, wins, dumps):
        decided = wn.census_of(orc, ("N", seed), wn.N_CFG, cd)
        assert int(decided[:, wn.N_PATTERNS].sum()) >= wn.N_MIN_DECIDED, (seed, int(decided[:, wn.N_PATTERNS].sum()))
        rep = sw.compare_exact(o, cd, o.scan(cd), items_g, decided=decided)
        assert rep["decided"] == int(decided[:, :depth].sum())
        report(parity_report, "N", rep)


@pytest.mark.parametrize("depth", (1, 6))
def test_n_zero_and_nonfinite_windows(hip, parity_report, depth):
    wins = wn.nonfinite_windows()
    dumps, _ = wn.gpu_scan(hip, sw.B_CFG, depth, wins)                           # the call returns
    (alone,), _ = wn.gpu_scan(hip, sw.B_CFG, depth, wins[0])
    assert wn.scan_bytes(dumps[0]) == wn.scan_bytes(alone), "the finite channel differs from its one-channel run"
    assert np.all(dumps[3]["pos"] == 0) and np.all(dumps[3]["xb"].view(np.uint32) == 0), "all-zero window: every slot stays (0, 0.0)"
    for c, items in enumerate(dumps):
        assert np.all(items["pos"] < sw.POSITIONS), ("a position outside the scanned range: softbits indexes with it", c, int(items["pos"].max()))
    report(parity_report, "E", dict(groups=4 * 5 * depth, positions_in_range=4 * 5 * depth))
