"""The scan's reduction without positions in the fold, on the CPU: (a) the numpy model of it (tests/scan_winners.py: per-run maxima,
the first lane of an octet, the first strict octet of a slice, the winning run walked again with strict >) names the lowest arg-max
of every slice - on random surfaces, on surfaces where every run ties, and on maxima at 245..252, which runs 22 and 23 both hold;
(b) the windows of tests/test_gpu_scan_winners.py meet, with the oracle alone, the census shares that test relies on.  These are
conditions on the inputs; the threshold is parity's."""
import numpy as np
import pytest

import scan_windows as sw
import scan_winners as wn


def check_surface(v, what):
    pos, val = wn.slice_winners(v)
    want_pos, want_val = wn.lowest_argmax(v)
    assert np.array_equal(pos, want_pos), (what, pos.tolist(), want_pos.tolist())
    assert np.array_equal(val.view(np.uint32), want_val.view(np.uint32)), what


def test_run_geometry():
    starts = [wn.run_start(r) for r in range(sw.SLICES * wn.RUNS_PER_SLICE)]
    assert starts[:3] == [0, 11, 22] and starts[22:25] == [242, 245, 256] and starts[-1] == 5365
    covered = np.zeros(sw.POSITIONS, dtype=int)
    for s in starts:
        covered[s:s + wn.RUN] += 1
    assert covered.min() == 1 and set(np.nonzero(covered == 2)[0] % sw.SLICE) == set(range(245, 253))      # runs 22 and 23 share 245..252


def test_model_is_the_lowest_argmax_on_random_surfaces():
    rng = np.random.default_rng(4100)
    for j in range(6):
        check_surface(rng.random(sw.POSITIONS, dtype=np.float32), ("uniform", j))
    for j in range(6):
        check_surface(rng.integers(0, 4, size=sw.POSITIONS).astype(np.float32), ("many exact ties and zeros", j))
    check_surface(np.zeros(sw.POSITIONS, dtype=np.float32), "all zero: position 0 of every slice")
    v = np.zeros(sw.POSITIONS, dtype=np.float32)
    v[700] = 1e-42                                                                                          # one denormal in an otherwise zero slice
    check_surface(v, "denormal")


def test_model_is_the_lowest_argmax_where_every_run_ties(orc):
    o = orc.Oracle(depth=8, threads=8, **sw.A_CFG)
    for d in sw.A_PERIODS:
        cd = sw.antiperiodic_window(d)
        for p in range(8):
            xb = o.scan_xb(cd, 0, p)
            assert np.array_equal(xb[d:].view(np.uint32), xb[:-d].view(np.uint32))                          # every run holds the maximum
            check_surface(xb, ("antiperiodic", d, p))
            pos, _ = wn.slice_winners(xb)
            assert np.all(pos - sw.SLICE * np.arange(sw.SLICES) < d), (d, p, pos.tolist())


@pytest.mark.parametrize("at", range(242, 256))
def test_model_is_the_lowest_argmax_in_the_overlapped_runs(at):
    """A maximum at 245..252 sits in run 22 and in run 23: the octet's first lane (run 22) stores, and its walk names the position once.
    Two equal maxima, one in each run's own part, keep the lower."""
    rng = np.random.default_rng(4200 + at)
    v = rng.random(sw.POSITIONS, dtype=np.float32)
    v[at::sw.SLICE] = 2.0
    check_surface(v, ("single", at))
    w = v.copy()
    w[254::sw.SLICE] = 2.0                                                                                  # run 23's own positions: 253..255
    check_surface(w, ("tie with 254", at))
    w = v.copy()
    w[243::sw.SLICE] = 2.0                                                                                  # run 22's own: 242..244
    check_surface(w, ("tie with 243", at))


# ---- (b) the census conditions of the GPU families, with the oracle alone ----
def test_family_r_geometry():
    starts = [wn.r_start(k) for k in range(wn.R_WINDOWS)]
    in_slice = [s % sw.SLICE for s in starts]
    assert sorted({min(i // wn.RUN, 23) if i < 245 else 23 for i in in_slice}) == list(range(24))          # every run of a slice
    assert {(5 * k) % wn.RUN for k in range(wn.R_WINDOWS)} == set(range(wn.RUN))                           # every position of a run
    assert len({s // sw.SLICE for s in starts}) == sw.SLICES                                                # every slice
    assert all(a > b for a, b in zip(wn.R_AMP, wn.R_AMP[1:]))
    for k in (0, 23):
        w = wn.r_window(k)
        assert w.dtype == np.complex64 and w.shape == (sw.N,) and np.isfinite(w).all() and w.tobytes() == wn.r_window(k).tobytes()


def test_family_r_census_shares(orc):
    """Measured: the minimum over the 24 windows is 29 of 40 groups decided, 799 of 960 overall; the on-frequency pattern-0 group is
    decided in every window but k = 8."""
    total = 0
    open_on_frequency = []
    for k in range(wn.R_WINDOWS):
        dec = wn.census_of(orc, ("R", k), sw.B_CFG, wn.r_window(k))
        assert dec.shape == (5, 8)
        n = int(dec.sum())
        print("family R window", k, "decided", n, "of", dec.size)
        assert n >= wn.R_MIN_DECIDED, (k, n)
        total += n
        if not dec[sw.B_BLOCK, 0]:
            open_on_frequency.append(k)
    print("family R decided overall", total, "of", 40 * wn.R_WINDOWS, "on-frequency pattern 0 open in", open_on_frequency)
    assert len(open_on_frequency) <= 1, open_on_frequency


def test_family_r_winner_is_the_strongest_burst(orc):
    """Where the on-frequency pattern-0 group is decided, its largest slot is the strongest burst, seen at r_start(k) or its ghost."""
    o = orc.Oracle(depth=1, threads=8, **sw.B_CFG)
    for k in (0, 7, 22, 23):
        cd = wn.r_window(k)
        if not wn.census_of(orc, ("R", k), sw.B_CFG, cd)[sw.B_BLOCK, 0]:
            continue
        g = o.scan(cd)[sw.B_BLOCK * 8:][:8]
        assert int(g["pos"][int(np.argmax(g["xb"]))]) in sw.peak_positions(wn.r_start(k)), (k, g["pos"].tolist())
        pos, val = wn.slice_winners(o.scan_xb(cd, sw.B_BLOCK, 0))
        want_pos, _ = wn.lowest_argmax(o.scan_xb(cd, sw.B_BLOCK, 0))
        assert np.array_equal(pos, want_pos)


def test_family_n_census_shares(orc):
    """Measured: 50, 52 and 47 of the 102 groups of patterns 0-4 and 7 decided; patterns 5 and 6 are periodic: 0 of 17 each."""
    for seed in wn.N_SEEDS:
        cd = wn.n_window(seed)
        dec = wn.census_of(orc, ("N", seed), wn.N_CFG, cd)
        assert dec.shape == (17, 8)
        n = int(dec[:, wn.N_PATTERNS].sum())
        print("family N seed", seed, "decided", n, "of", 17 * len(wn.N_PATTERNS), "periodic patterns decided", int(dec[:, 5].sum()), int(dec[:, 6].sum()))
        assert n >= wn.N_MIN_DECIDED, (seed, n)
        assert not dec[:, 5].any() and not dec[:, 6].any()
        o = orc.Oracle(depth=8, threads=8, **wn.N_CFG)
        for b, p in ((0, 0), (8, 4), (16, 7)):
            check_surface(o.scan_xb(cd, b, p), ("noise", seed, b, p))
