"""The synthetic LLR rows of tests/ldpc_rows.py meet, with the oracle alone, the conditions tests/test_gpu_ldpc_rows.py relies on:
every BP outcome is present often enough, the hard-error gate splits where it should, and the oracle's own decision is stable
on all but a number of rows well inside the GPU test's cap for tolerated differences."""
import numpy as np
import pytest

import ldpc_rows
import parity


@pytest.fixture(scope="module")
def rowset(orc):
    rs = ldpc_rows.finite_rows()
    return rs, ldpc_rows.oracle_outcomes(orc, rs.rows)


def test_families_are_complete_and_unique(rowset):
    rs, _ = rowset
    assert set(rs.family) == set(ldpc_rows.FINITE_FAMILIES)
    assert 2500 <= len(rs) <= 3500 and rs.rows.dtype == np.float32 and np.isfinite(rs.rows).all()
    again = ldpc_rows.finite_rows()
    assert again.rows.tobytes() == rs.rows.tobytes()                                   # seeded: the GPU file builds the same rows
    clean = rs.of("clean")
    assert (np.abs(rs.rows[clean][rs.tag[clean] == 0]) < np.finfo(np.float32).tiny).all()   # amplitude 1e-42 is a denormal
    er = rs.of("erasures")
    assert [(rs.rows[k] == 0.0).sum() for k in er] == [int(rs.tag[k]) for k in er]


def test_noisy_rows_cover_every_outcome(rowset):
    rs, out = rowset
    m = rs.of("noisy")
    accepted = out[m][out["ok"][m] == 1]
    per_iteration = np.bincount(accepted["it"], minlength=10)
    assert len(per_iteration) == 10 and per_iteration.min() >= 8, per_iteration
    assert (out["ok"][m] == 0).sum() >= 200
    ok = out["ok"][m] == 1
    assert np.array_equal(out["msg"][m][ok].astype(np.uint8), rs.msg[m][ok])           # near the threshold, but no false decode among them


def test_clean_and_bad_crc_rows(rowset):
    rs, out = rowset
    c = rs.of("clean")
    assert (out["ok"][c] == 1).all() and (out["it"][c] == 0).all() and (out["nh"][c] == 0).all()
    assert np.array_equal(out["msg"][c].astype(np.uint8), rs.msg[c])
    assert (out["ok"][rs.of("bad_crc")] == 0).all()


def test_gate_rows_split_at_18_hard_errors(rowset):
    rs, out = rowset
    g = rs.of("gate")
    flips = rs.tag[g]
    below = g[flips < 18]
    assert (out["ok"][below] == 1).all() and np.array_equal(out["nh"][below], rs.tag[below])
    assert (out["it"][below] >= 1).all()                                               # BP had to correct them first
    assert np.array_equal(out["msg"][below].astype(np.uint8), rs.msg[below])
    assert (out["ok"][g[flips >= 18]] == 0).all()
    assert sorted(set(flips.tolist())) == [16, 17, 18, 19]


def test_other_families_reach_their_targets(rowset):
    rs, out = rowset
    er = rs.of("erasures")
    assert (out["ok"][er[rs.tag[er] <= 8]] == 1).all() and (out["ok"][er] == 0).any()   # a few erasures are filled in, 38 are not
    sf = rs.of("strong_flips")
    assert (out["ok"][sf] == 1).any() and (out["ok"][sf] == 0).any()


def test_oracle_is_stable_on_all_but_half_the_cap(rowset, orc):
    """Rows whose (accept, iteration) the oracle itself changes under a relative 1e-6 perturbation (8 trials) spend the GPU
    test's cap without any fault of the kernel: they must be at most half of it."""
    rs, out = rowset
    unstable = ldpc_rows.oracle_unstable_rows(orc, rs.rows, out)
    cap = ldpc_rows.tolerated_cap(len(rs))
    assert cap == -(-len(rs) // 1000)
    assert len(unstable) <= cap // 2, (unstable, [str(rs.family[k]) for k in unstable])


def test_verify_marginal_moves_exact_zeros(rowset, orc):
    """The helper has verify_marginal_bp's contract (a stable difference raises) and its absolute term reaches erased positions."""
    rs, out = rowset
    k = int(rs.of("clean")[3])
    with pytest.raises(AssertionError, match="STABLE"):
        parity.verify_marginal_bp(orc, rs.rows[k], (False, -1), seed=1, absolute=True)
    with pytest.raises(AssertionError, match="STABLE"):
        parity.verify_marginal_bp(orc, rs.rows[k], (True, 2), seed=1, absolute=True)
    rng = np.random.default_rng(3)
    e = rs.rows[int(rs.of("erasures")[-1])]
    zeros = e == 0.0
    assert zeros.sum() == 38
    assert (parity.perturbed_llr(e, 1e-4, rng)[zeros] == 0.0).all()
    assert (parity.perturbed_llr(e, 1e-4, rng, absolute=True)[zeros] != 0.0).all()
    assert np.abs(parity.perturbed_llr(e, 1e-4, rng, absolute=True) - e).max() <= 1e-4 * (3.0 + 3.0) * 1.001
    # a row on a decision boundary, found by bisection between an accepted and a rejected noisy row: the oracle shows both
    # outcomes around it, so the one from across the boundary is tolerated - and an outcome from nowhere near still is not
    m = rs.of("noisy")
    lo, hi = rs.rows[m[out["ok"][m] == 1][0]].astype(np.float64), rs.rows[m[out["ok"][m] == 0][0]].astype(np.float64)
    o_lo = parity.bp_outcome(orc, lo.astype(np.float32))[:2]
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if parity.bp_outcome(orc, mid.astype(np.float32))[:2] == o_lo:
            lo = mid
        else:
            hi = mid
    o_hi = parity.bp_outcome(orc, hi.astype(np.float32))[:2]
    assert o_hi != o_lo and np.abs(hi - lo).max() <= 1e-6 * np.abs(lo).max()
    assert parity.verify_marginal_bp(orc, lo.astype(np.float32), o_hi, seed=5, absolute=True) == parity.BP_PERTURBATION_SCALES[0]
    with pytest.raises(AssertionError, match="STABLE"):
        parity.verify_marginal_bp(orc, lo.astype(np.float32), (True, 11), seed=5, absolute=True)


def test_nonfinite_rows(rowset, orc):
    rs, _ = rowset
    rows, desc = ldpc_rows.nonfinite_rows(rs)
    assert len(rows) == len(desc) and not np.isfinite(rows).all(axis=1).any()
    assert np.isnan(rows[-1]).all()
    for n in (1, 2, 64):
        assert ((~np.isfinite(rows)).sum(axis=1) == n).any()
    out = ldpc_rows.oracle_outcomes(orc, rows)
    assert ((out["ok"] == 1) & (out["it"] == 0)).sum() >= 4                            # the rows the GPU test holds to the oracle exactly
