"""The windows, plans and model of tests/softbits_positions.py meet, with the oracle and numpy alone, what
tests/test_gpu_softbits_positions.py relies on: the vectorised model is numpy_model.softbits, the plans cover what they claim, the
oracle's yardsticks exist, the nbadsync rule leaves few candidates open and the windows exercise both ends of the count.  These are
conditions on the inputs and on the reference; no kernel runs here."""
import numpy as np
import pytest

from msk144cudecoder_amd.protocol import PATTERN_MASK

import numpy_model
import softbits_positions as sp


def assert_is_numpy_model(m, k, mixed, pattern, pos):
    soft, llr, nbad = numpy_model.softbits(mixed, PATTERN_MASK[pattern], int(pos) % sp.N)
    assert np.abs(soft - m.soft[k]).max() <= 1e-12 * np.abs(soft).max(), (k, pattern, pos)
    assert np.abs(llr - m.L[k]).max() <= 1e-12 * np.abs(llr).max(), (k, pattern, pos)
    assert nbad == m.nbad[k], (k, pattern, pos)


@pytest.fixture(scope="module")
def family_a(orc):
    """(model, oracle rows, oracle nbadsync, yardsticks) of all 43008 candidates."""
    m = sp.model_a()
    o = orc.Oracle(depth=8, **sp.A_CFG)
    assert o.F == 1 and o.frequency(0) == 0.0
    plan = sp.plan_a().reshape(-1)
    rows, nbad = sp.oracle_rows(o, sp.window(), np.zeros(len(plan), dtype=int), np.arange(len(plan)) % 64 // 8, plan)
    return m, rows, nbad, sp.worst(sp.fit(rows, m))


@pytest.fixture(scope="module")
def family_c(orc):
    """Per shape: (model, oracle rows, oracle nbadsync, pos, blocks, patterns, channel of each candidate), rounds and channels flattened."""
    out = []
    for shape, (channels, cfg) in enumerate(sp.C_SHAPES):
        o = orc.Oracle(depth=8, **cfg)
        assert o.F * channels == sp.C_TILE_COUNTS[shape]
        freqs = [np.float32(o.frequency(b)) for b in range(o.F)]
        plan = sp.plan_c(shape)
        models, rows, nbads = [], [], []
        k = np.arange(o.F * 64)
        for r in range(plan.shape[0]):
            for c in range(channels):
                cd = sp.c_window(c)
                models.append(sp.model_of_channel(("C", c), cd, freqs, 8, plan[r, c]))
                g, nb = sp.oracle_rows(o, cd, k // 64, k % 64 // 8, plan[r, c])
                rows.append(g)
                nbads.append(nb)
        out.append(dict(model=sp.join(models), rows=np.concatenate(rows), nbad=np.concatenate(nbads), pos=plan.reshape(-1), F=o.F, freqs=freqs,
                        channel=np.tile(np.repeat(np.arange(channels), o.F * 64), plan.shape[0])))
    return out


@pytest.fixture(scope="module")
def yard_c(family_c):
    m = sp.join([f["model"] for f in family_c])
    return sp.worst(sp.fit(np.concatenate([f["rows"] for f in family_c]), m))


def test_windows_are_seeded_and_shaped():
    a = sp.window()
    assert a.dtype == np.complex64 and a.shape == (sp.N,) and np.isfinite(a).all() and a.tobytes() == sp.window().tobytes()
    assert sp.c_window(0).tobytes() != sp.c_window(1).tobytes() != a.tobytes()
    # the second ping is cut at the ring's end: the pings raise the power of their spans and nothing wraps to the start
    power = np.abs(a.astype(np.complex128)) ** 2
    assert power[700:700 + 3 * 864].mean() > 1.5 * power[:700].mean() and power[3900:].mean() > 2.5 * power[:700].mean()
    e = sp.e_windows()
    assert np.isnan(e[1, sp.E_SAMPLE].real) and np.isinf(e[2, sp.E_SAMPLE].real) and int((~np.isfinite(e)).sum()) == 2
    assert np.array_equal(e[0], a)
    for k in sp.D_EXPONENTS:
        assert np.array_equal(sp.d_window(k).view(np.float32), (a.view(np.float32) * np.float32(2.0) ** k))        # exact, no sample leaves the normal range


def test_plan_a_is_a_bijection_per_pattern_and_every_wave_meets_everything():
    plan = sp.plan_a().reshape(sp.A_TILES, 8, sp.SLOTS).astype(np.int64)
    assert plan.max() == sp.POSITIONS - 1                                         # never above 5375: the kernel subtracts the ring length once
    for p in range(8):
        assert np.array_equal(np.sort(plan[:, p, :].reshape(-1)), np.arange(sp.POSITIONS))
    ring = plan % sp.N
    for s in range(sp.SLOTS):                                                     # wave s owns slot s of every pattern
        assert np.array_equal(np.unique(plan[:, :, s]), np.arange(sp.POSITIONS))  # every position, so every residue and every base entry q
        assert set((ring[:, :, s] // 6).reshape(-1).tolist()) == set(range(sp.RING_Q))
        for p in range(8):
            assert set((ring[:, p, s] % 6).tolist()) == set(range(6)), (s, p)
            assert np.ptp(plan[:, p, s]) == sp.A_TILES - 1                         # 672 consecutive positions: 112 entries q of each residue
    # every (residue, pattern) meets every base entry q, 722..863 (a frame wraps inside the sub-ring's pad) included
    for p in range(8):
        for r in range(6):
            sel = ring[:, p, :] % 6 == r
            assert set((ring[:, p, :][sel] // 6).tolist()) == set(range(sp.RING_Q)), (p, r)
    # ring twins: p0 and p0 + 5184 for every p0 < 192 in every pattern
    assert sp.POSITIONS - sp.N == sp.TWINS
    # B and D take A's own tiles: the same candidates, the same model rows
    for depth in sp.B_DEPTHS:
        assert np.array_equal(sp.plan_a(sp.B_TILES, depth), sp.plan_a()[list(sp.B_TILES), :depth * 8])
    assert sp.A_TILES % 6 == 0 and sp.A_TILES * 8 == sp.POSITIONS


def test_plan_c_structural_positions_meet_every_pattern():
    assert len(sp.STRUCTURAL) == 102 and len(np.unique(sp.STRUCTURAL)) == 102 and sp.STRUCTURAL.max() == sp.POSITIONS - 1
    for shape, (channels, cfg) in enumerate(sp.C_SHAPES):
        tiles = sp.C_TILE_COUNTS[shape]
        assert tiles % 8 != 0
        plan = sp.plan_c(shape)
        assert plan.max() < sp.POSITIONS and np.array_equal(plan, sp.plan_c(shape))
        per_pattern = plan.reshape(plan.shape[0], tiles, 8, sp.SLOTS)
        for p in range(8):
            got = set(per_pattern[:, :, p, :].reshape(-1).tolist())
            assert set(sp.STRUCTURAL.tolist()) <= got, (shape, p)
            assert len(got) > len(sp.STRUCTURAL)                                  # and random positions beside them
        # the structural positions do not sit in one wave
        assert all(len(set(per_pattern[..., s].reshape(-1).tolist()) & set(sp.STRUCTURAL.tolist())) >= 40 for s in range(sp.SLOTS)), shape


def test_model_is_numpy_model_family_a_b_d_e(family_a):
    m = family_a[0]
    x = sp.window().astype(np.complex128)
    plan = sp.plan_a().reshape(-1)
    rng = np.random.default_rng(11)
    picks = np.concatenate([rng.integers(0, len(plan), 48), rng.choice(sp.a_rows(sp.B_TILES), 16), rng.choice(sp.a_rows(sp.D_TILES), 8), sp.a_rows([0])[::7]])
    for k in picks:
        assert_is_numpy_model(m, int(k), x, int(k) % 64 // 8, plan[k])
    # twins: the model sees one ring
    low = np.nonzero(plan < sp.TWINS)[0]
    assert len(low) == 8 * sp.TWINS
    # D: the model is scale-free
    idx = sp.a_rows(sp.D_TILES)
    for k in sp.D_EXPONENTS:
        md = sp.model_of_channel(("D", k), sp.d_window(k), [np.float32(0.0)], 8, sp.plan_a([3])[0])
        ma = sp.take(m, sp.a_rows([3]))
        assert np.abs(md.L - ma.L).max() <= 1e-12 * np.abs(ma.L).max() and np.array_equal(md.nbad, ma.nbad), k
        assert np.allclose(md.kappa, ma.kappa, rtol=1e-12)
    assert len(idx) == 6 * 64
    # E: the candidates whose frames miss the sample keep their model row, the others have none
    e = sp.e_windows()
    m0 = sp.take(m, sp.a_rows([0]))
    pos0 = sp.plan_a([0])[0].astype(np.int64)
    for c in (1, 2):
        me = sp.model_of_channel(("E", c), e[c], [np.float32(0.0)], 8, pos0)
        finite = np.isfinite(me.L).all(axis=1)
        hit = np.array([any(PATTERN_MASK[k // 8][f] and (sp.E_SAMPLE - pos0[k] - sp.FRAME * f) % sp.N < sp.FRAME for f in range(6)) for k in range(64)])
        assert np.array_equal(finite, ~hit) and 8 <= int(finite.sum()) <= 56, (c, int(finite.sum()))
        assert np.array_equal(me.L[finite], m0.L[finite]) and np.array_equal(me.nbad[finite], m0.nbad[finite])


def test_model_is_numpy_model_family_c(family_c):
    rng = np.random.default_rng(12)
    for shape, f in enumerate(family_c):
        for k in rng.integers(0, len(f["pos"]), 24):
            item = int(k) % (f["F"] * 64)
            c = int(f["channel"][k])
            mixed = numpy_model.mix(sp.c_window(c), f["freqs"][item // 64])
            assert_is_numpy_model(f["model"], int(k), mixed, item % 64 // 8, f["pos"][k])


def test_oracle_yardsticks_family_a(family_a):
    """Measured: rho 2.83e-6, alpha 2.10e-7, gamma 3.71e-6 over the 43008 candidates, where the plain max |dLLR| / max(1, |llr|) of the
    same rows is 9.3e-5: the fit takes the carrier angle of ill-conditioned candidates (kappa up to 324) out of the number."""
    m, rows, nbad, yard = family_a
    assert all(np.isfinite(v) and v > 0.0 for v in yard.values()), yard
    assert yard["rho"] < 1e-5 and yard["alpha"] < 1e-6 and yard["gamma"] < 1e-5, yard        # float32 rounding, not a structural difference
    assert np.isfinite(m.L).all() and np.isfinite(m.Q).all() and np.isfinite(m.kappa).all()
    # the oracle itself passes the rule it sets for the kernel
    sure, marg = sp.sync_bounds(m, sp.limits_of(yard))
    assert np.all((nbad >= sure) & (nbad <= sure + marg))


def test_oracle_yardsticks_family_c(family_c, yard_c):
    """Measured over the 8832 candidates of the four shapes (the 11-tile shape runs twice): rho 2.47e-6, alpha 1.27e-7, gamma 1.57e-6."""
    print("family C oracle yardsticks", yard_c)
    assert all(np.isfinite(v) and v > 0.0 for v in yard_c.values()), yard_c
    assert yard_c["rho"] < 1e-5 and yard_c["alpha"] < 1e-6 and yard_c["gamma"] < 1e-5, yard_c
    for f in family_c:
        sure, marg = sp.sync_bounds(f["model"], sp.limits_of(yard_c))
        assert np.all((f["nbad"] >= sure) & (f["nbad"] <= sure + marg))


def test_fit_names_what_is_wrong(family_a):
    """An angle, a gain and one moved softbit put into model rows come out as alpha, gamma and rho, each alone."""
    m = sp.take(family_a[0], np.arange(0, 43008, 97))
    n = len(m.L)
    f = sp.fit(m.L + 3e-5 * m.kappa[:, None] * m.Q, m)
    assert np.allclose(f.alpha, 3e-5) and f.rho.max() < 1e-12 and f.gamma.max() < 1e-12
    f = sp.fit(m.L * (1 + 2e-5), m)
    assert np.allclose(f.gamma, 2e-5) and f.rho.max() < 1e-12 and f.alpha.max() < 1e-12
    rows = m.L.copy()
    rows[:, 40] += 1e-3 * np.maximum(1.0, np.abs(rows[:, 40]))
    f = sp.fit(rows, m)
    assert f.rho.min() > 0.9e-3 and np.all(np.abs(f.rest).argmax(axis=1) == 40)
    assert n > 400


def test_marginal_share_and_nbadsync_span(family_a, family_c, yard_c):
    """Measured with the limits 4 x the oracle's: A 9 of 43008 candidates hold a marginal sync softbit (0.02 %), histogram 0..12;
    C 3 of 8832 (0.03 %), histogram 0..11.  B, D and E are subsets of A's candidates (768, 384 and 64 of them: 1, 0 and 0 marginal):
    their share is held to the same bound; their own histograms cannot reach 0 (no tile of theirs sits on a ping's frame start), so
    for the span A's histogram stands for them - the rows and counts they compare are A's."""
    m, _, _, yard = family_a
    assert sp.marginal_share(m, yard) <= sp.MARGINAL_SHARE
    hist = np.bincount(m.nbad)
    assert hist[0] > 0 and len(hist) - 1 >= 10 and np.all(hist[:11] > 0), hist
    for tiles in (sp.B_TILES, sp.D_TILES, (0,)):
        assert sp.marginal_share(sp.take(m, sp.a_rows(tiles)), yard) <= sp.MARGINAL_SHARE, tiles
    mc = sp.join([f["model"] for f in family_c])
    assert sp.marginal_share(mc, yard_c) <= sp.MARGINAL_SHARE
    hist = np.bincount(mc.nbad)
    print("family C nbadsync histogram", hist.tolist(), "marginal share", sp.marginal_share(mc, yard_c))
    assert hist[0] > 0 and len(hist) - 1 >= 10, hist


def test_family_d_oracle_stays_inside_its_yardsticks(orc, family_a):
    """The oracle at 2^-40 .. 2^40 times the window, on D's 384 candidates each: no exponent had to move."""
    m, _, _, yard = family_a
    o = orc.Oracle(depth=8, **sp.A_CFG)
    idx = sp.a_rows(sp.D_TILES)
    md = sp.take(m, idx)
    plan = sp.plan_a(sp.D_TILES).reshape(-1)
    for k in sp.D_EXPONENTS:
        rows, nbad = sp.oracle_rows(o, sp.d_window(k), np.zeros(len(plan), dtype=int), np.arange(len(plan)) % 64 // 8, plan)
        w = sp.worst(sp.fit(rows, md))
        assert all(w[name] <= yard[name] for name in yard), (k, w, yard)
        assert np.array_equal(nbad, family_a[2][idx]), k
