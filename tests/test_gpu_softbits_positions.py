"""softbits_kernel alone (the retained variant) at the planned positions of tests/softbits_positions.py: submit_analytic,
load_candidates, decode(STAGE_SOFTBITS), then the candidate dump.

  A  every position 0..5375 in every pattern, every wave at every residue mod 6 and base entry q: rows against the float64 model under
     4 x the oracle's own rho / alpha / gamma, nbadsync inside [sure, sure + marginal]; the 1536 ring twins bit for bit
  B  depths 1..7: the same bytes as the depth-8 run
  C  tile counts 11, 33, 65 and 18 at real frequencies, a window per channel: the same limits from this family's own oracle
     yardsticks, and every channel equal to its one-channel run
  D  the window times 2^-40 .. 2^40: A's model rows, A's limits
  E  a NaN and an Inf sample beside a finite channel

Which part a failure names: rho on one residue, q range or softbit is the plane (tap, fold base, wrap pad, lane map); rho on row entries
next to the sync words with alpha beside it, or alpha alone, is the phase sum (its edge term: u1[6], u2[56], u1[62], u2[0]); gamma is
the normalisation; nbadsync alone, with the rows right, is softbit 0 (the wrap sum u1[143] + u2[0]) or the sync pass's own fold."""
import collections

import numpy as np
import pytest

from msk144cudecoder_amd.hipdecoder import CANDIDATE_DTYPE, STAGE_SOFTBITS

import softbits_positions as sp

pytestmark = pytest.mark.gpu

Run = collections.namedtuple("Run", "items F D freqs")        # items: the dumps [channels][K]


def run_softbits(hip, cfg, depth, windows, pos):
    """The stage alone on seeded candidates: windows complex64 [channels][5184], pos [channels][K].  Checks what the stage must leave:
    pos and xb untouched, every nbadsync computed, no seeded LLR."""
    windows = np.ascontiguousarray(windows, dtype=np.complex64).reshape(-1, sp.N)
    n = len(windows)
    pos = np.asarray(pos).reshape(n, -1)
    assert int(pos.max()) < sp.POSITIONS                        # the kernel subtracts the ring length once and indexes LDS with the result
    with hip.HipDecoder(depth=depth, channels=n, llr_block_channels=n, **cfg) as d:
        assert d.K == pos.shape[1] and d.D == depth
        d.submit_analytic(windows)
        for c in range(n):
            d.load_candidates(sp.seed_items(CANDIDATE_DTYPE, pos[c]), c)
        d.decode(STAGE_SOFTBITS)                                # the call returns
        items = np.stack([d.dump_candidates(c) for c in range(n)])
        run = Run(items, d.F, d.D, [np.float32(d.frequency(b)) for b in range(d.F)])
    assert np.array_equal(items["pos"], pos) and np.all(items["xb"] == sp.SEEDED_XB)
    assert np.all((items["nbadsync"] >= 0) & (items["nbadsync"] <= 16)), np.unique(items["nbadsync"])
    assert not np.any(items["softbits_wo_sync"].view(np.uint32) == sp.SENTINEL.view(np.uint32)), "a seeded LLR was left in a row"
    return run


def same_bytes(a, b):
    """Candidates whose nbadsync and LLR row are equal byte for byte, as a mask."""
    return (a["nbadsync"] == b["nbadsync"]) & (a["softbits_wo_sync"].view(np.uint32) == b["softbits_wo_sync"].view(np.uint32)).all(axis=-1)


_A = {}


def run_a(hip):
    """The depth-8 run of all 672 tiles, flat in the order of sp.model_a(); made once and left unchanged."""
    if "items" not in _A:
        run = run_softbits(hip, sp.A_CFG, 8, np.broadcast_to(sp.window(), (sp.A_TILES, sp.N)), sp.plan_a())
        assert run.F == 1 and run.freqs[0] == 0.0
        items = run.items.reshape(-1)
        items.setflags(write=False)
        _A["items"] = items
    return _A["items"]


def yard_a(orc):
    if "yard" not in _A:
        o = orc.Oracle(depth=8, **sp.A_CFG)
        plan = sp.plan_a().reshape(-1)
        rows, _ = sp.oracle_rows(o, sp.window(), np.zeros(len(plan), dtype=int), np.arange(len(plan)) % 64 // 8, plan)
        _A["yard"] = sp.worst(sp.fit(rows, sp.model_a()))
    return _A["yard"]


# ------------------------------------------------------------------------------------------------
# A. every position
# ------------------------------------------------------------------------------------------------
def test_a_every_position(orc, hip, parity_report):
    items = run_a(hip)
    rep = sp.compare(sp.model_a(), yard_a(orc), items["softbits_wo_sync"], items["nbadsync"], items["pos"], 64)
    # ring twins: p0 and p0 + 5184 are one place, so one computation
    pos = items["pos"].astype(np.int64)
    pattern = np.arange(len(items)) % 64 // 8
    at = {(int(p), int(q)): k for k, (p, q) in enumerate(zip(pattern, pos)) if q < sp.TWINS or q >= sp.N}
    low = np.array([at[(p, q)] for p in range(8) for q in range(sp.TWINS)])
    high = np.array([at[(p, q + sp.N)] for p in range(8) for q in range(sp.TWINS)])
    same = same_bytes(items[low], items[high])
    assert same.all(), ("a ring twin differs from its position", dict(pattern=int(pattern[low[~same][0]]), pos=int(pos[low[~same][0]])))
    rep["twin_pairs_identical"] = int(same.sum())
    assert rep["twin_pairs_identical"] == 8 * sp.TWINS
    parity_report("softbits_positions_A", rep)


# ------------------------------------------------------------------------------------------------
# B. depth
# ------------------------------------------------------------------------------------------------
_B = {}


@pytest.mark.parametrize("depth", sp.B_DEPTHS)
def test_b_depth(hip, parity_report, depth):
    run = run_softbits(hip, sp.A_CFG, depth, np.broadcast_to(sp.window(), (len(sp.B_TILES), sp.N)), sp.plan_a(sp.B_TILES, depth))
    full = run_a(hip)[sp.a_rows(sp.B_TILES, depth)]
    got = run.items.reshape(-1)
    assert np.array_equal(got["pos"], full["pos"])
    same = same_bytes(got, full)
    assert same.all(), ("a candidate differs from the depth-8 run", dict(depth=depth, first=sp.where(int(np.nonzero(~same)[0][0]), got["pos"], depth * 8, depth)))
    _B[depth] = int(same.sum())
    parity_report("softbits_positions_B", dict(identical_to_depth_8_run=dict(_B), candidates=sum(_B.values())))


# ------------------------------------------------------------------------------------------------
# C. frequencies and the tile map
# ------------------------------------------------------------------------------------------------
_C = {}


def yard_c(orc):
    """This family's own oracle yardsticks, over the candidates of all four shapes; with them the models, per shape."""
    if "yard" not in _C:
        models, rows = [], []
        for shape, (channels, cfg) in enumerate(sp.C_SHAPES):
            o = orc.Oracle(depth=8, **cfg)
            freqs = [np.float32(o.frequency(b)) for b in range(o.F)]
            plan = sp.plan_c(shape)
            k = np.arange(o.F * 64)
            per_shape = []
            for r in range(plan.shape[0]):
                for c in range(channels):
                    per_shape.append(sp.model_of_channel(("C", c), sp.c_window(c), freqs, 8, plan[r, c]))
                    rows.append(sp.oracle_rows(o, sp.c_window(c), k // 64, k % 64 // 8, plan[r, c])[0])
            models.append(sp.join(per_shape))
            _C[("freqs", shape)] = freqs
        _C["models"] = models
        _C["yard"] = sp.worst(sp.fit(np.concatenate(rows), sp.join(models)))
    return _C["yard"]


@pytest.mark.parametrize("shape", range(len(sp.C_SHAPES)))
def test_c_frequencies_and_tile_map(orc, hip, parity_report, shape):
    channels, cfg = sp.C_SHAPES[shape]
    yard = yard_c(orc)
    plan = sp.plan_c(shape)
    wins = np.stack([sp.c_window(c) for c in range(channels)])
    runs = [run_softbits(hip, cfg, 8, wins, plan[r]) for r in range(plan.shape[0])]
    assert runs[0].F * channels == sp.C_TILE_COUNTS[shape]
    assert [f.tobytes() for f in runs[0].freqs] == [f.tobytes() for f in _C[("freqs", shape)]]        # the model mixed with the handle's float32 frequencies
    items = np.concatenate([r.items.reshape(-1) for r in runs])
    rep = sp.compare(_C["models"][shape], yard, items["softbits_wo_sync"], items["nbadsync"], items["pos"], runs[0].F * 64)
    # the tile map: a channel of the batch is its one-channel run
    alone = list(range(channels)) if channels <= 3 else list(sp.C_SINGLE_13)
    identical = 0
    for r in range(plan.shape[0]):
        for c in alone:
            one = run_softbits(hip, cfg, 8, wins[c], plan[r, c])
            same = same_bytes(one.items[0], runs[r].items[c])
            assert same.all(), ("a channel of the batch differs from its one-channel run", dict(shape=shape, channel=c, item=int(np.nonzero(~same)[0][0])))
            identical += int(same.sum())
    rep["identical_to_one_channel_run"] = identical
    _C.setdefault("report", {})[str(sp.C_TILE_COUNTS[shape]) + "_tiles"] = rep
    parity_report("softbits_positions_C", dict(_C["report"]))


# ------------------------------------------------------------------------------------------------
# D. dynamic range
# ------------------------------------------------------------------------------------------------
def test_d_power_of_two_scale(orc, hip, parity_report):
    wins = np.stack([sp.d_window(k) for k in sp.D_EXPONENTS for _ in sp.D_TILES])
    pos = np.concatenate([sp.plan_a(sp.D_TILES)] * len(sp.D_EXPONENTS))
    run = run_softbits(hip, sp.A_CFG, 8, wins, pos)
    idx = np.tile(sp.a_rows(sp.D_TILES), len(sp.D_EXPONENTS))
    items = run.items.reshape(-1)
    rep = sp.compare(sp.take(sp.model_a(), idx), yard_a(orc), items["softbits_wo_sync"], items["nbadsync"], items["pos"], 64)      # the model is scale-free
    rep["exponents"] = list(sp.D_EXPONENTS)
    rep["identical_to_unscaled_run"] = int(same_bytes(items, run_a(hip)[idx]).sum())                                                 # reported, not required
    parity_report("softbits_positions_D", rep)


# ------------------------------------------------------------------------------------------------
# E. non-finite samples beside a finite channel
# ------------------------------------------------------------------------------------------------
def test_e_nonfinite_samples(hip, parity_report):
    wins = sp.e_windows()
    pos0 = sp.plan_a([0])
    run = run_softbits(hip, sp.A_CFG, 8, wins, np.concatenate([pos0] * 3))        # the call returns, every nbadsync is in 0..16
    alone = run_softbits(hip, sp.A_CFG, 8, wins[0], pos0)
    assert same_bytes(run.items[0], alone.items[0]).all(), "the finite channel differs from its run alone"
    assert same_bytes(run.items[0], run_a(hip)[sp.a_rows([0])]).all(), "the finite channel differs from tile 0 of the 672-channel run"
    rep = {}
    for name, c in (("nan", 1), ("inf", 2)):
        finite = np.isfinite(sp.model_of_channel(("E", c), wins[c], [np.float32(0.0)], 8, pos0[0]).L).all(axis=1)
        same = same_bytes(run.items[c], run.items[0])
        assert same[finite].all(), ("a candidate whose frames miss the sample differs from the finite channel's", name, np.nonzero(finite & ~same)[0].tolist())
        assert not np.isfinite(run.items[c]["softbits_wo_sync"][~finite]).all(axis=1).any(), ("a finite row from a non-finite sample", name)
        rep[name] = dict(candidates=64, finite_in_model=int(finite.sum()), identical_to_finite_channel=int(same.sum()))
    parity_report("softbits_positions_E", rep)
