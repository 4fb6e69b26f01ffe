"""ldpc_kernel, index_kernel and the two collect kernels alone, on the synthetic LLR rows of tests/ldpc_rows.py: load_candidates,
decode(STAGE_INDEX | STAGE_LDPC | STAGE_COLLECT), then the candidate dump, the index list and the result list.

  A  every finite row against the oracle's BP, one row per wave; then a reload with rows gated out
  B  1024 channels, five or six rows per wave: the outcome of a row depends neither on its channel, its place in the list nor
     on the length of the list (equality with A's run, no oracle); hand-over markers in 64 channels
  C  the compactions at K = 8, 88, 1032 and 2056 with empty, full, one-item and sparse lists
  D  NaN and infinite rows beside finite ones
"""
import time

import numpy as np
import pytest

from msk144cudecoder_amd.hipdecoder import CANDIDATE_DTYPE, RESULT_DTYPE, STAGE_COLLECT, STAGE_INDEX, STAGE_LDPC
from msk144cudecoder_amd.protocol import PATTERN_NUM_AVG, SLOTS_PER_PATTERN

import ldpc_rows
import parity

pytestmark = pytest.mark.gpu

STAGES = STAGE_INDEX | STAGE_LDPC | STAGE_COLLECT
THRESHOLD = 16
GATED_OUT = 99
CFG = dict(center=1500.0, width=20.0, step=2.0, depth=8, nbadsync_threshold=THRESHOLD)    # F = 11, K = 11 * 8 * 8 = 704
K_ROWS = 704
LIST_LENGTHS = (0, 1, 2, 127, 128, 129, 255, 256, 257, 385, 511, 512, 513, 640, 703, 704)   # around multiples of the 128 waves per channel


# ------------------------------------------------------------------------------------------------
# host model of the index list and the result list
# ------------------------------------------------------------------------------------------------
def make_items(llr, nbad):
    """Candidates of one channel: the LLR rows and nbadsync values given, pos = item, xb = float(item)."""
    k = len(llr)
    items = np.zeros(k, dtype=CANDIDATE_DTYPE)
    items["softbits_wo_sync"] = llr
    items["nbadsync"] = nbad
    items["pos"] = np.arange(k)
    items["xb"] = np.arange(k, dtype=np.float32)
    return items


def source_items(nbad):
    """The item whose nbadsync and decode item k reports: itself, or for a marker -1 - s slot s of its own group."""
    k = np.arange(len(nbad))
    return np.where(nbad < 0, (k & ~(SLOTS_PER_PATTERN - 1)) + (-1 - nbad), k)


def index_list(nbad):
    return np.nonzero((nbad >= 0) & (nbad <= THRESHOLD))[0].astype(np.int32)


def outcomes_of(items):
    """ldpc_rows.OUTCOME_DTYPE of dumped candidates (the dump leaves every field of a slot without a decode 0)."""
    out = np.zeros(len(items), dtype=ldpc_rows.OUTCOME_DTYPE)
    out["ok"], out["it"], out["nh"], out["msg"] = items["is_message_present"], items["ldpc_num_iterations"], items["ldpc_num_hard_errors"], items["message"]
    return out


def frequencies(d):
    if not hasattr(d, "_grid"):
        d._grid = np.array([d.frequency(b) for b in range(d.F)], dtype=np.float32)
    return d._grid


def expected_records(d, channel, nbad, outcome):
    """The records of one channel in item order: `outcome` holds the BP outcome of the row in every item (read only where the
    item is in the index list); a marker reports nbadsync, iterations, hard errors and message of its source, pos and xb of its own."""
    src = source_items(nbad)
    keep = np.nonzero((nbad[src] >= 0) & (nbad[src] <= THRESHOLD) & (outcome["ok"][src] == 1))[0]
    per_freq = d.D * SLOTS_PER_PATTERN
    rec = np.zeros(len(keep), dtype=RESULT_DTYPE)
    rec["channel"] = channel
    rec["item"] = keep
    rec["f0"] = frequencies(d)[keep // per_freq]
    rec["pattern_idx"] = (keep % per_freq) // SLOTS_PER_PATTERN
    rec["num_avg"] = np.asarray(PATTERN_NUM_AVG)[rec["pattern_idx"]]
    rec["pos"] = keep
    rec["xb"] = keep.astype(np.float32)
    rec["nbadsync"] = nbad[src[keep]]
    rec["ldpc_iterations"] = outcome["it"][src[keep]]
    rec["ldpc_hard_errors"] = outcome["nh"][src[keep]]
    bits = np.concatenate([outcome["msg"][src[keep]].astype(np.uint8), np.zeros((len(keep), 3), dtype=np.uint8)], axis=1)
    rec["message"] = np.packbits(bits, axis=1) if len(keep) else 0
    return rec


def expected_candidates(d, llr, nbad, outcome):
    """The candidate dump of one channel: what was loaded, and a decode exactly where the item is in the index list."""
    exp = make_items(llr, nbad)
    k = np.arange(len(llr))
    per_freq = d.D * SLOTS_PER_PATTERN
    exp["block_idx"] = k // per_freq
    exp["pattern_idx"] = (k % per_freq) // SLOTS_PER_PATTERN
    exp["f0"] = frequencies(d)[exp["block_idx"]]
    exp["num_avg"] = np.asarray(PATTERN_NUM_AVG)[exp["pattern_idx"]]
    dec = index_list(nbad)
    dec = dec[outcome["ok"][dec] == 1]
    exp["is_message_present"][dec] = 1
    exp["ldpc_num_iterations"][dec] = outcome["it"][dec]
    exp["ldpc_num_hard_errors"][dec] = outcome["nh"][dec]
    exp["message"][dec] = outcome["msg"][dec]
    return exp


def assert_same_records(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    if got.tobytes() == exp.tobytes():
        return
    for name in got.dtype.names:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(exp[name])
        differs = (a.view(np.uint8).reshape(len(got), -1) != b.view(np.uint8).reshape(len(got), -1)).any(axis=1)
        assert not differs.any(), (what, name, int(np.nonzero(differs)[0][0]), got[differs][:1], exp[differs][:1])
    raise AssertionError((what, "records differ outside their named fields"))


# ------------------------------------------------------------------------------------------------
# the rows and the one-row-per-wave run every other test takes its expected outcomes from
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rowset(orc):
    rs = ldpc_rows.finite_rows()
    return rs, ldpc_rows.oracle_outcomes(orc, rs.rows)


@pytest.fixture(scope="module")
def run_a(rowset, hip):
    """Every finite row once, 704 to a channel (the grid then has one wave per item), nbadsync 0; then the same handle again with
    every second accepted row gated out."""
    rs, _ = rowset
    n = len(rs)
    channels = -(-n // K_ROWS)
    llr = np.zeros((channels * K_ROWS, 128), dtype=np.float32)
    llr[:n] = rs.rows
    nbad = np.full(channels * K_ROWS, GATED_OUT, dtype=np.int32)
    nbad[:n] = 0

    def run(d, nb):
        for c in range(channels):
            d.load_candidates(make_items(llr[c * K_ROWS:(c + 1) * K_ROWS], nb[c * K_ROWS:(c + 1) * K_ROWS]), c)
        d.decode(STAGES)
        return (np.concatenate([d.dump_candidates(c) for c in range(channels)]), [d.dump_indexes(c) for c in range(channels)], d.results().copy())

    with hip.HipDecoder(channels=channels, llr_block_channels=channels, **CFG) as d:
        assert (d.F, d.D, d.K) == (11, 8, K_ROWS)
        first = run(d, nbad)
        accepted = np.nonzero(first[0]["is_message_present"][:n])[0]
        nbad2 = nbad.copy()
        nbad2[accepted[::2]] = GATED_OUT
        second = run(d, nbad2)
        exp_records = [np.concatenate([expected_records(d, c, nb[c * K_ROWS:(c + 1) * K_ROWS], outcomes_of(items[c * K_ROWS:(c + 1) * K_ROWS])) for c in range(channels)])
                       for nb, items in ((nbad, first[0]), (nbad2, second[0]))]
    return dict(n=n, channels=channels, nbad=(nbad, nbad2), first=first, second=second, exp_records=exp_records, got=outcomes_of(first[0][:n]))


def test_a_every_finite_row_equals_the_oracle(rowset, run_a, orc, parity_report):
    rs, exp = rowset
    got, n = run_a["got"], run_a["n"]
    same = (got["ok"] == exp["ok"]) & (got["it"] == exp["it"]) & (got["nh"] == exp["nh"]) & (got["msg"] == exp["msg"]).all(axis=1)
    tolerated = []
    for k in np.nonzero(~same)[0]:
        g = (bool(got["ok"][k]), int(got["it"][k]) if got["ok"][k] else -1)
        o = (bool(exp["ok"][k]), int(exp["it"][k]) if exp["ok"][k] else -1)
        assert g != o, ("same accept and iteration as the oracle, other hard errors or message", int(k), str(rs.family[k]), got[k], exp[k])
        scale = parity.verify_marginal_bp(orc, rs.rows[k], g, seed=1000 + int(k), absolute=True)
        tolerated.append(dict(row=int(k), family=str(rs.family[k]), oracle=list(o), gpu=list(g), unstable_at_perturbation=scale))
    unstable = ldpc_rows.oracle_unstable_rows(orc, rs.rows, exp)
    cap = ldpc_rows.tolerated_cap(n)
    per_family = {f: dict(compared=int(len(rs.of(f))), equal=int(same[rs.of(f)].sum()), tolerated=sum(t["family"] == f for t in tolerated)) for f in ldpc_rows.FINITE_FAMILIES}
    parity_report("ldpc_rows_A", dict(compared=n, equal=int(same.sum()), tolerated=len(tolerated), cap=cap, oracle_unstable=len(unstable),
                                      per_family=per_family, tolerated_rows=tolerated,
                                      accepted_per_iteration=np.bincount(got["it"][got["ok"] == 1], minlength=10).tolist(), rejected=int((got["ok"] == 0).sum())))
    assert len(tolerated) <= cap, (len(tolerated), cap, tolerated)

    # what the families are for holds of the kernel's own outcomes, whatever was tolerated above
    c = rs.of("clean")
    assert (got["ok"][c] == 1).all() and (got["it"][c] == 0).all() and (got["nh"][c] == 0).all(), (rs.tag[c], got[c])
    assert np.array_equal(got["msg"][c].astype(np.uint8), rs.msg[c])
    assert (got["ok"][rs.of("bad_crc")] == 0).all()
    g = rs.of("gate")
    acc = g[got["ok"][g] == 1]
    assert len(acc) and np.isin(got["nh"][acc], (16, 17)).all() and (rs.tag[acc] < 18).all(), (rs.tag[acc], got["nh"][acc])

    # the index lists and the result list of the same run
    nbad = run_a["nbad"][0]
    for c in range(run_a["channels"]):
        assert np.array_equal(run_a["first"][1][c], index_list(nbad[c * K_ROWS:(c + 1) * K_ROWS])), c
    assert_same_records(run_a["first"][2], run_a["exp_records"][0], "result list of the first run")


def test_a_reload_leaves_nothing_stale(run_a):
    n = run_a["n"]
    first, second = run_a["first"][0], run_a["second"][0]
    nbad, nbad2 = run_a["nbad"]
    gated = np.nonzero(nbad != nbad2)[0]
    assert len(gated) > 400 and (first["is_message_present"][gated] == 1).all()
    assert (second["is_message_present"][gated] == 0).all() and (second["ldpc_num_iterations"][gated] == 0).all() and (second["message"][gated] == 0).all()
    kept = np.nonzero(nbad == nbad2)[0]
    assert first[kept].tobytes() == second[kept].tobytes()
    for c in range(run_a["channels"]):
        assert np.array_equal(run_a["second"][1][c], index_list(nbad2[c * K_ROWS:(c + 1) * K_ROWS])), c
    assert_same_records(run_a["second"][2], run_a["exp_records"][1], "result list after the reload")
    assert len(run_a["second"][2]) == len(run_a["first"][2]) - len(gated) and n > 0


# ------------------------------------------------------------------------------------------------
# B: launch shapes
# ------------------------------------------------------------------------------------------------
def pick_rows(rs, got, count, seed):
    """`count` rows across all families: up to 40 of every small family, six of every accept iteration, the rest drawn from all rows."""
    rng = np.random.default_rng(seed)
    chosen = []
    for f in ldpc_rows.FINITE_FAMILIES:
        m = rs.of(f)
        if f != "noisy":
            chosen.extend(m[np.linspace(0, len(m) - 1, min(len(m), 40)).astype(int)].tolist())
    for it in range(10):
        chosen.extend(np.nonzero((got["ok"] == 1) & (got["it"] == it))[0][:6].tolist())
    chosen = list(dict.fromkeys(chosen))
    rest = np.setdiff1d(np.arange(len(rs)), chosen)
    chosen.extend(rng.choice(rest, size=count - len(chosen), replace=False).tolist())
    return np.array(chosen[:count])


def test_b_outcome_is_independent_of_the_launch_shape(rowset, run_a, hip, parity_report):
    rs, _ = rowset
    got_a = run_a["got"]
    t0 = time.perf_counter()
    u = pick_rows(rs, got_a, K_ROWS, seed=8100)
    assert len(set(u.tolist())) == K_ROWS and set(rs.family[u]) == set(ldpc_rows.FINITE_FAMILIES)
    rows_u, out_u = rs.rows[u], got_a[u]
    channels = 1024
    marker_channels = [c for c in range(channels) if (c // 16) % 16 == 0]           # 64 channels, every list length four times
    sampled = list(range(32))                                                        # 16 with markers, 16 without: every list length twice
    assert len(marker_channels) == 64
    exp_rec, markers, marker_records, per_channel = [], 0, 0, {}
    with hip.HipDecoder(channels=channels, llr_block_channels=channels, max_results=1 << 20, **CFG) as d:
        assert d.K == K_ROWS and d.llr_block == channels
        for c in range(channels):
            rng = np.random.default_rng([8200, c])
            perm = rng.permutation(K_ROWS)
            nbad = np.full(K_ROWS, GATED_OUT, dtype=np.int32)
            inside = rng.choice(K_ROWS, size=LIST_LENGTHS[c % 16], replace=False)
            nbad[inside] = rng.integers(0, THRESHOLD + 1, size=len(inside))
            if c in marker_channels:
                for k in np.nonzero((nbad == GATED_OUT) & (np.arange(K_ROWS) % SLOTS_PER_PATTERN >= 1) & (rng.random(K_ROWS) < 0.5))[0]:
                    base = k & ~(SLOTS_PER_PATTERN - 1)
                    lower = [s for s in range(k - base) if nbad[base + s] >= 0]     # slot 0 never is a marker
                    nbad[k] = -1 - int(rng.choice(lower))
                markers += int((nbad < 0).sum())
            assert ((nbad >= -SLOTS_PER_PATTERN) & (nbad <= GATED_OUT)).all() and (source_items(nbad) <= np.arange(K_ROWS)).all() and (nbad[source_items(nbad)] >= 0).all()
            d.load_candidates(make_items(rows_u[perm], nbad), c)
            exp_rec.append(expected_records(d, c, nbad, out_u[perm]))
            marker_records += int((nbad[exp_rec[-1]["item"]] < 0).sum())
            if c in sampled:
                per_channel[c] = (perm, nbad)
        t_load = time.perf_counter()
        d.decode(STAGES)
        res = d.results()
        t_decode = time.perf_counter()
        exp_rec = np.concatenate(exp_rec)
        assert len(exp_rec) > 100000 and markers > 3000 and marker_records > 1000
        assert d.result_count() == len(exp_rec)
        assert_same_records(res, exp_rec, "result list of 1024 channels")
        assert d.copy_count() == markers
        for c, (perm, nbad) in per_channel.items():
            assert np.array_equal(d.dump_indexes(c), index_list(nbad)), c
            assert_same_records(d.dump_candidates(c), expected_candidates(d, rows_u[perm], nbad, out_u[perm]), f"candidates of channel {c}")
    assert sorted({len(index_list(nb)) for _, nb in per_channel.values()}) == sorted(LIST_LENGTHS)
    wall = time.perf_counter() - t0
    parity_report("ldpc_rows_B", dict(channels=channels, records=int(len(exp_rec)), markers=markers, marker_records=marker_records,
                                      wall_s=round(wall, 2), load_s=round(t_load - t0, 2), decode_and_results_s=round(t_decode - t_load, 2)))
    print(f"B: {len(exp_rec)} records, {markers} markers, wall {wall:.2f} s (load {t_load - t0:.2f} s, decode + results {t_decode - t_load:.2f} s)")


# ------------------------------------------------------------------------------------------------
# C: the compactions at small and large K
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,k_items", [(0.0, 8), (20.0, 88), (256.0, 1032), (512.0, 2056)])
def test_c_compaction_shapes(rowset, run_a, hip, width, k_items):
    rs, _ = rowset
    got_a = run_a["got"]
    rng = np.random.default_rng(8300 + k_items)
    pick = rng.permutation(len(rs))[:k_items]
    pick[[0, -1]] = rng.choice(np.nonzero(got_a["ok"] == 1)[0], size=2, replace=False)      # the one-item lists yield a record,
    pick[1] = rng.choice(np.nonzero(got_a["ok"] == 0)[0])                                   # the full list of 8 a rejected row too
    llr, outcome = rs.rows[pick], got_a[pick]
    every_65th = np.arange(0, k_items, 65)
    lists = dict(empty=[], full=np.arange(k_items), first=[0], last=[k_items - 1], every_65th=every_65th)
    with hip.HipDecoder(center=1500.0, width=width, step=2.0, depth=1, nbadsync_threshold=THRESHOLD, channels=1, llr_block_channels=1) as d:
        assert (d.D, d.K) == (1, k_items)
        for name, inside in lists.items():
            nbad = np.full(k_items, THRESHOLD + 1, dtype=np.int32)                  # just outside the gate
            nbad[np.asarray(inside, dtype=int)] = THRESHOLD                          # just inside
            d.load_candidates(make_items(llr, nbad), 0)
            d.decode(STAGES)
            assert np.array_equal(d.dump_indexes(0), np.asarray(inside, dtype=np.int32)), (name, k_items)
            exp = expected_records(d, 0, nbad, outcome)
            assert d.result_count() == len(exp), (name, k_items)
            assert_same_records(d.results(), exp, f"{name} list of {k_items}")
            assert_same_records(d.dump_candidates(0), expected_candidates(d, llr, nbad, outcome), f"candidates, {name} list of {k_items}")
    if k_items >= 88:
        assert (outcome["ok"] == 1).sum() >= 8 and (outcome["ok"] == 0).sum() >= 8     # accepted and rejected rows in every list but the short ones


# ------------------------------------------------------------------------------------------------
# D: non-finite rows
# ------------------------------------------------------------------------------------------------
def test_d_nonfinite_rows_disturb_nothing(rowset, run_a, orc, hip, parity_report):
    rs, _ = rowset
    got_a = run_a["got"]
    bad_rows, desc = ldpc_rows.nonfinite_rows(rs)
    bad_out = ldpc_rows.oracle_outcomes(orc, bad_rows)
    fin = np.random.default_rng(8400).permutation(len(rs))[:K_ROWS // 2]
    llr = np.zeros((K_ROWS, 128), dtype=np.float32)
    llr[0::2] = rs.rows[fin]
    which = np.arange(K_ROWS // 2) % len(bad_rows)                                  # every non-finite row three times, between finite ones
    llr[1::2] = bad_rows[which]
    nbad = np.zeros(K_ROWS, dtype=np.int32)
    with hip.HipDecoder(channels=1, llr_block_channels=1, **CFG) as d:
        d.load_candidates(make_items(llr, nbad), 0)
        d.decode(STAGES)                                                            # returns normally
        with_bad = d.dump_candidates(0)
        n_with = d.result_count()
        nbad[1::2] = GATED_OUT
        d.load_candidates(make_items(llr, nbad), 0)
        d.decode(STAGES)
        without = d.dump_candidates(0)
        n_without = d.result_count()
    assert with_bad[0::2].tobytes() == without[0::2].tobytes()
    assert np.array_equal(with_bad["softbits_wo_sync"].view(np.uint32), llr.view(np.uint32))       # the rows themselves come back bit for bit
    g_fin = outcomes_of(with_bad[0::2])
    assert g_fin.tobytes() == got_a[fin].tobytes()                                  # and every finite row decodes as it did in A
    assert (without["is_message_present"][1::2] == 0).all()
    g_bad = outcomes_of(with_bad[1::2])
    assert n_with - n_without == int(g_bad["ok"].sum()) and n_without == int(g_fin["ok"].sum())
    at_once = (bad_out["ok"] == 1) & (bad_out["it"] == 0)                           # decided before any message is formed
    assert at_once.sum() >= 4
    sel = at_once[which]
    assert g_bad[sel].tobytes() == bad_out[which][sel].tobytes(), [desc[j] for j in np.nonzero(at_once)[0]]
    differing = []
    for j in range(len(bad_rows)):
        if at_once[j]:
            continue
        g, o = g_bad[j], bad_out[j]                                                 # the row's first copy; the copies are compared below
        if g.tobytes() != o.tobytes():
            differing.append(dict(row=desc[j], oracle=[int(o["ok"]), int(o["it"]), int(o["nh"])], gpu=[int(g["ok"]), int(g["it"]), int(g["nh"])],
                                  same_message=bool((g["msg"] == o["msg"]).all())))
    for j in range(len(bad_rows), K_ROWS // 2):
        assert g_bad[j].tobytes() == g_bad[which[j]].tobytes(), desc[which[j]]       # the same row decodes the same wherever it sits
    parity_report("ldpc_rows_D", dict(nonfinite_rows=len(bad_rows), equal_to_oracle_at_iteration_0=int(at_once.sum()),
                                      others=int((~at_once).sum()), others_differing=len(differing), differing=differing))
