"""-m gpu: the softbits kernel's sync pass (one pass per wave for the sync check and carrier phase of all its candidates, then part two
per kept candidate) against the CPU oracle and against itself across the three kernel variants (retained store, blocked staging with
and without the hand-over).  One channel or two, width 20 / step 2 (F = 11)."""
import numpy as np
import pytest

from msk144cudecoder_amd import synth
from msk144cudecoder_amd.hipdecoder import STAGE_SOFTBITS

import parity

pytestmark = pytest.mark.gpu

BASE = dict(center=1500.0, width=20.0, step=2.0)
PERIOD = {5: 864, 6: 2592}
_ORACLE_RUNS = {}
_RETAINED_RUNS = {}


def _oracle_run(orc, depth):
    """Window, oracle and oracle candidates of one depth, computed once and left unchanged."""
    if depth not in _ORACLE_RUNS:
        cfg = dict(depth=depth, nbadsync_threshold=2, **BASE)
        rng = np.random.default_rng(430 + depth)
        x = synth.synth_audio(5184, [synth.Ping(synth.random_message(rng), 500, 6, 1504.0, 0.0, float(rng.uniform(0, 6.28)))], 1000.0, rng)
        o = orc.Oracle(threads=8, **cfg)
        cd = o.frontend_audio(x, 2)
        items_o, _ = o.decode_window(cd)
        items_o.setflags(write=False)
        _ORACLE_RUNS[depth] = (cfg, x, o, cd, items_o)
    return _ORACLE_RUNS[depth]


@pytest.mark.parametrize("depth", [1, 6, 8])
def test_retained_store_against_oracle(orc, hip, depth):
    """Positions from the oracle, with one tile (frequency 3) overwritten so that it holds a ring-wrap twin (p and p + 5184 in two slots
    of a pattern), a position at 5375, the residues and the ring's end, and from depth 6 on periodic copies of pattern 5 (p, p + 864);
    softbits stage alone, every LLR row and nbadsync compared with the oracle at those positions under parity's limits."""
    cfg, x, o, cd, items_o = _oracle_run(orc, depth)
    seed_items = items_o.copy()
    seed_items["softbits_wo_sync"] = 0
    seed_items["nbadsync"] = 99
    per_freq = 8 * depth
    t0 = 3 * per_freq
    pos = seed_items["pos"]
    pos[t0 + 0], pos[t0 + 1] = 100, 100 + 5184              # pattern 0: a ring-wrap twin
    pos[t0 + 2], pos[t0 + 3], pos[t0 + 4] = 5375, 0, 5183   # the last scanned position, the ring's start and end
    pos[t0 + 5], pos[t0 + 6], pos[t0 + 7] = 5179, 4321, 5184
    if depth >= 6:
        p5 = t0 + 8 * 5
        pos[p5 + 0], pos[p5 + 1], pos[p5 + 2], pos[p5 + 3] = 77, 77 + 864, 77 + 3 * 864, 77 + 5184   # periodic copies and a wrap twin
        pos[p5 + 4], pos[p5 + 5] = 5375, 5375 - 864
    with hip.HipDecoder(channels=1, **cfg) as d:
        d.submit_audio(x)
        d.load_candidates(seed_items.view(hip.CANDIDATE_DTYPE), 0)
        d.decode(STAGE_SOFTBITS)
        items_g = d.dump_candidates(0)
    assert np.array_equal(items_g["pos"], seed_items["pos"])
    assert (items_g["nbadsync"] >= 0).all() and (items_g["nbadsync"] <= 16).all()          # every slot computed on its own
    rep = parity.compare_softbits(o, cd, items_o, items_g)
    print(f"depth {depth}: {rep}")
    assert rep["nbadsync_marginal"] <= 1
    # a ring-wrap twin is the same computation: the same sync check and the same row, bit for bit
    tile = items_g[t0:t0 + per_freq]
    assert tile[0]["nbadsync"] == tile[1]["nbadsync"] and tile[0]["softbits_wo_sync"].tobytes() == tile[1]["softbits_wo_sync"].tobytes()
    if depth >= 6:
        assert tile[40]["nbadsync"] == tile[43]["nbadsync"] and tile[40]["softbits_wo_sync"].tobytes() == tile[43]["softbits_wo_sync"].tobytes()


def _two_windows():
    rng = np.random.default_rng(8086)
    msg = synth.random_message(rng)
    return np.stack([synth.synth_audio(5184, [synth.Ping(msg, 200, 6, 1500.0 + 3.3, 3.0, 1.1)], 1000.0, rng),
                     np.rint(rng.normal(0.0, 1000.0, 5184)).astype(np.int16)])


def _retained_run(hip, threshold):
    if threshold not in _RETAINED_RUNS:
        cfg = dict(depth=6, nbadsync_threshold=threshold, **BASE)
        with hip.HipDecoder(channels=2, llr_block_channels=2, max_results=1 << 16, **cfg) as d:
            d.submit_audio(_two_windows())
            d.decode()
            _RETAINED_RUNS[threshold] = (cfg, d.results().copy(), [d.dump_candidates(c) for c in range(2)], [d.dump_indexes(c) for c in range(2)])
    return _RETAINED_RUNS[threshold]


@pytest.mark.parametrize("handover", [True, False])
@pytest.mark.parametrize("threshold", [0, 3])
def test_blocked_staging_equals_the_retained_run(hip, threshold, handover):
    """Two channels in blocks of one (the gated kernels), against the retained run of the same windows.  A blocked handle does not expose
    its nbadsync array (dumps need retained rows), so the array is checked through everything that reads it: the index stage lists
    exactly the slots whose retained nbadsync is <= threshold, minus - with the hand-over - the slots that fold the same frames as a
    lower slot of their group (stored as -1 - s, which the index stage leaves out); the collect stage resolves -1 - s to slot s, so
    the result list, nbadsync field included, is byte-identical to the retained run's."""
    cfg, full, items, idx_full = _retained_run(hip, threshold)
    with hip.HipDecoder(channels=2, llr_block_channels=1, max_results=1 << 16, **cfg) as d:
        d.set_copy_handover(handover)
        d.submit_audio(_two_windows())
        d.decode()
        res = d.results().copy()
        idx = [d.dump_indexes(c) for c in range(2)]
        copies = d.copy_count()
    handed = 0
    for c in range(2):
        it = items[c]
        nb = it["nbadsync"]
        assert (nb >= 0).all()
        pos = it["pos"].astype(np.int64) % 5184
        drop = np.zeros(len(it), dtype=bool)
        if handover:
            for g0 in range(0, len(it), 8):
                r = pos[g0:g0 + 8] % PERIOD.get(int(it["pattern_idx"][g0]), 5184)
                for sl in range(1, 8):
                    drop[g0 + sl] = bool((r[:sl] == r[sl]).any())
        want = np.nonzero((nb <= threshold) & ~drop)[0].astype(np.int32)
        assert np.array_equal(idx[c], want), c
        assert np.array_equal(idx_full[c], np.nonzero(nb <= threshold)[0].astype(np.int32)), c
        handed += int(drop.sum())
    assert copies == handed and (handed > 40) == handover          # pattern 5 is mostly periodic copies
    assert res.tobytes() == full.tobytes()
    assert len(full) > 0                                           # the ping is strong: the list is not trivially empty


@pytest.mark.parametrize("kind", ["audio", "analytic"])
def test_zero_window_completes_with_the_parents_nbadsync(hip, kind):
    """An all-zero window.  Audio: the front end's 1/rms makes every sample NaN and the phasor takes its NaN branch; analytic zeros:
    every folded sum is 0 and the phasor takes its m2 == 0 branch, (1, 0).  Either way no softbit is negative, so every sync bit is
    read as +1 and each candidate disagrees with the four -1 bits of both sync words: nbadsync = 8 in every slot, as before the pass."""
    cfg = dict(depth=6, nbadsync_threshold=16, **BASE)
    with hip.HipDecoder(channels=1, **cfg) as d:
        if kind == "audio":
            d.submit_audio(np.zeros(5184, dtype=np.int16))
        else:
            d.submit_analytic(np.zeros(5184, dtype=np.complex64))
        d.decode()
        if kind == "audio":
            assert d.result_count() == 0
        items = d.dump_candidates(0)
    assert (items["nbadsync"] == 8).all(), np.unique(items["nbadsync"])
