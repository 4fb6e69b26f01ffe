"""-m gpu: the handle's phasor table (csrc/mix.h, mix_table_kernel) and the tile order of the scan and softbits kernels
(csrc/tile_map.h).

The table is held to the float32 model of tests/mix_table_model.py bit for bit.  The tile order only decides WHERE a (channel,
frequency) tile runs, so a batch of channels must leave, channel by channel, the bytes the same window leaves alone in a one-channel
handle; and blocked staging, whose channel blocks cut across the tile groups, must report the records of the retained run."""
import os
import re

import numpy as np
import pytest

from msk144cudecoder_amd import synth

import mix_table_model as M

pytestmark = pytest.mark.gpu

G = int(re.search(r"#define MSK144_TILE_GROUP (\d+)", open(os.path.join(M.CSRC, "tile_map.h")).read()).group(1))
MAX_CHANNELS = 2 * G + 3
WIDTH_OF_F = {1: 0.0, 5: 4.0, 17: 16.0}
FIELDS = ("pos", "xb", "nbadsync", "softbits_wo_sync")


# ---- the table ----

TABLE_HANDLES = {
    "audio": (dict(center=1500.0, width=500.0, step=1.0, read_mode=1), 501, (0, 250, 500)),
    "iq": (dict(center=0.0, width=500.0, step=1.0, read_mode=2), 501, (0, 250, 500)),
    "one": (dict(center=1500.0, width=0.0, step=1.0, read_mode=1), 1, (0,)),
}


@pytest.mark.parametrize("name", list(TABLE_HANDLES))
def test_table_rows_equal_the_model_bit_for_bit(hip, name):
    cfg, F, rows = TABLE_HANDLES[name]
    with hip.HipDecoder(channels=1, depth=1, **cfg) as d:
        assert d.F == F
        for b in rows:
            f = np.float32(d.frequency(b))
            got = d.dump_mix_table(b)
            want = M.table_row(f)
            diff = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
            print(f"{name} row {b} ({float(f):+.1f} Hz): {len(diff)} of {M.WINDOW} entries differ from the model")
            assert len(diff) == 0, (name, b, diff[:8], got[diff[:4]], want[diff[:4]])
            if f == 0.0:
                assert np.array_equal(got.view(np.uint32), np.tile(np.array([1.0, 0.0], np.float32).view(np.uint32), (M.WINDOW, 1)))
        if name == "iq":
            assert d.frequency(0) < 0.0 < d.frequency(500) and d.frequency(250) == 0.0


# ---- tile order: a batch against its channels one at a time ----

_WINDOWS = {}
_SINGLE = {}


def _windows(mode):
    """One noise-plus-ping window per channel, made once and left unchanged."""
    if mode not in _WINDOWS:
        rng = np.random.default_rng(1144 + (mode == "iq"))
        rows = []
        for c in range(MAX_CHANNELS):
            ping = synth.Ping(synth.random_message(rng), int(rng.integers(0, 2000)), 6, (1500.0 if mode == "audio" else 0.0) + float(rng.uniform(-2, 2)), 3.0,
                              float(rng.uniform(0, 6.28)))
            rows.append(synth.synth_audio(5184, [ping], 1000.0, rng) if mode == "audio" else synth.synth_iq(5184, [ping], 20.0, rng))
        w = np.stack(rows)
        w.setflags(write=False)
        _WINDOWS[mode] = w
    return _WINDOWS[mode]


def _cfg(mode, F, depth, threshold=2):
    return dict(center=1500.0 if mode == "audio" else 0.0, width=WIDTH_OF_F[F], step=1.0, depth=depth, nbadsync_threshold=threshold,
                read_mode=1 if mode == "audio" else 2)


def _submit(d, mode, w):
    d.submit_audio(w) if mode == "audio" else d.submit_iq(w)


def _single(hip, mode, F, depth):
    """dump_candidates of every window through a one-channel handle (one tile group of one channel: G plays no part)."""
    key = (mode, F, depth)
    if key not in _SINGLE:
        out = []
        with hip.HipDecoder(channels=1, **_cfg(mode, F, depth)) as d:
            assert d.F == F
            for w in _windows(mode):
                _submit(d, mode, w)
                d.decode()
                it = d.dump_candidates(0)
                it.setflags(write=False)
                out.append(it)
        _SINGLE[key] = out
    return _SINGLE[key]


@pytest.mark.parametrize("mode", ["audio", "iq"])
@pytest.mark.parametrize("depth", [1, 6, 8])
@pytest.mark.parametrize("F", [1, 5, 17])
@pytest.mark.parametrize("channels", sorted({1, max(G - 1, 1), G + 1, 2 * G + 3}))
def test_batch_equals_its_channels_one_at_a_time(hip, channels, F, depth, mode):
    single = _single(hip, mode, F, depth)
    with hip.HipDecoder(channels=channels, llr_block_channels=channels, **_cfg(mode, F, depth)) as d:
        _submit(d, mode, _windows(mode)[:channels])
        d.decode()
        for c in range(channels):
            got = d.dump_candidates(c)
            for f in FIELDS:
                assert got[f].tobytes() == single[c][f].tobytes(), (c, f)
            assert got.tobytes() == single[c].tobytes(), c      # and what LDPC made of those rows


# ---- blocked staging: channel blocks that cut across tile groups ----

_RETAINED = {}


def _retained(hip):
    if not _RETAINED:
        cfg = _cfg("audio", 5, 6, threshold=3)
        with hip.HipDecoder(channels=MAX_CHANNELS, llr_block_channels=MAX_CHANNELS, max_results=1 << 16, **cfg) as d:
            d.submit_audio(_windows("audio"))
            d.decode()
            _RETAINED["run"] = (cfg, d.results().copy())
    return _RETAINED["run"]


@pytest.mark.parametrize("handover", [True, False])
@pytest.mark.parametrize("block", sorted({3, G + 1}))
def test_blocked_staging_across_group_edges_equals_the_retained_run(hip, block, handover):
    cfg, full = _retained(hip)
    assert len(full) > 0 and MAX_CHANNELS % block != 0       # the pings decode; the last block is short
    with hip.HipDecoder(channels=MAX_CHANNELS, llr_block_channels=block, max_results=1 << 16, **cfg) as d:
        assert d.llr_block == block
        d.set_copy_handover(handover)
        d.submit_audio(_windows("audio"))
        d.decode()
        res = d.results().copy()
    assert len(res) == len(full)
    for f in full.dtype.names:
        assert np.array_equal(res[f], full[f]), f
