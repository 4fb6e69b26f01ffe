"""-m gpu: the refusals of msk144_push_hops and msk144_push_rate_hops, one table for both entries - the same code and, with the
entry's own names filled in, the same text - and a good push behind the whole table: a refused push leaves nothing half-done."""
import numpy as np
import pytest

from msk144cudecoder_amd import input_rate as ir
from msk144cudecoder_amd import synth
from msk144cudecoder_amd.hipdecoder import unpack_message

import input_rate_scene as S

pytestmark = pytest.mark.gpu
CH = 4
RATE = 24000
EINVAL, ESTATE = -1, -4

# the two entries, by the names their messages use: {push} the entry, {slot} the entry that hands out its pinned rows
ENTRIES = {"plain": dict(push="msk144_push_hops", slot="msk144_hop_slot"), "rate": dict(push="msk144_push_rate_hops", slot="msk144_rate_hop_slot")}

NOT_ASCENDING = "streams must be ascending stream numbers below channels"
# (slot, n, streams, is_first, code, text); the first case runs before the slot was asked for, the others behind it
BEFORE_SLOT = (0, 1, None, None, ESTATE, "{push} before {slot}")
TABLE = [
    (2, 1, [0], [1], EINVAL, "bad argument"),
    (0, 0, [0], [1], EINVAL, "n must be 1..channels"),
    (0, 5, [0], [1], EINVAL, "n must be 1..channels"),
    (0, 2, [3, 1], [1, 1], EINVAL, NOT_ASCENDING),
    (0, 2, [1, 1], [1, 1], EINVAL, NOT_ASCENDING),
    (0, 2, [0, 4], [1, 1], EINVAL, NOT_ASCENDING),
    (0, 2, [-1, 0], [1, 1], EINVAL, NOT_ASCENDING),
]
# the rate entry alone: a later hop before a first one; and with a position that is not ascending ahead of it, or at it, which wins
RATE_TABLE = [
    (0, 2, [0, 1], [1, 0], ESTATE, "{push}: stream 1 has a later hop before a first one (is_first = 0)"),
    (0, 3, [2, 1, 3], [1, 1, 0], EINVAL, NOT_ASCENDING),
    (0, 2, [1, 0], [1, 0], EINVAL, NOT_ASCENDING),
]


def _refusal(hip, fn):
    with pytest.raises(hip.Msk144Error) as e:
        fn()
    return e.value.code, str(e.value).split(": ", 1)[1]


def _run(hip, entry):
    """The whole table on one handle, then one good first hop of stream 0, decoded: (refusals got, refusals wanted, records, payload)."""
    names = ENTRIES[entry]
    rate = entry == "rate"
    # a 5184-sample 12 kHz window with one MSK144 frame, sample-held to RATE
    rng = np.random.default_rng(58)
    msg = synth.random_message(rng)
    xr = np.repeat(synth.synth_audio(5184, [synth.Ping(msg, 400, 6, 1502.0, 6.0, 0.7)], 1000.0, rng), RATE // 12000)
    row = ir.row_samples(RATE)
    with hip.HipDecoder(channels=CH, **S.CFG) as d:
        if rate:
            d.set_input_rate(RATE)
        push = d.push_rate_hops if rate else d.push_hops
        slot, n, _, _, code, text = BEFORE_SLOT
        got = [_refusal(hip, lambda: push(slot, n))]
        want = [(code, text.format(**names))]
        hops, first_halves, ids, is_first = d.rate_hop_slot(0) if rate else d.hop_slot(0)
        hops[:] = 0
        first_halves[:] = 0
        for slot, n, streams, firsts, code, text in TABLE + (RATE_TABLE if rate else []):
            ids[:len(streams)] = streams
            is_first[:len(streams)] = firsts
            got.append(_refusal(hip, lambda: push(slot, n)))
            want.append((code, text.format(**names)))
        # the rate entry takes the window at RATE, the plain one what the model makes of that: the same 12 kHz samples behind both
        if rate:
            first_halves[0, :], hops[0, :] = xr[:row], xr[row:]
        else:
            y, _ = ir.Resampler(CH, RATE).push([xr], [0], [1])
            first_halves[0, :], hops[0, :] = y[0][:2592], y[0][2592:]
        ids[0], is_first[0] = 0, 1
        push(0, 1)
        d.decode()
        d.fetch_async(0)
        records = d.fetch_wait(0)[0]
    return got, want, records, msg


@pytest.fixture(scope="module")
def runs(hip):
    return {entry: _run(hip, entry) for entry in ENTRIES}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals(runs, entry):
    got, want, _, _ = runs[entry]
    for g in got:
        print(entry, g)
    assert got == want


def test_a_good_push_behind_the_refusals(runs):
    """Each handle decodes the frame, and both the same records: a refused push left nothing half-done."""
    for entry, (_, _, records, msg) in runs.items():
        assert len(records) > 0, entry
        assert all(np.array_equal(unpack_message(r["message"]), msg) for r in records), entry
    assert runs["plain"][2].tobytes() == runs["rate"][2].tobytes()
