"""-m gpu: the gate of the wideband contract (include/msk144hip.h, csrc/gate.hip) - the plan kernel against wideband.Gate with no
tolerance, and the gated decode against an ungated handle byte for byte.

1. The plan kernel.  1, 63, 64, 65, 255, 256, 257 and 1000 channels (the wave and chunk edges of the plan kernel) at 240 ksps with
   overlapping offsets, white noise with three tone bursts, ratio_q4 = 21: on noise alone about half of the channel hops have an up
   block (asserted: between a quarter and three quarters).  Six pushes with hold 0 / 1 / 3 and min_up 1 / 3: wideband_gate() equals
   wideband.Gate fed the device's own wideband_pings() records; with max_channels below the qualifying count the count is
   max_channels, the total the model's and the list the model's first max_channels.
2. Decode identity.  Two handles on the 16-channel, 192 ksps, 8-push scene of wideband_gate_check.py: the gated records, mapped
   through the list, are the ungated handle's records of the listed channels; segment powers, hops, levels, clip count and ping
   records of every channel are the same bytes.  The scene gives records, windows that are not decoded, and a decoded window
   without a record.
3. An all-zero push lists nothing: the decode launches nothing and the fetch gives 0 records; the next push decodes.
4. always channels are decoded on every push, with the detector on and off.
5. set_wideband_gate(None): the records of a handle that never had the gate, and MSK144_ESTATE from the read entry; parameters out
   of range are refused and change nothing.
6. msk144hipdecoder --wideband-pings --wideband-gate through a pipe: the ungated run's lines, and the summary's counts are the
   model's.
"""
import re

import numpy as np
import pytest

import wideband_check as wc
import wideband_gate_check as gc
import wideband_gpu as wg
import wideband_options as wo
from msk144cudecoder_amd import wideband as wb
from wideband_options import EINVAL, code_of

pytestmark = pytest.mark.gpu

CFG = dict(center=0.0, width=20.0, step=2.0, depth=3, nbadsync_threshold=1, read_mode=2)
PROGRAM_ARGS = ["--search-width=20", "--search-step=2", "--scan-depth=3", "--nbadsync-threshold=1"]
RATIO_Q4 = 21           # 1.3125 x the reference: on white noise alone about half of the hops have an up block
NOISE_RATE, NOISE_PUSHES = 240000, 6
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)
SCENE_C, SCENE_HOPS = 16, 9


@pytest.fixture(scope="module")
def handles(hip):
    """One handle per channel count (two of the scene's), made on first use and kept for the module."""
    with wo.handle_cache(lambda key: hip.HipDecoder(channels=key[0], **CFG)) as get:
        yield lambda C, k=0: get((C, k))


def noise_offsets(C):
    """C different offsets 224 Hz apart (fewer channels: spread over the same span), so that neighbours overlap."""
    return (-111888 + 224 * (np.arange(C) * (999 // max(C - 1, 1)))).astype(np.int32)


_noise = {}


def noise_parts():
    """cs16 pushes of white noise at about 10 LSB per component behind gain 100, with three tone bursts of about 40 LSB."""
    if not _noise:
        rng = np.random.default_rng(17)
        N = (wb.FIRST_OUT + (NOISE_PUSHES - 1) * wb.HOP_OUT) * NOISE_RATE // 12000
        unit = 128.0 * 100.0
        sigma = 10.0 / (unit * float(np.linalg.norm(wb.default_taps_for_rate(NOISE_RATE))))
        x = sigma * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
        n = np.arange(N, dtype=np.float64)
        for f, m0, m1 in ((-111888, 3000, 4500), (0, 7000, 9800), (60032, 12000, 12400)):
            sl = slice(m0 * 20, m1 * 20)
            x[sl] += (40.0 / unit) * np.exp(2j * np.pi * f * n[sl] / NOISE_RATE)
        _noise["parts"] = wc.split_pushes(wb.write_samples(x, "cs16"), NOISE_RATE, NOISE_PUSHES)
    return _noise["parts"]


# ---- 1. the plan kernel against the model ----

@pytest.mark.parametrize("C", COUNTS)
def test_the_plan_kernel_equals_the_model(handles, C):
    d = handles(C)
    d.set_wideband(NOISE_RATE, noise_offsets(C), "cs16", gain=100.0)
    d.set_wideband_pings(ratio_q4=RATIO_Q4)
    first_records, largest = None, 0
    for hold, min_up in ((0, 1), (1, 1), (3, 1), (0, 3), (1, 3), (3, 3)):
        d.set_wideband_gate(hold, min_up)
        model, records = wb.Gate(C, hold, min_up), []
        for i, part in enumerate(noise_parts()):
            d.push_wideband(i % 2, part, first=i == 0)
            records.append(d.wideband_pings())
            got = d.wideband_gate()
            gc.assert_list(got, model.push(records[-1], i == 0), f"{C} channels hold {hold} min_up {min_up} push {i}")
            largest = max(largest, got[1])
        if first_records is None:
            first_records = records
        assert all(a.tobytes() == b.tobytes() for a, b in zip(records, first_records))           # the gate does not move the detector
    a = gc.hop_activity(first_records, 1)
    print(f"{C} channels: {int(a.sum())} of {a.size} hops active at min_up 1, {int(gc.hop_activity(first_records, 3).sum())} at min_up 3, largest total {largest}")
    if C >= 63:
        assert 0.25 <= a.mean() <= 0.75, f"{a.mean():.3f} of the hops are active"
        assert gc.hop_activity(first_records, 3).any()
    # a budget below the qualifying count: the first max_channels in ascending order, the total unchanged
    if C >= 63:
        g = wb.Gate(C, 1, 1)
        free = [g.push(r, i == 0) for i, r in enumerate(first_records)]
        cap = min(t for _, t in free) // 2
        assert cap >= 1
        d.set_wideband_gate(1, 1, cap)
        for i, part in enumerate(noise_parts()):
            d.push_wideband(i % 2, part, first=i == 0)
            lst, total = d.wideband_gate()
            assert len(lst) == cap and total == free[i][1] and list(lst) == list(free[i][0][:cap]), f"{C} channels max_channels {cap} push {i}"
    d.synchronize()
    d.set_wideband_gate(None)
    d.set_wideband_pings(None)


# ---- 2. decode identity ----

def scene_setup(d, gate=True, pings=True, **kw):
    d.set_wideband(gc.SCENE_RATE, gc.scene_offsets(SCENE_C), "cs16", gain=gc.SCENE_GAIN)
    d.set_wideband_pings() if pings else d.set_wideband_pings(None)
    if gate:
        d.set_wideband_gate(always=kw.pop("always", gc.SCENE_ALWAYS), **kw)
    else:
        d.set_wideband_gate(None)


def decode_fetch(d, s):
    d.decode()
    d.fetch_async(s)
    return d.fetch_wait(s)


def mapped(records, lst):
    """Gated records with the list position replaced by the channel."""
    r = records.copy()
    r["channel"] = np.asarray(lst, dtype=np.int32)[records["channel"]] if len(records) else records["channel"]
    return r


def of_channels(records, lst):
    return records[np.isin(records["channel"], lst)]


def test_the_gated_decode_is_the_ungated_one_of_the_listed_channels(handles):
    a, b = handles(SCENE_C, 0), handles(SCENE_C, 1)
    scene_setup(a)
    scene_setup(b, gate=False)
    model = wb.Gate(SCENE_C, always=gc.SCENE_ALWAYS)
    n_records = n_skipped = n_empty = 0
    for i, part in enumerate(gc.scene_parts(SCENE_C, SCENE_HOPS)):
        s = i % 2
        for d in (a, b):
            d.push_wideband(s, part, first=i == 0)
        rec = a.wideband_pings()
        assert rec.tobytes() == b.wideband_pings().tobytes(), f"push {i}: ping records"
        assert wg.dump_hops(a, range(SCENE_C)).tobytes() == wg.dump_hops(b, range(SCENE_C)).tobytes(), f"push {i}: hops"
        assert a.wideband_levels().tobytes() == b.wideband_levels().tobytes() and a.wideband_clip_count() == b.wideband_clip_count(), f"push {i}: levels"
        lst, total = a.wideband_gate()
        gc.assert_list((lst, total), model.push(rec, i == 0), f"push {i}")
        (ra, sa), (rb, sb) = decode_fetch(a, s), decode_fetch(b, s)
        assert sa.tobytes() == sb.tobytes() and sa.shape == (SCENE_C, 8), f"push {i}: segment powers"
        assert np.all(ra["channel"] < len(lst)), f"push {i}: a record past the list"
        assert mapped(ra, lst).tobytes() == of_channels(rb, lst).tobytes(), f"push {i}: the records of channels {list(lst)}"
        # no ungated record of a ping channel is lost
        assert set(rb["channel"][np.isin(rb["channel"], gc.SCENE_PING_CHANNELS)]) <= set(lst), f"push {i}: a ping channel with records is not listed"
        n_records += len(ra)
        n_skipped += SCENE_C - len(lst)
        n_empty += len(set(lst) - set(mapped(ra, lst)["channel"]))
        assert a.copy_count() >= 0
    print(f"{n_records} gated records, {n_skipped} channel windows not decoded, {n_empty} decoded windows without a record")
    assert n_records > 0 and n_skipped > 0 and n_empty > 0


# ---- 3. nothing listed ----

def test_a_push_that_lists_nothing_decodes_nothing_and_the_next_one_decodes(handles):
    d = handles(SCENE_C, 0)
    scene_setup(d, always=())
    parts = gc.scene_parts(SCENE_C, SCENE_HOPS)
    d.push_wideband(0, np.zeros_like(parts[0]), first=True)
    lst, total = d.wideband_gate()
    assert len(lst) == 0 and total == 0
    records, seg = decode_fetch(d, 0)
    assert len(records) == 0 and seg.shape == (SCENE_C, 8)
    assert d.result_count() == 0 and d.copy_count() == 0
    # hop 2 of the scene carries the first ping; behind silence every block of it is up
    d.push_wideband(1, parts[1], first=False)
    lst, total = d.wideband_gate()
    assert gc.SCENE_PING_CHANNELS[0] in lst and total == len(lst) > 0
    records, _ = decode_fetch(d, 1)
    assert len(records) > 0 and gc.SCENE_PING_CHANNELS[0] in set(mapped(records, lst)["channel"])


# ---- 4. always channels ----

@pytest.mark.parametrize("pings", [True, False])
def test_always_channels_are_decoded_on_every_push(handles, pings):
    a, b = handles(SCENE_C, 0), handles(SCENE_C, 1)
    always = (0, 5, 15)
    scene_setup(a, pings=pings, always=always)
    scene_setup(b, gate=False, pings=pings)
    for i, part in enumerate(gc.scene_parts(SCENE_C, SCENE_HOPS)[:4]):
        s = i % 2
        a.push_wideband(s, part, first=i == 0)
        b.push_wideband(s, part, first=i == 0)
        lst, total = a.wideband_gate()
        assert set(always) <= set(lst) and total == len(lst)
        if not pings:
            assert list(lst) == list(always)
        (ra, _), (rb, _) = decode_fetch(a, s), decode_fetch(b, s)
        assert mapped(ra, lst).tobytes() == of_channels(rb, lst).tobytes(), f"push {i}"


# ---- 5. switching off, refusals ----

def test_switching_off_and_refusals(hip, handles):
    a, b = handles(SCENE_C, 0), handles(SCENE_C, 1)
    scene_setup(a)
    scene_setup(b, gate=False)
    parts = gc.scene_parts(SCENE_C, SCENE_HOPS)
    for i, part in enumerate(parts[:3]):
        for d in (a, b):
            d.push_wideband(i % 2, part, first=i == 0)
            decode_fetch(d, i % 2)
    # out of range: refused, and the next push is still made with what was set
    for bad in (dict(hold=-1), dict(hold=17), dict(min_up=0), dict(min_up=28), dict(max_channels=-1), dict(max_channels=SCENE_C + 1)):
        assert code_of(hip, lambda: a.set_wideband_gate(**bad)) == EINVAL, bad
    with pytest.raises(ValueError):
        a.set_wideband_gate(always=(SCENE_C,))
    before = a.wideband_gate()
    a.push_wideband(1, parts[3], first=False)
    b.push_wideband(1, parts[3], first=False)
    lst, total = a.wideband_gate()
    assert set(gc.SCENE_ALWAYS) <= set(lst) and len(lst) < SCENE_C and len(before[0]) < SCENE_C
    decode_fetch(a, 1), decode_fetch(b, 1)
    a.set_wideband_gate(None)
    wo.unreadable(hip, [a.wideband_gate])
    for i, part in enumerate(parts[4:6]):
        for d in (a, b):
            d.push_wideband(i % 2, part, first=False)
        wo.unreadable(hip, [a.wideband_gate])
        (ra, sa), (rb, sb) = decode_fetch(a, i % 2), decode_fetch(b, i % 2)
        assert ra.tobytes() == rb.tobytes() and sa.tobytes() == sb.tobytes(), f"push {4 + i} after the gate was switched off"
    # set again: the read entry answers ESTATE until the next push made with it
    a.set_wideband_gate()
    wo.unreadable(hip, [a.wideband_gate])
    wo.refuses_outside_wideband_mode(hip, [hip.HipDecoder.set_wideband_gate, hip.HipDecoder.wideband_gate])


# ---- 6. the program ----

def test_the_program_prints_the_ungated_lines_and_counts_like_the_model(handles, tmp_path):
    parts = gc.scene_parts(SCENE_C, SCENE_HOPS)
    data = np.concatenate(parts).tobytes()
    args = PROGRAM_ARGS + [f"--wideband-rate={gc.SCENE_RATE}", "--wideband-format=cs16", "--channel-offsets=" + ",".join(str(int(f)) for f in gc.scene_offsets(SCENE_C)),
                           f"--wideband-pings={tmp_path}/pings.txt"]
    plain, _ = wg.run_program(args, data)
    gated, err = wg.run_program(args + ["--wideband-gate"], data)
    # the model, fed the device's own ping records, and the ungated records per push
    d = handles(SCENE_C, 1)
    scene_setup(d, gate=False)
    model, w = wb.Gate(SCENE_C), 0
    for i, part in enumerate(parts):
        d.push_wideband(i % 2, part, first=i == 0)
        lst, _ = model.push(d.wideband_pings(), i == 0)
        records, _ = decode_fetch(d, i % 2)
        assert set(records["channel"]) <= set(lst), f"push {i}: the ungated decode has records on a channel the gate does not list"
        w += len(lst)
    t = SCENE_C * len(parts)
    assert gated == plain and len(plain) > 0
    m = re.search(r"msk144hipdecoder: wideband gate: (\d+) of (\d+) channel windows decoded \(([\d.]+) %\), hold 1, min up 1, at most 16 per push, 0 dropped, busiest push (\d+) channels", err)
    assert m, err[-1500:]
    assert (int(m.group(1)), int(m.group(2))) == (w, t) and 0 < w < t
    assert {int(c) for c in re.findall(r"^\*\*\*  ch=(\d+);", "\n".join(gated), flags=re.M)} <= set(gc.SCENE_PING_CHANNELS)
