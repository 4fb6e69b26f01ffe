"""-m gpu: the two-stage wideband bank above 6.144 Msps (include/msk144hip.h; csrc/bank.hip, then csrc/channelise.hip at Fs/32).

1. The int8 hops agree with the float64 two-stage model (msk144cudecoder_amd/wideband.py, TwoStage) by the two-stage near-tie rule
   (tests/wideband_bank_check.py) at 8, 10, 20 and 61.44 Msps, in cu8, cs8 and cs16, with random non-symmetric taps for both stages,
   channels in several bands, at both sides of band boundaries and at +-(Fs/2 - 6000); clip counts as the model's.  The dumped
   sub-band streams agree with the stage-1 model within its own bound, so that a stage-1 error shows as one.
2. The stream: a first push after later ones restarts both stages; one handle reconfigured bank -> 1.92 Msps -> bank.
3. At 10 Msps a decode after msk144_push_wideband is byte-identical to one fed the same hops through msk144_push_hops.
4. A 10 Msps cu8 scene with pings in six bands decodes on its planted channels, through the API and through msk144hipdecoder.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import pack77
import wideband_bank_check as bc
import wideband_check as wc
from msk144cudecoder_amd import synth
from msk144cudecoder_amd import wideband as wb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE_CFG = dict(center=0.0, width=500.0, step=1.0, depth=6, nbadsync_threshold=1, read_mode=2)
SCENE_RATE = 10000000


def _check_stream(d, rate, fmt, offsets, taps, bank_taps, gain, parts, firsts, what):
    ref = bc.BankReference(rate, offsets, taps=taps, K=bc.K2, gain=gain, bank_taps=bank_taps)
    d.set_wideband(rate, offsets, fmt, taps=taps, taps_per_phase=bc.K2, gain=gain, bank_taps=bank_taps)
    for i, (part, first) in enumerate(zip(parts, firsts)):
        d.push_wideband(i % 2, part, first=first)
        y, dl = ref.push(wb.read_samples(part, fmt), first=first)
        for j, b in enumerate(ref.model.bands):
            s = d.dump_wideband_band(b if b < 32 else b - 64)
            s_ref = ref.model.last_subbands[j]
            e1 = bc.stage1_delta(ref.T1, ref.K1)
            assert s.shape == s_ref.shape
            over = (np.abs(s.real - s_ref.real) > e1) | (np.abs(s.imag - s_ref.imag) > e1)
            assert not over.any(), f"{what} push {i}: band {b} off the stage-1 bound at {np.flatnonzero(over)[:5]}"
        got = np.stack([d.dump_wideband_hop(c) for c in range(len(offsets))])
        assert got.shape == y.shape + (2,)
        bc.assert_hops(got, y, dl, gain, d.wideband_clip_count(), what=f"{what} push {i}")


@pytest.mark.parametrize("rate, fmt, n_pushes", bc.CASES)
def test_hops_match_the_two_stage_model(hip, rate, fmt, n_pushes):
    offsets, taps, bank_taps, gain, raw = bc.case(rate, fmt, n_pushes)
    with hip.HipDecoder(channels=len(offsets), **DECODE_CFG) as d:
        _check_stream(d, rate, fmt, offsets, taps, bank_taps, gain, wc.split_pushes(raw, rate, n_pushes), [True] + [False] * (n_pushes - 1),
                      f"{fmt} {rate}")


@pytest.mark.parametrize("fmt", ["cs8", "cs16"])
def test_other_formats_at_61p44_msps(hip, fmt):
    rate = 61440000
    offsets, taps, bank_taps, gain, raw = bc.case(rate, fmt, 1, seed=1)
    with hip.HipDecoder(channels=len(offsets), **DECODE_CFG) as d:
        _check_stream(d, rate, fmt, offsets, taps, bank_taps, gain, wc.split_pushes(raw, rate, 1), [True], f"{fmt} {rate}")


def test_restart_and_reconfigure(hip):
    rate = 10000000
    offsets, taps, bank_taps, gain, raw = bc.case(rate, "cs16", 3, seed=2)
    parts = wc.split_pushes(raw, rate, 3)
    with hip.HipDecoder(channels=len(offsets), **DECODE_CFG) as d:
        # first, later, then the first push again and a later one: the second first push restarts both stages
        _check_stream(d, rate, "cs16", offsets, taps, bank_taps, gain, [parts[0], parts[1], parts[0], parts[1]], [True, False, True, False], "restart")
        # the same handle at a single-stage rate, then back at a bank rate with the default bank
        lo = 1920000
        o2 = wc.offsets_for(lo, len(offsets), np.random.default_rng(5))
        ref = wc.Reference(lo, o2)
        d.set_wideband(lo, o2, "cu8")
        raw2 = wc.raw_input(lo, 2, "cu8", np.random.default_rng(6), 0.03)
        for i, part in enumerate(wc.split_pushes(raw2, lo, 2)):
            d.push_wideband(i % 2, part, first=i == 0)
            y, T, N = ref.push(wb.read_samples(part, "cu8"), first=i == 0)
            got = np.stack([d.dump_wideband_hop(c) for c in range(len(o2))])
            wc.assert_hops(got, y, T, N, ref.gain, d.wideband_clip_count(), what=f"1.92 Msps push {i}")
        rate2 = 20000000
        offsets3, taps3, _, gain3, raw3 = bc.case(rate2, "cu8", 2, seed=3)
        _check_stream(d, rate2, "cu8", offsets3, taps3, None, gain3, wc.split_pushes(raw3, rate2, 2), [True, False], "default bank")


def test_bank_taps_rules(hip):
    with hip.HipDecoder(channels=1, **DECODE_CFG) as d:
        with pytest.raises(hip.Msk144Error):     # bank taps at a single-stage rate
            d.set_wideband(1920000, [0], bank_taps=np.ones(512) / 512)
        with pytest.raises(hip.Msk144Error):     # not 64 K1 taps
            d.set_wideband(10000000, [0], bank_taps=np.ones(500) / 500)
        for rate in (6156000, 6144125, 12500000, 61448000):
            with pytest.raises(hip.Msk144Error) as e:
                d.set_wideband(rate, [0], taps=np.ones(16))
            assert "2 <= D <= 512" in str(e.value)


# ---- decode ----

def _scene(n_out, rate, channel_offsets, ping_channels, rng, snr_db=10.0):
    planted, pings = {}, []
    for k, c in enumerate(ping_channels):
        msg = pack77.pack_standard("CQ", "K%d%sZ" % (k % 10, "ABCDEFGHIJKLMNOPQRSTUVWXY"[k]), "FN42")
        start = 1500 + (k * 2311) % (n_out - 6 * 864 - 3000)
        p = synth.Ping(msg, start, 5, float(rng.uniform(-150, 150)), snr_db, float(rng.uniform(0, 6)))
        pings.append((int(channel_offsets[c]), p))
        planted[c] = bytes(np.asarray(msg, dtype=np.uint8))
    return wb.synth_wideband(n_out, rate, pings, 0.05, rng, "cu8"), planted


def _decode_wideband(d, parts):
    recs, hops = [], []
    for i, part in enumerate(parts):
        s = i % 2
        d.push_wideband(s, part, first=(i == 0))
        hops.append(np.stack([d.dump_wideband_hop(c) for c in range(d.channels)]))
        d.decode()
        d.fetch_async(s)
        r, _ = d.fetch_wait(s)
        recs.append(np.sort(r, order=["channel", "item"]))
    return recs, hops


def _decode_hops(d, hops):
    recs = []
    for i, h in enumerate(hops):
        s = i % 2
        hh, first, streams, is_first = d.hop_slot(s)
        n = h.shape[0]
        if i == 0:
            first[:n] = h[:, :2592].reshape(n, -1)
            hh[:n] = h[:, 2592:].reshape(n, -1)
        else:
            hh[:n] = h.reshape(n, -1)
        streams[:n] = np.arange(n)
        is_first[:n] = 1 if i == 0 else 0
        d.push_hops(s, n)
        d.decode()
        d.fetch_async(s)
        r, _ = d.fetch_wait(s)
        recs.append(np.sort(r, order=["channel", "item"]))
    return recs


@pytest.fixture(scope="module")
def scene(hip):
    """10 Msps cu8, 4 pushes: six channels in six bands (two at a band's edge) and a neighbour 12 kHz above each (one of them across
    the band edge); +10 dB pings on the six."""
    rng = np.random.default_rng(10)
    step = SCENE_RATE // 64
    base = [-30 * step + 1000, -17 * step - step // 2 + 1, -3 * step + 20000, 5 * step - 7000, 18 * step + step // 2 - 1, 31 * step]
    offsets = np.array(base + [f + 12000 for f in base], dtype=np.int32)
    n_out = wb.FIRST_OUT + 3 * wb.HOP_OUT
    raw, planted = _scene(n_out, SCENE_RATE, offsets, list(range(6)), rng)
    parts = wc.split_pushes(raw, SCENE_RATE, 4)
    with hip.HipDecoder(channels=len(offsets), **DECODE_CFG) as d:
        d.set_wideband(SCENE_RATE, offsets, "cu8", gain=16.0)
        recs, hops = _decode_wideband(d, parts)
        clipped = d.wideband_clip_count()
    return dict(offsets=offsets, raw=raw, planted=planted, recs=recs, hops=hops, clipped=clipped)


def _check_channels(got, planted, offsets):
    assert len({int(wb.bank_band(SCENE_RATE, [offsets[c]])[0]) for c in planted}) >= 4
    for c, msg in planted.items():
        assert msg in got.get(c, set()), f"message planted at {offsets[c]} Hz not decoded on ch={c}"
    for c, msgs in got.items():
        for m in msgs:
            owners = [pc for pc, pm in planted.items() if pm == m]
            assert owners, f"ch={c} decoded a message nobody planted"
            assert all(abs(int(offsets[c]) - int(offsets[pc])) < 12000 for pc in owners), f"message of ch={owners} also on ch={c}"


def test_decode_identity_with_push_hops(hip, scene):
    with hip.HipDecoder(channels=len(scene["offsets"]), **DECODE_CFG) as b:
        rec_b = _decode_hops(b, scene["hops"])
    assert sum(len(r) for r in scene["recs"]) > 0
    for ra, rb in zip(scene["recs"], rec_b):
        assert ra.tobytes() == rb.tobytes()


def test_scene_10_msps_decodes_on_own_channel_only(scene):
    assert scene["clipped"] == 0
    got = {}
    for r in np.concatenate(scene["recs"]):
        got.setdefault(int(r["channel"]), set()).add(bytes(np.unpackbits(r["message"])[:77]))
    _check_channels(got, scene["planted"], scene["offsets"])


def test_scene_through_the_program(scene):
    offsets = scene["offsets"]
    exe = os.path.join(ROOT, "msk144cudecoder_amd", "msk144hipdecoder")
    args = ["--wideband-rate=%d" % SCENE_RATE, "--wideband-format=cu8", "--channel-offsets=" + ",".join(str(int(f)) for f in offsets),
            "--wideband-gain=16", "--search-width=500", "--search-step=1", "--scan-depth=6", "--nbadsync-threshold=1", "--print-bits"]
    p = subprocess.run([exe] + args, input=scene["raw"].tobytes(), capture_output=True, timeout=300)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    n_bands = len({int(k) % 64 for k in wb.bank_band(SCENE_RATE, offsets)})
    assert f"64-band analysis bank, {n_bands} bands occupied, sub-band rate 312500 sps" in err
    assert "stage 2: resampling 625/24, filter 16 x 625 taps" in err
    got = {}
    for line in p.stdout.decode().strip().split("\n")[:-1]:
        m = re.match(r"^\*\*\*  ch=(\d+); .*bits='([01]{77})'", line)
        if m:
            got.setdefault(int(m.group(1)), set()).add(bytes(int(b) for b in m.group(2)))
    _check_channels(got, scene["planted"], offsets)
