"""-m gpu: the wideband channeliser (msk144_set_wideband .. msk144_wideband_clip_count, include/msk144hip.h).

1. The int8 hops the device writes agree with the float64 model of the contract (msk144cudecoder_amd/wideband.py).
2. A decode after msk144_push_wideband is byte-identical to one fed the same hops through msk144_push_hops.
3. A synthetic 1.92 Msps cu8 scene: every planted message is decoded on its own channel and on no channel 12 kHz or more away.
"""
import os
import re

import numpy as np
import pytest

import pack77
from msk144cudecoder_amd import synth
import wideband_check as wc
from msk144cudecoder_amd import wideband as wb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE_CFG = dict(center=0.0, width=500.0, step=1.0, depth=6, nbadsync_threshold=1, read_mode=2)


def _offsets_64(D):
    lim = D * 12000 // 2 - 6000
    rng = np.random.default_rng(D)
    fixed = [0, -lim, lim, 5999, -5999, 12000, -12000, 1, -1, lim - 1, -(lim - 1)]
    rest = rng.integers(-lim, lim + 1, size=64 - len(fixed))      # off any grid
    return np.array(fixed + list(rest), dtype=np.int32)


def _pushes(raw, D):
    sizes = wb.push_sizes(5, D)
    out, pos = [], 0
    for n in sizes:
        out.append(raw[pos:pos + n])
        pos += n
    return out


def _hops_match_the_model(d, fmt, D, tally=None):
    """Configure d for (fmt, D) and check the int8 hops of five pushes against the float64 model: within one LSB, and by the
    near-tie rule."""
    rate = D * 12000
    offsets = _offsets_64(D)
    rng = np.random.default_rng(1000 + D + len(fmt))
    n_out = wb.FIRST_OUT + 4 * wb.HOP_OUT
    x = 0.03 * (rng.normal(size=n_out * D) + 1j * rng.normal(size=n_out * D))
    raw = wb.write_samples(x, fmt)
    ref = wc.Reference(rate, offsets)
    total = exact = 0
    d.set_wideband(rate, offsets, fmt)
    for i, part in enumerate(_pushes(raw, D)):
        first = i == 0
        d.push_wideband(i % 2, part, first=first)
        y, T, N = ref.push(wb.read_samples(part, fmt), first=first)
        q_ref, clip_ref = wb.quantise(y, ref.gain)
        got = np.stack([d.dump_wideband_hop(c) for c in range(len(offsets))])
        assert got.shape == q_ref.shape
        diff = np.abs(got.astype(np.int16) - q_ref.astype(np.int16))
        assert diff.max() <= 1, f"push {i}: |dq| up to {diff.max()}"
        total += diff.size
        exact += int(np.count_nonzero(diff == 0))
        clip = d.wideband_clip_count()
        assert clip == clip_ref, f"push {i}"
        rep = wc.assert_hops(got, y, T, N, ref.gain, clip, what=f"{fmt} {rate} push {i}")     # the near-tie rule (tests/wideband_check.py)
        if tally is not None:
            tally.add(rep)
    d.synchronize()
    assert exact / total >= 0.999, f"{total - exact} of {total} components differ by one LSB"


@pytest.mark.parametrize("D", [80, 160])
@pytest.mark.parametrize("fmt", wb.FORMATS)
def test_hops_match_the_model(hip, parity_report, fmt, D):
    tally = wc.Tally()
    with hip.HipDecoder(channels=64, **DECODE_CFG) as d:
        _hops_match_the_model(d, fmt, D, tally=tally)
    parity_report(f"wideband_model_{D * 12000}_{fmt}", tally.report())


def test_reconfigured_handle_matches_the_model(hip):
    """msk144_set_wideband again on a handle that has pushed: another D, format and set of offsets (the same count) replace the
    first configuration entirely."""
    with hip.HipDecoder(channels=64, **DECODE_CFG) as d:
        _hops_match_the_model(d, "cu8", 80)
        _hops_match_the_model(d, "cs16", 160)


def test_later_push_before_first_is_refused(hip):
    with hip.HipDecoder(channels=2, **DECODE_CFG) as d:
        d.set_wideband(960000, [0, 1000])
        with pytest.raises(hip.Msk144Error) as e:
            d.push_wideband(0, first=False)
        assert e.value.code == -4
        with pytest.raises(hip.Msk144Error) as e:
            d.set_wideband(960000, [0, 480000])          # beyond Fs/2 - 6000
        assert e.value.code == -1 and "outside" in str(e.value)
        with pytest.raises(hip.Msk144Error):
            d.set_wideband(960000, [0])                  # count != channels
    with hip.HipDecoder(channels=1, center=1500.0) as d:       # audio handle
        with pytest.raises(hip.Msk144Error):
            d.set_wideband(960000, [0])


def _scene(n_out, D, channel_offsets, ping_channels, rng, snr_db=10.0):
    planted = {}
    pings = []
    for k, c in enumerate(ping_channels):
        # a standard message that unpacks to text, so that the program prints it (--print-bits appends the payload)
        msg = pack77.pack_standard("CQ", "K%d%sZ" % (k % 10, "ABCDEFGHIJKLMNOPQRSTUVWXY"[k]), "FN42")
        start = 1500 + (k * 2311) % (n_out - 6 * 864 - 3000)
        p = synth.Ping(msg, start, 5, float(rng.uniform(-150, 150)), snr_db, float(rng.uniform(0, 6)))
        pings.append((int(channel_offsets[c]), p))
        planted[c] = bytes(np.asarray(msg, dtype=np.uint8))
    return wb.synth_wideband(n_out, D * 12000, pings, 0.05, rng, "cu8"), planted


def _decode_wideband(hip, d, parts):
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


def _decode_hops(hip, d, hops):
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


def test_decode_identity_with_push_hops(hip):
    D, C = 160, 64
    rng = np.random.default_rng(77)
    offsets = np.array([-900000 + 28000 * i for i in range(C)], dtype=np.int32)
    n_out = wb.FIRST_OUT + 2 * wb.HOP_OUT
    raw, planted = _scene(n_out, D, offsets, list(range(0, C, 5)), rng)
    parts = [raw[:2 * wb.FIRST_OUT * D], raw[2 * wb.FIRST_OUT * D:2 * (wb.FIRST_OUT + wb.HOP_OUT) * D], raw[2 * (wb.FIRST_OUT + wb.HOP_OUT) * D:]]
    with hip.HipDecoder(channels=C, **DECODE_CFG) as a:
        a.set_wideband(D * 12000, offsets, "cu8", gain=16.0)
        rec_a, hops = _decode_wideband(hip, a, parts)
    with hip.HipDecoder(channels=C, **DECODE_CFG) as b:
        rec_b = _decode_hops(hip, b, hops)
    assert sum(len(r) for r in rec_a) > 0
    for ra, rb in zip(rec_a, rec_b):
        assert ra.tobytes() == rb.tobytes()


SCENE_DECODE_ARGS = ["--search-width=500", "--search-step=1", "--scan-depth=6", "--nbadsync-threshold=1", "--print-bits"]


@pytest.fixture(scope="module")
def scene(hip):
    """1.92 Msps cu8, 1.94 s: 16 channels 100 kHz apart, each with a neighbour 12 kHz above it; +10 dB pings in 8 of the 16."""
    D = 160
    rng = np.random.default_rng(2024)
    base = [-800000 + 100000 * i for i in range(16)]
    offsets = np.array(base + [f + 12000 for f in base], dtype=np.int32)
    n_out = wb.FIRST_OUT + 7 * wb.HOP_OUT
    raw, planted = _scene(n_out, D, offsets, [0, 2, 3, 5, 8, 11, 13, 15], rng)
    parts = [raw[:2 * wb.FIRST_OUT * D]] + [raw[2 * (wb.FIRST_OUT + i * wb.HOP_OUT) * D:2 * (wb.FIRST_OUT + (i + 1) * wb.HOP_OUT) * D] for i in range(7)]
    with hip.HipDecoder(channels=len(offsets), **DECODE_CFG) as d:
        d.set_wideband(D * 12000, offsets, "cu8", gain=16.0)
        recs, hops = _decode_wideband(hip, d, parts)
        clipped = d.wideband_clip_count()
    return dict(D=D, offsets=offsets, raw=raw, planted=planted, recs=recs, hops=hops, clipped=clipped)


def _check_channels(got, planted, offsets):
    for c, msg in planted.items():
        assert msg in got.get(c, set()), f"message planted at {offsets[c]} Hz not decoded on ch={c}"
    for c, msgs in got.items():
        for m in msgs:
            owners = [pc for pc, pm in planted.items() if pm == m]
            assert owners, f"ch={c} decoded a message nobody planted"
            assert all(abs(int(offsets[c]) - int(offsets[pc])) < 12000 for pc in owners), f"message of ch={owners} also on ch={c}"


def test_scene_1p92_msps_decodes_on_own_channel_only(scene):
    assert scene["clipped"] == 0
    got = {}
    for r in np.concatenate(scene["recs"]):
        got.setdefault(int(r["channel"]), set()).add(bytes(np.unpackbits(r["message"])[:77]))
    _check_channels(got, scene["planted"], scene["offsets"])


def _program(args, data):
    import subprocess
    exe = os.path.join(ROOT, "msk144cudecoder_amd", "msk144hipdecoder")
    p = subprocess.run([exe] + args, input=data, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().strip().split("\n")
    assert lines[-1] == "Done"
    return [re.sub(r"date=\d{14}", "date=X", l) for l in lines[:-1]], p.stderr.decode()


def test_scene_through_the_program(scene):
    offsets = scene["offsets"]
    args = ["--wideband-rate=%d" % (scene["D"] * 12000), "--wideband-format=cu8", "--channel-offsets=" + ",".join(str(int(f)) for f in offsets),
            "--wideband-gain=16"] + SCENE_DECODE_ARGS
    lines, err = _program(args, scene["raw"].tobytes())
    assert "ch=31 offset %d Hz" % offsets[31] in err
    assert "wideband: 0 of %d channel I/Q components clipped" % (2 * len(offsets) * (wb.FIRST_OUT + 7 * wb.HOP_OUT)) in err
    got = {}
    for line in lines:
        m = re.match(r"^\*\*\*  ch=(\d+); .*bits='([01]{77})'", line)
        assert line.startswith("***  ch="), line
        if not m:
            continue                                  # --print-bits appends the payload only to a line whose text unpacks
        got.setdefault(int(m.group(1)), set()).add(bytes(int(b) for b in m.group(2)))
    _check_channels(got, scene["planted"], offsets)
    # the same channels as 32 interleaved 12 kHz IQ streams (the hops the channeliser wrote): the same stdout, line for line
    C = len(offsets)
    block = b"".join(h.tobytes() for h in scene["hops"])          # push after push, channel after channel
    ref, _ = _program(["--read-mode=2", "--interleaved=%d" % C] + SCENE_DECODE_ARGS, block)
    assert lines == ref
