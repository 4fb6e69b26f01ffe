"""-m gpu: the decode behind the wideband channeliser, over one synthetic cu8 scene per kind of rate - 1.92 Msps (integer),
2.048 Msps (rational, 512/3) and 10 Msps (the two-stage bank).

1. A decode after msk144_push_wideband is byte-identical to one fed the same hops through msk144_push_hops.
2. Every planted message is decoded on its own channel and on no channel 12 kHz or more away, through the API and through
   msk144hipdecoder --wideband-rate, whose summary names the configuration.
"""
import numpy as np
import pytest

import wideband_check as wc
import wideband_gpu as wg
from msk144cudecoder_amd import wideband as wb

pytestmark = pytest.mark.gpu
GAIN = 16.0


def _with_neighbours(base):
    """Every channel of base, then a neighbour 12 kHz above each."""
    return np.array(base + [f + 12000 for f in base], dtype=np.int32)


def _clip_line(offsets, pushes):
    return "wideband: 0 of %d channel I/Q components clipped" % (2 * len(offsets) * (wb.FIRST_OUT + (pushes - 1) * wb.HOP_OUT))


# A row: the scene (rate, seed, offsets, channels with a +10 dB ping, pushes), what the program's stderr must hold, and
# - identity: (seed, 64 offsets) of the three-push scene, a ping on every fifth channel, that the identity test runs instead of the
#   row's own scene; None: it uses the row's scene;
# - min_bands: the planted channels must lie in at least this many bands of the two-stage bank; 0: a single-stage rate;
# - as_interleaved: the program is run once more on the dumped hops as --interleaved streams and must print the same lines.
_O1920 = _with_neighbours([-800000 + 100000 * i for i in range(16)])
_O2048 = _with_neighbours([-850000 + 110000 * i for i in range(16)])
_STEP = 10000000 // 64
_O10M = _with_neighbours([-30 * _STEP + 1000, -17 * _STEP - _STEP // 2 + 1, -3 * _STEP + 20000, 5 * _STEP - 7000, 18 * _STEP + _STEP // 2 - 1, 31 * _STEP])
SCENES = [
    # 1.92 Msps, 1.94 s: 16 channels 100 kHz apart, each with a neighbour 12 kHz above it; pings in 8 of the 16
    dict(rate=1920000, seed=2024, offsets=_O1920, pings=[0, 2, 3, 5, 8, 11, 13, 15], pushes=8, min_bands=0, as_interleaved=True,
         identity=(77, np.array([-900000 + 28000 * i for i in range(64)], dtype=np.int32)),
         stderr=["ch=31 offset %d Hz" % _O1920[31], _clip_line(_O1920, 8)]),
    # 2.048 Msps (512/3), 1.94 s: the same layout 110 kHz apart
    dict(rate=2048000, seed=2048, offsets=_O2048, pings=[0, 2, 3, 5, 8, 11, 13, 15], pushes=8, min_bands=0, as_interleaved=True,
         identity=(78, np.array([-960000 + 30000 * i for i in range(64)], dtype=np.int32)),
         stderr=["resampling 512/3, filter 16 x 512 taps", _clip_line(_O2048, 8)]),
    # 10 Msps, 4 pushes: six channels in six bands (two at a band's edge) and a neighbour 12 kHz above each (one of them across the
    # band edge); pings on the six
    dict(rate=10000000, seed=10, offsets=_O10M, pings=list(range(6)), pushes=4, min_bands=4, as_interleaved=False, identity=None,
         stderr=["64-band analysis bank, %d bands occupied, sub-band rate 312500 sps" % len({int(k) % 64 for k in wb.bank_band(10000000, _O10M)}),
                 "stage 2: resampling 625/24, filter 16 x 625 taps"]),
]


def _planted_and_decoded(hip, rate, offsets, pings, pushes, rng):
    raw, planted = wg.plant_scene(wb.FIRST_OUT + (pushes - 1) * wb.HOP_OUT, rate, offsets, pings, rng)
    with hip.HipDecoder(channels=len(offsets), **wg.DECODE_CFG) as d:
        d.set_wideband(rate, offsets, "cu8", gain=GAIN)
        recs, hops = wg.decode_wideband(d, wc.split_pushes(raw, rate, pushes))
        clipped = d.wideband_clip_count()
    return dict(raw=raw, planted=planted, recs=recs, hops=hops, clipped=clipped)


@pytest.fixture(scope="module", params=SCENES, ids=[str(s["rate"]) for s in SCENES])
def scene(hip, request):
    s = request.param
    return dict(s, **_planted_and_decoded(hip, s["rate"], s["offsets"], s["pings"], s["pushes"], np.random.default_rng(s["seed"])))


def _check_channels(got, scene):
    offsets = scene["offsets"]
    if scene["min_bands"]:
        assert len({int(wb.bank_band(scene["rate"], [offsets[c]])[0]) for c in scene["planted"]}) >= scene["min_bands"]
    wg.check_channels(got, scene["planted"], offsets)


def test_decode_identity_with_push_hops(hip, scene):
    a = scene
    if scene["identity"]:
        seed, offsets = scene["identity"]
        a = _planted_and_decoded(hip, scene["rate"], offsets, list(range(0, 64, 5)), 3, np.random.default_rng(seed))
    with hip.HipDecoder(channels=a["hops"][0].shape[0], **wg.DECODE_CFG) as b:
        rec_b = wg.decode_hops(b, a["hops"])
    assert sum(len(r) for r in a["recs"]) > 0
    for ra, rb in zip(a["recs"], rec_b):
        assert ra.tobytes() == rb.tobytes()


def test_scene_decodes_on_own_channel_only(scene):
    assert scene["clipped"] == 0
    _check_channels(wg.messages_by_channel(scene["recs"]), scene)


def test_scene_through_the_program(scene):
    offsets = scene["offsets"]
    args = ["--wideband-rate=%d" % scene["rate"], "--wideband-format=cu8", "--channel-offsets=" + ",".join(str(int(f)) for f in offsets),
            "--wideband-gain=16"] + wg.SCENE_DECODE_ARGS
    lines, err = wg.run_program(args, scene["raw"].tobytes())
    for fragment in scene["stderr"]:
        assert fragment in err
    _check_channels(wg.messages_by_channel_in_lines(lines), scene)
    if scene["as_interleaved"]:
        # the same channels as interleaved 12 kHz IQ streams (the hops the channeliser wrote): the same stdout, line for line
        block = b"".join(h.tobytes() for h in scene["hops"])          # push after push, channel after channel
        ref, _ = wg.run_program(["--read-mode=2", "--interleaved=%d" % len(offsets)] + wg.SCENE_DECODE_ARGS, block)
        assert lines == ref
