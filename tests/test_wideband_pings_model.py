"""CPU: the ping detector of the wideband contract (include/msk144hip.h) - wideband.Pings and wideband.PingEvents, the Python model the
device is held to byte for byte - against values worked out by hand, and the C++ rule and event tracker of csrc/wideband.h (what the
kernel and the program run, through libmsk144host.so) against that model.

- Hand-made int8 hops: an all-zero channel, a channel of all -128 (the largest E, no overflow), one louder block at either end of
  the push, two equal maxima, and an E exactly on R x ratio_q4 / 16 and one above it.
- Memory: a quiet push and then a push that is 22/27 ping keeps the ping visible; with memory = 0 it is lost; a changed scale
  restarts the history.
- Events: a run across a push boundary is one event, a run of min_blocks - 1 blocks is dropped, close() flushes an open run, the
  peak is the run's largest E at its lowest block with the R of that push.
- 200 random record sequences: the C++ rule equals the model record for record, the C++ tracker event for event, and the line of
  the log is the model's.
- The planted scene (wideband_pings_check.py) through the float64 channeliser model: every block inside a +10 dB ping is up, no
  block away from one, none on a noise channel, and the ping across a push boundary is one event.
"""
import numpy as np
import pytest

import wideband_pings_check as pc
from msk144cudecoder_amd import wideband as wb

FULL = 96 * 2 * 128 * 128      # E of a block of all -128


def constant(nb, i, q_=0, channels=1):
    """int8 hops [channels][96 nb][2] of constant I = i, Q = q_."""
    h = np.zeros((channels, 96 * nb, 2), dtype=np.int8)
    h[:, :, 0], h[:, :, 1] = i, q_
    return h


def test_the_record_is_32_bytes_with_the_fields_of_the_header():
    assert wb.PING_DTYPE.itemsize == 32
    assert wb.PING_DTYPE.names == ("up_mask", "blocks", "history", "quiet", "reference", "peak", "peak_block")
    assert [wb.PING_DTYPE.fields[n][1] for n in wb.PING_DTYPE.names] == [0, 8, 12, 16, 20, 24, 28]
    assert wb.PINGS_DEFAULTS == dict(ratio_q4=32, memory=8, min_ref=96)


@pytest.mark.parametrize("nb", [27, 54])
def test_block_energies_and_the_extremes(nb):
    h = np.concatenate([constant(nb, 0), constant(nb, -128, -128), constant(nb, 3, -4)])
    E = wb.ping_blocks(h)
    assert E.shape == (3, nb) and E.dtype == np.int64
    assert not E[0].any() and np.all(E[1] == FULL) and FULL == 3145728 < 2 ** 22 and np.all(E[2] == 96 * 25)
    r = wb.Pings(3).push(h, 100.0)
    assert list(r["blocks"]) == [nb] * 3 and list(r["history"]) == [0] * 3
    # silence: E = 0, the reference held at min_ref, nothing up, the peak at block 0
    assert (r["quiet"][0], r["reference"][0], r["up_mask"][0], r["peak"][0], r["peak_block"][0]) == (0, 96, 0, 0, 0)
    # full scale everywhere: q = R = E, nothing up, no overflow in E x 16
    assert (r["quiet"][1], r["reference"][1], r["up_mask"][1], r["peak"][1], r["peak_block"][1]) == (FULL, FULL, 0, FULL, 0)
    assert (r["quiet"][2], r["reference"][2], r["up_mask"][2], r["peak"][2]) == (2400, 2400, 0, 2400)


@pytest.mark.parametrize("nb", [27, 54])
def test_one_louder_block_and_two_equal_maxima(nb):
    for loud in ([0], [nb - 1], [5, nb - 2], [nb - 2, 5]):
        h = constant(nb, 10, 10)                        # E = 96 x 200 = 19200
        for b in loud:
            h[0, 96 * b:96 * b + 96] = (30, 30)         # 96 x 1800 = 172800 = 9 x
        r = wb.Pings(1).push(h, 100.0)[0]
        assert r["quiet"] == r["reference"] == 19200 and r["peak"] == 172800
        assert r["peak_block"] == min(loud) and r["up_mask"] == sum(1 << b for b in loud)
    assert wb.ping_blocks(constant(nb, 10, 10))[0, nb // 4] == 19200 and pc.host().msk144host_wideband_ping_rank(nb) == nb // 4 == {27: 6, 54: 13}[nb]


def test_an_energy_on_the_threshold_is_not_up_and_one_above_it_is():
    # R = 96 x 4 = 384 (I = 2), ratio 2.0: the threshold is E = 768.  I^2 + Q^2 = 8 in every sample gives exactly 768; one sample
    # with 9 instead gives 769
    h = constant(27, 2)
    h[0, 96:192] = (2, 2)
    h[0, 192:288] = (2, 2)
    h[0, 200] = (3, 0)
    det = wb.Pings(1)
    r = det.push(h, 100.0)[0]
    assert r["reference"] == 384 and det.energies[0, 1] == 768 and det.energies[0, 2] == 769
    assert r["up_mask"] == 1 << 2 and r["peak"] == 769 and r["peak_block"] == 2
    assert pc.host().msk144host_wideband_ping_up(768, 384, 32) == 0 and pc.host().msk144host_wideband_ping_up(769, 384, 32) == 1
    # 64-bit arithmetic: the largest E against the largest ratio
    assert pc.host().msk144host_wideband_ping_up(FULL, 1 << 22, 65535) == 0 and pc.host().msk144host_wideband_ping_up(FULL, 96, 65535) == 1
    # under-driven: the reference is held at min_ref, so a block of mean power 1.5 LSB^2 stays down and one above 2 goes up
    h = constant(27, 0)
    h[0, 0:96:2] = (1, 1)                               # E = 96
    h[0, 96:192] = (1, 1)                               # E = 192 = 2 x min_ref: not up
    h[0, 192:288] = (1, 1)
    h[0, 192] = (2, 1)                                  # E = 195
    r = wb.Pings(1).push(h, 100.0)[0]
    assert (r["quiet"], r["reference"], r["up_mask"]) == (0, 96, 1 << 2)


def ping_push(blocks_up=22):
    h = constant(27, 10, 10)
    h[0, :96 * blocks_up] = (30, 30)
    return h


def test_memory_keeps_a_ping_that_fills_most_of_a_push_visible():
    det = wb.Pings(1)
    assert det.push(constant(54, 10, 10), 100.0)[0]["up_mask"] == 0
    r = det.push(ping_push(), 100.0)[0]
    # the push's own quartile is a ping block; the quiet level of the push before it is the reference
    assert (r["history"], r["quiet"], r["reference"], r["up_mask"]) == (1, 172800, 19200, (1 << 22) - 1)
    r = det.push(constant(27, 10, 10), 100.0)[0]
    assert (r["history"], r["quiet"], r["reference"], r["up_mask"]) == (2, 19200, 19200, 0)
    # without memory the ping is lost
    det = wb.Pings(1, memory=0)
    det.push(constant(54, 10, 10), 100.0)
    r = det.push(ping_push(), 100.0)[0]
    assert (r["history"], r["reference"], r["up_mask"]) == (0, 172800, 0)


def test_memory_reaches_back_exactly_memory_pushes():
    det = wb.Pings(1, memory=2)
    det.push(constant(54, 5, 5), 100.0)                  # q = 4800
    for k in range(2):
        r = det.push(constant(27, 10, 10), 100.0)[0]     # q = 19200
        assert (r["history"], r["reference"]) == (k + 1, 4800)
    r = det.push(constant(27, 10, 10), 100.0)[0]
    assert (r["history"], r["reference"]) == (2, 19200)  # the quiet first push is three pushes back
    # 16 is the most
    det = wb.Pings(1, memory=16)
    det.push(constant(54, 5, 5), 100.0)
    for k in range(16):
        r = det.push(constant(27, 10, 10), 100.0)[0]
        assert (r["history"], r["reference"]) == (k + 1, 4800)
    r = det.push(constant(27, 10, 10), 100.0)[0]
    assert (r["history"], r["reference"]) == (16, 19200)


def test_a_changed_scale_restarts_the_history():
    det = wb.Pings(2)
    det.push(constant(54, 10, 10, channels=2), [100.0, 100.0])
    det.push(constant(27, 10, 10, channels=2), [100.0, 100.0])
    h = np.concatenate([ping_push(), ping_push()])
    r = det.push(h, np.array([100.0, 50.0], dtype=np.float32))
    assert list(r["history"]) == [2, 0]
    assert list(r["reference"]) == [19200, 172800] and list(r["up_mask"]) == [(1 << 22) - 1, 0]
    r = det.push(h, np.array([100.0, 50.0], dtype=np.float32))
    assert list(r["history"]) == [3, 1]
    det.reset()                                          # a first push, or msk144_set_wideband_pings
    assert list(det.push(h, np.array([100.0, 50.0], dtype=np.float32))["history"]) == [0, 0]


def test_parameters_out_of_range_are_refused_by_the_model_and_by_the_library_rule():
    for bad in (dict(ratio_q4=15), dict(ratio_q4=65536), dict(memory=-1), dict(memory=17), dict(min_ref=0), dict(min_ref=(1 << 22) + 1)):
        with pytest.raises(ValueError):
            wb.Pings(1, **bad)
        assert pc.host_check(**bad) != "", bad
    for good in (dict(), dict(ratio_q4=16), dict(ratio_q4=65535), dict(memory=0), dict(memory=16), dict(min_ref=1), dict(min_ref=1 << 22)):
        wb.Pings(1, **good)
        assert pc.host_check(**good) == "", good
    with pytest.raises(TypeError):
        wb.Pings(1, ratio=2)
    with pytest.raises(ValueError):
        wb.PingEvents(0)
    with pytest.raises(ValueError):
        wb.PingEvents(65)


# ---- events ----

def records_of(masks, nb=27, reference=100):
    r = np.zeros(len(masks), dtype=wb.PING_DTYPE)
    r["up_mask"], r["blocks"], r["reference"] = masks, nb, reference
    return r


def energies_of(masks, nb=27, up=1000, down=10):
    return np.array([[up + b if (m >> b) & 1 else down for b in range(nb)] for m in masks], dtype=np.int64)


@pytest.mark.parametrize("tracker", [lambda c, m: wb.PingEvents(m), pc.HostTracker], ids=["python", "c++"])
def test_events(tracker):
    t = tracker(2, 3)
    # push 0 (54 blocks): ch 0 a run of 3 inside and a run of 2 (dropped); ch 1 a run that reaches the last block
    m0 = [(0b111 << 4) | (0b11 << 20), 0b11 << 52]
    assert t.push(records_of(m0, 54, 100), energies_of(m0, 54)) == [dict(channel=0, start=4, blocks=3, peak=1006, reference=100)]
    # push 1: ch 1 goes on for 1 block - one event of 3 across the boundary; its largest E lies in push 0, whose R it carries
    m1 = [0, 0b1]
    e1 = energies_of(m1)
    e1[1, 0] = 1053                                          # equals the run's largest so far: the lower block keeps it
    assert t.push(records_of(m1, 27, 200), e1) == [dict(channel=1, start=52, blocks=3, peak=1053, reference=100)]
    # push 2: ch 0 a run to the end of the push, a larger E here: the R of this push; nothing closes yet
    m2 = [0b11 << 25, 0]
    assert t.push(records_of(m2, 27, 300), energies_of(m2)) == []
    # ch 0's run ends with 2 blocks, fewer than min_blocks: dropped; ch 1's run of 3 is open when the stream ends
    m3 = [0, 0b111 << 24]
    assert t.push(records_of(m3, 27, 400), energies_of(m3)) == []
    assert t.close() == [dict(channel=1, start=54 + 27 + 27 + 24, blocks=3, peak=1026, reference=400)]
    assert t.close() == []


def test_an_event_takes_the_reference_of_the_push_its_peak_lies_in():
    for tracker in (wb.PingEvents(2), pc.HostTracker(1, 2)):
        m = [0b1 << 26]
        e = energies_of(m)
        assert tracker.push(records_of(m, 27, 111), e) == []
        m = [0b11]
        e = energies_of(m)
        e[0, 1] = 5000
        assert tracker.push(records_of(m, 27, 222), e) == [dict(channel=0, start=26, blocks=3, peak=5000, reference=222)]


def test_the_line_of_the_log():
    ev = dict(channel=17, start=1234, blocks=45, peak=285815, reference=74125)
    want = "ping ch=17 offset=-48000 start=9.872 dur=0.360 blocks=45 peak=285815 ref=74125 peak_db=5.9"
    assert wb.ping_event_line(ev, -48000) == pc.host_line(ev, -48000) == want
    d = pc.parse_line(want)
    assert (int(d["ch"]), int(d["offset"]), d["start"], d["dur"]) == (17, -48000, "9.872", "0.360")
    ev = dict(channel=0, start=0, blocks=1, peak=96, reference=96)
    assert wb.ping_event_line(ev, 0) == pc.host_line(ev, 0) == "ping ch=0 offset=0 start=0.000 dur=0.008 blocks=1 peak=96 ref=96 peak_db=0.0"


# ---- the C++ rule and tracker against the model, on random sequences ----

def test_cpp_rule_and_tracker_equal_the_model_on_200_random_sequences():
    rng = np.random.default_rng(2024)
    lines = 0
    for seq in range(200):
        C_ = int(rng.integers(1, 5))
        params = dict(ratio_q4=int(rng.choice([16, 24, 32, 40, 4000])), memory=int(rng.integers(0, 17)), min_ref=int(rng.choice([1, 96, 5000, 1 << 22])))
        min_blocks = int(rng.integers(1, 5))
        py, cc = wb.Pings(C_, **params), pc.HostPings(C_, **params)
        pye, cce = wb.PingEvents(min_blocks), pc.HostTracker(C_, min_blocks)
        scales = np.full(C_, 100.0, dtype=np.float32)
        for push in range(int(rng.integers(2, 24))):
            nb = 54 if push == 0 else 27
            if push and rng.random() < 0.08:                 # a first push in mid-sequence: the detector restarts, the tracker goes on
                nb = 54
                py.reset()
                cc.reset()
            if rng.random() < 0.2:                           # an AGC step or new gains on some channels
                k = rng.random(C_) < 0.5
                scales = np.where(k, scales * np.float32(rng.choice([0.5, 2.0])), scales).astype(np.float32)
            # few distinct levels, so that ties at the rank, at the threshold and at the peak are common
            base = rng.choice([0, 1, 50, 100, 20000, FULL], size=(C_, 1))
            E = (base * rng.choice([0, 1, 1, 1, 2, 3, 8], size=(C_, nb)) + rng.choice([0, 0, 0, 1], size=(C_, nb))).astype(np.int64)
            E = np.minimum(E, FULL)
            # the model takes hops; feed it the energies through ping_blocks' place
            want = _push_energies(py, E, scales)
            got = cc.push_energies(E, scales)
            assert got.tobytes() == want.tobytes(), (seq, push, params, got, want)
            ev_py, ev_cc = pye.push(want, E), cce.push(got, E)
            assert ev_py == ev_cc, (seq, push)
            for e in ev_py:
                assert wb.ping_event_line(e, 12000 * e["channel"]) == pc.host_line(e, 12000 * e["channel"])
                lines += 1
        assert pye.close() == cce.close()
        assert cce.counts()[1:] == (pye.up_blocks, pye.total_blocks)
    assert lines > 500


def _push_energies(det, E, scales):
    """wideband.Pings.push on block energies instead of hops (ping_blocks is tested above)."""
    real = wb.ping_blocks
    wb.ping_blocks = lambda q: np.asarray(q)
    try:
        return det.push(E, scales)
    finally:
        wb.ping_blocks = real


# ---- the scene ----

def test_the_scene_through_the_channeliser_model():
    hops = pc.scene_model_hops()
    rms = [float(np.sqrt(np.mean(hops[0][c].astype(np.float64) ** 2))) for c in pc.SCENE_NOISE_CHANNELS]
    assert all(abs(v - pc.SCENE_LSB) < 1.0 for v in rms), rms
    records, up, events = pc.model_run(hops)
    print("events", events, "up per channel", up.sum(axis=1))
    pc.assert_scene(up, events, "model")
    # the first ping fills 22 of the second push's 27 blocks: its own quartile is a ping block, the memory holds the reference down
    c = pc.SCENE_PINGS[0][0]
    assert records[1]["quiet"][c] > 2 * records[1]["reference"][c] and records[1]["reference"][c] == records[0]["quiet"][c]
    _, up0, _ = pc.model_run(hops, memory=0)
    assert up[c][54:81].sum() >= 21 and up0[c][54:81].sum() == 0
    # the C++ tracker on the same records
    det, t = wb.Pings(len(pc.SCENE_OFFSETS)), pc.HostTracker(len(pc.SCENE_OFFSETS))
    got = []
    for q in hops:
        got += t.push(det.push(q, pc.SCENE_GAIN), det.energies)
    assert got + t.close() == events
