"""The stream-ping contract on the CPU (include/msk144hip.h, "Stream levels and pings"): block energies and levels against plain
Python loops, StreamPings against hand-built sequences, the host library's C++ against the Python model, the default ratio on noise."""
import numpy as np
import pytest

from msk144cudecoder_amd import stream_pings as sp
from msk144cudecoder_amd.wideband import PingEvents, Pings

CAP = (1 << 22) - 1


def loop_energies(x, shift):
    out = []
    for b in range(len(x) // 96):
        total = 0
        for v in x[96 * b:96 * (b + 1)]:
            total += int(v) * int(v)
        out.append(min(CAP, total >> shift))
    return out


def hop(levels_per_block):
    """A hop whose block b is the constant `levels_per_block[b]` with alternating sign: E[b] = 96 v^2 >> shift."""
    x = np.repeat(np.asarray(levels_per_block, dtype=np.int64), 96)
    return (x * np.where(np.arange(x.size) % 2 == 0, 1, -1)).astype(np.int16)


@pytest.mark.parametrize("shift", [0, 5, 12, 24])
def test_block_energies_equal_a_plain_loop(shift):
    rng = np.random.default_rng(shift)
    for scale in (3, 300, 32768):
        x = rng.integers(-scale, scale, size=5184).astype(np.int16)
        assert [int(v) for v in sp.block_energies(x, shift)] == loop_energies(x, shift)
    with pytest.raises(ValueError):
        sp.block_energies(np.zeros(100, dtype=np.int16), shift)
    with pytest.raises(ValueError):
        sp.block_energies(np.zeros(96, dtype=np.int16), 25)


def test_saturation_and_levels_at_full_scale():
    x = np.full(2592, -32768, dtype=np.int16)
    for shift in range(0, 15):
        assert np.all(sp.block_energies(x, shift) == CAP)
    assert int(sp.block_energies(x, 15)[0]) == (96 << 30) >> 15 < CAP
    assert int(sp.block_energies(x, 24)[0]) == 6144
    l = sp.levels(x, 12)
    assert int(l["sum_sq"]) == 27 * 96 * 2 ** 30 and int(l["sum"]) == -32768 * 2592
    assert int(l["peak"]) == 32768 and int(l["full_scale"]) == 2592 and int(l["samples"]) == 2592 and int(l["saturated_blocks"]) == 27
    assert int(sp.levels(x, 15)["saturated_blocks"]) == 0
    y = np.array([32767, -32767, 5, -32768] * 24, dtype=np.int16)
    l = sp.levels(y, 0)
    assert int(l["peak"]) == 32768 and int(l["full_scale"]) == 48 and int(l["sum"]) == 24 * (5 - 32768)
    assert int(l["sum_sq"]) == 24 * (2 * 32767 ** 2 + 25 + 32768 ** 2)


def test_history_longer_than_sixteen_hops_a_restart_and_partial_lists():
    """Three streams, shift 0, memory 16, block levels chosen by hand: E = 96 v^2."""
    m = sp.StreamPings(3, ratio_q4=32, memory=16, min_ref=1, shift=0)
    E = lambda v: 96 * v * v
    # stream 0 gets quieter every hop for 20 hops: the reference is the minimum of the last 16 quiet levels and its own
    for k in range(20):
        v = 40 - k                                                    # 96 (4 v)^2 stays under the cap
        first = k == 0
        blocks = [v] * (54 if first else 27)
        blocks[3] = 4 * v                                             # one block 16 x the quiet energy: up at ratio 2
        ids, firsts, rows = [0], [first], [hop(blocks)]
        if k in (0, 4, 5):                                            # stream 2 is listed three times only
            ids, firsts, rows = [0, 2], [first, k == 0], [hop(blocks), hop([10 + k] * (54 if k == 0 else 27))]
        rec, lev, en, ev = m.push(ids, firsts, rows)
        assert int(rec["history"][0]) == min(k, 16) and int(rec["quiet"][0]) == E(v) and int(rec["reference"][0]) == E(v)
        assert int(rec["up_mask"][0]) == 1 << 3 and int(rec["peak_block"][0]) == 3 and int(rec["peak"][0]) == E(4 * v)
        if len(ids) == 2:
            assert int(rec["history"][1]) == {0: 0, 4: 1, 5: 2}[k]    # untouched while unlisted
            assert int(rec["reference"][1]) == E(10)                  # the lowest of its own three
    # now louder again: the reference stays at the minimum of the 16 hops before, which no longer holds hops 0..3
    rec, _, _, _ = m.push([0], [False], [hop([90] * 27)])
    assert int(rec["history"][0]) == 16 and int(rec["reference"][0]) == E(21) and int(rec["up_mask"][0]) == (1 << 27) - 1
    # stream 1 appears late, without is_first: its first listed hop restarts it; stream 0 restarts by is_first, stream 2 goes on
    rec, _, _, _ = m.push([0, 1, 2], [True, False, False], [hop([7] * 54), hop([9] * 27), hop([20] * 27)])
    assert [int(v) for v in rec["history"]] == [0, 0, 3]
    assert [int(v) for v in rec["reference"]] == [E(7), E(9), E(10)]
    assert [int(v) for v in rec["blocks"]] == [54, 27, 27]
    with pytest.raises(ValueError):
        m.push([1, 0], [False, False], [hop([1] * 27)] * 2)
    with pytest.raises(ValueError):
        m.push([0], [True], [hop([1] * 27)])


def test_events_count_blocks_per_stream_and_stay_open_across_hops():
    m = sp.StreamPings(2, min_blocks=2, ratio_q4=32, memory=8, min_ref=1, shift=0)
    quiet, loud = 10, 100
    a = [quiet] * 54
    a[52:54] = [loud, loud]                       # open at the end of the first hop ...
    b = [quiet] * 27
    b[0:3] = [loud] * 3                           # ... and three more blocks into the next
    _, _, _, ev = m.push([0], [True], [hop(a)])
    assert ev == []
    _, _, _, ev = m.push([0, 1], [False, True], [hop(b), hop([quiet] * 53 + [loud])])
    assert ev == [dict(channel=0, start=52, blocks=5, peak=96 * loud * loud, reference=96 * quiet * quiet)]
    assert sp.stream_ping_line(ev[0]) == "ping ch=0 start=0.416 dur=0.040 blocks=5 peak=960000 ref=9600 peak_db=20.0"
    assert sp.host_ping_line(ev[0]) == sp.stream_ping_line(ev[0])
    # stream 1 ends with a single block up: shorter than min_blocks, nothing is reported
    assert m.close() == []
    assert m.up_blocks(0) == 5 and m.total_blocks(0) == 81 and m.up_blocks(1) == 1 and m.total_blocks(1) == 54


def test_the_model_reuses_the_wideband_rule():
    m = sp.StreamPings(2)
    assert all(type(p) is Pings and p.channels == 1 for p in m.pings) and all(type(e) is PingEvents for e in m.events)


@pytest.mark.parametrize("params", [dict(), dict(ratio_q4=16, memory=16, min_ref=1, shift=0), dict(ratio_q4=40, memory=3, min_ref=4096, shift=24), dict(memory=0, shift=7)])
def test_the_host_library_equals_the_python_model(params):
    rng = np.random.default_rng(11)
    C = 4
    model, host = sp.StreamPings(C, **params), sp.HostStreamPings(C, **params)
    saturated = 0
    for k in range(24):
        ids = sorted(rng.choice(C, size=int(rng.integers(1, C + 1)), replace=False).tolist()) if k else list(range(C))
        firsts = [k == 0 or (k == 11 and s == 2) for s in ids]
        rows = []
        for s, f in zip(ids, firsts):
            x = rng.normal(0.0, (30.0, 400.0, 5000.0, 40000.0)[s], size=5184 if f else 2592)
            b = int(rng.integers(0, 27))
            x[96 * b:96 * (b + 2)] *= 6.0
            rows.append(np.clip(np.rint(x), -32768, 32767).astype(np.int16))
        rec, lev, en, _ = model.push(ids, firsts, rows)
        h_rec, h_lev, h_en = host.push(ids, firsts, rows)
        assert rec.tobytes() == h_rec.tobytes() and lev.tobytes() == h_lev.tobytes() and np.array_equal(en, h_en)
        saturated += int(lev["saturated_blocks"].sum())
    assert saturated > 0 or params.get("shift", 12) > 12    # the loud stream reaches the cap


def test_defaults_and_checks_agree_with_the_header():
    assert sp.host_defaults() == sp.STREAM_PINGS_DEFAULTS
    assert sp.host_check() == ""
    for bad in (dict(ratio_q4=15), dict(ratio_q4=65536), dict(memory=-1), dict(memory=17), dict(min_ref=0), dict(min_ref=(1 << 22) + 1), dict(shift=-1), dict(shift=25)):
        assert sp.host_check(**bad) != ""
        with pytest.raises((ValueError, TypeError)):
            sp.StreamPings(1, **bad)
    for good in (dict(ratio_q4=16, memory=0, min_ref=1, shift=0), dict(ratio_q4=65535, memory=16, min_ref=1 << 22, shift=24)):
        assert sp.host_check(**good) == ""
        sp.StreamPings(1, **good)


def test_no_block_of_noise_is_up_at_the_default_ratio():
    """The table of csrc/stream_pings.h, shortened: band-limited Gaussian noise at rms 30, 100 and 1000 LSB, 300 hops, the floor out of
    the way - no block is up at the default ratio, and some are at 2.0, so the run does look at the tail."""
    rng = np.random.default_rng(5)
    hops = 300
    n = (hops + 1) * 2592

    def band_noise(rms):
        X = np.fft.rfft(rng.standard_normal(n))
        f = np.fft.rfftfreq(n, 1.0 / 12000.0)
        X[(f < 300.0) | (f > 2700.0)] = 0.0
        x = np.fft.irfft(X, n)
        return np.rint(x * (rms / np.sqrt(np.mean(x * x)))).astype(np.int16)

    x = [band_noise(r) for r in (30, 100, 1000)]
    at_default, at_two = sp.StreamPings(3, min_ref=1), sp.StreamPings(3, ratio_q4=32, min_ref=1)
    for k in range(hops):
        rows = [v[:5184] if k == 0 else v[(k + 1) * 2592:(k + 2) * 2592] for v in x]
        rec, _, _, _ = at_default.push([0, 1, 2], [k == 0] * 3, rows)
        assert not rec["up_mask"].any(), (k, rec)
        at_two.push([0, 1, 2], [k == 0] * 3, rows)
    assert all(at_default.total_blocks(s) == 27 * (hops + 1) for s in range(3))
    assert sum(at_two.up_blocks(s) for s in range(3)) > 0
