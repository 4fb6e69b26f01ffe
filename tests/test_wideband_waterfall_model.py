"""CPU: the per-channel waterfall of the wideband contract (include/msk144hip.h) - wideband.Waterfall, the float64 model the device is
held to, wideband.PingSpectra and the line of the program's log - against numpy's FFT, values worked out by hand, and the C++ rules
of csrc/wideband.h (what the program runs, through libmsk144host.so).

- The model equals np.fft.fft of the windowed blocks, rolled by 48, for the Hann, an all-ones and a random window.
- With an all-ones window the sum over a row is 96 x the block energy of wideband.ping_blocks, exactly in float64 (Parseval on
  integers).
- A tone at +1375 Hz reads j = 59 and one at -2500 Hz j = 28 in every block; a constant 127 + 127j hop reads 2 (127 sum w)^2 at j = 48.
- The default window, the check, (sum w)^2, the dB scale and the line are the C++ ones; the bound's helpers behave.
- wideband.PingSpectra equals the exported C++ rule on random up masks and rows, with runs across push boundaries and runs shorter
  than min_blocks, and its frequencies pair with the events of wideband.PingEvents one to one.
- The parser of --wideband-waterfall=FILE[:CHANNELS].
"""
import math

import numpy as np
import pytest

import wideband_waterfall_check as wc
from msk144cudecoder_amd import wideband as wb

WINDOWS = {"hann": None, "ones": np.ones(96), "random": wc.random_window(1)}


def random_hops(seed, channels=3, nb=27):
    return np.random.default_rng(seed).integers(-128, 128, size=(channels, 96 * nb, 2)).astype(np.int8)


@pytest.mark.parametrize("nb", [27, 54])
@pytest.mark.parametrize("name", list(WINDOWS))
def test_the_model_is_the_fft_of_the_windowed_blocks(name, nb):
    m = wb.Waterfall(WINDOWS[name])
    q = random_hops(11, nb=nb)
    rows = m.push(q)
    assert rows.shape == (3, nb, 96) and rows.dtype == np.float64
    x = (q[..., 0].astype(np.float64) + 1j * q[..., 1]).reshape(3, nb, 96) * m.window
    want = np.roll(np.abs(np.fft.fft(x, axis=2)) ** 2, 48, axis=2)
    assert np.all(np.abs(rows - want) <= 1e-12 * np.sum(want, axis=2, keepdims=True))
    # the window is the f32 the device stores
    assert np.array_equal(m.window, m.window.astype(np.float32).astype(np.float64))


def test_an_all_ones_window_gives_96_times_the_block_energy_exactly():
    q = random_hops(12, channels=4, nb=54)
    rows = wb.Waterfall(np.ones(96)).push(q)
    E = wb.ping_blocks(q)
    # Parseval; float64 carries the 23-bit sums exactly only up to rounding of the irrational twiddles, so compare after rounding
    assert np.array_equal(np.rint(np.sum(rows, axis=2)).astype(np.int64), 96 * E)
    assert np.all(np.abs(np.sum(rows, axis=2) - 96.0 * E) <= 1e-12 * 96.0 * E)


@pytest.mark.parametrize("f_hz, j", [(1375.0, 59), (-2500.0, 28), (0.0, 48), (-6000.0, 0), (5875.0, 95)])
def test_a_tone_reads_its_slot_in_every_block(f_hz, j):
    assert wb.waterfall_hz(j) == f_hz
    rows = wb.Waterfall().push(wc.tone_hop(f_hz)[None])[0]
    assert list(np.argmax(rows, axis=1)) == [j] * 27
    # amplitude 100 on a bin centre: (A sum w)^2 within the rounding of the samples to integers
    full = wb.waterfall_full()
    assert np.all(np.abs(10.0 * np.log10(rows[:, j] / full) - 40.0) < 0.05)


def test_a_constant_hop_reads_its_power_at_the_centre():
    q = np.full((1, 2592, 2), 127, dtype=np.int8)
    for name, w in WINDOWS.items():
        m = wb.Waterfall(w)
        rows = m.push(q)[0]
        want = 2.0 * (127.0 * float(np.sum(m.window))) ** 2
        assert np.all(np.abs(rows[:, 48] - want) <= 1e-12 * want), name
        assert wb.waterfall_full(w) == pytest.approx(float(np.sum(m.window)) ** 2, rel=1e-15)


def test_the_cpp_window_check_scale_and_line():
    assert np.array_equal(wc.host_window(), wb.waterfall_window())
    assert wc.host_check(None) == "" and wc.host_check(np.ones(96)) == "" and wc.host_check(-np.ones(96)) == ""
    for bad in (np.nan, np.inf, -np.inf):
        w = np.ones(96)
        w[17] = bad
        assert "17" in wc.host_check(w)
        with pytest.raises(ValueError):
            wb.Waterfall(w)
    for w in WINDOWS.values():
        assert wc.host_full(w) == wb.waterfall_full(w)
    full = wb.waterfall_full()
    assert full == pytest.approx(48.0 ** 2, rel=1e-6)           # the Hann window sums to 48
    assert list(wb.waterfall_db([full, 100.0 * full, 0.0, 1e-11 * full, 2e-10 * full], full)) == pytest.approx([0.0, 20.0, -100.0, -100.0, 10.0 * math.log10(2e-10)], abs=1e-9)
    for p in (0.0, 1.0, 3.7e5, 1e-9, full):
        assert float(wb.waterfall_db(p, full)) == wc.host().msk144host_wideband_waterfall_db(p, full)
    rng = np.random.default_rng(5)
    for k in range(20):
        row = (rng.uniform(0.0, 1.0, 96) ** 8 * 1e9).astype(np.float32)
        row[k] = 0.0
        row[95 - k] = np.float32(full * (1.0 - 1e-4))          # just under 0 dB: "-0.00" is written as "0.00"
        line = wb.waterfall_line(k, -12000 + k, 1000 * k + 3, row, full)
        assert line == wc.host_line(k, -12000 + k, 1000 * k + 3, row, full)
        d = wc.parse_line(line)
        assert (int(d["ch"]), int(d["offset"]), int(d["block"])) == (k, -12000 + k, 1000 * k + 3) and d["t"] == "%.3f" % (0.008 * (1000 * k + 3))
        db = d["db"].split(",")
        assert db[k] == "-100.00" and db[95 - k] == "0.00" and "-0.00" not in db


def test_the_bound_and_needed_u():
    rows = wb.Waterfall().push(random_hops(13))
    got = rows.astype(np.float32).astype(np.float64)
    assert wc.needed_u(rows, rows) == 0.0 and wc.needed_u(got, rows) < 3e-8      # rounding to f32 alone lies inside v P
    off = rows * (1.0 + 1e-3)
    need = wc.needed_u(off, rows)
    assert np.all(np.abs(off - rows) <= wc.bound(rows, need * (1.0 + 1e-9))) and not np.all(np.abs(off - rows) <= wc.bound(rows, need * 0.99))
    with pytest.raises(AssertionError):
        wc.assert_rows(off, rows, wc.U, "a relative error of 1e-3")
    zero = np.zeros((1, 2, 96))
    assert wc.needed_u(zero, zero) == 0.0 and wc.needed_u(zero + 1.0, zero) == np.inf
    assert wc.U < wc.CEILING == 98.0 * 2.0 ** -24


def test_sums_add_the_f32_rows_in_order():
    rows = (np.random.default_rng(3).uniform(0, 1, (2, 27, 96)) * 1e7).astype(np.float32)
    s = wb.waterfall_sums(rows)
    want = np.zeros((2, 96))
    for b in range(27):
        want += rows[:, b].astype(np.float64)
    assert s.dtype == np.float64 and s.tobytes() == want.tobytes()


@pytest.mark.parametrize("min_blocks", [1, 2, 4])
def test_ping_spectra_equals_the_cpp_rule_and_pairs_with_the_events(min_blocks):
    rng = np.random.default_rng([7, min_blocks])
    for trial in range(30):
        C_ = int(rng.integers(1, 6))
        py, cc, ev = wb.PingSpectra(C_, min_blocks), wc.HostSpectra(C_, min_blocks), wb.PingEvents(min_blocks)
        n_events = n_freqs = 0
        for push in range(5):
            nb = 54 if push == 0 else 27
            rec = np.zeros(C_, dtype=wb.PING_DTYPE)
            rec["blocks"] = nb
            rec["reference"] = 100
            # runs of random length, often up at either end of the push: across the boundary, and shorter than min_blocks
            up = rng.random((C_, nb)) < rng.choice([0.15, 0.6, 0.9])
            up[:, -1] |= rng.random(C_) < 0.5
            up[:, 0] |= rng.random(C_) < 0.5
            rec["up_mask"] = [sum(1 << b for b in range(nb) if up[c, b]) for c in range(C_)]
            rows = (rng.uniform(0.0, 1.0, (C_, nb, 96)) ** 4 * 1e8).astype(np.float32)
            rows[:, :, 40] = rows[:, :, 41]                        # ties between neighbours: the lowest j wins
            E = rng.integers(200, 100000, (C_, nb))
            f_py, f_cc = py.push(rec, rows), cc.push(rec, rows)
            assert f_py == f_cc, (trial, push)
            n_events += len(ev.push(rec, E))
            n_freqs += len(f_py)
            assert n_events == n_freqs
            assert all(f % 125 == 0 and -6000 <= f <= 5875 for f in f_py)
        f_py, f_cc = py.close(), cc.close()
        assert f_py == f_cc and n_events + len(ev.close()) == n_freqs + len(f_py)


def test_ping_spectra_holds_exactly_the_rows_of_the_event():
    rec = np.zeros(1, dtype=wb.PING_DTYPE)
    rows = np.zeros((1, 27, 96), dtype=np.float32)
    rows[0, 3, 10] = 5.0           # a lone up block ahead: cleared by block 4
    rows[0, 20:27, 70] = 1.0       # the event: blocks 20..26 of push 0 and 0..2 of push 1, strongest at j = 70 ...
    rows[0, 22, 30] = 6.5          # ... but for one block that is louder elsewhere, yet less than the event's 10 at j = 70
    rec["blocks"], rec["up_mask"] = 27, (1 << 3) | sum(1 << b for b in range(20, 27))
    s = wb.PingSpectra(1, 2)
    assert s.push(rec, rows) == []
    nxt = np.zeros((1, 27, 96), dtype=np.float32)
    nxt[0, 0:3, 70] = 1.0
    nxt[0, 5, 12] = 9.0            # not up: never added
    rec["up_mask"] = 0b111
    assert s.push(rec, nxt) == [wb.waterfall_hz(70)] == [2750]
    assert s.close() == []


def test_the_parser():
    assert wc.host_parse("f") == (True, [], 1)
    assert wc.host_parse("some/file.txt:pings") == (True, [], 13)
    assert wc.host_parse("f:0") == (False, [0], 1) and wc.host_parse("f:3,1,2") == (False, [3, 1, 2], 1)
    assert wc.host_parse("f:" + ",".join(map(str, range(16)))) == (False, list(range(16)), 1)
    for bad in ("", ":", ":3", "f:", "f:x", "f:-1", "f:1,", "f:,1", "f:1,,2", "f:1,1", "f:1:2", "f:pings,1", "f:" + ",".join(map(str, range(17))), "f:99999999999"):
        assert wc.host_parse(bad) is None, bad
