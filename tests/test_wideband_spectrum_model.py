"""CPU: the float64 model of the wideband input spectrum (wideband.Spectrum, include/msk144hip.h).

1. A full-scale tone (amplitude 1.0) on a bin centre reads 0.00 dBFS in its ascending-frequency slot, for cu8, cs8 and cs16, at
   negative and positive frequencies and at k = B/2 (slot 0, -Fs/2); where an 8-bit format cannot hold the tone (k = 0 and B/2
   put every sample on a rail at exactly +-1) it reads what the format kept, 0.03 dB less.
2. Parseval: sum P = B sum_s ||w x_s||^2.
3. The N mod B tail and whatever a caller prepends as history do not matter: a push's spectrum is a function of its own first S B samples.
4. A zeroed run of samples lowers T by exactly what the run held (rectangular window, one segment).
5. The default window equals msk144host_wideband_spectrum_window, and both are the periodic Hann window.
6. spectrum_dbfs floors at -200.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import wideband_spectrum_check as sc
from msk144cudecoder_amd import wideband as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "msk144cudecoder_amd", "host")


@pytest.fixture(scope="module")
def host_lib():
    subprocess.run(["make", "-s", "-C", HOST, "../libmsk144host.so"], check=True)
    L = C.CDLL(wb.HOST_LIB)
    L.msk144host_wideband_spectrum_window.argtypes = [C.c_int, C.c_void_p]
    L.msk144host_wideband_spectrum_window.restype = C.c_int
    return L


@pytest.mark.parametrize("k", [-97, -1, 0, 1, 37, 127, -128])
@pytest.mark.parametrize("fmt", wb.FORMATS)
def test_a_full_scale_tone_reads_0_dbfs_in_its_slot(fmt, k):
    B, S = 256, 3
    n = np.arange(S * B + 11)
    tone = np.exp(2j * np.pi * k * n / B)
    raw = wb.write_samples(tone, fmt)
    m = wb.Spectrum(fmt, B)
    power, segments = m.push(raw)
    assert segments == S and power.shape == (B,)
    db = wb.spectrum_dbfs(power, segments, m.window)
    slot = (k + B // 2) % B            # k = -128 = B/2: slot 0, at -Fs/2
    assert int(np.argmax(db)) == slot
    # what the format kept of the tone, by plain correlation: amplitude 1 to within its rounding for a rotating tone.  At k = 0 and
    # k = B/2 every sample sits on a rail at exactly +-1, which an 8-bit format cannot hold (cu8 127.5/128, cs8 +127/128): -0.03 dB
    kept = abs(np.mean(wb.read_samples(raw, fmt)[:S * B] * np.conj(tone[:S * B])))
    assert abs(db[slot] - 20.0 * np.log10(kept)) < 0.005, (db[slot], kept)   # half a unit of the program's last decimal
    if fmt == "cs16" or k not in (0, -128):
        assert f"{db[slot] + 0.0:.2f}" in ("0.00", "-0.00"), db[slot]
    else:
        assert -0.08 < db[slot] < 0.0
    # everything else is the format's rounding under a Hann window: the neighbours -6.02 dB, the rest far below
    assert abs(db[(slot + 1) % B] - db[slot] + 6.02) < 0.05 and abs(db[(slot - 1) % B] - db[slot] + 6.02) < 0.05
    others = np.delete(db, [(slot - 1) % B, slot, (slot + 1) % B])
    assert np.all(others < (-45.0 if fmt != "cs16" else -90.0))


@pytest.mark.parametrize("fmt", wb.FORMATS)
def test_parseval(fmt):
    B = 512
    raw = sc.pushes(240000, fmt, 2)[1]
    w = sc.random_window(B, 1)
    m = wb.Spectrum(fmt, B, w)
    power, S = m.push(raw)
    x = wb.read_samples(raw, fmt)[:S * B].reshape(S, B) * m.window[None, :]
    assert S == len(raw) // 2 // B
    assert np.isclose(power.sum(), B * np.sum(np.abs(x) ** 2), rtol=1e-12, atol=0.0)


def test_the_tail_and_the_history_do_not_matter():
    B = 1024
    raw = sc.pushes(240000, "cs16", 2)[1]
    n = len(raw) // 2
    assert n % B != 0
    m = wb.Spectrum("cs16", B)
    power, S = m.push(raw)
    changed = raw.copy()
    changed[2 * S * B:] = 12345                      # the N mod B samples at the end
    again, S2 = m.push(changed)
    assert S2 == S and np.array_equal(again, power)
    # the model keeps nothing: pushing something else in between changes nothing, and history a caller prepends is other input
    m.push(sc.pushes(240000, "cs16", 2)[0])
    assert np.array_equal(m.push(raw)[0], power)
    with_history = np.concatenate([np.full(2 * 99, 777, dtype=np.int16), raw])
    assert not np.array_equal(m.push(with_history)[0], power)


def test_a_zeroed_run_lowers_the_total_by_what_it_held():
    B = 256
    raw = np.array(sc.pushes(240000, "cs16", 1)[0][:2 * B])
    m = wb.Spectrum("cs16", B, np.ones(B))
    total = m.push(raw)[0].sum()
    held = np.sum(np.abs(wb.read_samples(raw, "cs16")[40:51]) ** 2)
    raw[2 * 40:2 * 51] = 0
    assert np.isclose(total - m.push(raw)[0].sum(), B * held, rtol=1e-10, atol=0.0)


@pytest.mark.parametrize("B", sc.BINS)
def test_the_default_window_is_the_librarys(host_lib, B):
    w = np.empty(B, dtype=np.float64)
    assert host_lib.msk144host_wideband_spectrum_window(B, w.ctypes.data_as(C.c_void_p)) == B
    mine = wb.spectrum_window(B)
    # two cosine routines: equal to an ulp of 1 in double, and the same f32 the device stores
    assert np.max(np.abs(w - mine)) <= 2.0 ** -52
    assert np.array_equal(w.astype(np.float32), mine.astype(np.float32))
    assert np.array_equal(wb.Spectrum("cu8", B).window, w.astype(np.float32).astype(np.float64))
    i = np.arange(B)
    assert np.allclose(w, np.sin(np.pi * i / B) ** 2, rtol=0.0, atol=1e-15) and w[0] == 0.0 and w[B // 2] == 1.0
    assert abs(w.sum() - B / 2) < 1e-9


def test_the_library_refuses_other_sizes(host_lib):
    for B in (0, 128, 255, 300, 16384, -256):
        assert host_lib.msk144host_wideband_spectrum_window(B, None) == -1


def test_the_model_refuses_what_the_contract_refuses():
    for B in (128, 300, 16384):
        with pytest.raises(ValueError):
            wb.Spectrum("cu8", B)
    with pytest.raises(ValueError):
        wb.Spectrum("cu8", 256, np.full(256, np.nan))
    with pytest.raises(ValueError):
        wb.Spectrum("cu8", 256, np.ones(255))
    with pytest.raises(ValueError):
        wb.Spectrum("cf32", 256)


def test_dbfs_floors_at_minus_200():
    w = wb.spectrum_window(256)
    db = wb.spectrum_dbfs(np.array([0.0, 1e-300, 128.0 ** 2 * 3, 1e-25]), 3, w)
    assert db[0] == -200.0 and db[1] == -200.0 and db[3] == -200.0
    assert abs(db[2]) < 1e-9


def test_the_tests_constant_is_the_headers_and_lies_below_the_ceiling():
    with open(os.path.join(ROOT, "include", "msk144hip.h")) as f:
        m = re.search(r"^#define MSK144_SPECTRUM_U\s+(\S+)", f.read(), re.M)
    assert m and float(m.group(1)) == sc.U
    assert 0.0 < sc.U <= min(sc.ceiling(B) for B in sc.BINS)


def test_the_bound_holds_a_perturbed_model_spectrum_exactly_at_the_u_it_needs():
    """needed_u inverts the contract's bound: on the model's spectrum of the test stream, with an error of the size f32 leaves."""
    want, _ = wb.Spectrum("cs16", 512).push(sc.pushes(240000, "cs16", 2)[1])
    got = want + np.random.default_rng(8).normal(size=512) * 1e-7 * np.sqrt(want * want.sum())
    u = sc.needed_u(got, want)
    assert 1e-8 < u < 1e-6
    assert np.all(np.abs(got - want) <= sc.bound(want, u * (1 + 1e-9)))
    assert not np.all(np.abs(got - want) <= sc.bound(want, u * (1 - 1e-6)))
