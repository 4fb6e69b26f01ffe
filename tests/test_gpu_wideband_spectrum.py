"""-m gpu: the power spectrum of the wideband input stream (include/msk144hip.h) against its float64 model, wideband.Spectrum.

Every comparison holds every bin to the contract's bound |P^[k] - P[k]| <= 2 u sqrt(P[k] T) + u^2 T + v P[k] with u = U
(wideband_spectrum_check.py: where U comes from), prints the u it needed first, and `segments` is exact.  The stream is the one
of wideband_spectrum_check.py: noise, a full-scale tone on a bin centre, a tone between bins at -40 dB, one impulse per push.

1. Every size: 240 ksps (pushes of 103 680 and 51 840 samples, N mod B != 0 from B = 256 up), 5 channels, 3 pushes, B = 256 .. 8192
   x cu8, cs8, cs16 with the default window, and a seeded random positive window at B = 256 and 8192.  The largest u each (B, format)
   needed goes to the parity report.
2. Odd lengths: 24 125 sps (pushes of 10 422 / 5 211 samples, no whole 16-byte loads) at B = 256 and 4096, cu8 and cs16; B = 8192 is
   longer than a push there: EINVAL.
3. Many segments: the 8 Msps bank shape (1 728 000 samples per later push) at B = 8192 and 256, cs16, two pushes - more rounds than
   workgroups, so the partial-sum rows and the fixed-order reduction are exercised, and the spectrum is that of the stream at Fs,
   ahead of stage 1.
4. With the blanker on the spectrum is that of the model fed wideband.Blanker's stream, from cu8.  (No full-scale tone in this
   stream: with one the push's mean power is 1 and no impulse exceeds 16 x it.)  What the impulses' flat pedestal added to the
   total is gone: T drops by what the model says.
5. It changes nothing: two handles, the same pushes, the spectrum on and off, at the three shapes of wideband_levels_check.py:
   hops, clip counts and levels are byte-identical, and at 24 125 sps the decoded records are.
6. Order: the same stream pushed twice gives the same bytes; `set` between pushes takes effect at the next push;
   msk144_set_wideband switches the spectrum off; every EINVAL / ESTATE case of the contract.
"""
import numpy as np
import pytest

import wideband_check as wc
import wideband_levels_check as lc
import wideband_options as wo
import wideband_spectrum_check as sc
from msk144cudecoder_amd import wideband as wb
from wideband_options import EINVAL, code_of

pytestmark = pytest.mark.gpu

RATE = 240000
OFFSETS = np.array([-114000, -30000, 0, 12345, 114000], dtype=np.int32)


@pytest.fixture(scope="module")
def handles(hip):
    """Two handles per channel count, made on first use and kept for the module."""
    with wo.handle_cache(wo.decode_pair(hip)) as get:
        yield get


def push_and_compare(d, model, parts, what):
    """Push parts (the first a first push) to d and to the model; every bin inside the bound, segments exact.  The largest u needed."""
    need = 0.0
    for i, part in enumerate(parts):
        d.push_wideband(i % 2, part, first=i == 0)
        want, segments = model.push(part)
        got, got_segments = d.wideband_spectrum()
        assert got_segments == segments == len(part) // 2 // model.bins and got.shape == want.shape
        need = max(need, sc.assert_within(got, want, sc.U, f"{what} push {i}"))
    return need


# ---- 1. every size ----

@pytest.mark.parametrize("fmt", wb.FORMATS)
@pytest.mark.parametrize("B, window_seed", [(B, None) for B in sc.BINS] + [(256, 11), (8192, 12)])
def test_every_size_against_the_model(handles, parity_report, B, window_seed, fmt):
    d, _ = handles(len(OFFSETS))
    parts = sc.pushes(RATE, fmt, 3)
    assert [len(p) // 2 for p in parts] == [103680, 51840, 51840] and all((len(p) // 2) % B for p in parts[1:])
    window = None if window_seed is None else sc.random_window(B, window_seed)
    d.set_wideband(RATE, OFFSETS, fmt)
    d.set_wideband_spectrum(B, window)
    what = f"{fmt} B={B}" + ("" if window is None else " random window")
    need = push_and_compare(d, wb.Spectrum(fmt, B, window), parts, what)
    assert need <= sc.ceiling(B), "above the textbook ceiling: a bug in the kernel, not a tolerance"
    # the tone sits in its slot, close to full scale (less what the format clipped of tone plus noise)
    if window is None:
        got, S = d.wideband_spectrum()
        db = wb.spectrum_dbfs(got, S, wb.Spectrum(fmt, B).window)
        assert int(np.argmax(db)) == sc.tone_slot(B) and -1.0 < db[sc.tone_slot(B)] < 0.05
    parity_report(f"wideband_spectrum_u_{fmt}_{B}" + ("" if window is None else "_random_window"), dict(u_needed=need, u_contract=sc.U, ceiling=sc.ceiling(B)))


# ---- 2. odd lengths ----

@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
def test_odd_push_lengths(hip, handles, parity_report, fmt):
    shape = lc.SHAPES["rat"]
    d, _ = handles(len(shape["offsets"]))
    parts = sc.pushes(shape["rate"], fmt, 3)
    assert [len(p) // 2 for p in parts] == [10422, 5211, 5211]
    d.set_wideband(shape["rate"], shape["offsets"], fmt)
    assert code_of(hip, lambda: d.set_wideband_spectrum(8192)) == EINVAL        # longer than a later push
    for B in (256, 4096):
        d.set_wideband_spectrum(B)
        need = push_and_compare(d, wb.Spectrum(fmt, B), parts, f"24125 sps {fmt} B={B}")
        parity_report(f"wideband_spectrum_u_odd_{fmt}_{B}", dict(u_needed=need, u_contract=sc.U, ceiling=sc.ceiling(B)))


# ---- 3. many segments ----

@pytest.mark.parametrize("B", [8192, 256])
def test_many_segments_at_a_bank_rate(handles, parity_report, B):
    shape = lc.SHAPES["bank"]
    d, _ = handles(len(shape["offsets"]))
    parts = sc.pushes(shape["rate"], "cs16", 2)
    assert len(parts[1]) // 2 == 1728000
    d.set_wideband(shape["rate"], shape["offsets"], "cs16")
    d.set_wideband_spectrum(B)
    need = push_and_compare(d, wb.Spectrum("cs16", B), parts, f"8 Msps cs16 B={B}")
    parity_report(f"wideband_spectrum_u_bank_cs16_{B}", dict(u_needed=need, u_contract=sc.U, ceiling=sc.ceiling(B)))


# ---- 4. with the blanker on ----

def blanker_pushes():
    """cu8: noise, the -40 dB tone and one full-scale impulse per push - 400 x the mean power, a hit at the default 16 x."""
    rng = np.random.default_rng(44)
    sizes = [k // 2 for k in wb.push_sizes_for_rate(3, RATE)]
    n = sum(sizes)
    x = sc.SIGMA * (rng.normal(size=n) + 1j * rng.normal(size=n))
    x += 0.01 * np.exp(2j * np.pi * (np.mod(sc.BETWEEN_BIN_OF_16384 * np.arange(n, dtype=np.int64), 16384) / 16384.0))
    # inside a segment and near the window's peak at both B of the test: sample 1152 of a block of 2048
    at = np.cumsum([0] + sizes[:-1]) + np.array([(k // 2) // 2048 * 2048 + 1152 for k in sizes])
    x[at] = 1.0 + 1.0j
    raw = wb.write_samples(x, "cu8")
    return wc.split_pushes(raw, RATE, 3)


@pytest.mark.parametrize("B", [256, 2048])
def test_with_the_blanker_on(handles, B):
    a, b = handles(len(OFFSETS))
    parts = blanker_pushes()
    for d in (a, b):
        d.set_wideband(RATE, OFFSETS, "cu8")
        d.set_wideband_spectrum(B)
    a.set_wideband_blanker()
    blanker, blanked_model, raw_model = wb.Blanker("cu8"), wb.Spectrum("cs16", B), wb.Spectrum("cu8", B)
    for i, part in enumerate(parts):
        for d in (a, b):
            d.push_wideband(i % 2, part, first=i == 0)
        stream, st = blanker.push(part)
        assert st["hits"] == 1 and a.wideband_blanker_stats() == st
        want, S = blanked_model.push(stream)
        got, got_S = a.wideband_spectrum()
        assert got_S == S
        sc.assert_within(got, want, sc.U, f"blanked cu8 B={B} push {i}")
        raw_want, _ = raw_model.push(part)
        raw_got, _ = b.wideband_spectrum()
        sc.assert_within(raw_got, raw_want, sc.U, f"raw cu8 B={B} push {i}")
        # the pedestal: the blanked samples' share of the total is gone, to what the two bounds leave of a sum over the bins
        drop, model_drop = raw_got.sum() - got.sum(), raw_want.sum() - want.sum()
        slack = sc.bound(raw_want, sc.U).sum() + sc.bound(want, sc.U).sum()
        print(f"push {i}: T drops by {drop:.6g}, the model's by {model_drop:.6g} (slack {slack:.3g})")
        assert model_drop > 10.0 * slack and abs(drop - model_drop) <= slack


# ---- 5. it changes nothing ----

@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_it_changes_nothing(handles, name):
    shape = lc.SHAPES[name]
    rate, offsets, K = shape["rate"], shape["offsets"], shape["K"]
    a, b = handles(len(offsets))
    if name == "rat":
        parts, planted, fmt, gain = wo.rat_scene()
    else:
        parts, fmt, gain = sc.pushes(rate, "cs16", 2), "cs16", 4.0
    for d in (a, b):
        d.set_wideband(rate, offsets, fmt, taps_per_phase=K, gain=gain)
    a.set_wideband_spectrum(1024)
    seen = wo.leaves_unchanged(a, b, parts, decode=name == "rat")
    assert a.wideband_spectrum()[1] == len(parts[-1]) // 2 // 1024
    if name == "rat":
        assert sum(len(s["records"]) for s in seen) > 0 and planted     # the scene decodes to something


# ---- 6. order ----

def test_order_and_refusals(hip, handles):
    a, _ = handles(len(OFFSETS))
    parts = sc.pushes(RATE, "cs8", 3)
    wo.refuses_outside_wideband_mode(hip, [hip.HipDecoder.set_wideband_spectrum, hip.HipDecoder.wideband_spectrum])
    a.set_wideband(RATE, OFFSETS, "cs8")
    for bad in (0, 128, 255, 300, 1000, 16384, -1024):
        assert code_of(hip, lambda: a.set_wideband_spectrum(bad)) == EINVAL, bad
    for bad in (np.nan, np.inf, -np.inf):
        w = np.ones(256)
        w[200] = bad
        assert code_of(hip, lambda: a.set_wideband_spectrum(256, w)) == EINVAL, bad
    wo.unreadable(hip, [a.wideband_spectrum])                                           # before any push
    a.push_wideband(0, parts[0], first=True)
    wo.unreadable(hip, [a.wideband_spectrum])                                           # ... and after one made without the spectrum

    # the same stream pushed twice gives the same bytes
    a.set_wideband_spectrum(512)
    last = wo.same_bytes_twice(a, parts, hip.HipDecoder.wideband_spectrum)[2]

    # `set` between pushes: the last push's spectrum stays readable, the next push has the new size and window
    window = sc.random_window(2048, 3)
    a.set_wideband_spectrum(2048, window)
    p, s = a.wideband_spectrum()
    assert s == last[1] and p.tobytes() == last[0].tobytes()
    a.push_wideband(1, parts[1], first=False)
    want, segments = wb.Spectrum("cs8", 2048, window).push(parts[1])
    got, got_segments = a.wideband_spectrum()
    assert got_segments == segments and got.shape == (2048,)
    sc.assert_within(got, want, sc.U, "after set in mid-stream")

    # switched off: from the next push on there is nothing to read; on again: there is
    a.set_wideband_spectrum(None)
    a.push_wideband(0, parts[2], first=False)
    wo.unreadable(hip, [a.wideband_spectrum])
    a.set_wideband_spectrum(256)
    a.push_wideband(1, parts[2], first=False)
    sc.assert_within(a.wideband_spectrum()[0], wb.Spectrum("cs8", 256).push(parts[2])[0], sc.U, "switched on again")

    # msk144_set_wideband switches the spectrum off
    a.set_wideband(RATE, OFFSETS, "cs8")
    a.push_wideband(0, parts[0], first=True)
    wo.unreadable(hip, [a.wideband_spectrum])
