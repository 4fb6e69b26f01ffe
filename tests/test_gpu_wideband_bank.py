"""-m gpu: the two-stage wideband bank above 6.144 Msps (include/msk144hip.h; csrc/bank.hip, then csrc/channelise.hip at Fs/32).

1. The int8 hops agree with the float64 two-stage model (msk144cudecoder_amd/wideband.py, TwoStage) by the two-stage near-tie rule
   (tests/wideband_bank_check.py) at 8, 10, 20 and 61.44 Msps, in cu8, cs8 and cs16, with random non-symmetric taps for both stages,
   channels in several bands, at both sides of band boundaries and at +-(Fs/2 - 6000); clip counts as the model's.  The dumped
   sub-band streams agree with the stage-1 model within its own bound, so that a stage-1 error shows as one.
2. The stream: a first push after later ones restarts both stages; one handle reconfigured bank -> 1.92 Msps -> bank.
The decode behind the bank (a 10 Msps scene) is in test_gpu_wideband_decode.py.
"""
import numpy as np
import pytest

import wideband_bank_check as bc
import wideband_check as wc
import wideband_gpu as wg

pytestmark = pytest.mark.gpu


def _check_stream(d, rate, fmt, offsets, taps, bank_taps, gain, parts, firsts, what):
    ref = bc.BankReference(rate, offsets, taps=taps, K=bc.K2, gain=gain, bank_taps=bank_taps)
    d.set_wideband(rate, offsets, fmt, taps=taps, taps_per_phase=bc.K2, gain=gain, bank_taps=bank_taps)

    def subbands_within_the_stage1_bound(i, got, y, clip):
        for j, b in enumerate(ref.model.bands):
            s = d.dump_wideband_band(b if b < 32 else b - 64)
            s_ref = ref.model.last_subbands[j]
            e1 = bc.stage1_delta(ref.T1, ref.K1)
            assert s.shape == s_ref.shape
            over = (np.abs(s.real - s_ref.real) > e1) | (np.abs(s.imag - s_ref.imag) > e1)
            assert not over.any(), f"{what} push {i}: band {b} off the stage-1 bound at {np.flatnonzero(over)[:5]}"

    wg.check_stream(d, ref, fmt, parts, firsts, what, on_push=subbands_within_the_stage1_bound)


@pytest.mark.parametrize("rate, fmt, n_pushes", bc.CASES)
def test_hops_match_the_two_stage_model(hip, rate, fmt, n_pushes):
    offsets, taps, bank_taps, gain, raw = bc.case(rate, fmt, n_pushes)
    with hip.HipDecoder(channels=len(offsets), **wg.DECODE_CFG) as d:
        _check_stream(d, rate, fmt, offsets, taps, bank_taps, gain, wc.split_pushes(raw, rate, n_pushes), [True] + [False] * (n_pushes - 1),
                      f"{fmt} {rate}")


@pytest.mark.parametrize("fmt", ["cs8", "cs16"])
def test_other_formats_at_61p44_msps(hip, fmt):
    rate = 61440000
    offsets, taps, bank_taps, gain, raw = bc.case(rate, fmt, 1, seed=1)
    with hip.HipDecoder(channels=len(offsets), **wg.DECODE_CFG) as d:
        _check_stream(d, rate, fmt, offsets, taps, bank_taps, gain, wc.split_pushes(raw, rate, 1), [True], f"{fmt} {rate}")


def test_restart_and_reconfigure(hip):
    rate = 10000000
    offsets, taps, bank_taps, gain, raw = bc.case(rate, "cs16", 3, seed=2)
    parts = wc.split_pushes(raw, rate, 3)
    with hip.HipDecoder(channels=len(offsets), **wg.DECODE_CFG) as d:
        # first, later, then the first push again and a later one: the second first push restarts both stages
        _check_stream(d, rate, "cs16", offsets, taps, bank_taps, gain, [parts[0], parts[1], parts[0], parts[1]], [True, False, True, False], "restart")
        # the same handle at a single-stage rate, then back at a bank rate with the default bank
        lo = 1920000
        o2 = wc.offsets_for(lo, len(offsets), np.random.default_rng(5))
        d.set_wideband(lo, o2, "cu8")
        raw2 = wc.raw_input(lo, 2, "cu8", np.random.default_rng(6), 0.03)
        wg.check_stream(d, wc.Reference(lo, o2), "cu8", wc.split_pushes(raw2, lo, 2), [True, False], "1.92 Msps")
        rate2 = 20000000
        offsets3, taps3, _, gain3, raw3 = bc.case(rate2, "cu8", 2, seed=3)
        _check_stream(d, rate2, "cu8", offsets3, taps3, None, gain3, wc.split_pushes(raw3, rate2, 2), [True, False], "default bank")


def test_bank_taps_rules(hip):
    with hip.HipDecoder(channels=1, **wg.DECODE_CFG) as d:
        with pytest.raises(hip.Msk144Error):     # bank taps at a single-stage rate
            d.set_wideband(1920000, [0], bank_taps=np.ones(512) / 512)
        with pytest.raises(hip.Msk144Error):     # not 64 K1 taps
            d.set_wideband(10000000, [0], bank_taps=np.ones(500) / 500)
        for rate in (6156000, 6144125, 12500000, 61448000):
            with pytest.raises(hip.Msk144Error) as e:
                d.set_wideband(rate, [0], taps=np.ones(16))
            assert "2 <= D <= 512" in str(e.value)
