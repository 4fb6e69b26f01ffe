"""-m gpu: the wideband channeliser (msk144_set_wideband .. msk144_wideband_clip_count, include/msk144hip.h) at integer rates
Fs = 12000 D.

1. The int8 hops the device writes agree with the float64 model of the contract (msk144cudecoder_amd/wideband.py).
2. A handle reconfigured for another D, format and set of offsets matches the model again.
3. What the contract refuses: a later push before a first, offsets beyond Fs/2 - 6000, a wrong channel count, an audio handle.
Rational rates are in test_gpu_wideband_rational.py, the bank in test_gpu_wideband_bank.py, the decode in test_gpu_wideband_decode.py.
"""
import pytest

import wideband_check as wc
import wideband_gpu as wg
from msk144cudecoder_amd import wideband as wb

pytestmark = pytest.mark.gpu


def _case(D, fmt, pushes=5):
    """(rate, format, pushes, offsets seed, input seed, level per rail) of wideband_gpu.hops_match_the_model at D x 12000 Hz."""
    return D * 12000, fmt, pushes, D, 1000 + D + len(fmt), 0.03


@pytest.mark.parametrize("D", [80, 160])
@pytest.mark.parametrize("fmt", wb.FORMATS)
def test_hops_match_the_model(hip, parity_report, fmt, D):
    tally = wc.Tally()
    with hip.HipDecoder(channels=64, **wg.DECODE_CFG) as d:
        wg.hops_match_the_model(d, *_case(D, fmt), tally=tally)
    parity_report(f"wideband_model_{D * 12000}_{fmt}", tally.report())


def test_reconfigured_handle_matches_the_model(hip):
    """msk144_set_wideband again on a handle that has pushed: another D, format and set of offsets (the same count) replace the
    first configuration entirely."""
    with hip.HipDecoder(channels=64, **wg.DECODE_CFG) as d:
        wg.hops_match_the_model(d, *_case(80, "cu8"))
        wg.hops_match_the_model(d, *_case(160, "cs16"))


def test_later_push_before_first_is_refused(hip):
    with hip.HipDecoder(channels=2, **wg.DECODE_CFG) as d:
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
