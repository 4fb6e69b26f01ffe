"""-m gpu: the wideband channeliser at rational rates Fs = 12000 P/Q (include/msk144hip.h).

1. The int8 hops the device writes agree with the float64 model of the contract (msk144cudecoder_amd/wideband.py) at 2.048 Msps
   (512/3, every format), 250 ksps (125/6), 96.125 ksps (769/96) and 6.142 Msps (3071/6).
2. One handle reconfigured integer -> rational -> integer matches the model each time.
3. The rate rule and the tap count K x P are enforced.
The decode at 2.048 Msps is in test_gpu_wideband_decode.py.
"""
import numpy as np
import pytest

import wideband_check as wc
import wideband_gpu as wg
from msk144cudecoder_amd import wideband as wb

pytestmark = pytest.mark.gpu
RTL_RATE = 2048000


def _case(rate, fmt, pushes=5):
    """(rate, format, pushes, offsets seed, input seed, level per rail) of wideband_gpu.hops_match_the_model: seeded by the rate, at
    the in-channel level of the 1.92 Msps tests, so that clipping stays rare."""
    return rate, fmt, pushes, rate, 1000 + rate + len(fmt), 0.03 * np.sqrt(rate / 1920000)


def _model_case(hip, parity_report, rate, fmt, n_pushes=5):
    tally = wc.Tally()
    with hip.HipDecoder(channels=64, **wg.DECODE_CFG) as d:
        wg.hops_match_the_model(d, *_case(rate, fmt, n_pushes), tally=tally)
    parity_report(f"wideband_model_{rate}_{fmt}", tally.report())


@pytest.mark.parametrize("fmt", wb.FORMATS)
def test_hops_match_the_model_2p048_msps(hip, parity_report, fmt):
    _model_case(hip, parity_report, RTL_RATE, fmt)


@pytest.mark.parametrize("rate, n_pushes", [(250000, 5), (96125, 5), (6142000, 3)])
def test_hops_match_the_model_other_rates(hip, parity_report, rate, n_pushes):
    _model_case(hip, parity_report, rate, "cs16", n_pushes)


def test_reconfigured_integer_rational_integer(hip):
    with hip.HipDecoder(channels=64, **wg.DECODE_CFG) as d:
        wg.hops_match_the_model(d, *_case(960000, "cu8", 3))
        wg.hops_match_the_model(d, *_case(RTL_RATE, "cs8", 3))
        wg.hops_match_the_model(d, *_case(1920000, "cs16", 3))


def test_rational_rate_rule_is_enforced(hip):
    with hip.HipDecoder(channels=1, **wg.DECODE_CFG) as d:
        for rate in (2048001, 23875, 6144125):
            with pytest.raises(hip.Msk144Error) as e:
                d.set_wideband(rate, [0], taps=np.ones(16, dtype=np.float64))
            assert e.value.code == -1
        with pytest.raises(hip.Msk144Error) as e:     # K x P taps, not K x floor(Fs/12000)
            d.set_wideband(RTL_RATE, [0], taps=np.full(16 * 170, 1.0 / (16 * 170)))
        assert e.value.code == -1 and "taps" in str(e.value)
