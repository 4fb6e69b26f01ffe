"""msk144hipdecoder --wideband-rate above 6.144 Msps (the two-stage bank), on the CPU: the rate rule (exit 2 before any library call)
and the wideband loop against the stand-in library, whose slots hold 5184 Fs/12000 samples (checks: wideband_cli_check.py)."""
import pytest

import wideband_cli_check as cli


@pytest.fixture(scope="module")
def exe():
    return cli.program()


@pytest.mark.parametrize("rate, message", [
    ("6152001", "multiple of 125"),           # above 6.144 Msps and not a multiple of 125
    ("61448000", "2 <= D <= 512"),            # a multiple of 8000 above 61.44 Msps
    ("12500000", "2 <= D <= 512"),            # a multiple of 125, not of 8000
    ("6156000", "2 <= D <= 512"),
    ("6144125", "2 <= D <= 512"),
    ("23875", "2 <= D <= 512"),
    ("44100", "multiple of 125"),
])
def test_refused_rates_exit_2(exe, rate, message):
    cli.check_refused_rate(exe, rate, message)


def test_offset_limit_at_a_bank_rate(exe):
    cli.check_refused(exe, ["--wideband-rate=10000000", "--channel-offsets=0,4994001"], ["outside"])


@pytest.mark.parametrize("rate, fmt, sample_bytes, pushes", [(6152000, "cu8", 2, 3), (8000000, "cs8", 2, 3), (10000000, "cs16", 4, 3),
                                                             (20000000, "cu8", 2, 2), (61440000, "cu8", 2, 2)])
def test_bank_rates_decode_every_push_on_every_channel(exe, rate, fmt, sample_bytes, pushes):
    lim = rate // 2 - 6000
    offsets = [-lim, -rate // 128, rate // 128, lim]
    P2, Q2 = cli.ratio(rate // 32)
    stage2 = f"decimation {P2}" if Q2 == 1 else f"resampling {P2}/{Q2}"
    cli.check_loop(exe, rate, fmt, sample_bytes, pushes, offsets, "--channel-offsets=" + ",".join(map(str, offsets)),
                   f"stage 1: 64-band analysis bank, 3 bands occupied, sub-band rate {rate // 32} sps, filter 8 x 64 taps; stage 2: {stage2}, filter 16 x {P2} taps")


def test_help_documents_the_bank_range(exe):
    cli.check_help(exe)
