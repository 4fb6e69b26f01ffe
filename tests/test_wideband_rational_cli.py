"""msk144hipdecoder --wideband-rate at rational rates (12000 x P/Q), on the CPU: the rate rule (exit 2 before any library call) and
the wideband loop against the stand-in library, whose slots hold 5184 P/Q samples (checks: wideband_cli_check.py)."""
import pytest

import wideband_cli_check as cli
from host_stub import run


@pytest.fixture(scope="module")
def exe():
    return cli.program()


@pytest.mark.parametrize("rate, message", [
    ("44100", "multiple of 12000"),           # the 44.1 kHz family: not a multiple of 125
    ("2048001", "multiple of 12000"),
    ("23875", "2 <= D <= 512"),               # a multiple of 125 below 24000
    ("6144125", "2 <= D <= 512"),             # ... above 6144000
])
def test_refused_rates_exit_2(exe, rate, message):
    cli.check_refused_rate(exe, rate, message)


@pytest.mark.parametrize("rate, P, Q, fmt, sample_bytes", [(2048000, 512, 3, "cu8", 2), (250000, 125, 6, "cs16", 4), (96125, 769, 96, "cs8", 2)])
def test_rational_loop_decodes_every_push_on_every_channel(exe, rate, P, Q, fmt, sample_bytes):
    assert cli.ratio(rate) == (P, Q)
    cli.check_loop(exe, rate, fmt, sample_bytes, 5, [-18000 + 12000 * c for c in range(4)], "--channel-grid=-18000:12000:4",
                   f"resampling {P}/{Q}, filter 16 x {P} taps")


def test_integer_rate_summary_is_unchanged(exe):
    D, pushes = 4, 2
    data = bytes((5184 + (pushes - 1) * 2592) * D * 2)
    r = run(exe, ["--wideband-rate=48000", "--channel-offsets=0,6000"], data)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert "wideband input 48000 sps cu8 on stdin, decimation 4, filter 16 x 4 taps, gain 100, 2 channels" in err
    assert "resampling" not in err


def test_help_documents_the_rate_rule(exe):
    cli.check_help(exe)
