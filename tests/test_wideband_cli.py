"""msk144hipdecoder --wideband-rate on the CPU: option checks (exit 2 before any library call) and the wideband loop against the
stand-in library - tests/stub_hip/msk144hip_stub.cpp plus the wideband entries of tests/stub_hip/wideband_stub.cpp, whose push
hands every channel a marked hop.  The checks themselves are in wideband_cli_check.py, with those of the rational and bank rates."""
import pytest

import wideband_cli_check as cli
from host_stub import run, shared_program


@pytest.fixture(scope="module")
def exe():
    return cli.program()


@pytest.fixture(scope="module")
def exe_old_stub():
    """The program against a library without the wideband entries: it still links (they are resolved only for --wideband-rate)."""
    return shared_program()


@pytest.mark.parametrize("args, message", [
    (["--wideband-rate=1920000", "--channel-offsets=0", "--inputs=a,b"], "excludes --inputs"),
    (["--wideband-rate=1920000", "--channel-offsets=0", "--interleaved=4"], "excludes --inputs"),
    (["--wideband-rate=1920000", "--channel-offsets=0", "--devices=0,1"], "--devices"),
    (["--wideband-rate=1920000", "--channel-offsets=0", "--read-mode=1"], "--read-mode=1"),
    (["--wideband-rate=1920000"], "exactly one of --channel-offsets"),
    (["--wideband-rate=1920000", "--channel-offsets=0", "--channel-grid=0:1000:4"], "exactly one of --channel-offsets"),
    (["--channel-offsets=0,1000"], "need --wideband-rate"),
    (["--wideband-rate=1920001", "--channel-offsets=0"], "multiple of 12000"),
    (["--wideband-rate=12000", "--channel-offsets=0"], "2 <= D <= 512"),
    (["--wideband-rate=6156000", "--channel-offsets=0"], "2 <= D <= 512"),
    (["--wideband-rate=1920000", "--channel-offsets=954001"], "outside +-(rate/2 - 6000) = +-954000 Hz"),
    (["--wideband-rate=1920000", "--channel-grid=-954000:1000:3000"], "outside"),
    (["--wideband-rate=1920000", "--channel-offsets=1,x"], "bad value for --channel-offsets"),
    (["--wideband-rate=1920000", "--channel-offsets=0", "--wideband-format=cu16"], "bad value for --wideband-format"),
    (["--wideband-rate=1920000", "--channel-offsets=0", "--taps-per-phase=65"], "bad value for --taps-per-phase"),
    (["--wideband-rate=1920000", "--channel-offsets=0", "--wideband-gain=-1"], "gain must be a positive"),
    (["--wideband-rate=1920000", "--channel-offsets=0", "--wideband-gain=3e38"], "gain must be a positive finite number no larger than 1e36"),
])
def test_bad_combinations_exit_2(exe, args, message):
    cli.check_refused(exe, args, [message])


def test_missing_library_entries_are_an_error_not_a_fallback(exe_old_stub):
    r = run(exe_old_stub, ["--wideband-rate=24000", "--channel-offsets=0"])
    assert r.returncode == 2 and b"no wideband channeliser" in r.stderr


def test_help_lists_the_wideband_options(exe):
    cli.check_help(exe)


@pytest.mark.parametrize("fmt, sample_bytes", [("cu8", 2), ("cs16", 4)])
def test_wideband_loop_decodes_every_push_on_every_channel(exe, fmt, sample_bytes):
    cli.check_loop(exe, 48000, fmt, sample_bytes, 5, [-15000 + 6000 * c for c in range(6)], "--channel-grid=-15000:6000:6", "Center Frequency: 0Hz",
                   ["--wideband-gain=3.5", "--taps-per-phase=8"], K=8, gain="3.5", within=0.0)
