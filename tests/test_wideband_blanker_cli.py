"""CPU: msk144hipdecoder --wideband-blanker against the stand-in library (tests/stub_hip).

- The bare option makes exactly one msk144_set_wideband_blanker call, with the defaults of include/msk144hip.h, before the first push;
  =RATIO[:PRE[:POST]] passes rint(16 RATIO) and the guards; the statistics are read once, at the end, and their totals are in the
  summary line.
- A malformed value ends the program (exit 2) before it calls the library.
- Against the stand-in without the entries (the stubs as they were) the option is an error that names the missing entry.
- Without the option the program calls none of the new entries and prints what it printed before.
"""
import re

import pytest

from host_stub import run, shared_program

RATE, OFFSETS, PUSHES = 240000, [-24000, 0, 12000, 36000, 48000], 4
ARGS = [f"--wideband-rate={RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, OFFSETS))]
DATA = bytes((5184 + (PUSHES - 1) * 2592) * RATE // 12000 * 2)


@pytest.fixture(scope="module")
def new():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_blanker_stub.cpp"))


@pytest.fixture(scope="module")
def old():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp"))


@pytest.mark.parametrize("option, call, said", [
    ("--wideband-blanker", "threshold_q4 256, pre 2, post 8", "threshold 16 x mean power, guard 2+8 samples"),
    ("--wideband-blanker=8:0:4", "threshold_q4 128, pre 0, post 4", "threshold 8 x mean power, guard 0+4 samples"),
    ("--wideband-blanker=2.53", "threshold_q4 40, pre 2, post 8", "threshold 2.5 x mean power, guard 2+8 samples"),
    ("--wideband-blanker=20:7", "threshold_q4 320, pre 7, post 8", "threshold 20 x mean power, guard 7+8 samples"),
])
def test_one_set_call_and_the_summary_line(new, option, call, said):
    r = run(new, ARGS + [option], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    assert err.count("stub: msk144_set_wideband_blanker(") == 1 and f"stub: msk144_set_wideband_blanker({call})" in err
    assert err.count("stub: msk144_wideband_blanker_stats") == 1
    # set once behind msk144_set_wideband, ahead of everything the pushes print; read once, behind the clip summary
    assert err.index("stub: msk144_set_wideband(") < err.index("stub: msk144_set_wideband_blanker(") < err.index("stub: msk144_wideband_blanker_stats")
    assert err.index("channel I/Q components clipped") < err.index("msk144hipdecoder: wideband blanker:")
    assert f"msk144hipdecoder: wideband blanker: {said}, 1234 hits, 56789 of 98765432 samples blanked (0.0575 %)" in err


@pytest.mark.parametrize("bad", ["=", "=0", "=5000", "=16:-1", "=16:2:4097", "=x", "=16:", "=16:2:", "=16:2:8:1", "=0.9"])
def test_a_malformed_value_ends_the_program_before_any_library_call(new, bad):
    r = run(new, ARGS + ["--wideband-blanker" + bad], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-blanker" in r.stderr, bad
    assert b"Done" not in r.stdout


def test_the_option_needs_wideband_mode(new):
    r = run(new, ["--wideband-blanker"], DATA)
    assert r.returncode == 2 and b"--wideband-rate" in r.stderr and b"stub:" not in r.stderr


def test_a_library_without_the_entries_is_an_error(old):
    r = run(old, ARGS + ["--wideband-blanker"], DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_set_wideband_blanker" in err and "stub: msk144_set_wideband(" not in err
    assert b"Done" not in r.stdout


def test_no_option_no_new_call(new, old):
    outs = []
    for exe in (new, old):
        r = run(exe, ARGS, DATA, timeout=120)
        err = r.stderr.decode()
        assert r.returncode == 0
        assert "blanker" not in err
        outs.append((re.sub(rb"date=\d{14}", b"date=X", r.stdout), re.sub(r"worst latency \d+ ms", "worst latency X ms", re.sub(r"\d+ late", "N late", err))))
    assert outs[0] == outs[1]


def test_help_names_the_option(new):
    out = run(new, ["--help"]).stdout.decode()
    assert "--wideband-blanker[=RATIO[:PRE[:POST]]]" in out
    assert out.index("--wideband-levels") < out.index("--wideband-blanker")
