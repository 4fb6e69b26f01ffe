"""CPU: msk144hipdecoder --wideband-gain=auto and --wideband-levels against the stand-in library (tests/stub_hip).

- With both options the program makes exactly one msk144_set_wideband_agc call, with the defaults of include/msk144hip.h, reads the
  levels once per push and prints the table: one line per channel and the line that names the most clipped and quietest channels.
- Against the stand-in without the new entries (the stubs as they were) the same options are an error, not a fallback.
- Without the options the program calls none of the new entries and prints what it printed before.
"""
import math
import re

import pytest

from host_stub import run, shared_program

RATE, OFFSETS, PUSHES = 240000, [-24000, 0, 12000, 36000, 48000], 4
ARGS = [f"--wideband-rate={RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, OFFSETS))]
DATA = bytes((5184 + (PUSHES - 1) * 2592) * RATE // 12000 * 2)


@pytest.fixture(scope="module")
def new():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_levels_stub.cpp"))


@pytest.fixture(scope="module")
def old():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp"))


def stub_level(c, i):
    """What tests/stub_hip/wideband_levels_stub.cpp reports for channel c at read i."""
    n = 5184 if i == 0 else 2592
    return dict(samples=n, sum_sq=2 * n * (c + 1) ** 2, clipped=3 * c if i == 0 else c, exponent=c % 3 - 1 - i % 2)


def test_auto_gain_and_levels(new):
    r = run(new, ARGS + ["--wideband-gain=auto", "--wideband-levels"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    assert err.count("stub: msk144_set_wideband_agc(") == 1
    assert "stub: msk144_set_wideband_agc(lo_sq 64, hi_sq 1024, clip_ppm 1000, hold 4, min_exp -20, max_exp 20)" in err
    assert "gain 100, " in err.replace(" x 2^e (AGC, e within +-20)", "") and "AGC" in err
    assert "stub: msk144_set_wideband_gains" not in err
    assert "lower --wideband-gain" not in err
    lines = re.findall(r"msk144hipdecoder: wideband level ch=(\d+) offset=(-?\d+) Hz rms=([0-9.]+) LSB clipped=(\d+) gain=([0-9.e+-]+) exp=(-?\d+)\.\.(-?\d+)", err)
    assert [int(l[0]) for l in lines] == list(range(len(OFFSETS))) and [int(l[1]) for l in lines] == OFFSETS
    for c, l in enumerate(lines):
        lv = [stub_level(c, i) for i in range(PUSHES)]
        rms = math.sqrt(sum(v["sum_sq"] for v in lv) / (2 * sum(v["samples"] for v in lv)))
        assert abs(float(l[2]) - rms) < 0.006 and int(l[3]) == sum(v["clipped"] for v in lv)
        assert float(l[4]) == 100.0 * 2.0 ** lv[-1]["exponent"]
        assert (int(l[5]), int(l[6])) == (min(v["exponent"] for v in lv), max(v["exponent"] for v in lv))
    assert err.index("channel I/Q components clipped") < err.index("wideband level ch=0")
    assert "wideband levels: most clipped ch=4 (24) ch=3 (18) ch=2 (12); quietest ch=0 (1.00 LSB) ch=1 (2.00 LSB) ch=2 (3.00 LSB)" in err


def test_base_gain_and_levels_alone(new):
    r = run(new, ARGS + ["--wideband-gain=auto:3.5"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0 and "gain 3.5, " in err.replace(" x 2^e (AGC, e within +-20)", "")
    assert err.count("stub: msk144_set_wideband_agc(") == 1 and "wideband level ch=" not in err and "stub: msk144_wideband_levels" not in err
    r = run(new, ARGS + ["--wideband-levels"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0 and "stub: msk144_set_wideband_agc" not in err and err.count("wideband level ch=") == len(OFFSETS)
    for bad in ("auto:", "auto:x", "autox", "auto:0", "auto:1e36"):
        r = run(new, ARGS + [f"--wideband-gain={bad}"], DATA)
        assert r.returncode == 2 and b"stub:" not in r.stderr, bad


@pytest.mark.parametrize("options", [["--wideband-gain=auto"], ["--wideband-levels"], ["--wideband-gain=auto:50", "--wideband-levels"]])
def test_a_library_without_the_entries_is_an_error(old, options):
    r = run(old, ARGS + options, DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_wideband_levels" in err and "stub: msk144_set_wideband(" not in err
    assert b"Done" not in r.stdout


def test_no_new_option_no_new_call(new, old):
    outs = []
    for exe in (new, old):
        r = run(exe, ARGS + ["--wideband-gain=100"], DATA, timeout=120)
        err = r.stderr.decode()
        assert r.returncode == 0
        assert "msk144_set_wideband_agc" not in err and "msk144_wideband_levels" not in err and "msk144_set_wideband_gains" not in err
        assert "wideband level" not in err and "lower --wideband-gain" in err
        outs.append((re.sub(rb"date=\d{14}", b"date=X", r.stdout), re.sub(r"worst latency \d+ ms", "worst latency X ms", re.sub(r"\d+ late", "N late", err))))
    assert outs[0] == outs[1]


def test_help_names_the_options(new):
    out = run(new, ["--help"]).stdout.decode()
    assert "--wideband-gain=auto[:G0]" in out and "--wideband-levels" in out
