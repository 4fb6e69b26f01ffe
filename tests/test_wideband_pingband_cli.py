"""CPU: msk144hipdecoder --wideband-pings-band against the stand-in library (tests/stub_hip).

- [=HALFWIDTH[:CENTRE]] makes exactly one msk144_set_wideband_ping_band call, with the taps and the shift of the host design
  (libmsk144host.so) for the parsed values, behind msk144_set_wideband and ahead of the first read; CENTRE defaults to
  --center-frequency, wherever on the line that stands.
- The detector's RATIO default becomes the band's (3.25) only when --wideband-pings carries no RATIO.
- The ping lines are what they were; the summary line names the band.
- Malformed values, out-of-range values and the option without --wideband-pings end the program (exit 2) before any library call;
  against a stand-in without the entry the option is an error that names it.
- Without the option the new entry is not called and the output is what it was.
"""
import os
import re

import pytest

import wideband_pingband_check as bc
from host_stub import run, shared_program
from msk144cudecoder_amd import wideband as wb

RATE, OFFSETS, PUSHES = 240000, [-24000, 0, 12000, 36000, 48000], 4
ARGS = [f"--wideband-rate={RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, OFFSETS))]
DATA = bytes((5184 + (PUSHES - 1) * 2592) * RATE // 12000 * 2)


@pytest.fixture(scope="module")
def new():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_pings_stub.cpp", "wideband_pingband_stub.cpp"))


@pytest.fixture(scope="module")
def old():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_pings_stub.cpp"))


def band_call(centre, halfwidth):
    taps, shift = wb.ping_band_taps(centre, halfwidth)
    return f"stub: msk144_set_wideband_ping_band(shift {shift}, taps {taps.tobytes().hex()})", shift


@pytest.mark.parametrize("extra, option, centre, halfwidth", [
    ([], "--wideband-pings-band", 0, 1500),
    ([], "--wideband-pings-band=", 0, 1500),      # an empty value is no value
    ([], "--wideband-pings-band=1000", 0, 1000),
    ([], "--wideband-pings-band=500:-5500", -5500, 500),
    ([], "--wideband-pings-band=3000:0", 0, 3000),
    (["--center-frequency=1200"], "--wideband-pings-band", 1200, 1500),
    (["--center-frequency=1200"], "--wideband-pings-band=1234:137", 137, 1234),
])
@pytest.mark.parametrize("centre_first", [True, False])
def test_one_set_call_with_the_host_design(new, tmp_path, extra, option, centre, halfwidth, centre_first):
    path = str(tmp_path / "pings.txt")
    args = ARGS + (extra + [option] if centre_first else [option] + extra) + [f"--wideband-pings={path}"]
    r = run(new, args, DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    call, shift = band_call(centre, halfwidth)
    assert err.count("stub: msk144_set_wideband_ping_band(") == 1 and call in err
    assert err.index("stub: msk144_set_wideband(") < err.index(call) < err.index("stub: msk144_wideband_pings read 0")
    # no RATIO: the band's default
    assert err.count("stub: msk144_set_wideband_pings(") == 1
    assert f"stub: msk144_set_wideband_pings(ratio_q4 {wb.PING_BAND_RATIO_Q4}, memory 8, min_ref 96)" in err and wb.PING_BAND_RATIO_Q4 == 52
    assert re.search(r"msk144hipdecoder: wideband pings: \d+ events on \d+ of 5 channels, 14 of \d+ blocks up, band %d \+-%d Hz shift %d; most active" % (centre, halfwidth, shift), err)


@pytest.mark.parametrize("value, ratio_q4", [(":2", 32), (":3.25", 52), (":1.75:1", 28), ("", 52)])
@pytest.mark.parametrize("band_first", [True, False])
def test_the_ratio_default_switches_only_without_a_ratio(new, tmp_path, value, ratio_q4, band_first):
    pings = f"--wideband-pings={tmp_path / 'pings.txt'}{value}"
    r = run(new, ARGS + (["--wideband-pings-band", pings] if band_first else [pings, "--wideband-pings-band"]), DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert f"stub: msk144_set_wideband_pings(ratio_q4 {ratio_q4}, memory 8, min_ref 96)" in err


def test_the_ping_lines_keep_their_format(new, tmp_path):
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    assert run(new, ARGS + [f"--wideband-pings={a}"], DATA, timeout=120).returncode == 0
    assert run(new, ARGS + [f"--wideband-pings={b}", "--wideband-pings-band=1000:250"], DATA, timeout=120).returncode == 0
    with open(a) as fa, open(b) as fb:
        la, lb = fa.read(), fb.read()
    assert la and la == lb      # the stand-in's records do not depend on the band


def test_the_parser():
    assert bc.host_parse("") == (1500, 0) and bc.host_parse("", 1200) == (1500, 1200)
    assert bc.host_parse("1000") == (1000, 0) and bc.host_parse("1000", -300) == (1000, -300)
    assert bc.host_parse("500:-5500") == (500, -5500) and bc.host_parse("3000:3000", 99) == (3000, 3000)
    for bad in (":", "x", "1500:", "1500:x", ":0", "499", "3001", "1500:4501", "1500:-4501", "1500:0:0", "1e3", "1500.0"):
        assert bc.host_parse(bad) is None, bad
    assert bc.host_parse("", 4501) is None and bc.host_parse("500", 5500) == (500, 5500)


@pytest.mark.parametrize("bad", ["=:", "=x", "=1500:", "=1500:x", "=499", "=3001", "=1500:4501", "=500:-5501", "=1500:0:0", "=1500.5"])
def test_a_malformed_value_ends_the_program_before_any_library_call(new, tmp_path, bad):
    path = tmp_path / "p.txt"
    r = run(new, ARGS + [f"--wideband-pings={path}", "--wideband-pings-band" + bad], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-pings-band" in r.stderr, bad
    assert b"Done" not in r.stdout and not os.path.exists(path)


def test_a_centre_frequency_outside_the_band_rule_is_refused(new, tmp_path):
    r = run(new, ARGS + ["--center-frequency=5000", f"--wideband-pings={tmp_path / 'p.txt'}", "--wideband-pings-band"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-pings-band" in r.stderr


def test_the_option_needs_the_detector_and_wideband_mode(new, tmp_path):
    r = run(new, ARGS + ["--wideband-pings-band"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-pings-band needs --wideband-pings" in r.stderr and b"Done" not in r.stdout
    r = run(new, ["--wideband-pings-band=1000"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-rate" in r.stderr


def test_a_library_without_the_entry_is_an_error(old, tmp_path):
    r = run(old, ARGS + [f"--wideband-pings={tmp_path / 'pings.txt'}", "--wideband-pings-band"], DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_set_wideband_ping_band" in err and "stub: msk144_set_wideband(" not in err
    assert b"Done" not in r.stdout and not os.path.exists(tmp_path / "pings.txt")


def test_no_option_no_new_call(new, old, tmp_path):
    outs = []
    for k, exe in enumerate((new, old)):
        r = run(exe, ARGS + [f"--wideband-pings={tmp_path / ('p%d.txt' % k)}"], DATA, timeout=120)
        err = r.stderr.decode()
        assert r.returncode == 0
        assert "ping_band" not in err and ", band " not in err
        assert "stub: msk144_set_wideband_pings(ratio_q4 32, memory 8, min_ref 96)" in err
        # what does not depend on timing: the standard output, every call the stand-in reports, and the program's own summary lines
        outs.append((re.sub(rb"date=\d{14}", b"date=X", r.stdout), sorted(l for l in err.splitlines() if l.startswith("stub:") or l.startswith("msk144hipdecoder: wideband"))))
    assert outs[0] == outs[1]
    with open(tmp_path / "p0.txt") as f0, open(tmp_path / "p1.txt") as f1:
        assert f0.read() == f1.read() != ""


def test_help_names_the_option(new):
    out = run(new, ["--help"]).stdout.decode()
    assert "--wideband-pings-band[=HALFWIDTH[:CENTRE]]" in out
    assert out.index("--wideband-pings=") < out.index("--wideband-pings-band") < out.index("--wideband-waterfall")
