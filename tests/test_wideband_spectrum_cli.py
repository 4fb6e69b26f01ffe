"""CPU: msk144hipdecoder --wideband-spectrum against the stand-in library (tests/stub_hip).

- FILE[:BINS[:HOPS]] makes exactly one msk144_set_wideband_spectrum call with the parsed bins and the default window, behind
  msk144_set_wideband and ahead of every read; the spectrum is read once per push.
- 4 pushes at HOPS 1, 3 and 5 give 4, 2 and 1 lines, the last group shorter, with the fields of the contract: the index of the last
  push, the rate, the bins, the summed segments, and one two-decimal dBFS value per bin in ascending frequency.
- The stderr summary names the floor (median bin) and the highest bin with its frequency.
- A malformed value, a FILE that cannot be opened and the option without --wideband-rate end the program (exit 2) before it calls
  the library; against the stand-in without the entries the option is an error that names the missing entry.
- Without the option the program calls none of the new entries and prints what it printed before.
"""
import os
import re

import pytest

from host_stub import run, shared_program

RATE, OFFSETS, PUSHES = 240000, [-24000, 0, 12000, 36000, 48000], 4
ARGS = [f"--wideband-rate={RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, OFFSETS))]
DATA = bytes((5184 + (PUSHES - 1) * 2592) * RATE // 12000 * 2)


@pytest.fixture(scope="module")
def new():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_spectrum_stub.cpp"))


@pytest.fixture(scope="module")
def old():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp"))


def lines_of(path):
    with open(path) as f:
        return [dict(field.split("=", 1) for field in line.split()) for line in f.read().splitlines()]


@pytest.mark.parametrize("value, bins, groups", [
    (":256:1", 256, [(0, 100), (1, 101), (2, 102), (3, 103)]),
    (":512:3", 512, [(2, 303), (3, 103)]),
    ("", 1024, [(3, 406)]),                      # the defaults: 1024 bins, 5 pushes per line; the one group is the shorter last one
    (":2048", 2048, [(3, 406)]),
    (":256:5", 256, [(3, 406)]),
])
def test_one_set_call_one_read_per_push_and_the_lines(new, tmp_path, value, bins, groups):
    path = str(tmp_path / "spectrum.txt")
    r = run(new, ARGS + [f"--wideband-spectrum={path}{value}"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    assert err.count("stub: msk144_set_wideband_spectrum(") == 1 and f"stub: msk144_set_wideband_spectrum(bins {bins}, window default)" in err
    assert [int(v) for v in re.findall(r"stub: msk144_wideband_spectrum read (\d+)", err)] == list(range(PUSHES))
    assert err.index("stub: msk144_set_wideband(") < err.index("stub: msk144_set_wideband_spectrum(") < err.index("stub: msk144_wideband_spectrum read 0")
    lines = lines_of(path)
    assert [(int(l["hop"]), int(l["segments"])) for l in lines] == groups
    want = ",".join(f"{-(j % 64) + 0.0:.2f}" for j in range(bins))
    for l in lines:
        assert list(l) == ["hop", "rate", "bins", "segments", "dbfs"]
        assert int(l["rate"]) == RATE and int(l["bins"]) == bins
        assert l["dbfs"] == want
    assert err.index("channel I/Q components clipped") < err.index("msk144hipdecoder: wideband spectrum:")
    assert (f"msk144hipdecoder: wideband spectrum: {bins} bins of {RATE / bins:.1f} Hz over 406 segments, floor (median bin) -31.00 dBFS, "
            f"highest bin 0.00 dBFS at -120000 Hz") in err


def test_the_file_is_appended_to(new, tmp_path):
    path = str(tmp_path / "spectrum.txt")
    for _ in range(2):
        assert run(new, ARGS + [f"--wideband-spectrum={path}:256"], DATA, timeout=120).returncode == 0
    assert [int(l["hop"]) for l in lines_of(path)] == [3, 3]


@pytest.mark.parametrize("bad", ["", ":", ":0", ":255", ":300", ":16384", ":256:0", ":256:-1", ":256:x", ":x", ":256:", ":256:1:2", ":128"])
def test_a_malformed_value_ends_the_program_before_any_library_call(new, tmp_path, bad):
    value = bad if bad == "" else str(tmp_path / "s.txt") + bad
    r = run(new, ARGS + ["--wideband-spectrum=" + value], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-spectrum" in r.stderr, bad
    assert b"Done" not in r.stdout


def test_bins_longer_than_a_push_are_refused(new, tmp_path):
    # 24 125 sps: a later push has 5211 samples
    r = run(new, ["--wideband-rate=24125", "--channel-offsets=0", f"--wideband-spectrum={tmp_path / 's.txt'}:8192"], b"")
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-spectrum" in r.stderr and b"5211" in r.stderr


def test_a_file_that_cannot_be_opened_ends_the_program_before_any_library_call(new, tmp_path):
    path = str(tmp_path / "no_such_directory" / "spectrum.txt")
    r = run(new, ARGS + [f"--wideband-spectrum={path}:256:1"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"cannot open" in r.stderr and path.encode() in r.stderr
    assert b"Done" not in r.stdout


def test_the_option_needs_wideband_mode(new, tmp_path):
    path = str(tmp_path / "spectrum.txt")
    r = run(new, [f"--wideband-spectrum={path}"], DATA)
    assert r.returncode == 2 and b"--wideband-rate" in r.stderr and b"stub:" not in r.stderr
    assert not os.path.exists(path)


def test_a_library_without_the_entries_is_an_error(old, tmp_path):
    r = run(old, ARGS + [f"--wideband-spectrum={tmp_path / 'spectrum.txt'}"], DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_set_wideband_spectrum" in err and "stub: msk144_set_wideband(" not in err
    assert b"Done" not in r.stdout
    assert not os.path.exists(tmp_path / "spectrum.txt")        # no empty file is left behind


def test_no_option_no_new_call(new, old):
    outs = []
    for exe in (new, old):
        r = run(exe, ARGS, DATA, timeout=120)
        err = r.stderr.decode()
        assert r.returncode == 0
        assert "spectrum" not in err
        outs.append((re.sub(rb"date=\d{14}", b"date=X", r.stdout), re.sub(r"worst latency \d+ ms", "worst latency X ms", re.sub(r"\d+ late", "N late", err))))
    assert outs[0] == outs[1]


def test_help_names_the_option(new):
    out = run(new, ["--help"]).stdout.decode()
    assert "--wideband-spectrum=FILE[:BINS[:HOPS]]" in out
    assert out.index("--wideband-blanker") < out.index("--wideband-spectrum")
