"""CPU: msk144hipdecoder --wideband-pings against the stand-in library (tests/stub_hip).

- FILE[:RATIO[:MIN_BLOCKS[:MEMORY]]] makes exactly one msk144_set_wideband_pings call with the parsed parameters, behind
  msk144_set_wideband and ahead of every read; records and block energies are read once per push, where its clip count is read.
- FILE holds, line for line, the events wideband.PingEvents makes of the stand-in's records, formatted by wideband.ping_event_line:
  a run across a push boundary is one line, a run shorter than MIN_BLOCKS none, and the run that is open when the stream ends is
  written then.  The file is appended to.
- The stderr summary names the events, the channels that had any, the up blocks and the most active channels.
- The parser (through libmsk144host.so) keeps RATIO as rint(16 x RATIO) and refuses what the library would refuse; a malformed
  value, a FILE that cannot be opened and the option without --wideband-rate end the program (exit 2) before it calls the library;
  against the stand-in without the entries the option is an error that names the missing entry.
- Without the option the program calls none of the new entries and prints what it printed before.
"""
import os
import re

import numpy as np
import pytest

import wideband_pings_check as pc
from host_stub import run, shared_program
from msk144cudecoder_amd import wideband as wb

RATE, OFFSETS, PUSHES = 240000, [-24000, 0, 12000, 36000, 48000], 4
ARGS = [f"--wideband-rate={RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, OFFSETS))]
DATA = bytes((5184 + (PUSHES - 1) * 2592) * RATE // 12000 * 2)


@pytest.fixture(scope="module")
def new():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_pings_stub.cpp"))


@pytest.fixture(scope="module")
def old():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp"))


def stub_up(i, c, b):
    """The rule of tests/stub_hip/wideband_pings_stub.cpp."""
    if c == 0:
        return i >= 1 and b in (25, 26)
    if c == 1:
        return (i == 0 and b >= 50) or (i == 1 and b <= 2)
    return c == 3 and i == 2 and b == 5


def stub_events(min_blocks):
    """(the events wideband.PingEvents makes of the stand-in's records, the tracker)."""
    t, events = wb.PingEvents(min_blocks), []
    for i in range(PUSHES):
        nb = 54 if i == 0 else 27
        rec = np.zeros(len(OFFSETS), dtype=wb.PING_DTYPE)
        E = np.zeros((len(OFFSETS), nb), dtype=np.int64)
        for c in range(len(OFFSETS)):
            R = 1000 * (c + 1) + i
            rec[c]["blocks"], rec[c]["reference"] = nb, R
            rec[c]["up_mask"] = sum(1 << b for b in range(nb) if stub_up(i, c, b))
            E[c] = [10 * R + b if stub_up(i, c, b) else R // 2 for b in range(nb)]
        events += t.push(rec, E)
    return events + t.close(), t


@pytest.mark.parametrize("value, params, min_blocks", [
    ("", (32, 8, 96), 2),
    (":2.5", (40, 8, 96), 2),
    (":1.75:1", (28, 8, 96), 1),
    (":2:3:0", (32, 0, 96), 3),
    (":4095.9:64:16", (65534, 16, 96), 64),
])
def test_one_set_call_one_read_per_push_and_the_lines(new, tmp_path, value, params, min_blocks):
    path = str(tmp_path / "pings.txt")
    r = run(new, ARGS + [f"--wideband-pings={path}{value}"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    assert err.count("stub: msk144_set_wideband_pings(") == 1
    assert "stub: msk144_set_wideband_pings(ratio_q4 %d, memory %d, min_ref %d)" % params in err
    assert [int(v) for v in re.findall(r"stub: msk144_wideband_pings read (\d+)", err)] == list(range(PUSHES))
    assert [int(v) for v in re.findall(r"stub: msk144_wideband_ping_blocks\(channel -1\) after read (\d+)", err)] == list(range(PUSHES))
    assert err.index("stub: msk144_set_wideband(") < err.index("stub: msk144_set_wideband_pings(") < err.index("stub: msk144_wideband_pings read 0")
    events, t = stub_events(min_blocks)
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines == [wb.ping_event_line(e, OFFSETS[e["channel"]]) for e in events]
    if min_blocks <= 2:
        # the run across the boundary is one line, the run that was open at the end of the stream is the last, in integers as worked out by hand
        assert "ping ch=1 offset=0 start=0.400 dur=0.056 blocks=7 peak=20053 ref=2000 peak_db=10.0" in lines
        assert lines[-1] == "ping ch=0 offset=-24000 start=1.064 dur=0.016 blocks=2 peak=10056 ref=1003 peak_db=10.0"
        assert sum("ch=3" in l for l in lines) == (1 if min_blocks == 1 else 0)
    if min_blocks == 64:
        assert lines == []
    for l in lines:
        pc.parse_line(l)
    per_channel = [sum(e["channel"] == c for e in events) for c in range(len(OFFSETS))]
    active = sorted((c for c in range(len(OFFSETS)) if per_channel[c]), key=lambda c: -per_channel[c])
    want = (f"msk144hipdecoder: wideband pings: {len(events)} events on {len(active)} of {len(OFFSETS)} channels, "
            f"{t.up_blocks} of {t.total_blocks} blocks up" + ("; most active" + "".join(f" ch={c} ({per_channel[c]})" for c in active[:3]) if active else ""))
    assert want in err and t.total_blocks == len(OFFSETS) * (54 + 27 * (PUSHES - 1)) and t.up_blocks == 14
    assert err.index("channel I/Q components clipped") < err.index("msk144hipdecoder: wideband pings:")


def test_the_file_is_appended_to(new, tmp_path):
    path = str(tmp_path / "pings.txt")
    for _ in range(2):
        assert run(new, ARGS + [f"--wideband-pings={path}"], DATA, timeout=120).returncode == 0
    with open(path) as f:
        lines = f.read().splitlines()
    assert len(lines) == 2 * len(stub_events(2)[0]) and lines[:len(lines) // 2] == lines[len(lines) // 2:]


def test_the_parser():
    assert pc.host_parse("f") == (32, 2, 8, 1)
    assert pc.host_parse("some/file.txt:1.75:3:0") == (28, 3, 0, 13)
    assert pc.host_parse("f:1") == (16, 2, 8, 1) and pc.host_parse("f:4095.9") == (65534, 2, 8, 1)
    assert pc.host_parse("f:2.03") == (32, 2, 8, 1) and pc.host_parse("f:2.04") == (33, 2, 8, 1)      # rint(16 x RATIO)
    assert pc.host_parse("f:2:1:16") == (32, 1, 16, 1) and pc.host_parse("f:2:64") == (32, 64, 8, 1)
    for bad in ("", ":", ":2", "f:", "f:x", "f:0.9", "f:4096", "f:-1", "f:2:", "f:2:0", "f:2:65", "f:2:x", "f:2:2:", "f:2:2:-1", "f:2:2:17", "f:2:2:8:1", "f:2:2:8:"):
        assert pc.host_parse(bad) is None, bad


@pytest.mark.parametrize("bad", ["", ":", ":0.5", ":4096", ":x", ":2:0", ":2:65", ":2:2:17", ":2:2:-1", ":2:2:8:1", ":2:"])
def test_a_malformed_value_ends_the_program_before_any_library_call(new, tmp_path, bad):
    value = bad if bad == "" else str(tmp_path / "p.txt") + bad
    r = run(new, ARGS + ["--wideband-pings=" + value], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-pings" in r.stderr, bad
    assert b"Done" not in r.stdout
    assert not os.path.exists(tmp_path / "p.txt")


def test_a_file_that_cannot_be_opened_ends_the_program_before_any_library_call(new, tmp_path):
    path = str(tmp_path / "no_such_directory" / "pings.txt")
    r = run(new, ARGS + [f"--wideband-pings={path}:2:2"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"cannot open" in r.stderr and path.encode() in r.stderr
    assert b"Done" not in r.stdout


def test_the_option_needs_wideband_mode(new, tmp_path):
    path = str(tmp_path / "pings.txt")
    r = run(new, [f"--wideband-pings={path}"], DATA)
    assert r.returncode == 2 and b"--wideband-rate" in r.stderr and b"stub:" not in r.stderr
    assert not os.path.exists(path)


def test_a_library_without_the_entries_is_an_error(old, tmp_path):
    r = run(old, ARGS + [f"--wideband-pings={tmp_path / 'pings.txt'}"], DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_set_wideband_pings" in err and "stub: msk144_set_wideband(" not in err
    assert b"Done" not in r.stdout
    assert not os.path.exists(tmp_path / "pings.txt")        # no empty file is left behind


def test_no_option_no_new_call(new, old):
    outs = []
    for exe in (new, old):
        r = run(exe, ARGS, DATA, timeout=120)
        err = r.stderr.decode()
        assert r.returncode == 0
        assert "pings" not in err and "ping_blocks" not in err
        outs.append((re.sub(rb"date=\d{14}", b"date=X", r.stdout), re.sub(r"worst latency \d+ ms", "worst latency X ms", re.sub(r"\d+ late", "N late", err))))
    assert outs[0] == outs[1]


def test_help_names_the_option(new):
    out = run(new, ["--help"]).stdout.decode()
    assert "--wideband-pings=FILE[:RATIO[:MIN_BLOCKS[:MEMORY]]]" in out
    assert out.index("--wideband-spectrum") < out.index("--wideband-pings") < out.index("--taps-per-phase=K")
