"""CPU: msk144hipdecoder --wideband-capture against the stand-in library (tests/stub_hip).

- DIR[:CHANNELS[:POST[:PRE]]] makes exactly one msk144_set_wideband_capture call with the parsed parameters and
  max_units = min(2 x channels, 512), behind msk144_set_wideband and ahead of every read; the units are read once per push, behind
  that push's ping records.
- DIR holds the segment files wideband.CaptureSegments makes of the stand-in's units, byte for byte, and capture.log its lines: a
  gap (the stand-in drops a unit) ends a segment, the end of the stream ends the rest.  A second run into the same DIR starts
  capture.log afresh.
- With --wideband-pings every ping line gains ` file=<name> at=<sample>`, ` file=-` for the event whose hop was dropped; up to that
  field the ping lines, and the decode lines altogether, are those of a run without the option.
- The stderr summary names segments, hops written, bytes and dropped units.
- The parser (through libmsk144host.so) and the refusals: a malformed value, `pings` without --wideband-pings, a channel that does
  not exist, a DIR that cannot be made and the option without --wideband-rate end the program (exit 2) before it calls the library;
  against the stand-in without the entries the option is an error that names the missing entry, and every other mode still runs.
- Without the option the program calls none of the new entries and prints what it printed before.
"""
import os
import re

import numpy as np
import pytest

import wideband_capture_check as cc
from host_stub import run, shared_program
from msk144cudecoder_amd import wideband as wb

RATE, OFFSETS, PUSHES = 240000, [-24000, 0, 12000, 36000, 48000], 4
ARGS = [f"--wideband-rate={RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, OFFSETS))]
DATA = bytes((5184 + (PUSHES - 1) * 2592) * RATE // 12000 * 2)
# (read, channel, hop, flags): the rule of tests/stub_hip/wideband_capture_stub.cpp; read 2 also reports one unit dropped
PLAN = [(0, 1, 0, 4), (0, 1, 1, 1), (1, 0, 1, 4), (1, 0, 2, 1), (1, 1, 2, 1), (2, 0, 3, 1), (2, 1, 3, 8), (2, 3, 2, 4), (3, 0, 4, 1), (3, 3, 4, 8)]


@pytest.fixture(scope="module")
def new():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_pings_stub.cpp", "wideband_capture_stub.cpp"))


@pytest.fixture(scope="module")
def old():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_pings_stub.cpp"))


def stub_units(i, listed=()):
    u = [(c, k, f) for r, c, k, f in PLAN if r == i]
    for k in ((0, 1) if i == 0 else (i + 1,)):
        u += [(c, k, 2) for c in listed]
    u.sort(key=lambda x: (x[0], x[1]))
    units = np.array([(c, f, k) for c, k, f in u], dtype=wb.CAPTURE_DTYPE)
    j = np.arange(wb.CAPTURE_UNIT_BYTES)
    data = np.stack([((31 * c + 7 * k + j) % 251 - 125).astype(np.int8) for c, k, _ in u])
    return units, data


def model_dir(path, listed=()):
    """What wideband.CaptureSegments writes for the stand-in's units; returns the segments object."""
    os.makedirs(path)
    seg = wb.CaptureSegments(path, OFFSETS)
    for i in range(PUSHES):
        seg.push(*stub_units(i, listed))
    return seg


def same_files(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    for n in names:
        with open(os.path.join(a, n), "rb") as f, open(os.path.join(b, n), "rb") as g:
            assert f.read() == g.read(), n
    return names


def read_lines(path):
    with open(path) as f:
        return f.read().splitlines()


def test_pings_mode_writes_the_segments_and_the_file_fields(new, old, tmp_path):
    pings, plain, out = str(tmp_path / "pings.txt"), str(tmp_path / "plain.txt"), str(tmp_path / "cap")
    r = run(new, ARGS + [f"--wideband-pings={pings}:2:1", f"--wideband-capture={out}"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    assert err.count("stub: msk144_set_wideband_capture(") == 1 and "stub: msk144_set_wideband_capture(pre 1, post 1, max_units 10, listed)" in err
    assert err.index("stub: msk144_set_wideband(") < err.index("stub: msk144_set_wideband_capture(") < err.index("stub: msk144_wideband_capture read 0")
    assert re.findall(r"stub: msk144_wideband_capture read (\d+): (\d+) of (\d+) units", err) == [("0", "2", "2"), ("1", "3", "3"), ("2", "3", "4"), ("3", "2", "2")]
    for i in range(PUSHES):       # behind the same push's ping records
        assert err.index(f"stub: msk144_wideband_pings read {i}\n") < err.index(f"stub: msk144_wideband_capture read {i}:")
        if i + 1 < PUSHES:
            assert err.index(f"stub: msk144_wideband_capture read {i}:") < err.index(f"stub: msk144_wideband_pings read {i + 1}\n")
    # the files are the model's, and they are what the rule says
    seg = model_dir(str(tmp_path / "want"))
    seg.close()
    names = same_files(out, str(tmp_path / "want"))
    assert names == ["capture.log", "ch0_hop1.cs8", "ch1_hop0.cs8", "ch3_hop2.cs8", "ch3_hop4.cs8"]
    assert [os.path.getsize(os.path.join(out, n)) for n in names[1:]] == [4 * 5184, 4 * 5184, 5184, 5184]
    assert read_lines(os.path.join(out, "capture.log")) == [
        "capture ch=3 offset=36000 hop=2 t=0.432 hops=1 file=ch3_hop2.cs8",          # ended by the gap: hop 3 was dropped
        "capture ch=0 offset=-24000 hop=1 t=0.216 hops=4 file=ch0_hop1.cs8",
        "capture ch=1 offset=0 hop=0 t=0.000 hops=4 file=ch1_hop0.cs8",
        "capture ch=3 offset=36000 hop=4 t=0.864 hops=1 file=ch3_hop4.cs8"]
    assert "msk144hipdecoder: wideband capture: 4 segments, 10 hops written, 51840 bytes, 1 units dropped" in err
    assert err.index("msk144hipdecoder: wideband pings:") < err.index("msk144hipdecoder: wideband capture:")
    # the ping lines: those of a run without capture, plus the file fields of the model
    q = run(old, ARGS + [f"--wideband-pings={plain}:2:1"], DATA, timeout=120)
    masked = [re.sub(rb"date=\d{14}", b"date=X", p.stdout) for p in (q, r)]
    assert q.returncode == 0 and masked[0] == masked[1] and masked[0].count(b"\n") > 4
    before, got = read_lines(plain), read_lines(pings)
    assert len(before) == len(got) == 5
    fields = []
    for b, g in zip(before, got):
        assert g.startswith(b + " file=")
        d = dict(f.split("=") for f in b.split()[1:])
        start = round(float(d["start"]) / 0.008)
        assert g == b + seg.locate(int(d["ch"]), start)
        fields.append(g[len(b):])
    # in the tracker's order, by the push an event closes in: the run of channel 1 across the first boundary (g = 50: hop 1, block 23,
    # the file's second hop), the run of channel 0 in hop 2, the one-block run of channel 3 in the dropped hop 3, the run of channel 0
    # in hop 3, and the one still open at the end
    assert fields == [" file=ch1_hop0.cs8 at=%d" % (2592 + 23 * 96), " file=ch0_hop1.cs8 at=%d" % (2592 + 25 * 96), " file=-", " file=ch0_hop1.cs8 at=%d" % (2 * 2592 + 25 * 96),
                      " file=ch0_hop1.cs8 at=%d" % (3 * 2592 + 25 * 96)]


@pytest.mark.parametrize("value, call, listed", [
    (":2", "pre 1, post 1, max_units 10, listed 2", [2]),
    (":4,2:3", "pre 1, post 3, max_units 10, listed 4 2", [4, 2]),
    (":2:0:0", "pre 0, post 0, max_units 10, listed 2", [2]),
])
def test_a_list_without_the_ping_detector(new, tmp_path, value, call, listed):
    out = str(tmp_path / "cap")
    r = run(new, ARGS + [f"--wideband-capture={out}{value}"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert f"stub: msk144_set_wideband_capture({call})" in err and "pings" not in err
    assert len(re.findall(r"stub: msk144_wideband_capture read", err)) == PUSHES
    seg = model_dir(str(tmp_path / "want"), listed)
    seg.close()
    names = same_files(out, str(tmp_path / "want"))
    assert "ch2_hop0.cs8" in names and os.path.getsize(os.path.join(out, "ch2_hop0.cs8")) == 5 * 5184        # a listed channel: one segment, every hop
    assert f"msk144hipdecoder: wideband capture: {seg.segments} segments, {seg.hops} hops written, {seg.bytes} bytes, 1 units dropped" in err


def test_a_second_run_into_the_same_directory_starts_the_log_afresh(new, tmp_path):
    """A run overwrites the segments of the same name, so capture.log holds that run's lines alone: every line names a file of the
    length it states.  A segment only the first run wrote (ch4_hop0.cs8) stays, with no line."""
    out = str(tmp_path / "cap")
    for value in (":4,2", ":2"):
        r = run(new, ARGS + [f"--wideband-capture={out}{value}"], DATA, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
    seg = model_dir(str(tmp_path / "want"), [2])
    seg.close()
    assert read_lines(os.path.join(out, "capture.log")) == read_lines(str(tmp_path / "want" / "capture.log"))
    assert sorted(set(os.listdir(out)) - set(os.listdir(tmp_path / "want"))) == ["ch4_hop0.cs8"]
    for line in read_lines(os.path.join(out, "capture.log")):
        d = dict(f.split("=") for f in line.split()[1:])
        assert os.path.getsize(os.path.join(out, d["file"])) == int(d["hops"]) * wb.CAPTURE_UNIT_BYTES, line


def test_pings_with_explicit_fields(new, tmp_path):
    out = str(tmp_path / "cap")
    r = run(new, ARGS + [f"--wideband-pings={tmp_path / 'p.txt'}", f"--wideband-capture={out}:pings:16:0"], DATA, timeout=120)
    assert r.returncode == 0 and "stub: msk144_set_wideband_capture(pre 0, post 16, max_units 10, listed)" in r.stderr.decode()


def test_the_parser():
    assert cc.host_parse("dir") == dict(by_pings=True, post=1, pre=1, dir_len=3, channels=[])
    assert cc.host_parse("d:pings:0:0") == dict(by_pings=True, post=0, pre=0, dir_len=1, channels=[])
    assert cc.host_parse("d:3,1,2:16") == dict(by_pings=False, post=16, pre=1, dir_len=1, channels=[3, 1, 2])
    assert cc.host_parse("d:" + ",".join(map(str, range(16))))["channels"] == list(range(16))
    for bad in ("", ":1", "d:", "d:x", "d:-1", "d:1,", "d:1,1", "d:" + ",".join(map(str, range(17))), "d:1:17", "d:1:-1", "d:1:1:2", "d:1:1:-1", "d:1:1:1:1", "d:pings:x", "d:1::1"):
        assert cc.host_parse(bad) is None, bad
    assert [cc.host_default_max_units(c) for c in (1, 5, 255, 256, 257, 4096)] == [2, 10, 510, 512, 512, 512]
    assert [wb.capture_default_max_units(c) for c in (1, 5, 255, 256, 257, 4096)] == [2, 10, 510, 512, 512, 512]


@pytest.mark.parametrize("bad", ["", ":", ":x", ":-1", ":1,", ":1,1", ":5", ":0,5", ":" + ",".join(map(str, range(17))), ":1:17", ":1:1:2", ":1:1:1:1", ":pings", None])
def test_a_malformed_value_ends_the_program_before_any_library_call(new, tmp_path, bad):
    # ":5": there are five channels, 0..4; ":pings" and the bare DIR (None) need --wideband-pings
    value = "" if bad == "" else str(tmp_path / "cap") + (bad or "")
    r = run(new, ARGS + ["--wideband-capture=" + value], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-capture" in r.stderr, bad
    assert b"Done" not in r.stdout
    assert not os.path.exists(tmp_path / "cap")


def test_a_directory_that_cannot_be_made_ends_the_program_before_any_library_call(new, tmp_path):
    path = str(tmp_path / "no_such_directory" / "cap")
    r = run(new, ARGS + [f"--wideband-capture={path}:0"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"cannot write under" in r.stderr and path.encode() in r.stderr
    assert b"Done" not in r.stdout


def test_the_option_needs_wideband_mode(new, tmp_path):
    path = str(tmp_path / "cap")
    r = run(new, [f"--wideband-capture={path}:0"], DATA)
    assert r.returncode == 2 and b"--wideband-rate" in r.stderr and b"stub:" not in r.stderr
    assert not os.path.exists(path)


def test_a_library_without_the_entries_is_an_error_and_runs_every_other_mode(old, tmp_path):
    r = run(old, ARGS + [f"--wideband-capture={tmp_path / 'cap'}:0"], DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_set_wideband_capture" in err and "stub: msk144_set_wideband(" not in err
    assert b"Done" not in r.stdout
    assert not os.path.exists(tmp_path / "cap")        # no empty directory is left behind
    assert run(old, ARGS, DATA, timeout=120).returncode == 0
    assert run(old, ARGS + [f"--wideband-pings={tmp_path / 'p.txt'}"], DATA, timeout=120).returncode == 0


def test_no_option_no_new_call(new, old, tmp_path):
    outs = []
    for k, exe in enumerate((new, old)):
        path = str(tmp_path / f"pings{k}.txt")
        r = run(exe, ARGS + [f"--wideband-pings={path}"], DATA, timeout=120)
        err = r.stderr.decode()
        assert r.returncode == 0
        assert "capture" not in err
        outs.append((re.sub(rb"date=\d{14}", b"date=X", r.stdout), read_lines(path), re.sub(r"worst latency \d+ ms", "worst latency X ms", re.sub(r"\d+ late", "N late", err))))
    assert outs[0] == outs[1] and not any("file=" in l for l in outs[0][1])


def test_help_names_the_option(new):
    out = run(new, ["--help"]).stdout.decode()
    assert "--wideband-capture=DIR[:CHANNELS[:POST[:PRE]]]" in out and "capture.log" in out and "min(2 x channels, 512)" in out
    assert out.index("--wideband-waterfall") < out.index("--wideband-capture") < out.index("--taps-per-phase=K")
