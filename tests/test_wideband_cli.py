"""msk144hipdecoder --wideband-rate on the CPU: option checks (exit 2 before any library call) and the wideband loop against the
stand-in library - tests/stub_hip/msk144hip_stub.cpp plus the wideband entries of tests/stub_hip/wideband_stub.cpp, whose push
hands every channel a marked hop."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "msk144cudecoder_amd", "host")
PROGRAM_SOURCES = ("snr_tracker.cpp", "result_filter.cpp", "unpack77.cpp", "postprocess.cpp", "window_decoder.cpp", "stream_loop.cpp", "main.cpp")


def _build(d, stubs):
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", os.path.join(d, "libmsk144hip.so")]
                   + [os.path.join(ROOT, "tests", "stub_hip", s) for s in stubs], check=True)
    out = os.path.join(d, "msk144hipdecoder_stub")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-o", out] + [os.path.join(HOST, f) for f in PROGRAM_SOURCES]
                   + ["-L" + d, "-lmsk144hip", "-Wl,-rpath," + d], check=True)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("wbstub")), ["msk144hip_stub.cpp", "wideband_stub.cpp"])


@pytest.fixture(scope="module")
def exe_old_stub(tmp_path_factory):
    """The program against a library without the wideband entries: it still links (they are resolved only for --wideband-rate)."""
    return _build(str(tmp_path_factory.mktemp("oldstub")), ["msk144hip_stub.cpp"])


def _run(exe, args, data=b"", timeout=60):
    return subprocess.run([exe] + args, input=data, capture_output=True, timeout=timeout)


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
    r = _run(exe, args)
    assert r.returncode == 2, (args, r.stderr.decode())
    assert message in r.stderr.decode()
    assert b"stub:" not in r.stderr                       # refused before the library was asked for anything


def test_missing_library_entries_are_an_error_not_a_fallback(exe_old_stub):
    r = _run(exe_old_stub, ["--wideband-rate=24000", "--channel-offsets=0"])
    assert r.returncode == 2 and b"no wideband channeliser" in r.stderr


def test_help_lists_the_wideband_options(exe):
    out = _run(exe, ["--help"]).stdout.decode()
    for opt in ("--wideband-rate=HZ", "--wideband-format=FMT", "--channel-offsets=", "--channel-grid=", "--wideband-gain=G", "--taps-per-phase=K"):
        assert opt in out


def _windows_seen(stdout, n):
    seen = {c: [] for c in range(n)}
    for line in stdout.strip().split("\n"):
        if line == "Done":
            continue
        m = re.match(r"^\*\*\*  (?:ch=(\d+); )?.*msg='([0-9A-F]+)'; $", line)
        assert m, line
        v = int(m.group(2), 16)
        seen[int(m.group(1) or 0)].append(((v >> 16) & 0xFFFF, v & 0xFFFF))
    return seen


@pytest.mark.parametrize("fmt, sample_bytes", [("cu8", 2), ("cs16", 4)])
def test_wideband_loop_decodes_every_push_on_every_channel(exe, fmt, sample_bytes):
    D, pushes, n = 4, 5, 6
    data = bytes((5184 + (pushes - 1) * 2592) * D * sample_bytes + 100)     # a short tail: the reference's end-of-input message
    r = _run(exe, ["--wideband-rate=48000", f"--wideband-format={fmt}", "--channel-grid=-15000:6000:6", "--wideband-gain=3.5", "--taps-per-phase=8"], data)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    taps = re.search(r"stub: msk144_set_wideband\(rate 48000, format (\d), K 8, gain 3.5, (\d+) taps summing to ([0-9.]+), 6 offsets, first -15000, last 15000\)", err)
    assert taps and int(taps.group(1)) == (0 if fmt == "cu8" else 2) and int(taps.group(2)) == 32 and float(taps.group(3)) == 1.0
    for c in range(n):
        assert f"ch={c} offset {-15000 + 6000 * c} Hz" in err
    assert "Center Frequency: 0Hz" in err
    seen = _windows_seen(r.stdout.decode(), n)
    for c in range(n):
        assert seen[c] == [(100 * c + k, 100 * c + k + 1) for k in range(pushes)], c
    assert "Incomplete read error. rc=" in err
    assert re.search(rf"wideband: {7 * pushes} of {2 * n * (5184 + (pushes - 1) * 2592)} channel I/Q components clipped", err)
