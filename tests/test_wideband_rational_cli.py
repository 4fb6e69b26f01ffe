"""msk144hipdecoder --wideband-rate at rational rates (12000 x P/Q), on the CPU: the rate rule (exit 2 before any library call) and
the wideband loop against the stand-in library - tests/stub_hip/msk144hip_stub.cpp plus tests/stub_hip/wideband_stub.cpp,
whose slots hold 5184 P/Q samples and whose push hands every channel a marked hop."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "msk144cudecoder_amd", "host")
PROGRAM_SOURCES = ("snr_tracker.cpp", "result_filter.cpp", "unpack77.cpp", "postprocess.cpp", "window_decoder.cpp", "stream_loop.cpp", "main.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("wbrstub"))
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", os.path.join(d, "libmsk144hip.so")]
                   + [os.path.join(ROOT, "tests", "stub_hip", s) for s in ("msk144hip_stub.cpp", "wideband_stub.cpp")], check=True)
    out = os.path.join(d, "msk144hipdecoder_stub")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-o", out] + [os.path.join(HOST, f) for f in PROGRAM_SOURCES]
                   + ["-L" + d, "-lmsk144hip", "-Wl,-rpath," + d], check=True)
    return out


def _run(exe, args, data=b"", timeout=120):
    return subprocess.run([exe] + args, input=data, capture_output=True, timeout=timeout)


@pytest.mark.parametrize("rate, message", [
    ("44100", "multiple of 12000"),           # the 44.1 kHz family: not a multiple of 125
    ("2048001", "multiple of 12000"),
    ("23875", "2 <= D <= 512"),               # a multiple of 125 below 24000
    ("6144125", "2 <= D <= 512"),             # ... above 6144000
])
def test_refused_rates_exit_2(exe, rate, message):
    r = _run(exe, [f"--wideband-rate={rate}", "--channel-offsets=0"])
    err = r.stderr.decode()
    assert r.returncode == 2, err
    assert message in err
    assert "multiple of 125" in err or "2 <= D <= 512" in err
    assert b"stub:" not in r.stderr


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


@pytest.mark.parametrize("rate, P, Q, fmt, sample_bytes", [(2048000, 512, 3, "cu8", 2), (250000, 125, 6, "cs16", 4), (96125, 769, 96, "cs8", 2)])
def test_rational_loop_decodes_every_push_on_every_channel(exe, rate, P, Q, fmt, sample_bytes):
    pushes, n = 5, 4
    data = bytes((5184 + (pushes - 1) * 2592) * P // Q * sample_bytes + 100)   # a short tail: the end-of-input message
    r = _run(exe, [f"--wideband-rate={rate}", f"--wideband-format={fmt}", "--channel-grid=-18000:12000:4"], data)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    taps = re.search(rf"stub: msk144_set_wideband\(rate {rate}, format \d, K 16, gain 100, (\d+) taps summing to ([0-9.]+), 4 offsets", err)
    assert taps and int(taps.group(1)) == 16 * P and abs(float(taps.group(2)) - Q) < 1e-6
    assert f"resampling {P}/{Q}, filter 16 x {P} taps" in err
    seen = _windows_seen(r.stdout.decode(), n)
    for c in range(n):
        assert seen[c] == [(100 * c + k, 100 * c + k + 1) for k in range(pushes)], c
    assert "Incomplete read error. rc=" in err


def test_integer_rate_summary_is_unchanged(exe):
    D, pushes = 4, 2
    data = bytes((5184 + (pushes - 1) * 2592) * D * 2)
    r = _run(exe, ["--wideband-rate=48000", "--channel-offsets=0,6000"], data)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert "wideband input 48000 sps cu8 on stdin, decimation 4, filter 16 x 4 taps, gain 100, 2 channels" in err
    assert "resampling" not in err


def test_help_documents_the_rate_rule(exe):
    out = _run(exe, ["--help"]).stdout.decode()
    assert "multiple of 125" in out and "2048000" in out
