"""msk144hipdecoder --wideband-rate above 6.144 Msps (the two-stage bank), on the CPU: the rate rule (exit 2 before any library call)
and the wideband loop against the stand-in library - tests/stub_hip/msk144hip_stub.cpp plus tests/stub_hip/wideband_stub.cpp,
whose slots hold 5184 Fs/12000 samples and whose push hands every channel a marked hop."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "msk144cudecoder_amd", "host")
PROGRAM_SOURCES = ("snr_tracker.cpp", "result_filter.cpp", "unpack77.cpp", "postprocess.cpp", "window_decoder.cpp", "stream_loop.cpp", "main.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("wbbstub"))
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", os.path.join(d, "libmsk144hip.so")]
                   + [os.path.join(ROOT, "tests", "stub_hip", s) for s in ("msk144hip_stub.cpp", "wideband_stub.cpp")], check=True)
    out = os.path.join(d, "msk144hipdecoder_stub")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-o", out] + [os.path.join(HOST, f) for f in PROGRAM_SOURCES]
                   + ["-L" + d, "-lmsk144hip", "-Wl,-rpath," + d], check=True)
    return out


def _run(exe, args, data=b"", timeout=300):
    return subprocess.run([exe] + args, input=data, capture_output=True, timeout=timeout)


@pytest.mark.parametrize("rate, message", [
    ("6152001", "multiple of 125"),           # above 6.144 Msps and not a multiple of 125
    ("61448000", "2 <= D <= 512"),            # a multiple of 8000 above 61.44 Msps
    ("12500000", "2 <= D <= 512"),            # a multiple of 125, not of 8000
    ("6156000", "2 <= D <= 512"),
    ("6144125", "2 <= D <= 512"),
    ("23875", "2 <= D <= 512"),
    ("44100", "multiple of 125"),
])
def test_refused_rates_exit_2(exe, rate, message):
    r = _run(exe, [f"--wideband-rate={rate}", "--channel-offsets=0"])
    err = r.stderr.decode()
    assert r.returncode == 2, err
    assert message in err
    assert b"stub:" not in r.stderr


def test_offset_limit_at_a_bank_rate(exe):
    r = _run(exe, ["--wideband-rate=10000000", "--channel-offsets=0,4994001"])
    assert r.returncode == 2 and "outside" in r.stderr.decode()


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


@pytest.mark.parametrize("rate, fmt, sample_bytes, pushes", [(6152000, "cu8", 2, 3), (8000000, "cs8", 2, 3), (10000000, "cs16", 4, 3),
                                                             (20000000, "cu8", 2, 2), (61440000, "cu8", 2, 2)])
def test_bank_rates_decode_every_push_on_every_channel(exe, rate, fmt, sample_bytes, pushes):
    n = 4
    lim = rate // 2 - 6000
    offsets = [-lim, -rate // 128, rate // 128, lim]
    data = bytes((5184 + (pushes - 1) * 2592) * rate // 12000 * sample_bytes + 100)   # a short tail: the end-of-input message
    r = _run(exe, [f"--wideband-rate={rate}", f"--wideband-format={fmt}", "--channel-offsets=" + ",".join(map(str, offsets))], data)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    rate2 = rate // 32
    from math import gcd
    P2, Q2 = rate2 // gcd(rate2, 12000), 12000 // gcd(rate2, 12000)
    taps = re.search(rf"stub: msk144_set_wideband\(rate {rate}, format \d, K 16, gain 100, (\d+) taps summing to ([0-9.]+), 4 offsets", err)
    assert taps and int(taps.group(1)) == 16 * P2 and abs(float(taps.group(2)) - Q2) < 1e-6
    stage2 = f"decimation {P2}" if Q2 == 1 else f"resampling {P2}/{Q2}"
    assert f"stage 1: 64-band analysis bank, 3 bands occupied, sub-band rate {rate2} sps, filter 8 x 64 taps; stage 2: {stage2}, filter 16 x {P2} taps" in err
    seen = _windows_seen(r.stdout.decode(), n)
    for c in range(n):
        assert seen[c] == [(100 * c + k, 100 * c + k + 1) for k in range(pushes)], c
    assert "Incomplete read error. rc=" in err


def test_help_documents_the_bank_range(exe):
    out = _run(exe, ["--help"]).stdout.decode()
    assert "multiple of 125" in out and "2048000" in out
    assert "multiple of 8000 up to 61440000" in out and "HZ/32" in out
