"""msk144hipdecoder on the CPU: the real host sources linked against tests/stub_hip, a stand-in for libmsk144hip.so that decodes
nothing and reports, per hop, which window it was handed.  The one build recipe, and the marked streams the stub's records are
read back from, for test_host_loop.py, the test_wideband*_cli.py files, test_host_sanitizers.py and tools/host_loop_stress.py."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "msk144cudecoder_amd", "host")
PROGRAM_SOURCES = ("snr_tracker.cpp", "result_filter.cpp", "unpack77.cpp", "postprocess.cpp", "window_decoder.cpp", "stream_loop.cpp", "main.cpp")


# every wideband entry the stand-in has, and the one command line that switches every wideband option on (five channels, PUSHES pushes)
WIDEBAND_STUBS = ("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_levels_stub.cpp", "wideband_blanker_stub.cpp", "wideband_spectrum_stub.cpp", "wideband_pings_stub.cpp",
                  "wideband_pingband_stub.cpp", "wideband_waterfall_stub.cpp", "wideband_capture_stub.cpp")
WIDEBAND_RATE, WIDEBAND_OFFSETS, WIDEBAND_PUSHES = 240000, (-24000, 0, 12000, 36000, 48000), 4
WIDEBAND_DATA = bytes((5184 + (WIDEBAND_PUSHES - 1) * 2592) * WIDEBAND_RATE // 12000 * 2)


def wideband_all_options(dir):
    """The arguments; the spectrum, ping and waterfall files and the capture directory lie under `dir`."""
    d = str(dir)
    return [f"--wideband-rate={WIDEBAND_RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, WIDEBAND_OFFSETS)), "--wideband-gain=auto", "--wideband-levels",
            "--wideband-blanker", f"--wideband-spectrum={d}/spectrum.txt:256:2", f"--wideband-pings={d}/pings.txt", "--wideband-pings-band", f"--wideband-waterfall={d}/waterfall.txt",
            f"--wideband-capture={d}/capture"]


def build_program(dir, stubs=("msk144hip_stub.cpp",), flags=("-O1",)):
    """Compile the stand-in library from `stubs` and the program against it, both in `dir`; returns the program's path."""
    d = str(dir)
    common = ["g++", *flags, "-std=c++17", "-pthread"]
    subprocess.run(common + ["-fPIC", "-shared", "-o", os.path.join(d, "libmsk144hip.so")]
                   + [os.path.join(ROOT, "tests", "stub_hip", s) for s in stubs], check=True)
    out = os.path.join(d, "msk144hipdecoder_stub")
    subprocess.run(common + ["-ffp-contract=off", "-o", out] + [os.path.join(HOST, f) for f in PROGRAM_SOURCES]
                   + ["-L" + d, "-lmsk144hip", "-Wl,-rpath," + d], check=True)
    return out


@functools.lru_cache(maxsize=None)
def shared_program(stubs=("msk144hip_stub.cpp",)):
    """build_program once per session and set of stubs, for the test modules that only run the program."""
    d = tempfile.mkdtemp(prefix="msk144hipdecoder_stub_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return build_program(d, stubs)


def run(exe, args, data=b"", timeout=60):
    return subprocess.run([exe] + args, input=data, capture_output=True, timeout=timeout)


def marked_stream(n_hops, tag):
    """Stream of n_hops + 1 windows; half-window k (2592 samples) starts with 0x7777, tag + k: the stub reports, per window, the
    second sample of both halves."""
    x = np.zeros(5184 + n_hops * 2592, dtype=np.int16)
    for k in range(n_hops + 2):
        x[k * 2592] = 0x7777
        x[k * 2592 + 1] = tag + k
    return x


def windows_seen(stdout, n_streams, devices=None):
    """{channel: [(first half id, second half id), ...]} in output order, from the telemetry text of the stub's records.
    `devices` (a dict) receives {channel: set of device ordinals whose handle decoded it}."""
    seen = {c: [] for c in range(n_streams)}
    for line in stdout.strip().split("\n"):
        if line == "Done":
            continue
        m = re.match(r"^\*\*\*  (?:ch=(\d+); )?.*msg='([0-9A-F]+)'; $", line)
        assert m, line
        v = int(m.group(2), 16)
        ch = int(m.group(1) or 0)     # the stream the host attributes the record to; v >> 32 is only its position in the compact batch
        seen[ch].append(((v >> 16) & 0xFFFF, v & 0xFFFF))
        if devices is not None:
            devices.setdefault(ch, set()).add(v >> 56)
    return seen
