"""CPU: msk144hipdecoder --wideband-audio against the stand-in library (tests/stub_hip/wideband_audio_stub.cpp, which takes the
capture's stand-in in as it is).

- The option makes exactly one msk144_set_wideband_audio call with the default design of its arguments, behind
  msk144_set_wideband_capture and ahead of every read; the audio rows are read once per push, behind that push's units.
- Beside every DIR/ch<c>_hop<k0>.cs8 lies DIR/ch<c>_hop<k0>.wav: the 44-byte header - PCM, one channel, 12000 Hz, 16 bits, block
  align 2, byte rate 24000, both sizes those of the finished segment - and hops x 5184 data bytes, the stand-in's rows in the
  segment's order; the file is wideband.wav_bytes of those rows.  The .cs8 files are those of a run without the option.
- The segment's line in capture.log gains ` wav=<name>`; the stderr summary gains the audio line.
- The parser (through libmsk144host.so) and the refusals: without --wideband-capture, a malformed value and arguments the design
  refuses - with the design's own message - end the program (exit 2) before it calls the library; against a stand-in without the
  entries the option is an error that names the missing entry.
- Without the option the program calls none of the new entries and leaves capture.log and DIR as they are today.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from host_stub import run, shared_program
from msk144cudecoder_amd import wideband as wb

RATE, OFFSETS, PUSHES = 240000, [-24000, 0, 12000, 36000, 48000], 4
ARGS = [f"--wideband-rate={RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, OFFSETS))]
DATA = bytes((5184 + (PUSHES - 1) * 2592) * RATE // 12000 * 2)
# the segments the capture's stand-in gives in `pings` mode (tests/test_wideband_capture_cli.py): name -> (channel, hops)
SEGMENTS = {"ch0_hop1": (0, [1, 2, 3, 4]), "ch1_hop0": (1, [0, 1, 2, 3]), "ch3_hop2": (3, [2]), "ch3_hop4": (3, [4])}


@pytest.fixture(scope="module")
def new():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_pings_stub.cpp", "wideband_audio_stub.cpp"))


@pytest.fixture(scope="module")
def old():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_pings_stub.cpp", "wideband_capture_stub.cpp"))


def stub_row(c, k):
    return (3 * ((17 * c + 5 * k + np.arange(wb.HOP_OUT)) % 2001 - 1000)).astype(np.int16)


def host_parse(arg, centre_default=0):
    """((halfwidth, centre, tone), '') as the program parses --wideband-audio=arg, else (None, the design's refusal text or '')."""
    L = C.CDLL(wb.HOST_LIB)
    out = np.zeros(3, dtype=np.int32)
    why = C.create_string_buffer(256)
    rc = L.msk144host_wideband_audio_parse(arg.encode(), C.c_int32(centre_default), out.ctypes.data_as(C.c_void_p), why, len(why))
    return (tuple(int(v) for v in out), "") if rc == 0 else (None, why.value.decode())


def read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def read_lines(path):
    with open(path) as f:
        return f.read().splitlines()


def test_the_wav_files_the_log_and_the_summary(new, old, tmp_path):
    pings, out, plain = str(tmp_path / "pings.txt"), str(tmp_path / "cap"), str(tmp_path / "plain")
    r = run(new, ARGS + [f"--wideband-pings={pings}:2:1", f"--wideband-capture={out}", "--wideband-audio"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    taps, phasor, shift = wb.audio_design(0, 1250, 1500)
    call = f"stub: msk144_set_wideband_audio(shift {shift}, tap31 {taps[31][0]} {taps[31][1]}, phasor1 {phasor[1][0]} {phasor[1][1]}, phasor95 {phasor[95][0]} {phasor[95][1]})"
    assert err.count("stub: msk144_set_wideband_audio(") == 1 and call in err
    assert err.index("stub: msk144_set_wideband_capture(") < err.index("stub: msk144_set_wideband_audio(") < err.index("stub: msk144_wideband_capture read 0")
    assert re.findall(r"stub: msk144_wideband_capture_audio read (\d+): (\d+) rows", err) == [("0", "2"), ("1", "3"), ("2", "3"), ("3", "2")]
    for i in range(PUSHES):       # behind the same push's units
        assert err.index(f"stub: msk144_wideband_capture read {i}:") < err.index(f"stub: msk144_wideband_capture_audio read {i}:")
        if i + 1 < PUSHES:
            assert err.index(f"stub: msk144_wideband_capture_audio read {i}:") < err.index(f"stub: msk144_wideband_capture read {i + 1}:")
    assert sorted(os.listdir(out)) == sorted(["capture.log"] + [n + e for n in SEGMENTS for e in (".cs8", ".wav")])
    for name, (c, hops) in SEGMENTS.items():
        b = read_bytes(os.path.join(out, name + ".wav"))
        le = lambda at, n: int.from_bytes(b[at:at + n], "little")
        data = len(hops) * 5184
        assert len(b) == 44 + data, name
        assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and b[36:40] == b"data"
        assert (le(4, 4), le(16, 4), le(20, 2), le(22, 2), le(24, 4), le(28, 4), le(32, 2), le(34, 2), le(40, 4)) == (36 + data, 16, 1, 1, 12000, 24000, 2, 16, data), name
        assert b == wb.wav_bytes(np.stack([stub_row(c, k) for k in hops])), name
        assert os.path.getsize(os.path.join(out, name + ".cs8")) == data
    assert read_lines(os.path.join(out, "capture.log")) == [
        "capture ch=3 offset=36000 hop=2 t=0.432 hops=1 file=ch3_hop2.cs8 wav=ch3_hop2.wav",
        "capture ch=0 offset=-24000 hop=1 t=0.216 hops=4 file=ch0_hop1.cs8 wav=ch0_hop1.wav",
        "capture ch=1 offset=0 hop=0 t=0.000 hops=4 file=ch1_hop0.cs8 wav=ch1_hop0.wav",
        "capture ch=3 offset=36000 hop=4 t=0.864 hops=1 file=ch3_hop4.cs8 wav=ch3_hop4.wav"]
    clamped = sum(c + k for c, hops in SEGMENTS.values() for k in hops)
    assert "msk144hipdecoder: wideband capture: 4 segments, 10 hops written, 51840 bytes, 1 units dropped" in err
    assert f"msk144hipdecoder: wideband audio: 4 WAV files, 25920 samples, {clamped} clamped, band 0 +-1250 Hz at 1500 Hz, shift {shift}" in err
    assert err.index("msk144hipdecoder: wideband capture:") < err.index("msk144hipdecoder: wideband audio:")
    # without the option: the same .cs8 files and ping lines, a log without the field, no .wav, no new call - with the stand-in that
    # has the entries and with the one that does not
    for k, exe in enumerate((new, old)):
        p2, o2 = str(tmp_path / f"pings{k}.txt"), plain + str(k)
        q = run(exe, ARGS + [f"--wideband-pings={p2}:2:1", f"--wideband-capture={o2}"], DATA, timeout=120)
        assert q.returncode == 0 and b"audio" not in q.stderr
        assert sorted(os.listdir(o2)) == sorted(["capture.log"] + [n + ".cs8" for n in SEGMENTS])
        for n in SEGMENTS:
            assert read_bytes(os.path.join(o2, n + ".cs8")) == read_bytes(os.path.join(out, n + ".cs8"))
        assert read_lines(os.path.join(o2, "capture.log")) == [l.split(" wav=")[0] for l in read_lines(os.path.join(out, "capture.log"))]
        assert read_lines(p2) == read_lines(pings)
        assert re.sub(rb"date=\d{14}", b"date=X", q.stdout) == re.sub(rb"date=\d{14}", b"date=X", r.stdout)


@pytest.mark.parametrize("value, centre, design", [
    ("=1000", [], (0, 1000, 1500)),
    ("=500:250:625", [], (250, 500, 625)),
    ("", ["--center-frequency=1500"], (1500, 1250, 1500)),
    ("=1250:-1000", ["--center-frequency=1500"], (-1000, 1250, 1500)),
    ("=3000:0:3000", [], (0, 3000, 3000)),
])
def test_the_arguments_reach_the_design(new, tmp_path, value, centre, design):
    out = str(tmp_path / "cap")
    r = run(new, ARGS + centre + [f"--wideband-capture={out}:2", "--wideband-audio" + value], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    taps, phasor, shift = wb.audio_design(*design)
    assert f"stub: msk144_set_wideband_audio(shift {shift}, tap31 {taps[31][0]} {taps[31][1]}, phasor1 {phasor[1][0]} {phasor[1][1]}, phasor95 {phasor[95][0]} {phasor[95][1]})" in err
    assert f"band {design[0]} +-{design[1]} Hz at {design[2]} Hz, shift {shift}" in err
    # a listed channel: one segment of every hop, one WAV file of all its rows
    assert read_bytes(os.path.join(out, "ch2_hop0.wav")) == wb.wav_bytes(np.stack([stub_row(2, k) for k in range(5)]))
    assert any(l.endswith(" hops=5 file=ch2_hop0.cs8 wav=ch2_hop0.wav") for l in read_lines(os.path.join(out, "capture.log")))


def test_the_parser():
    assert host_parse("") == ((1250, 0, 1500), "")
    assert host_parse("", 1500) == ((1250, 1500, 1500), "")
    assert host_parse("1000") == ((1000, 0, 1500), "")
    assert host_parse("1000:500") == ((1000, 500, 1500), "")
    assert host_parse("1000:-500:2000", 1500) == ((1000, -500, 2000), "")
    for bad in ("x", "1000:", "1000:x", "1000:0:", "1000:0:1500:1", ":", "1e3"):
        assert host_parse(bad) == (None, ""), bad
    # (the value, the design's arguments (centre, halfwidth, tone) it stands for, a word of the refusal)
    for bad, design, text in (("499", (0, 499, 1500), "half-width"), ("3001:0:3000", (0, 3001, 3000), "half-width"), ("1250:4751:4751", (4751, 1250, 4751), "|centre|"),
                              ("1250:0:1249", (0, 1250, 1249), "tone"), ("1250:0:4751", (0, 1250, 4751), "tone"), ("1250:0:1501", (0, 1250, 1501), "125"),
                              ("1250:100", (100, 1250, 1500), "125")):
        got = host_parse(bad)
        assert got[0] is None and text in got[1], bad
        with pytest.raises(ValueError) as e:
            wb.audio_design(*design)
        assert str(e.value) == got[1]        # the design's own message


@pytest.mark.parametrize("value, text", [
    ("=x", "bad value for --wideband-audio"), ("=1000:", "bad value for --wideband-audio"), ("=1000:0:1500:1", "bad value for --wideband-audio"),
    ("=499", "audio half-width must lie within 500..3000 Hz"), ("=1250:0:1501", "multiple of 125 Hz"), ("=1250:0:1000", "audio tone must lie within"),
    ("=1250:5000:5000", "|centre| + half-width <= 6000"),
])
def test_a_refused_value_ends_the_program_before_any_library_call(new, tmp_path, value, text):
    r = run(new, ARGS + [f"--wideband-capture={tmp_path / 'cap'}:2", "--wideband-audio" + value], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and text.encode() in r.stderr and b"--wideband-audio" in r.stderr, value
    assert b"Done" not in r.stdout and not os.path.exists(tmp_path / "cap")


def test_the_centre_default_is_checked_too(new, tmp_path):
    # --center-frequency=1400: tone 1500 - centre 1400 is no multiple of 125
    r = run(new, ARGS + ["--center-frequency=1400", f"--wideband-capture={tmp_path / 'cap'}:2", "--wideband-audio"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"multiple of 125 Hz" in r.stderr


def test_the_option_needs_the_capture_and_wideband_mode(new, tmp_path):
    r = run(new, ARGS + ["--wideband-audio"], DATA)
    assert r.returncode == 2 and b"--wideband-audio needs --wideband-capture=DIR" in r.stderr and b"stub:" not in r.stderr
    r = run(new, ["--wideband-audio=1000"], DATA)
    assert r.returncode == 2 and b"--wideband-audio needs --wideband-rate=HZ" in r.stderr and b"stub:" not in r.stderr


def test_a_library_without_the_entries_is_an_error_and_runs_every_other_mode(old, tmp_path):
    r = run(old, ARGS + [f"--wideband-capture={tmp_path / 'cap'}:0", "--wideband-audio"], DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_set_wideband_audio" in err and "--wideband-audio needs it" in err and "stub: msk144_set_wideband(" not in err
    assert b"Done" not in r.stdout and not os.path.exists(tmp_path / "cap")
    assert run(old, ARGS + [f"--wideband-capture={tmp_path / 'cap'}:0"], DATA, timeout=120).returncode == 0


def test_help_names_the_option(new):
    out = run(new, ["--help"]).stdout.decode()
    assert "--wideband-audio[=HALFWIDTH[:CENTRE[:TONE]]]" in out and "--skip-wav-header" in out and "31.5 samples" in out and "wav=<name>" in out
    assert out.index("--wideband-capture") < out.index("--wideband-audio") < out.index("--taps-per-phase=K")
