"""msk144hipdecoder --stream-pings / --stream-levels on the CPU: the real host sources against the stand-in library with
tests/stub_hip/stream_pings_stub.cpp, which works the records of a hop out with the host rule of csrc/stream_pings.h.  What is under
test is the program: the options and their refusals, which hop reaches which stream's tracker, the event log, both end-of-run
summaries, and that stdout does not change - all against stream_pings.StreamPings and StreamReport fed the same samples."""
import os
import re
import subprocess

import numpy as np
import pytest

from msk144cudecoder_amd import stream_pings as sp

import host_stub

STUBS = ("msk144hip_stub.cpp", "input_rate_stub.cpp", "stream_pings_stub.cpp")
DEFAULTS = dict(sp.STREAM_PINGS_DEFAULTS, min_blocks=2)


@pytest.fixture(scope="module")
def exe():
    return host_stub.shared_program(STUBS)


@pytest.fixture(scope="module")
def plain_exe():
    return host_stub.shared_program()


def undated(p):
    return re.sub(r"date=\d{14}", "date=X", p.stdout.decode())


def stream(n_hops, tag, seed, bursts=(), sigma=300.0):
    """A marked stream (host_stub.marked_stream: the stub decodes a record per window from the marks) of noise, with bursts
    (first sample, samples) twelve times as strong."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, sigma, size=5184 + n_hops * 2592)
    for at, n in bursts:
        x[at:at + n] *= 12.0
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    m = host_stub.marked_stream(n_hops, tag)
    x[m != 0] = m[m != 0]
    return x


def cut(x):
    """The stream as the program cuts it: a first hop of 5184 samples, then whole hops of 2592."""
    return [x[:5184]] + [x[5184 + 2592 * k:5184 + 2592 * (k + 1)] for k in range((len(x) - 5184) // 2592)] if len(x) >= 5184 else []


def expected(streams, **params):
    """(log lines per stream, the pings summary, the levels lines) of the model on the streams, hop k of every stream that has one."""
    p = dict(DEFAULTS, **params)
    model = sp.StreamPings(len(streams), min_blocks=p["min_blocks"], **{k: p[k] for k in ("ratio_q4", "memory", "min_ref", "shift")})
    report = sp.StreamReport(len(streams))
    hops = [cut(x) for x in streams]
    events = []
    for k in range(max(len(h) for h in hops)):
        ids = [c for c, h in enumerate(hops) if k < len(h)]
        _, lev, _, ev = model.push(ids, [k == 0] * len(ids), [hops[c][k] for c in ids])
        report.add(ids, lev, ev)
        events += ev
    tail = model.close()
    report.add_events(tail)
    events += tail
    return [[sp.stream_ping_line(e) for e in events if e["channel"] == c] for c in range(len(streams))], report.pings_line(model, p), report.levels_lines()


def check_run(p, log, streams, levels=True, **params):
    assert p.returncode == 0, p.stderr.decode()
    want_log, want_pings, want_levels = expected(streams, **params)
    got = log.read_text().splitlines()
    for c in range(len(streams)):
        assert [l for l in got if l.startswith(f"ping ch={c} ")] == want_log[c]
    assert len(got) == sum(len(l) for l in want_log)
    err = p.stderr.decode().splitlines()
    assert want_pings in err, [l for l in err if "stream pings" in l]
    assert [l for l in err if l.startswith("msk144hipdecoder: stream levels:")] == (want_levels if levels else [])
    return want_log


def scene():
    """Three streams: 0 has a burst across the boundary of its hops 1 and 2 and a short one; 1 ends two hops early, inside a burst;
    2 is silence."""
    a = stream(5, 10, 1, bursts=((5184 + 2592 - 96 * 3, 96 * 7), (5184 + 3 * 2592 + 960, 96 * 2)))
    b = stream(3, 40, 2, bursts=((5184 + 3 * 2592 - 96 * 4, 96 * 4),))
    c = np.zeros(5184 + 5 * 2592, dtype=np.int16)
    return [a, b, c]


def write(tmp_path, streams):
    paths = []
    for c, x in enumerate(streams):
        f = tmp_path / f"s{c}.raw"
        f.write_bytes(x.tobytes())
        paths.append(str(f))
    return paths


def test_option_parsing():
    assert sp.host_parse("f.log") == dict(ratio_q4=DEFAULTS["ratio_q4"], min_blocks=2, memory=8, shift=12, file_len=5)
    assert sp.host_parse("f:2.25:3:16:0") == dict(ratio_q4=36, min_blocks=3, memory=16, shift=0, file_len=1)
    assert sp.host_parse("f::5::24") == dict(ratio_q4=DEFAULTS["ratio_q4"], min_blocks=5, memory=8, shift=24, file_len=1)
    for bad in ("", ":2", "f:0.9", "f:4096", "f:x", "f:2:0", "f:2:65", "f:2:2:-1", "f:2:2:17", "f:2:2:8:-1", "f:2:2:8:25", "f:2:2:8:12:1"):
        assert sp.host_parse(bad) is None, bad


def test_refusals(exe, plain_exe, tmp_path):
    log = tmp_path / "p.log"
    for args, text in ((["--stream-pings=f:0.5"], "bad value for --stream-pings: 'f:0.5'"), (["--stream-pings=f:2:2:8:25"], "bad value for --stream-pings"),
                       ([f"--stream-pings={log}", "--read-mode=2"], "--stream-pings reads 16-bit audio: it excludes --read-mode=2"),
                       (["--stream-levels", "--read-mode=2"], "--stream-levels reads 16-bit audio: it excludes --read-mode=2"),
                       ([f"--stream-pings={log}", "--wideband-rate=240000", "--channel-offsets=0"], "--stream-pings reads the audio streams' hops: it excludes --wideband-rate"),
                       (["--stream-levels", "--wideband-rate=240000", "--channel-offsets=0"], "--stream-levels reads the audio streams' hops: it excludes --wideband-rate"),
                       ([f"--stream-pings={tmp_path}/none/p.log"], "--stream-pings: cannot open")):
        p = host_stub.run(exe, args, b"")
        assert p.returncode == 2 and text in p.stderr.decode(), (args, p.stderr.decode())
        assert p.stdout == b""
    assert not log.exists()
    # a library without the entries: refused by name, and the program without the options still runs against it
    p = host_stub.run(plain_exe, ["--stream-levels"], b"")
    assert p.returncode == 2 and "has no stream pings (msk144_set_stream_pings)" in p.stderr.decode()
    assert host_stub.run(plain_exe, [], b"").returncode == 0


def test_inputs_log_and_summaries_equal_the_model(exe, tmp_path):
    streams = scene()
    paths = write(tmp_path, streams)
    log = tmp_path / "pings.log"
    plain = host_stub.run(exe, ["--inputs=" + ",".join(paths)])
    p = host_stub.run(exe, ["--inputs=" + ",".join(paths), f"--stream-pings={log}", "--stream-levels"])
    want_log = check_run(p, log, streams)
    assert undated(p) == undated(plain) and "msg=" in undated(plain)
    assert f"stub: msk144_set_stream_pings(ratio_q4 {DEFAULTS['ratio_q4']}, memory 8, min_ref 96, shift 12, 3 streams)" in p.stderr.decode()
    # the run across the hop boundary is one event of seven blocks; stream 1's last event is closed by the end of the stream
    assert any(" blocks=7 " in l and " start=0.624 " in l for l in want_log[0])
    assert any(" blocks=4 " in l for l in want_log[1]) and want_log[2] == []
    assert "all hops zero ch=2" in p.stderr.decode()
    assert "stream pings" not in plain.stderr.decode() and "stream levels" not in plain.stderr.decode()


def test_parameters_reach_the_library_and_the_tracker(exe, tmp_path):
    streams = scene()[:2]
    paths = write(tmp_path, streams)
    log = tmp_path / "pings.log"
    p = host_stub.run(exe, ["--inputs=" + ",".join(paths), f"--stream-pings={log}:2.5:1:4:10"])
    check_run(p, log, streams, levels=False, ratio_q4=40, min_blocks=1, memory=4, shift=10)
    assert "stub: msk144_set_stream_pings(ratio_q4 40, memory 4, min_ref 96, shift 10, 2 streams)" in p.stderr.decode()


def test_levels_alone_write_no_log(exe, tmp_path):
    streams = scene()
    paths = write(tmp_path, streams)
    p = host_stub.run(exe, ["--inputs=" + ",".join(paths), "--stream-levels"])
    assert p.returncode == 0, p.stderr.decode()
    err = p.stderr.decode().splitlines()
    assert [l for l in err if l.startswith("msk144hipdecoder: stream levels:")] == expected(streams)[2]
    assert not any("stream pings:" in l for l in err) and sorted(os.listdir(tmp_path)) == sorted(os.path.basename(f) for f in paths)


def test_single_stdin_stream(exe, tmp_path):
    """One stream on stdin goes through the library's hop ring when an option is given: same stdout, a partial hop at the end."""
    x = scene()[0]
    log = tmp_path / "pings.log"
    data = x.tobytes() + bytes(14)
    plain = host_stub.run(exe, [], data)
    p = host_stub.run(exe, [f"--stream-pings={log}", "--stream-levels"], data)
    check_run(p, log, [x])
    assert p.stdout == plain.stdout or undated(p) == undated(plain)
    assert "ch=" not in p.stdout.decode() and "Incomplete read error. rc=7" in p.stderr.decode()
    assert host_stub.windows_seen(p.stdout.decode(), 1)[0] == [(10 + k, 11 + k) for k in range(6)]


def test_interleaved_on_two_devices(exe, tmp_path):
    """--interleaved with --devices: stream numbers in the log and the summaries are the program's, not a device's own."""
    streams = scene()[:1] + [stream(5, 70, 3, bursts=((9000, 96 * 3),)), scene()[2]]
    blocks = [np.stack([x[:5184] for x in streams]).tobytes()] + [np.stack([x[5184 + 2592 * k:5184 + 2592 * (k + 1)] for x in streams]).tobytes() for k in range(5)]
    log = tmp_path / "pings.log"
    env = dict(os.environ, MSK144_STUB_DEVICES="2")
    args = ["--interleaved=3", "--devices=0,1"]
    plain = subprocess.run([exe] + args, input=b"".join(blocks), capture_output=True, timeout=60, env=env)
    p = subprocess.run([exe] + args + [f"--stream-pings={log}", "--stream-levels"], input=b"".join(blocks), capture_output=True, timeout=60, env=env)
    check_run(p, log, streams)
    assert plain.returncode == 0 and sorted(undated(p).splitlines()) == sorted(undated(plain).splitlines())
    assert p.stderr.decode().count("stub: msk144_set_stream_pings(") == 2


def test_with_an_input_rate(exe, tmp_path):
    """--input-rate: the levels and pings are those of the 12 kHz hops behind the resampler - the stand-in's carry two samples of
    every input row and zeros."""
    row = 4 * 2592
    x = np.zeros(5 * row, dtype=np.int16)
    for k in range(5):
        x[k * row], x[k * row + 1] = 0x7777, 20 + k
    at_12k = np.zeros(5 * 2592, dtype=np.int16)
    for k in range(5):
        at_12k[k * 2592], at_12k[k * 2592 + 1] = 0x7777, 20 + k
    log = tmp_path / "pings.log"
    p = host_stub.run(exe, ["--input-rate=48000", f"--stream-pings={log}:2:1", "--stream-levels"], x.tobytes())
    check_run(p, log, [at_12k], ratio_q4=32, min_blocks=1)
    assert "input rate 48000 Hz" in p.stderr.decode()
