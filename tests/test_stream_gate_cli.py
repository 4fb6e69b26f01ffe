"""msk144hipdecoder --stream-gate on the CPU: the real host sources against the stand-in library of
tests/stub_hip/stream_gate_stub.cpp, which works the list of a hop out with the host rules of csrc/stream_pings.h and
csrc/stream_gate.h.  What is under test is the program: the option and its refusals, which hop's list reaches which stream, that
streams the gate did not list still get their SNR update, the summary line, stdout against the ungated run and the model, and the
ALWAYS streams of each device's decoder - all against stream_pings.StreamPings and StreamGate fed the same samples."""
import os
import re
import subprocess

import numpy as np
import pytest

from msk144cudecoder_amd import stream_pings as sp

import host_stub
from test_stream_pings_cli import cut, scene, stream, write

STUBS = ("stream_gate_stub.cpp",)
LINE = re.compile(r"^\*\*\*  (?:ch=(\d+); )?(.*)msg='([0-9A-F]+)'; $")


@pytest.fixture(scope="module")
def exe():
    return host_stub.shared_program(STUBS)


@pytest.fixture(scope="module")
def plain_exe():
    return host_stub.shared_program(("msk144hip_stub.cpp", "input_rate_stub.cpp", "stream_pings_stub.cpp"))


def lines_of(p):
    """stdout as {stream: [(everything ahead of the message with the date masked - snr= is in it, (first half id, second half id))]}:
    the stand-in's message also carries the window's index in the decoded batch and the device, which a gate changes and the
    program never prints on their own."""
    out = {}
    text = p.stdout.decode().strip().split("\n")
    assert p.returncode == 0 and text[-1] == "Done", p.stderr.decode()
    for l in text[:-1]:
        m = LINE.match(l)
        assert m, l
        v = int(m.group(3), 16)
        out.setdefault(int(m.group(1) or 0), []).append((re.sub(r"date=\d{14}", "date=X", m.group(2)), ((v >> 16) & 0xFFFF, v & 0xFFFF)))
    return out


def model_lists(streams, detector=None, **gate):
    """{stream: the hops k at which the gate lists it}, the stream windows decoded, pushed, dropped and the busiest hop, from the
    models on the streams, hop k of every stream that has one.  detector None: the defaults."""
    pings, g = sp.StreamPings(len(streams), **(detector or {})), sp.StreamGate(len(streams), **gate)
    hops = [cut(x) for x in streams]
    listed = {c: [] for c in range(len(streams))}
    decoded = pushed = dropped = busiest = 0
    for k in range(max(len(h) for h in hops)):
        ids = [c for c, h in enumerate(hops) if k < len(h)]
        rec, _, en, _ = pings.push(ids, [k == 0] * len(ids), [hops[c][k] for c in ids])
        positions, total = g.push(ids, [k == 0] * len(ids), rec, en)
        for j in positions:
            listed[ids[j]].append(k)
        decoded += len(positions)
        pushed += len(ids)
        dropped += total - len(positions)
        busiest = max(busiest, len(positions))
    return listed, decoded, pushed, dropped, busiest


def summary_of(p):
    l = [x for x in p.stderr.decode().splitlines() if x.startswith("msk144hipdecoder: stream gate:")]
    assert len(l) == 1, p.stderr.decode()
    return l[0]


def check_stdout(p, plain, listed, tag_of):
    """Every stream's lines are the ungated run's lines of the windows the gate lists, snr= included; window k of a stream carries
    the ids (tag + k, tag + k + 1)."""
    got, want = lines_of(p), lines_of(plain)
    for c, ks in listed.items():
        ids = [(tag_of[c] + k, tag_of[c] + k + 1) for k in ks] if tag_of[c] is not None else []
        assert [w for _, w in got.get(c, [])] == ids, (c, got.get(c), ids)
        assert got.get(c, []) == [l for l in want.get(c, []) if l[1] in ids]


def test_option_parsing():
    assert sp.host_gate_parse("") == dict(hold=1, min_up=1, max_streams=0, ratio_q4=0, always=[])
    assert sp.host_gate_parse("2:3:4:2.5:0,7") == dict(hold=2, min_up=3, max_streams=4, ratio_q4=40, always=[0, 7])
    assert sp.host_gate_parse("::::5") == dict(hold=1, min_up=1, max_streams=0, ratio_q4=0, always=[5])
    assert sp.host_gate_parse("0:27:0:0") == dict(hold=0, min_up=27, max_streams=0, ratio_q4=0, always=[])
    assert sp.host_gate_parse(":::1.75")["ratio_q4"] == 28
    for bad in ("17", "-1", "x", "1:0", "1:28", "1:1:-1", "1:1:1:0.5", "1:1:1:4096", "1:1:1:x", "1:1:1:2:1,1", "1:1:1:2:-1", "1:1:1:2:a", "1:1:1:2:3:4"):
        assert sp.host_gate_parse(bad) is None, bad


def test_refusals(exe, plain_exe, tmp_path):
    paths = write(tmp_path, scene())
    inputs = "--inputs=" + ",".join(paths)
    for args, text in ((["--stream-gate=17"], "bad value for --stream-gate: '17'"), (["--stream-gate=1:1:1:0.5"], "bad value for --stream-gate"),
                       (["--stream-gate", "--read-mode=2"], "--stream-gate reads the pings of 16-bit audio: it excludes --read-mode=2"),
                       (["--stream-gate", "--wideband-rate=240000", "--channel-offsets=0"], "--stream-gate gates the audio streams' windows: it excludes --wideband-rate"),
                       ([inputs, "--stream-gate=1:1:4"], "--stream-gate: MAX must lie within 1..3, or be 0 for all"),
                       ([inputs, "--stream-gate=::::3"], "--stream-gate: stream 3 is not one of the 3 streams"),
                       (["--stream-gate=::::1"], "--stream-gate: stream 1 is not one of the 1 streams")):
        p = host_stub.run(exe, args, b"")
        assert p.returncode == 2 and text in p.stderr.decode(), (args, p.stderr.decode())
        assert p.stdout == b""
    # a library without the entries: refused by name, and the program without the option still runs against it
    p = host_stub.run(plain_exe, ["--stream-gate"], b"")
    assert p.returncode == 2 and "has no stream gate (msk144_set_stream_gate)" in p.stderr.decode()
    assert host_stub.run(plain_exe, [], b"").returncode == 0


def test_inputs_lists_snr_and_summary_equal_the_model(exe, tmp_path):
    """Three --inputs streams - bursts, a stream that ends early inside a burst, silence.  The detector is switched on with its
    defaults and writes no log; each stream's lines are those of the hops the model lists, with the snr= of the ungated run although
    the streams sat most hops out; the summary carries the model's counts."""
    streams = scene()
    paths = write(tmp_path, streams)
    plain = host_stub.run(exe, ["--inputs=" + ",".join(paths)])
    p = host_stub.run(exe, ["--inputs=" + ",".join(paths), "--stream-gate"])
    assert p.returncode == 0 and plain.returncode == 0, p.stderr.decode()
    listed, decoded, pushed, dropped, busiest = model_lists(streams)
    assert listed[0] and listed[1] and not listed[2] and 0 < decoded < pushed == 6 + 4 + 6
    check_stdout(p, plain, listed, {0: 10, 1: 40, 2: None})
    snrs = {re.search(r"snr=\s*(-?\d+)", l).group(1) for l, _ in lines_of(plain)[0]}
    assert len(snrs) > 1                                  # the stand-in's segment powers do move snr= from hop to hop
    err = p.stderr.decode()
    d = sp.STREAM_PINGS_DEFAULTS
    assert f"stub: msk144_set_stream_pings(ratio_q4 {d['ratio_q4']}, memory {d['memory']}, min_ref {d['min_ref']}, shift {d['shift']}, 3 streams)" in err
    assert "stub: msk144_set_stream_gate(hold 1, min_up 1, max_streams 0, ratio_q4 0, 3 streams, always)" in err
    assert summary_of(p) == (f"msk144hipdecoder: stream gate: {decoded} of {pushed} stream windows decoded, {dropped} dropped over max, busiest hop {busiest} "
                             "(hold 1, min up 1, max 0, ratio the detector's, 0 always)")
    assert "stream pings:" not in err and "stream gate" not in plain.stderr.decode()
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(f) for f in paths)          # no log


def test_parameters_cap_and_always(exe, tmp_path):
    """HOLD 0, MIN_UP 2, MAX 1, the gate's own RATIO and an ALWAYS stream, beside --stream-pings at another ratio: the lists are
    the model's, the windows over MAX are dropped and counted, and the log is that of the run without the gate."""
    streams = scene()
    paths = write(tmp_path, streams)
    log, log0 = tmp_path / "p.log", tmp_path / "p0.log"
    plain = host_stub.run(exe, ["--inputs=" + ",".join(paths), f"--stream-pings={log0}:3"])
    p = host_stub.run(exe, ["--inputs=" + ",".join(paths), f"--stream-pings={log}:3", "--stream-gate=0:2:1:2.5:2"])
    assert p.returncode == 0 and plain.returncode == 0, p.stderr.decode()
    listed, decoded, pushed, dropped, busiest = model_lists(streams, detector=dict(ratio_q4=48), hold=0, min_up=2, max_streams=1, ratio_q4=40, always=[2])
    assert dropped > 0 and busiest == 1 and listed[2]
    check_stdout(p, plain, listed, {0: 10, 1: 40, 2: None})
    assert "stub: msk144_set_stream_gate(hold 0, min_up 2, max_streams 1, ratio_q4 40, 3 streams, always 2)" in p.stderr.decode()
    assert summary_of(p) == (f"msk144hipdecoder: stream gate: {decoded} of {pushed} stream windows decoded, {dropped} dropped over max, busiest hop 1 "
                             "(hold 0, min up 2, max 1, ratio 2.5, 1 always)")
    assert sorted(log.read_text().splitlines()) == sorted(log0.read_text().splitlines()) and log0.read_text()


def test_single_stdin_stream(exe):
    """One stream on stdin goes through the library's hop ring when the option is given; ALWAYS 0 decodes every window: stdout is
    the ungated run's."""
    x = scene()[0]
    data = x.tobytes() + bytes(14)
    plain = host_stub.run(exe, ["--stream-levels"], data)      # the ungated run over the hop ring
    p = host_stub.run(exe, ["--stream-gate=::::0"], data)
    assert p.returncode == 0, p.stderr.decode()
    assert lines_of(p) == lines_of(plain) and len(lines_of(p)[0]) == 6
    assert "ch=" not in p.stdout.decode() and "Incomplete read error. rc=7" in p.stderr.decode()
    assert summary_of(p).startswith("msk144hipdecoder: stream gate: 6 of 6 stream windows decoded, 0 dropped over max, busiest hop 1 ")
    # every half window of a marked stream begins with one loud sample: MIN_UP 2 asks for more than that block
    gated = host_stub.run(exe, ["--stream-gate=:2"], data)
    listed = model_lists([x], min_up=2)[0]
    check_stdout(gated, plain, listed, {0: 10})
    assert 0 < len(listed[0]) < 6


def test_interleaved_on_two_devices(exe):
    """--interleaved with --devices: ALWAYS is given in the program's stream numbers and each device's decoder gets its share by its
    base - device 0 decodes streams 0 and 1, device 1 stream 2, which is stream 0 of its handle."""
    streams = scene()[:1] + [stream(5, 70, 3, bursts=((9000, 96 * 3),)), stream(5, 90, 4)]
    blocks = [np.stack([x[:5184] for x in streams]).tobytes()] + [np.stack([x[5184 + 2592 * k:5184 + 2592 * (k + 1)] for x in streams]).tobytes() for k in range(5)]
    env = dict(os.environ, MSK144_STUB_DEVICES="2")
    args = ["--interleaved=3", "--devices=0,1"]
    plain = subprocess.run([exe] + args, input=b"".join(blocks), capture_output=True, timeout=60, env=env)
    p = subprocess.run([exe] + args + ["--stream-gate=:2:::1,2"], input=b"".join(blocks), capture_output=True, timeout=60, env=env)
    assert p.returncode == 0 and plain.returncode == 0, p.stderr.decode()
    listed, decoded, pushed, dropped, busiest = model_lists(streams, min_up=2, always=[1, 2])
    assert listed[1] == listed[2] == list(range(6)) and 0 < len(listed[0]) < 6
    check_stdout(p, plain, listed, {0: 10, 1: 70, 2: 90})
    err = p.stderr.decode()
    assert "stub: msk144_set_stream_gate(hold 1, min_up 2, max_streams 0, ratio_q4 0, 2 streams, always 1)" in err
    assert "stub: msk144_set_stream_gate(hold 1, min_up 2, max_streams 0, ratio_q4 0, 1 streams, always 0)" in err
    assert summary_of(p).startswith(f"msk144hipdecoder: stream gate: {decoded} of 18 stream windows decoded, 0 dropped over max, busiest hop ")


def test_with_an_input_rate(exe):
    """--input-rate: the gate runs behind the resampler - the stand-in's 12 kHz hops carry two samples of every input row - and
    ALWAYS 0 keeps every window."""
    row = 4 * 2592
    x = np.zeros(5 * row, dtype=np.int16)
    for k in range(5):
        x[k * row], x[k * row + 1] = 0x7777, 20 + k
    plain = host_stub.run(exe, ["--input-rate=48000"], x.tobytes())
    p = host_stub.run(exe, ["--input-rate=48000", "--stream-gate=::::0"], x.tobytes())
    assert p.returncode == 0, p.stderr.decode()
    assert lines_of(p) == lines_of(plain) and [w for _, w in lines_of(p)[0]] == [(20 + k, 21 + k) for k in range(4)]
    assert "input rate 48000 Hz" in p.stderr.decode() and "stub: msk144_push_rate_hops(slot 0, n 1, firsts 1, row 10368)" in p.stderr.decode()
    assert summary_of(p).startswith("msk144hipdecoder: stream gate: 4 of 4 stream windows decoded")
    # the one loud sample of every hop is one block up: MIN_UP 2 lists nothing
    none = host_stub.run(exe, ["--input-rate=48000", "--stream-gate=:2"], x.tobytes())
    assert none.returncode == 0 and none.stdout == b"Done\n" and summary_of(none).startswith("msk144hipdecoder: stream gate: 0 of 4 stream windows decoded")
