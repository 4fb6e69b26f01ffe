"""CPU: msk144hipdecoder --wideband-waterfall against the stand-in library (tests/stub_hip).

- FILE[:CHANNELS] makes exactly one msk144_set_wideband_waterfall call with the default window, behind msk144_set_wideband and ahead
  of every read; the sums are read once per push, the rows only for the channels that need them - one by one up to a handful, in one
  copy of all beyond it.
- FILE holds, line for line, wideband.waterfall_line of the stand-in's rows: every block of the listed channels, or with `pings`
  (the default beside --wideband-pings) every up block of every channel.  The file is appended to.
- With both options every ping line gains ` freq=<Hz>`, the frequency wideband.PingSpectra gives for the stand-in's records and rows;
  up to that field the ping lines, and the decode lines altogether, are those of a run without --wideband-waterfall.
- The stderr summary names the rows written and the channels with a carrier.
- A malformed value, `pings` without --wideband-pings, a channel that does not exist, a FILE that cannot be opened and the option
  without --wideband-rate end the program (exit 2) before it calls the library; against the stand-in without the entries the option
  is an error that names the missing entry, and every other mode still runs.
- Without the option the program calls none of the new entries and prints what it printed before.
"""
import functools
import math
import os
import re

import numpy as np
import pytest

import wideband_waterfall_check as wc
from host_stub import run, shared_program
from msk144cudecoder_amd import wideband as wb

RATE, OFFSETS, PUSHES = 240000, [-24000, 0, 12000, 36000, 48000], 4
ARGS = [f"--wideband-rate={RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, OFFSETS))]
DATA = bytes((5184 + (PUSHES - 1) * 2592) * RATE // 12000 * 2)
TONE = [(40, 0), (28, 28), (0, 40), (-28, 28), (-40, 0), (-28, -28), (0, -40), (28, -28)]
BLOCKS = [54] + [27] * (PUSHES - 1)


@pytest.fixture(scope="module")
def new():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_pings_stub.cpp", "wideband_waterfall_stub.cpp"))


@pytest.fixture(scope="module")
def old():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_pings_stub.cpp"))


def stub_up(i, c, b):
    """The rule of tests/stub_hip/wideband_pings_stub.cpp."""
    if c == 0:
        return i >= 1 and b in (25, 26)
    if c == 1:
        return (i == 0 and b >= 50) or (i == 1 and b <= 2)
    return c == 3 and i == 2 and b == 5


@functools.lru_cache(maxsize=None)
def stub_rows(i):
    """float32 [channel][nb][96]: the rule of tests/stub_hip/wideband_waterfall_stub.cpp for read i, operation for operation."""
    nb, B = BLOCKS[i], 96
    w = wb.waterfall_window().astype(np.float32).astype(np.float64)
    cs = np.array([math.cos(2.0 * math.pi * m / B) for m in range(B)])
    sn = np.array([math.sin(2.0 * math.pi * m / B) for m in range(B)])
    n = np.arange(B)
    xr = np.zeros((len(OFFSETS), nb, B))
    xi = np.zeros((len(OFFSETS), nb, B))
    for c in range(len(OFFSETS)):
        for b in range(nb):
            q = (c + b + i) % 7 - 3
            e = (7 * n + 3 * c + b) % 5 - 2
            t = np.array(TONE)[(q * n) % 8]
            xr[c, b], xi[c, b] = t[:, 0] + e, t[:, 1] + e
    k = (np.arange(B) + B // 2) % B
    re = np.zeros((len(OFFSETS), nb, B))
    im = np.zeros((len(OFFSETS), nb, B))
    for s in range(B):
        m = (s * k) % B
        re += w[s] * (xr[:, :, s, None] * cs[m] + xi[:, :, s, None] * sn[m])
        im += w[s] * (xi[:, :, s, None] * cs[m] - xr[:, :, s, None] * sn[m])
    out = (re * re + im * im).astype(np.float32)
    out.setflags(write=False)
    return out


def stub_records(i):
    rec = np.zeros(len(OFFSETS), dtype=wb.PING_DTYPE)
    for c in range(len(OFFSETS)):
        rec[c]["blocks"], rec[c]["reference"] = BLOCKS[i], 1000 * (c + 1) + i
        rec[c]["up_mask"] = sum(1 << b for b in range(BLOCKS[i]) if stub_up(i, c, b))
    return rec


def wf_lines(channels=None):
    """The lines of the whole run: every block of `channels`, or (None) every up block of every channel."""
    full, out, base = wb.waterfall_full(), [], 0
    for i in range(PUSHES):
        rows = stub_rows(i)
        for c in (channels if channels is not None else range(len(OFFSETS))):
            for b in range(BLOCKS[i]):
                if channels is not None or stub_up(i, c, b):
                    out.append(wb.waterfall_line(c, OFFSETS[c], base + b, rows[c][b], full))
        base += BLOCKS[i]
    return out


def read_lines(path):
    with open(path) as f:
        return f.read().splitlines()


def test_the_stub_rows_are_what_the_model_gives():
    # the stand-in's rule is a transform of integer samples: the float64 model agrees with it to rounding
    i, rows = 1, stub_rows(1)
    q = np.zeros((len(OFFSETS), 96 * 27, 2), dtype=np.int8)
    n = np.arange(96)
    for c in range(len(OFFSETS)):
        for b in range(27):
            e = (7 * n + 3 * c + b) % 5 - 2
            q[c, 96 * b:96 * b + 96] = np.array(TONE)[(((c + b + i) % 7 - 3) * n) % 8] + e[:, None]
    want = wb.Waterfall().push(q)
    wc.assert_rows(rows, want, 1e-9, "the stand-in's rows")
    assert [int(np.argmax(rows[2][b])) for b in range(7)] == [48 + 12 * ((2 + b + 1) % 7 - 3) for b in range(7)]


def test_pings_mode_writes_the_up_blocks_and_the_frequencies(new, old, tmp_path):
    pings, wf, plain = str(tmp_path / "pings.txt"), str(tmp_path / "wf.txt"), str(tmp_path / "plain.txt")
    r = run(new, ARGS + [f"--wideband-pings={pings}", f"--wideband-waterfall={wf}"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    assert err.count("stub: msk144_set_wideband_waterfall(") == 1 and "stub: msk144_set_wideband_waterfall(window default)" in err
    assert err.index("stub: msk144_set_wideband(") < err.index("stub: msk144_set_wideband_waterfall(") < err.index("stub: msk144_wideband_waterfall_sums read 0")
    assert [int(v) for v in re.findall(r"stub: msk144_wideband_waterfall_sums read (\d+)", err)] == list(range(PUSHES))
    # rows only of the channels with an up block in the push, one by one: 1; 0 and 1; 0 and 3; 0
    reads = [(int(c), int(i)) for c, i in re.findall(r"stub: msk144_wideband_waterfall\(channel (-?\d+)\) read (\d+)", err)]
    assert reads == [(1, 0), (0, 1), (1, 1), (0, 2), (3, 2), (0, 3)]
    want = wf_lines()
    got = read_lines(wf)
    assert got == want and len(want) == 14
    for line in got:
        wc.parse_line(line)
    # the ping lines: those of a run without the waterfall, plus the frequency of wideband.PingSpectra
    q = run(old, ARGS + [f"--wideband-pings={plain}"], DATA, timeout=120)
    masked = [re.sub(rb"date=\d{14}", b"date=X", p.stdout) for p in (q, r)]       # the decode lines carry the wall clock
    assert q.returncode == 0 and masked[0] == masked[1] and masked[0].count(b"\n") > 4
    spectra, freqs = wb.PingSpectra(len(OFFSETS)), []
    for i in range(PUSHES):
        freqs += spectra.push(stub_records(i), stub_rows(i))
    freqs += spectra.close()
    before = read_lines(plain)
    assert len(before) == len(freqs) >= 4
    assert read_lines(pings) == [f"{l} freq={f}" for l, f in zip(before, freqs)]
    assert len(set(freqs)) > 1 and all(f % 1500 == 0 for f in freqs)      # the stand-in's tones lie on multiples of 1500 Hz
    assert f"msk144hipdecoder: wideband waterfall: {len(want)} rows written; " in err
    assert err.index("msk144hipdecoder: wideband pings:") < err.index("msk144hipdecoder: wideband waterfall:")


@pytest.mark.parametrize("value, channels, copies", [
    (":2", [2], False),
    (":4,0", [4, 0], False),
    (":0,1,2,3", [0, 1, 2, 3], False),
    (":0,1,2,3,4", [0, 1, 2, 3, 4], True),          # more than a handful: one copy of all
])
def test_a_list_writes_every_block_of_its_channels(new, tmp_path, value, channels, copies):
    path = str(tmp_path / "wf.txt")
    r = run(new, ARGS + [f"--wideband-waterfall={path}{value}"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert "pings" not in err
    reads = [(int(c), int(i)) for c, i in re.findall(r"stub: msk144_wideband_waterfall\(channel (-?\d+)\) read (\d+)", err)]
    assert reads == ([(-1, i) for i in range(PUSHES)] if copies else [(c, i) for i in range(PUSHES) for c in channels])
    got = read_lines(path)
    assert got == wf_lines(channels) and len(got) == len(channels) * sum(BLOCKS)
    assert f"msk144hipdecoder: wideband waterfall: {len(got)} rows written; " in err


def test_a_list_beside_the_ping_detector(new, tmp_path):
    pings, wf = str(tmp_path / "pings.txt"), str(tmp_path / "wf.txt")
    r = run(new, ARGS + [f"--wideband-waterfall={wf}:2", f"--wideband-pings={pings}:2:1"], DATA, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert read_lines(wf) == wf_lines([2])
    spectra, freqs = wb.PingSpectra(len(OFFSETS), 1), []
    for i in range(PUSHES):
        freqs += spectra.push(stub_records(i), stub_rows(i))
    freqs += spectra.close()
    lines = read_lines(pings)
    assert [int(l.rsplit(" freq=", 1)[1]) for l in lines] == freqs and sum("ch=3" in l for l in lines) == 1


def test_the_summary_names_a_carrier(new, tmp_path):
    # the stand-in's tone moves by 1500 Hz per block through seven slots, so every channel's summed spectrum has seven bins far above
    # its median bin: the three channels with the largest excess are named, with the frequency of their highest bin
    r = run(new, ARGS + [f"--wideband-waterfall={tmp_path / 'wf.txt'}:0"], DATA, timeout=120)
    err = r.stderr.decode()
    run_sum = np.zeros((len(OFFSETS), 96))
    for i in range(PUSHES):
        run_sum += wb.waterfall_sums(stub_rows(i))
    excess = [10.0 * math.log10(s.max() / np.sort(s)[48]) for s in run_sum]
    order = sorted(range(len(OFFSETS)), key=lambda c: -excess[c])[:3]
    assert min(excess) > wb.WATERFALL_CARRIER_DB
    want = "; a bin 10 dB or more over the channel's median bin:" + "".join(f" ch={c} {wb.waterfall_hz(int(np.argmax(run_sum[c]))):+d} Hz (+{excess[c]:.1f} dB)" for c in order)
    assert want in err, err[-600:]


def test_the_file_is_appended_to(new, tmp_path):
    path = str(tmp_path / "wf.txt")
    for _ in range(2):
        assert run(new, ARGS + [f"--wideband-waterfall={path}:1"], DATA, timeout=120).returncode == 0
    lines = read_lines(path)
    assert len(lines) == 2 * sum(BLOCKS) and lines[:len(lines) // 2] == lines[len(lines) // 2:]


@pytest.mark.parametrize("bad", ["", ":", ":x", ":-1", ":1,", ":1,1", ":1:2", ":5", ":0,5", ":" + ",".join(map(str, range(17))), ":pings", None])
def test_a_malformed_value_ends_the_program_before_any_library_call(new, tmp_path, bad):
    # ":5": there are five channels, 0..4; ":pings" and the bare FILE (None) need --wideband-pings
    value = "" if bad == "" else str(tmp_path / "w.txt") + (bad or "")
    r = run(new, ARGS + ["--wideband-waterfall=" + value], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-waterfall" in r.stderr, bad
    assert b"Done" not in r.stdout
    assert not os.path.exists(tmp_path / "w.txt")


def test_a_file_that_cannot_be_opened_ends_the_program_before_any_library_call(new, tmp_path):
    path = str(tmp_path / "no_such_directory" / "wf.txt")
    r = run(new, ARGS + [f"--wideband-waterfall={path}:0"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"cannot open" in r.stderr and path.encode() in r.stderr
    assert b"Done" not in r.stdout


def test_the_option_needs_wideband_mode(new, tmp_path):
    path = str(tmp_path / "wf.txt")
    r = run(new, [f"--wideband-waterfall={path}:0"], DATA)
    assert r.returncode == 2 and b"--wideband-rate" in r.stderr and b"stub:" not in r.stderr
    assert not os.path.exists(path)


def test_a_library_without_the_entries_is_an_error_and_runs_every_other_mode(old, tmp_path):
    r = run(old, ARGS + [f"--wideband-waterfall={tmp_path / 'wf.txt'}:0"], DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_set_wideband_waterfall" in err and "stub: msk144_set_wideband(" not in err
    assert b"Done" not in r.stdout
    assert not os.path.exists(tmp_path / "wf.txt")        # no empty file is left behind
    assert run(old, ARGS, DATA, timeout=120).returncode == 0
    assert run(old, ARGS + [f"--wideband-pings={tmp_path / 'p.txt'}"], DATA, timeout=120).returncode == 0


def test_no_option_no_new_call(new, old, tmp_path):
    outs = []
    for k, exe in enumerate((new, old)):
        path = str(tmp_path / f"pings{k}.txt")
        r = run(exe, ARGS + [f"--wideband-pings={path}"], DATA, timeout=120)
        err = r.stderr.decode()
        assert r.returncode == 0
        assert "waterfall" not in err
        outs.append((re.sub(rb"date=\d{14}", b"date=X", r.stdout), read_lines(path), re.sub(r"worst latency \d+ ms", "worst latency X ms", re.sub(r"\d+ late", "N late", err))))
    assert outs[0] == outs[1] and not any("freq=" in l for l in outs[0][1])


def test_help_names_the_option(new):
    out = run(new, ["--help"]).stdout.decode()
    assert "--wideband-waterfall=FILE[:CHANNELS]" in out and "10 dB (a design parameter)" in out
    assert out.index("--wideband-pings") < out.index("--wideband-waterfall") < out.index("--taps-per-phase=K")
