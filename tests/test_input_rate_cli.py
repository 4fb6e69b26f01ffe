"""msk144hipdecoder --input-rate on the CPU: the real host sources against the stand-in library with tests/stub_hip/input_rate_stub.cpp,
which hands every input row's first two samples to the stub's own hop ring.  Marked streams at the input rate then show that the
program cuts every stream into hops of 2592 P/Q samples (5184 P/Q first), with partial batches, early ends, the refusals and
--input-rate=wav.  The scene of the GPU decode test is decoded here by the oracle from the model's output."""
import re
import struct

import numpy as np
import pytest

from msk144cudecoder_amd import input_rate as ir

import host_stub
import input_rate_scene as S

STUBS = ("msk144hip_stub.cpp", "input_rate_stub.cpp")


@pytest.fixture(scope="module")
def exe():
    return host_stub.shared_program(STUBS)


@pytest.fixture(scope="module")
def plain_exe():
    return host_stub.shared_program()


def marked(rate, n_hops, tag):
    """n_hops + 1 windows at the input rate: input row k (2592 P/Q samples) starts with 0x7777, tag + k."""
    row = ir.row_samples(rate)
    x = np.zeros((n_hops + 2) * row, dtype=np.int16)
    for k in range(n_hops + 2):
        x[k * row] = 0x7777
        x[k * row + 1] = tag + k
    return x


def expected(n_hops, tag):
    return [(tag + k, tag + k + 1) for k in range(n_hops + 1)]


def undated(p):
    """The program's stdout with the wall-clock stamp of every line taken out, as tests/test_gpu_cli.py compares two runs."""
    return re.sub(r"date=\d{14}", "date=X", p.stdout.decode())


def pushes(stderr):
    return [tuple(map(int, m)) for m in re.findall(r"stub: msk144_push_rate_hops\(slot \d, n (\d+), firsts (\d+), row (\d+)\)", stderr)]


def wav_header(rate, channels=1, bits=16, tag=1, samples=0):
    block = channels * bits // 8
    return b"RIFF" + struct.pack("<I", 36 + samples * block) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, tag, channels, rate, rate * block, block, bits) + b"data" + struct.pack("<I", samples * block)


@pytest.mark.parametrize("rate", [48000, 32000, 96125])
def test_single_stdin_stream(exe, rate):
    x = marked(rate, 3, 10)
    extra = np.zeros(7, dtype=np.int16)                       # a partial hop at the end
    p = host_stub.run(exe, [f"--input-rate={rate}"], x.tobytes() + extra.tobytes())
    assert p.returncode == 0, p.stderr.decode()
    out, err = p.stdout.decode(), p.stderr.decode()
    assert "ch=" not in out and out.strip().endswith("Done")
    assert host_stub.windows_seen(out, 1)[0] == expected(3, 10)
    row = ir.row_samples(rate)
    assert pushes(err) == [(1, 1, row)] + [(1, 0, row)] * 3
    assert "Incomplete read error. rc=7" in err
    P, Q = ir.rate_ratio(rate)
    h = ir.default_taps(rate, 16)
    assert f"stub: msk144_set_input_rate(rate {rate}, shift 14, {len(h)} taps summing to {int(h.astype(np.int64).sum())}, row {row})" in err
    assert f"msk144hipdecoder: input rate {rate} Hz = 12000 x {P}/{Q}, {len(h)} taps (16 per phase), shift 14, 12 samples clamped" in err


def test_taps_per_phase_applies(exe):
    p = host_stub.run(exe, ["--input-rate=48000", "--taps-per-phase=4"], marked(48000, 0, 1).tobytes())
    h = ir.default_taps(48000, 4)
    assert p.returncode == 0 and f"16 taps summing to {int(h.astype(np.int64).sum())}" in p.stderr.decode() and "(4 per phase)" in p.stderr.decode()
    p = host_stub.run(exe, ["--input-rate=48000", "--taps-per-phase=65"], b"")
    assert p.returncode == 2 and "--taps-per-phase" in p.stderr.decode()
    p = host_stub.run(exe, ["--taps-per-phase=4"], b"")       # without either rate option it is the wideband one
    assert p.returncode == 2 and "need --wideband-rate" in p.stderr.decode()
    # ... and with another wideband option beside it the line is a wideband one, --input-rate or not
    p = host_stub.run(exe, ["--input-rate=48000", "--taps-per-phase=4", "--wideband-levels"], b"")
    assert p.returncode == 2 and "need --wideband-rate" in p.stderr.decode()


def test_inputs_with_partial_batches_and_an_early_end(exe, tmp_path):
    rate = 48000
    row = ir.row_samples(rate)
    lens = (4, 1, 2)
    paths = []
    for c, n in enumerate(lens):
        f = tmp_path / f"s{c}.raw"
        f.write_bytes(marked(rate, n, 100 * c).tobytes() + bytes(2 * c))   # streams 1 and 2 end inside a hop
        paths.append(str(f))
    p = host_stub.run(exe, [f"--input-rate={rate}", "--inputs=" + ",".join(paths)])
    assert p.returncode == 0, p.stderr.decode()
    out, err = p.stdout.decode(), p.stderr.decode()
    seen = host_stub.windows_seen(out, 3)
    for c, n in enumerate(lens):
        assert seen[c] == expected(n, 100 * c)
    got = pushes(err)
    assert all(r == row for _, _, r in got)
    assert sum(n for n, _, _ in got) == sum(n + 1 for n in lens) and sum(f for _, f, _ in got) == 3
    assert any(n < 3 for n, _, _ in got)                      # the longer streams go on alone
    for c in range(3):
        assert f"ch={c}: Incomplete read error. rc={c}" in err
    assert f"{3 * sum(n + 1 for n in lens)} samples clamped" in err


def test_interleaved_blocks(exe):
    rate, n = 32000, 2
    row = ir.row_samples(rate)
    streams = [marked(rate, 2, 100 * c) for c in range(n)]
    data = b"".join(s[:2 * row].tobytes() for s in streams)
    for k in range(2, 4):
        data += b"".join(s[k * row:(k + 1) * row].tobytes() for s in streams)
    p = host_stub.run(exe, [f"--input-rate={rate}", f"--interleaved={n}"], data)
    assert p.returncode == 0, p.stderr.decode()
    seen = host_stub.windows_seen(p.stdout.decode(), n)
    for c in range(n):
        assert seen[c] == expected(2, 100 * c)
    assert pushes(p.stderr.decode()) == [(2, 2, row), (2, 0, row), (2, 0, row)]


def test_rate_12000_is_the_program_without_the_option(exe):
    x = host_stub.marked_stream(2, 5)
    a = host_stub.run(exe, ["--input-rate=12000"], x.tobytes())
    b = host_stub.run(exe, [], x.tobytes())
    assert a.returncode == 0 and undated(a) == undated(b) and a.stderr == b.stderr
    assert "msk144_set_input_rate" not in a.stderr.decode() and host_stub.windows_seen(a.stdout.decode(), 1)[0] == expected(2, 5)


@pytest.mark.parametrize("args,why", [
    (["--input-rate=48000", "--read-mode=2"], "excludes --read-mode=2"),
    (["--input-rate=48000", "--wideband-rate=240000", "--channel-offsets=0"], "excludes --wideband-rate"),
    (["--input-rate=44100"], "multiple of 125"),
    (["--input-rate=22050"], "outside"),
    (["--input-rate=384000"], "outside"),
    (["--input-rate=abc"], "bad value for --input-rate"),
    (["--input-rate=wav"], "needs --skip-wav-header"),
    (["--input-rate=wav", "--skip-wav-header", "--interleaved=2"], "give the rate in Hz"),
    (["--input-rate=wav", "--skip-wav-header", "--inputs=/dev/null"], "give the rate in Hz"),
])
def test_refusals(exe, args, why):
    p = host_stub.run(exe, args, b"")
    assert p.returncode == 2 and why in p.stderr.decode(), p.stderr.decode()
    assert p.stdout == b""


def test_input_rate_wav(exe):
    x = marked(48000, 2, 20)
    p = host_stub.run(exe, ["--skip-wav-header", "--input-rate=wav"], wav_header(48000, samples=len(x)) + x.tobytes())
    assert p.returncode == 0, p.stderr.decode()
    assert host_stub.windows_seen(p.stdout.decode(), 1)[0] == expected(2, 20)
    assert pushes(p.stderr.decode()) == [(1, 1, 10368), (1, 0, 10368), (1, 0, 10368)] and "input rate 48000 Hz = 12000 x 4/1" in p.stderr.decode()
    # a 12 kHz header: no resampler, the program with --skip-wav-header alone
    y = host_stub.marked_stream(2, 30)
    a = host_stub.run(exe, ["--skip-wav-header", "--input-rate=wav"], wav_header(12000, samples=len(y)) + y.tobytes())
    b = host_stub.run(exe, ["--skip-wav-header"], wav_header(12000, samples=len(y)) + y.tobytes())
    assert a.returncode == 0 and undated(a) == undated(b) and a.stderr == b.stderr and "msk144_set_input_rate" not in a.stderr.decode()
    assert host_stub.windows_seen(a.stdout.decode(), 1)[0] == expected(2, 30)
    for header, why in ((wav_header(48000, channels=2), "2 channels"), (wav_header(48000, bits=8), "8 bits"), (wav_header(48000, tag=3), "format tag is 3"),
                        (wav_header(44100), "multiple of 125"), (wav_header(48000)[:30], "ended inside"), (b"RIFX" + wav_header(48000)[4:], "canonical")):
        p = host_stub.run(exe, ["--skip-wav-header", "--input-rate=wav"], header + x.tobytes()[:0])
        assert p.returncode == 2 and why in p.stderr.decode() and p.stdout == b"", p.stderr.decode()


def test_program_without_the_entries(plain_exe, tmp_path):
    """Built against msk144hip_stub.cpp alone the program links, runs every other mode and refuses --input-rate."""
    x = host_stub.marked_stream(2, 7)
    p = host_stub.run(plain_exe, [], x.tobytes())
    assert p.returncode == 0 and host_stub.windows_seen(p.stdout.decode(), 1)[0] == expected(2, 7)
    f = tmp_path / "a.raw"
    f.write_bytes(x.tobytes())
    p = host_stub.run(plain_exe, [f"--inputs={f},{f}"])
    assert p.returncode == 0 and host_stub.windows_seen(p.stdout.decode(), 2)[1] == expected(2, 7)
    p = host_stub.run(plain_exe, ["--interleaved=1"], x.tobytes())
    assert p.returncode == 0 and host_stub.windows_seen(p.stdout.decode(), 1)[0] == expected(2, 7)
    p = host_stub.run(plain_exe, ["--input-rate=12000"], x.tobytes())
    assert p.returncode == 0 and host_stub.windows_seen(p.stdout.decode(), 1)[0] == expected(2, 7)
    p = host_stub.run(plain_exe, ["--input-rate=48000"], b"")
    assert p.returncode == 2 and "the loaded libmsk144hip has no input-rate resampler (msk144_set_input_rate)" in p.stderr.decode() and p.stdout == b""


def test_help_lists_the_option(exe):
    out = host_stub.run(exe, ["--help"]).stdout.decode()
    assert "--input-rate=HZ|wav" in out and out.index("--input-rate") > out.index("Additions of msk144hipdecoder")


@pytest.mark.parametrize("rate", [48000, 32000])
def test_the_gpu_scene_decodes_from_the_model_output(orc, rate):
    """What test_gpu_input_rate.py's decode identity compares is not an empty list: the oracle decodes the model's 12 kHz output."""
    o = orc.Oracle(threads=4, **S.CFG)
    found = 0
    for k, row in enumerate(S.windows(rate)):
        for w in row:
            items, _ = o.decode_window(o.frontend_audio(w, 2))
            found += int(np.count_nonzero(items["is_message_present"] == 1))
    assert found >= 1
