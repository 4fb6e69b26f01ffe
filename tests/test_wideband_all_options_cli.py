"""CPU: msk144hipdecoder with every wideband option at once, against the stand-in library built from all of tests/stub_hip.

The other test_wideband_*_cli.py files switch one option on, or two that depend on each other.  Here gain=auto, levels, blanker,
spectrum, pings, ping band, waterfall and capture run together, which is the case the one read path of WidebandRun
(host/wideband_run_impl.h) has to get right:
- every `set` call is made once, in the order set, agc, spectrum, ping band, pings, waterfall, capture, blanker;
- after every push each read entry is called once, in the order levels, spectrum, pings (records, then block energies), waterfall
  (rows, then sums), capture, and a push is read completely before the next one is;
- every file the options write, capture.log included, has content, and the ping lines carry both the waterfall's and the capture's
  fields;
- the summary has one line per option, in the order channeliser, blanker, spectrum, pings, waterfall, capture, levels.
"""
import os
import re

import pytest

from host_stub import WIDEBAND_DATA, WIDEBAND_OFFSETS, WIDEBAND_PUSHES, WIDEBAND_STUBS, run, shared_program, wideband_all_options


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    d = tmp_path_factory.mktemp("all_options")
    return d, run(shared_program(WIDEBAND_STUBS), wideband_all_options(d), WIDEBAND_DATA, timeout=120)


def test_the_run_ends_in_order(result):
    _, r = result
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode().strip().split("\n")
    assert out[-1] == "Done" and len(out) == 1 + len(WIDEBAND_OFFSETS) * WIDEBAND_PUSHES     # one line per channel and push of the stand-in


def test_every_set_call_once_in_order(result):
    _, r = result
    calls = re.findall(r"^stub: (msk144_set_wideband\w*)\(", r.stderr.decode(), re.M)
    assert calls == ["msk144_set_wideband", "msk144_set_wideband_agc", "msk144_set_wideband_spectrum", "msk144_set_wideband_ping_band", "msk144_set_wideband_pings",
                     "msk144_set_wideband_waterfall", "msk144_set_wideband_capture", "msk144_set_wideband_blanker"]


def test_every_read_once_per_push_in_order(result):
    _, r = result
    err = r.stderr.decode()
    reads = re.findall(r"^stub: (msk144_wideband_(?!blanker_stats)\w+).*?(?:read (\d+)|$)", err, re.M)
    # the stand-in's levels entry reports its first call only, and its waterfall entry is called once per channel that has rows to
    # read, a number the ping records decide: both are checked below, the fixed part of the order here
    assert reads[0] == ("msk144_wideband_levels", "")
    fixed = [(n, int(i)) for n, i in reads[1:] if n != "msk144_wideband_waterfall"]
    assert fixed == [(n, i) for i in range(WIDEBAND_PUSHES) for n in ("msk144_wideband_spectrum", "msk144_wideband_pings", "msk144_wideband_ping_blocks", "msk144_wideband_waterfall_sums",
                                                                       "msk144_wideband_capture")]
    for i in range(WIDEBAND_PUSHES):     # the rows between the push's block energies and its sums
        rows = [m.start() for m in re.finditer(rf"^stub: msk144_wideband_waterfall\(channel \d+\) read {i}$", err, re.M)]
        assert rows and err.index(f"msk144_wideband_ping_blocks(channel -1) after read {i}\n") < rows[0] and rows[-1] < err.index(f"msk144_wideband_waterfall_sums read {i}\n")
    # levels: the stand-in gives channel c 3c clipped components at its first read and c at every later one
    assert re.findall(r"wideband level ch=(\d) .* clipped=(\d+) ", err) == [(str(c), str((3 + WIDEBAND_PUSHES - 1) * c)) for c in range(len(WIDEBAND_OFFSETS))]


def test_every_file_has_content(result):
    d, _ = result
    for name in ("spectrum.txt", "pings.txt", "waterfall.txt", "capture/capture.log"):
        assert os.path.getsize(d / name) > 0, name
    segments = [n for n in os.listdir(d / "capture") if n.endswith(".cs8")]
    assert segments and all(os.path.getsize(d / "capture" / n) % 5184 == 0 and os.path.getsize(d / "capture" / n) > 0 for n in segments)
    assert len((d / "spectrum.txt").read_text().splitlines()) == WIDEBAND_PUSHES // 2     # one line per two pushes
    pings = (d / "pings.txt").read_text().splitlines()
    assert pings and all(re.fullmatch(r"ping ch=\d .* freq=-?\d+ file=(-|ch\d_hop\d+\.cs8 at=\d+)", l) for l in pings), pings
    assert all(l.startswith("wf ch=") for l in (d / "waterfall.txt").read_text().splitlines())
    assert all(l.startswith("capture ch=") for l in (d / "capture" / "capture.log").read_text().splitlines())


def test_one_summary_line_per_option_in_order(result):
    _, r = result
    lines = re.findall(r"^msk144hipdecoder: (wideband(?: \w+)?)[: ]", r.stderr.decode(), re.M)
    assert lines == ["wideband input", "wideband", "wideband blanker", "wideband spectrum", "wideband pings", "wideband waterfall", "wideband capture"] + \
        ["wideband level"] * len(WIDEBAND_OFFSETS) + ["wideband levels"]
    err = r.stderr.decode()
    assert "band 0 +-1500 Hz shift" in err and "(AGC, e within +-20)" in err and "lower --wideband-gain" not in err
