"""CPU: msk144hipdecoder --wideband-notch against the stand-in library (tests/stub_hip, with wideband_notch_stub.cpp).

- The parser (through libmsk144host.so): fixed tables, auto with its fields, the half-width, and every refusal.
- A fixed table makes exactly one msk144_set_wideband_notch call, with the channels ascending and the taps and shift of the host
  design for each, behind msk144_set_wideband and ahead of the first push's reads; the stats are read once per push and the
  summary line adds them up.
- auto switches the stand-in's waterfall on without --wideband-waterfall (and writes no file), feeds every push's sums to the rule
  and hands over the whole table at every change: the calls, the stderr lines and the summary are those of wideband.NotchPlanner on
  the stand-in's sums.
- Malformed values, a channel that does not exist and the option without --wideband-rate end the program (exit 2) before any library
  call; against a stand-in without the entries the option is an error that names the missing one.
- Without the option no new entry is called.
"""
import os
import re

import pytest

import wideband_notch_check as nc
from host_stub import run, shared_program
from msk144cudecoder_amd import wideband as wb
from test_wideband_waterfall_cli import stub_rows

RATE, OFFSETS, PUSHES = 240000, [-24000, 0, 12000, 36000, 48000], 4
ARGS = [f"--wideband-rate={RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, OFFSETS))]
DATA = bytes((5184 + (PUSHES - 1) * 2592) * RATE // 12000 * 2)
STUBS = ("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_waterfall_stub.cpp", "wideband_notch_stub.cpp")


@pytest.fixture(scope="module")
def new():
    return shared_program(STUBS)


@pytest.fixture(scope="module")
def old():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_waterfall_stub.cpp"))


@pytest.fixture(scope="module")
def no_waterfall():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_notch_stub.cpp"))


def set_call(table, halfwidth=100):
    """The stand-in's report of msk144_set_wideband_notch for {channel: [Hz, ...]}."""
    parts = []
    for c in sorted(table):
        taps, shift = wb.notch_taps(table[c], halfwidth)
        parts.append(f" ch={c} shift {shift} taps {taps.tobytes().hex()}")
    return f"stub: msk144_set_wideband_notch({len(table)} channels:" + "".join(parts) + ")"


def summary(table, clamped, halfwidth=100):
    which = "".join(("; " if i == 0 else " ") + f"ch={c} " + ",".join(f"{f:+d}" for f in table[c]) + " Hz" for i, c in enumerate(sorted(table)[:3]))
    return (f"msk144hipdecoder: wideband notch: {len(table)} of {len(OFFSETS)} channels notched, {sum(len(f) for f in table.values())} notches of +-{halfwidth} Hz, "
            f"{clamped} components clamped{which}")


# ---- the parser ----

def test_the_parser():
    base = dict(auto=False, halfwidth=100, db=10.0, period=23, persist=2)
    assert nc.host_parse("1:300") == dict(base, table={1: [300]})
    assert nc.host_parse("1:300+-700,3:0") == dict(base, table={1: [300, -700], 3: [0]})
    assert nc.host_parse("4:-5900,0:+250+1250/60") == dict(base, halfwidth=60, table={4: [-5900], 0: [250, 1250]})
    assert nc.host_parse("0:5500/500") == dict(base, halfwidth=500, table={0: [5500]})
    assert nc.host_parse("auto") == dict(base, auto=True, table={})
    assert nc.host_parse("auto:12.5") == dict(base, auto=True, db=12.5, table={})
    assert nc.host_parse("auto:6:5:3/250") == dict(base, auto=True, db=6.0, period=5, persist=3, halfwidth=250, table={})
    for bad in ("", "/100", "1", "1:", ":300", "1:x", "x:300", "-1:300", "1:300,", ",1:300", "1:300,1:900", "1:300+", "1:300+800", "1:300+1300+2300", "1:5901", "1:5501/500",
                "1:300/49", "1:300/501", "1:300/", "1:300/100/100", "1:300.5", "1:3e2", "auto:", "auto:x", "auto:0.5", "auto:101", "auto:10:0", "auto:10:100001", "auto:10:23:0",
                "auto:10:23:1001", "auto:10:23:2:1", "auto:10:2.5", "automatic", "auto,1:300", "1:300,auto"):
        assert nc.host_parse(bad) is None, bad


# ---- a fixed table ----

@pytest.mark.parametrize("value, table, halfwidth", [
    ("1:300", {1: [300]}, 100),
    ("3:0,1:300+-700", {1: [300, -700], 3: [0]}, 100),
    ("0:-2000,1:300+1300,2:0,4:5000/250", {0: [-2000], 1: [300, 1300], 2: [0], 4: [5000]}, 250),
])
def test_a_fixed_table_is_handed_over_once(new, value, table, halfwidth):
    r = run(new, ARGS + [f"--wideband-notch={value}"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    call = set_call(table, halfwidth)
    assert err.count("stub: msk144_set_wideband_notch(") == 1 and call in err
    assert err.index("stub: msk144_set_wideband(") < err.index(call) < err.index("stub: msk144_wideband_notch_stats read 0")
    assert [err.count(f"stub: msk144_wideband_notch_stats read {i}\n") for i in range(PUSHES + 1)] == [1] * PUSHES + [0]
    assert "msk144_set_wideband_waterfall" not in err and "msk144_wideband_waterfall_sums" not in err
    assert "wideband notch: ch=" not in err                      # nothing is added to a fixed table
    assert summary(table, PUSHES * sum(10 * c + 1 for c in table), halfwidth) in err, err[-800:]


# ---- auto ----

def planned(db, period, persist, halfwidth=100):
    """[(push, channel, hz, excess)] and the final table of wideband.NotchPlanner on the stand-in's sums."""
    planner = wb.NotchPlanner(len(OFFSETS), db=db, period=period, persist=persist, halfwidth_hz=halfwidth)
    added = []
    for i in range(PUSHES):
        added += [(i, c, hz, ex) for c, hz, ex in planner.push(wb.waterfall_sums(stub_rows(i)))]
    return added, {c: f for c, f in enumerate(planner.notches) if f}


@pytest.mark.parametrize("value, plan", [("auto:10:1:2", (10.0, 1, 2)), ("auto:10:1:1/150", (10.0, 1, 1)), ("auto:10:2:1", (10.0, 2, 1)), ("auto", (10.0, 23, 2)),
                                         ("auto:80:1:1", (80.0, 1, 1))])
@pytest.mark.parametrize("with_file", [False, True])
def test_auto_follows_the_planner_on_the_stand_ins_sums(new, tmp_path, value, plan, with_file):
    halfwidth = int(value.split("/")[1]) if "/" in value else 100
    added, table = planned(*plan, halfwidth)
    wf = tmp_path / "wf.txt"
    r = run(new, ARGS + [f"--wideband-notch={value}"] + ([f"--wideband-waterfall={wf}:0"] if with_file else []), DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    # the waterfall is on either way, its sums are read once per push, and only the option writes a file
    assert err.count("stub: msk144_set_wideband_waterfall(window default)") == 1
    assert [err.count(f"stub: msk144_wideband_waterfall_sums read {i}\n") for i in range(PUSHES + 1)] == [1] * PUSHES + [0]
    assert os.path.exists(wf) == with_file and ("wideband waterfall:" in err) == with_file
    if not with_file:
        assert "stub: msk144_wideband_waterfall(channel" not in err
    # every added notch is one line, at the newest hop of its push: the first push carries hops 0 and 1
    lines = [l for l in err.splitlines() if l.startswith("msk144hipdecoder: wideband notch: ch=")]
    assert lines == [nc.host_line(c, hz, ex, OFFSETS[c], i + 1) for i, c, hz, ex in added]
    for i, c, hz, ex in added:
        assert f"msk144hipdecoder: wideband notch: ch={c} offset={OFFSETS[c]} notch={hz} excess={ex:.1f} at hop {i + 1}" in lines
    # the whole table at every change, in the order of the changes
    calls = [l for l in err.splitlines() if l.startswith("stub: msk144_set_wideband_notch(")]
    want, so_far = [], {}
    for i in sorted({a[0] for a in added}):
        for _, c, hz, _ in [a for a in added if a[0] == i]:
            so_far[c] = so_far.get(c, []) + [hz]
        want.append(set_call(so_far, halfwidth))
    assert calls == want
    # the stats are read for every push made with a table; the stand-in clamps 10 c + 1 components per push on a channel of the table
    clamped, so_far = 0, {}
    for i in range(PUSHES):
        clamped += sum(10 * c + 1 for c in so_far)
        for _, c, hz, _ in [a for a in added if a[0] == i]:
            so_far[c] = so_far.get(c, []) + [hz]
    assert summary(table, clamped, halfwidth) in err, err[-800:]
    if plan[0] == 10.0 and plan[1] < 23:
        assert added                                               # the stand-in's tones are far over the median
    if plan == (10.0, 1, 1):
        assert len(table) == len(OFFSETS) and added[0][0] == 0     # with PERSIST 1 every channel gets a notch at the first push
    if value in ("auto", "auto:80:1:1"):
        assert not added and "0 of 5 channels notched, 0 notches of +-100 Hz, 0 components clamped\n" in err


# ---- refusals ----

@pytest.mark.parametrize("bad", ["=", "=1", "=1:", "=1:x", "=1:300+800", "=1:5901", "=1:300/49", "=1:300,1:900", "=auto:", "=auto:0.5", "=auto:10:0", "=automatic", "=5:300", "=1:300,7:0"])
def test_a_malformed_value_ends_the_program_before_any_library_call(new, bad):
    r = run(new, ARGS + ["--wideband-notch" + bad], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-notch" in r.stderr, bad
    assert b"Done" not in r.stdout


def test_the_option_needs_wideband_mode(new):
    r = run(new, ["--wideband-notch=1:300"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-notch needs --wideband-rate" in r.stderr


def test_a_library_without_the_entries_is_an_error(old, no_waterfall):
    r = run(old, ARGS + ["--wideband-notch=1:300"], DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_set_wideband_notch" in err and "--wideband-notch needs it" in err and "stub: msk144_set_wideband(" not in err
    assert b"Done" not in r.stdout
    # auto needs the waterfall's entries too; a fixed table does not
    r = run(no_waterfall, ARGS + ["--wideband-notch=auto"], DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_set_wideband_waterfall" in err and "--wideband-notch=auto needs it" in err and "stub: msk144_set_wideband(" not in err
    assert run(no_waterfall, ARGS + ["--wideband-notch=1:300"], DATA, timeout=120).returncode == 0


def test_no_option_no_new_call(new, old):
    outs = []
    for exe in (new, old):
        r = run(exe, ARGS, DATA, timeout=120)
        err = r.stderr.decode()
        assert r.returncode == 0
        assert "notch" not in err and "waterfall" not in err
        outs.append((re.sub(rb"date=\d{14}", b"date=X", r.stdout), sorted(l for l in err.splitlines() if l.startswith("stub:") or l.startswith("msk144hipdecoder: wideband"))))
    assert outs[0] == outs[1]


def test_help_names_the_option(new):
    out = run(new, ["--help"]).stdout.decode()
    assert "--wideband-notch=SPEC[/HALFWIDTH]" in out and "auto[:DB[:PERIOD[:PERSIST]]]" in out
    assert out.index("--wideband-capture=") < out.index("--wideband-notch=") < out.index("--taps-per-phase=K")
