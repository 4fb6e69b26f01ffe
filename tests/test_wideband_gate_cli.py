"""CPU: msk144hipdecoder --wideband-gate against the stand-in library with the gate (tests/stub_hip/wideband_gate_stub.cpp, which
takes the base stand-in in as it is).

- The parser (through libmsk144host.so): the bare option, every field, empty fields, and every refusal.
- The option makes exactly one msk144_set_wideband_gate call with its parameters and always flags, behind msk144_set_wideband; the
  list is read after every push, by the decoder and by the summary.
- The stand-in's list is sparse (channels with (c + k) % 3 == 0 at push k, none at push 1, plus the always channels): every line
  carries the true ch=, and stdout is exactly the ungated run's lines for the listed (channel, push) pairs - the snr= in them too,
  which the stand-in makes differ by channel and push, so every channel's tracker saw every push's segment powers.
- The summary line, with a budget that drops channels.
- Malformed values, a channel that does not exist, a budget above the channels, the option without --wideband-pings and without
  --wideband-rate end the program (exit 2) before any library call; against a stand-in without the entries the option is an error
  that names the missing one.  Without the option no new entry is called.
"""
import re

import pytest

import wideband_gate_check as gc
from host_stub import run, shared_program

RATE, OFFSETS, PUSHES = 240000, [-24000, 0, 12000, 36000, 48000], 4
ARGS = [f"--wideband-rate={RATE}", "--wideband-format=cs8", "--channel-offsets=" + ",".join(map(str, OFFSETS))]
DATA = bytes((5184 + (PUSHES - 1) * 2592) * RATE // 12000 * 2)
C = len(OFFSETS)


@pytest.fixture(scope="module")
def new():
    return shared_program(("wideband_gate_stub.cpp", "wideband_pings_stub.cpp"))


@pytest.fixture(scope="module")
def old():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp", "wideband_pings_stub.cpp"))


def stub_lists(always=(), max_channels=0):
    """[(list, total)] of the stand-in's fixed rule, push by push."""
    out = []
    for k in range(PUSHES):
        chosen = [c for c in range(C) if c in always or (k != 1 and (c + k) % 3 == 0)]
        out.append((chosen[:max_channels or C], len(chosen)))
    return out


def lines_by_pair(stdout):
    """{(channel, push): line} of a run, the date masked: the stand-in's payload names the window's halves 100 c + k, 100 c + k + 1."""
    out = {}
    lines = stdout.decode().strip().split("\n")
    assert lines[-1] == "Done"
    for line in lines[:-1]:
        m = re.match(r"^\*\*\*  ch=(\d+); .*msg='([0-9A-F]+)'; $", line)
        assert m, line
        ch, v = int(m.group(1)), int(m.group(2), 16)
        first_half = (v >> 16) & 0xFFFF
        assert first_half // 100 == ch and (v & 0xFFFF) == first_half + 1, f"ch={ch} printed with the window of channel {first_half // 100}: {line}"
        assert (ch, first_half % 100) not in out
        # above the two halves the payload holds the window's position in the decoded batch, which is what the gate changes
        out[(ch, first_half % 100)] = re.sub(r"msg='[0-9A-F]+'", "msg='%08X'" % (v & 0xFFFFFFFF), re.sub(r"date=\d{14}", "date=X", line))
    return out


def summary(lists, hold=1, min_up=1, max_channels=0):
    w, t = sum(len(l) for l, _ in lists), C * PUSHES
    return (f"msk144hipdecoder: wideband gate: {w} of {t} channel windows decoded ({100.0 * w / t:.1f} %), hold {hold}, min up {min_up}, at most {max_channels or C} per push, "
            f"{sum(n - len(l) for l, n in lists)} dropped, busiest push {max(len(l) for l, _ in lists)} channels")


# ---- the parser ----

def test_the_parser():
    base = dict(hold=1, min_up=1, max_channels=0, always=[])
    assert gc.host_parse(None) == base
    assert gc.host_parse("") == base
    assert gc.host_parse("0") == dict(base, hold=0)
    assert gc.host_parse("16:27") == dict(base, hold=16, min_up=27)
    assert gc.host_parse("3:2:100") == dict(base, hold=3, min_up=2, max_channels=100)
    assert gc.host_parse("2:3:0:4,0,7") == dict(hold=2, min_up=3, max_channels=0, always=[4, 0, 7])
    assert gc.host_parse(":::5") == dict(base, always=[5])
    assert gc.host_parse(":3") == dict(base, min_up=3)
    assert gc.host_parse("1:1:2:" + ",".join(map(str, range(40))))["always"] == list(range(40))          # not capped at 16
    for bad in ("-1", "17", "x", "1.5", "1:0", "1:28", "1:x", "1:1:-1", "1:1:x", "1:1:1:x", "1:1:1:-1", "1:1:1:3,3", "1:1:1:3,", "1:1:1:3:4", "1:1:1:3 4", "1 "):
        assert gc.host_parse(bad) is None, bad


# ---- a gated run ----

@pytest.mark.parametrize("value, hold, min_up, max_channels, always", [
    ("", 1, 1, 0, ()),
    ("=0:3", 0, 3, 0, ()),
    ("=2:1:0:1,4", 2, 1, 0, (1, 4)),
    ("=1:1:1", 1, 1, 1, ()),
    ("=:::0,1,2,3,4", 1, 1, 0, (0, 1, 2, 3, 4)),
])
def test_the_gated_run_prints_the_ungated_lines_of_the_listed_pairs(new, tmp_path, value, hold, min_up, max_channels, always):
    pings = [f"--wideband-pings={tmp_path}/pings.txt"]
    plain = run(new, ARGS + pings, DATA, timeout=120)
    assert plain.returncode == 0, plain.stderr.decode()[-1500:]
    want_all = lines_by_pair(plain.stdout)
    assert sorted(want_all) == [(c, k) for c in range(C) for k in range(PUSHES)]
    assert len({re.search(r"snr=\s*(-?\d+)", l).group(1) for l in want_all.values()}) > 1, "the stand-in's segment powers give every line the same snr"

    r = run(new, ARGS + pings + ["--wideband-gate" + value], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    lists = stub_lists(always, max_channels)
    call = f"stub: msk144_set_wideband_gate(hold {hold}, min_up {min_up}, max_channels {max_channels}, always" + "".join(f" {c}" for c in sorted(always)) + ")"
    assert err.count("stub: msk144_set_wideband_gate(") == 1 and call in err
    assert err.index("stub: msk144_set_wideband(") < err.index(call) < err.index("stub: msk144_wideband_gate read 0")
    # the decoder takes the list behind every decode, the summary's counts read it once more per push
    assert [err.count(f"stub: msk144_wideband_gate read {i}\n") for i in range(2 * PUSHES + 1)] == [1] * (2 * PUSHES) + [0]
    got = lines_by_pair(r.stdout)
    want = {(c, k): want_all[(c, k)] for k, (l, _) in enumerate(lists) for c in l}
    assert got == want
    assert 0 < len(want) and (len(want) < len(want_all) or len(always) == C)
    assert summary(lists, hold, min_up, max_channels) in err, err[-800:]


def test_always_channels_need_no_detector(new):
    r = run(new, ARGS + ["--wideband-gate=1:1:0:2"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert "msk144_set_wideband_pings" not in err
    assert set(lines_by_pair(r.stdout)) == {(c, k) for k, (l, _) in enumerate(stub_lists((2,))) for c in l}
    assert summary(stub_lists((2,))) in err


# ---- refusals ----

@pytest.mark.parametrize("bad", ["=-1", "=17", "=x", "=1:0", "=1:28", "=1:1:-1", "=1:1:6", "=1:1:0:5", "=1:1:0:1,1", "=1:1:0:1:2", "=1:1:0:x"])
def test_a_malformed_value_ends_the_program_before_any_library_call(new, tmp_path, bad):
    r = run(new, ARGS + [f"--wideband-pings={tmp_path}/pings.txt", "--wideband-gate" + bad], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-gate" in r.stderr, bad
    assert b"Done" not in r.stdout


def test_the_option_needs_the_detector_or_always_channels_and_wideband_mode(new):
    r = run(new, ARGS + ["--wideband-gate"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-gate needs --wideband-pings=FILE, or a list of channels that are always decoded" in r.stderr
    r = run(new, ARGS + ["--wideband-gate=2:2"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-gate needs --wideband-pings" in r.stderr
    r = run(new, ["--wideband-gate"], DATA)
    assert r.returncode == 2 and b"stub:" not in r.stderr and b"--wideband-gate needs --wideband-rate" in r.stderr


def test_a_library_without_the_entries_is_an_error(old, tmp_path):
    r = run(old, ARGS + [f"--wideband-pings={tmp_path}/pings.txt", "--wideband-gate"], DATA)
    err = r.stderr.decode()
    assert r.returncode == 2 and "msk144_set_wideband_gate" in err and "--wideband-gate needs it" in err and "stub: msk144_set_wideband(" not in err
    assert b"Done" not in r.stdout


def test_no_option_no_new_call(new, tmp_path):
    r = run(new, ARGS + [f"--wideband-pings={tmp_path}/pings.txt"], DATA, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0 and "wideband_gate" not in err and "wideband gate" not in err


def test_help_names_the_option(new):
    out = run(new, ["--help"]).stdout.decode()
    assert "--wideband-gate[=HOLD[:MIN_UP[:MAX[:ALWAYS]]]]" in out
    assert out.index("--wideband-notch=") < out.index("--wideband-gate") < out.index("--taps-per-phase=K")
