"""What the -m gpu test files of the wideband channeliser share: the loop that pushes a stream and holds every push to the
near-tie rule (tests/wideband_check.py) against either reference, the single-stage agreement with the float64 model at the default
taps, and the kit of the decode tests - planted scenes, the decode after msk144_push_wideband and after msk144_push_hops, the
messages per channel, and msk144hipdecoder itself."""
import os
import re
import subprocess

import numpy as np

import pack77
import wideband_check as wc
from msk144cudecoder_amd import synth
from msk144cudecoder_amd import wideband as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE_CFG = dict(center=0.0, width=500.0, step=1.0, depth=6, nbadsync_threshold=1, read_mode=2)
SCENE_DECODE_ARGS = ["--search-width=500", "--search-step=1", "--scan-depth=6", "--nbadsync-threshold=1", "--print-bits"]


def dump_hops(d, channels):
    return np.stack([d.dump_wideband_hop(int(c)) for c in channels])


def check_stream(d, ref, fmt, parts, firsts, what, tally=None, sample=None, on_push=None):
    """Push parts to d (configured by the caller; firsts[i]: a first push) and to ref - a wideband_check.Reference or a
    wideband_bank_check.BankReference of the same configuration - and hold every push to the near-tie rule.  sample: the channels
    ref models, when not all of them; the clip count covers every channel, so it is compared only then.
    on_push(i, got, y, clip): the caller's own, more specific assertions on push i, made before the rule's."""
    channels = np.arange(d.channels) if sample is None else np.asarray(sample)
    for i, (part, first) in enumerate(zip(parts, firsts)):
        d.push_wideband(i % 2, part, first=first)
        y, dl = ref.push(wb.read_samples(part, fmt), first=first)
        got = dump_hops(d, channels)
        assert got.shape == y.shape + (2,)
        clip = d.wideband_clip_count() if len(channels) == d.channels else None
        if on_push is not None:
            on_push(i, got, y, clip)
        rep = wc.assert_hops(got, y, dl, ref.gain, clip, what=f"{what} push {i}")
        if tally is not None:
            tally.add(rep)


def offsets_64(rate, seed):
    lim = rate // 2 - 6000
    rng = np.random.default_rng(seed)
    fixed = [0, -lim, lim, 5999, -5999, 12000, -12000, 1, -1, lim - 1, -(lim - 1)]
    rest = rng.integers(-lim, lim + 1, size=64 - len(fixed))      # off any grid
    return np.array(fixed + list(rest), dtype=np.int32)


def hops_match_the_model(d, rate, fmt, n_pushes, offsets_seed, input_seed, level, tally=None):
    """Configure the 64-channel handle d for (rate, fmt) with the default taps and check the int8 hops of n_pushes pushes of white
    input (level per rail) against the float64 model: by the near-tie rule, within one LSB with 99.9 % exact, and with the model's
    clip count.  The seeds are the caller's data."""
    P, Q = wb.rate_ratio(rate)
    offsets = offsets_64(rate, offsets_seed)
    rng = np.random.default_rng(input_seed)
    n_in = (wb.FIRST_OUT + (n_pushes - 1) * wb.HOP_OUT) * P // Q
    raw = wb.write_samples(level * (rng.normal(size=n_in) + 1j * rng.normal(size=n_in)), fmt)
    ref = wc.Reference(rate, offsets)
    d.set_wideband(rate, offsets, fmt)
    assert d.wideband_slot(0).size == 2 * wb.FIRST_OUT * P // Q
    diffs = []

    def older_check(i, got, y, clip):
        q_ref, clip_ref = wb.quantise(y, ref.gain)
        diff = np.abs(got.astype(np.int16) - q_ref.astype(np.int16))
        assert diff.max() <= 1, f"push {i}: |dq| up to {diff.max()}"
        assert clip == clip_ref, f"push {i}"
        diffs.append(diff.ravel())

    check_stream(d, ref, fmt, wc.split_pushes(raw, rate, n_pushes), [True] + [False] * (n_pushes - 1), f"{fmt} {rate}", tally, on_push=older_check)
    d.synchronize()
    diff = np.concatenate(diffs)
    exact = np.count_nonzero(diff == 0)
    assert exact / diff.size >= 0.999, f"{diff.size - exact} of {diff.size} components differ by one LSB"


# ---- decode ----

def plant_scene(n_out, rate, offsets, ping_channels, rng, snr_db=10.0):
    """cu8 input of n_out output samples with one ping on each of ping_channels; returns (raw, {channel: message})."""
    planted, pings = {}, []
    for k, c in enumerate(ping_channels):
        # a standard message that unpacks to text, so that the program prints it (--print-bits appends the payload)
        msg = pack77.pack_standard("CQ", "K%d%sZ" % (k % 10, "ABCDEFGHIJKLMNOPQRSTUVWXY"[k]), "FN42")
        start = 1500 + (k * 2311) % (n_out - 6 * 864 - 3000)
        p = synth.Ping(msg, start, 5, float(rng.uniform(-150, 150)), snr_db, float(rng.uniform(0, 6)))
        pings.append((int(offsets[c]), p))
        planted[c] = bytes(np.asarray(msg, dtype=np.uint8))
    return wb.synth_wideband(n_out, rate, pings, 0.05, rng, "cu8"), planted


def _decode(d, s):
    d.decode()
    d.fetch_async(s)
    r, _ = d.fetch_wait(s)
    return np.sort(r, order=["channel", "item"])


def decode_wideband(d, parts):
    """(records, int8 hops [C][M][2]) of every push."""
    recs, hops = [], []
    for i, part in enumerate(parts):
        d.push_wideband(i % 2, part, first=(i == 0))
        hops.append(dump_hops(d, range(d.channels)))
        recs.append(_decode(d, i % 2))
    return recs, hops


def decode_hops(d, hops):
    """The records of the same pushes fed as hops through msk144_push_hops."""
    recs = []
    for i, h in enumerate(hops):
        s = i % 2
        hh, first, streams, is_first = d.hop_slot(s)
        n = h.shape[0]
        if i == 0:
            first[:n] = h[:, :2592].reshape(n, -1)
            hh[:n] = h[:, 2592:].reshape(n, -1)
        else:
            hh[:n] = h.reshape(n, -1)
        streams[:n] = np.arange(n)
        is_first[:n] = 1 if i == 0 else 0
        d.push_hops(s, n)
        recs.append(_decode(d, s))
    return recs


def messages_by_channel(recs):
    got = {}
    for r in np.concatenate(recs):
        got.setdefault(int(r["channel"]), set()).add(bytes(np.unpackbits(r["message"])[:77]))
    return got


def messages_by_channel_in_lines(lines):
    got = {}
    for line in lines:
        m = re.match(r"^\*\*\*  ch=(\d+); .*bits='([01]{77})'", line)
        assert line.startswith("***  ch="), line
        if not m:
            continue                                  # --print-bits appends the payload only to a line whose text unpacks
        got.setdefault(int(m.group(1)), set()).add(bytes(int(b) for b in m.group(2)))
    return got


def check_channels(got, planted, offsets):
    """Every planted message is decoded on its own channel, and on no channel 12 kHz or more away."""
    for c, msg in planted.items():
        assert msg in got.get(c, set()), f"message planted at {offsets[c]} Hz not decoded on ch={c}"
    for c, msgs in got.items():
        for m in msgs:
            owners = [pc for pc, pm in planted.items() if pm == m]
            assert owners, f"ch={c} decoded a message nobody planted"
            assert all(abs(int(offsets[c]) - int(offsets[pc])) < 12000 for pc in owners), f"message of ch={owners} also on ch={c}"


def run_program(args, data):
    """msk144hipdecoder with data on stdin: (stdout lines before "Done", the date masked; stderr)."""
    exe = os.path.join(ROOT, "msk144cudecoder_amd", "msk144hipdecoder")
    p = subprocess.run([exe] + args, input=data, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().strip().split("\n")
    assert lines[-1] == "Done"
    return [re.sub(r"date=\d{14}", "date=X", l) for l in lines[:-1]], p.stderr.decode()
