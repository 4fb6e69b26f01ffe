"""-m gpu: the wideband entries as one state machine (include/msk144hip.h), whatever file of the library they are compiled from.

1. The state table: every read entry in each of four states - no configuration, configured with no push, a push made with the
   entry's option off, a push made with it on - answers the return code and the error text written down here from the contract;
   msk144_set_wideband called again returns every option to off.
2. Options do not disturb one another: with spectrum, pings with the ping band, waterfall and capture on together, every option
   leaves byte for byte what it leaves when it runs alone on the same stream, and the hops of every run are the same - at 48000 Hz
   and at 6152000 Hz (the two-stage bank), without and with the blanker and the AGC.  No tolerance and no model: equality only.
"""
import ctypes as C

import numpy as np
import pytest

import wideband_check as wc
import wideband_gpu as wg
from wideband_options import EINVAL, ESTATE, OK

pytestmark = pytest.mark.gpu


# ---- 1. the state table ----

def _mode(entry):
    return (EINVAL, f"msk144_{entry} needs wideband mode (msk144_set_wideband)")


DONE = (OK, None)
NO_PUSH = (ESTATE, "no wideband push has been made")
NO_BANK = (ESTATE, "the wideband configuration has no bank (rate <= 6144000 Hz)")
NO_BLANKER = (ESTATE, "the running wideband stream has no blanker")
NO_PINGS = (ESTATE, "the last wideband push was made without the ping detector")
NO_WATERFALL = (ESTATE, "the last wideband push was made without the waterfall")

# entry: (no configuration, configured and no push, a push made with its option off, a push made with it on).  The first four
# entries have no option; at 48000 Hz there is no bank, with a push or without
TABLE = {
    "wideband_clip_count": ((ESTATE, "no wideband configuration"), DONE, DONE, DONE),
    "wideband_levels": (_mode("wideband_levels"), NO_PUSH, DONE, DONE),
    "dump_wideband_hop": (NO_PUSH, NO_PUSH, DONE, DONE),
    "dump_wideband_band": (NO_PUSH, NO_PUSH, NO_BANK, NO_BANK),
    "wideband_blanker_stats": (_mode("wideband_blanker_stats"), NO_PUSH, NO_BLANKER, DONE),
    "dump_wideband_blanked": (NO_PUSH, NO_PUSH, NO_BLANKER, DONE),
    "wideband_spectrum": (_mode("wideband_spectrum"), NO_PUSH, (ESTATE, "the last wideband push was made without a spectrum"), DONE),
    "wideband_pings": (_mode("wideband_pings"), NO_PUSH, NO_PINGS, DONE),
    "wideband_ping_blocks": (_mode("wideband_ping_blocks"), NO_PUSH, NO_PINGS, DONE),
    "wideband_waterfall": (_mode("wideband_waterfall"), NO_PUSH, NO_WATERFALL, DONE),
    "wideband_waterfall_sums": (_mode("wideband_waterfall_sums"), NO_PUSH, NO_WATERFALL, DONE),
    "wideband_capture": (_mode("wideband_capture"), NO_PUSH, (ESTATE, "no wideband push has been made with capture on since it was last set"), DONE),
    "wideband_notch_stats": (_mode("wideband_notch_stats"), NO_PUSH, (ESTATE, "no wideband push has been made with the notch on since it was last set"), DONE),
    "wideband_gate": (_mode("wideband_gate"), NO_PUSH, (ESTATE, "no wideband push has been made with the gate on since it was last set"), DONE),
}


def _read(hip, d, entry):
    """(code, error text or None) of one read entry, called on the library itself with room for whatever it writes: the most is
    dump_wideband_blanked's 5184 x 4 cs16 samples (2 channels at 48000 Hz, capture of 4 units)."""
    a, b = np.zeros(1 << 15, dtype=np.int64), np.zeros(1 << 15, dtype=np.int64)
    n, m = C.c_int32(), C.c_int32()

    def p(buf, ctype):
        return C.cast(buf.ctypes.data, C.POINTER(ctype))

    L, h = d.L, d.h
    rc = {
        "wideband_clip_count": lambda: L.msk144_wideband_clip_count(h, p(a, C.c_int64)),
        "wideband_levels": lambda: L.msk144_wideband_levels(h, a.ctypes.data),
        "dump_wideband_hop": lambda: L.msk144_dump_wideband_hop(h, 0, a.ctypes.data),
        "dump_wideband_band": lambda: L.msk144_dump_wideband_band(h, 0, a.ctypes.data),
        "wideband_blanker_stats": lambda: L.msk144_wideband_blanker_stats(h, p(a, hip.WidebandBlankerCounts)),
        "dump_wideband_blanked": lambda: L.msk144_dump_wideband_blanked(h, a.ctypes.data),
        "wideband_spectrum": lambda: L.msk144_wideband_spectrum(h, p(a, C.c_double), p(b, C.c_int64)),
        "wideband_pings": lambda: L.msk144_wideband_pings(h, p(a, hip.WidebandPing)),
        "wideband_ping_blocks": lambda: L.msk144_wideband_ping_blocks(h, -1, p(a, C.c_int32), C.byref(n)),
        "wideband_waterfall": lambda: L.msk144_wideband_waterfall(h, -1, p(a, C.c_float), C.byref(n)),
        "wideband_waterfall_sums": lambda: L.msk144_wideband_waterfall_sums(h, p(a, C.c_double)),
        "wideband_capture": lambda: L.msk144_wideband_capture(h, p(a, hip.WidebandCaptureUnit), p(b, C.c_int8), C.byref(n), C.byref(m)),
        "wideband_notch_stats": lambda: L.msk144_wideband_notch_stats(h, p(a, hip.WidebandNotchCount)),
        "wideband_gate": lambda: L.msk144_wideband_gate(h, p(a, C.c_int32), C.byref(n), C.byref(m)),
    }[entry]()
    return rc, None if rc == OK else (L.msk144_last_error(h) or b"").decode()


def _assert_column(hip, d, column, state):
    for entry, cells in TABLE.items():
        assert _read(hip, d, entry) == cells[column], f"{entry}, {state}"


def test_read_entries_by_state(hip):
    rng = np.random.default_rng(41)
    first = rng.integers(118, 138, size=2 * 5184 * 4, dtype=np.uint8)   # a first push at 48000 Hz, D = 4
    with hip.HipDecoder(center=0.0, width=0.0, step=1.0, depth=1, read_mode=2, channels=2) as d:
        _assert_column(hip, d, 0, "no configuration")
        d.set_wideband(48000, [-6000, 6000], "cu8")
        _assert_column(hip, d, 1, "configured, no push")
        d.push_wideband(0, first, first=True)
        _assert_column(hip, d, 2, "a push with every option off")
        d.set_wideband_blanker()
        d.set_wideband_spectrum(256)
        d.set_wideband_pings()
        d.set_wideband_ping_band()
        d.set_wideband_waterfall()
        d.set_wideband_capture(channels=[0])
        d.set_wideband_notch({0: [0]})
        d.set_wideband_gate()
        d.push_wideband(1, first, first=True)                           # a first push: the blanker applies from one
        _assert_column(hip, d, 3, "a push with every option on")
        # msk144_set_wideband again: no push yet, and every option back to off, so the next push is one made without each
        d.set_wideband(48000, [-6000, 6000], "cu8")
        _assert_column(hip, d, 1, "configured again, no push")
        d.push_wideband(0, first, first=True)
        _assert_column(hip, d, 2, "a push after msk144_set_wideband again")
        d.synchronize()


# ---- 2. options do not disturb one another ----

CHANNELS = 33            # a second wave of 32 slots
LISTED = [1, 32]         # captured whether active or not: one channel of each wave
OPTIONS = ("spectrum", "pings", "waterfall", "capture")


def _int(v):
    return int(v).to_bytes(8, "little", signed=True)


def _run(d, rate, offsets, parts, on, extras):
    """Push parts (the first a first push) with the options `on`, behind a fresh configuration; `extras`: the blanker and the AGC as
    well.  Returns {what: [bytes left by push 0, 1, ..]}.  The ping band runs with the detector, and capture with both, so that the
    records it follows are those of the run with everything on."""
    d.set_wideband(rate, offsets, "cu8")
    if extras:
        d.set_wideband_blanker()
        d.set_wideband_agc()
    if "spectrum" in on:
        d.set_wideband_spectrum(256)
    if "pings" in on or "capture" in on:
        d.set_wideband_pings()
        d.set_wideband_ping_band()
    if "waterfall" in on:
        d.set_wideband_waterfall()
    if "capture" in on:
        d.set_wideband_capture(channels=LISTED)
    left = {what: [] for what in ("hops",) + tuple(on)}
    for i, part in enumerate(parts):
        d.push_wideband(i % 2, part, first=(i == 0))
        left["hops"].append(wg.dump_hops(d, range(CHANNELS)).tobytes() + d.wideband_levels().tobytes() + _int(d.wideband_clip_count()))
        if "spectrum" in on:
            power, segments = d.wideband_spectrum()
            left["spectrum"].append(power.tobytes() + _int(segments))
        if "pings" in on:
            left["pings"].append(d.wideband_pings().tobytes() + d.wideband_ping_blocks().tobytes())
        if "waterfall" in on:
            left["waterfall"].append(d.wideband_waterfall().tobytes() + d.wideband_waterfall_sums().tobytes())
        if "capture" in on:
            units, data, total = d.wideband_capture()
            left["capture"].append(units.tobytes() + data.tobytes() + _int(total))
    d.synchronize()
    return left


@pytest.fixture(scope="module")
def handle(hip):
    with hip.HipDecoder(center=0.0, width=0.0, step=1.0, depth=1, read_mode=2, channels=CHANNELS) as d:
        yield d


@pytest.mark.parametrize("rate", [48000, 6152000])
def test_options_alone_and_together(handle, rate):
    d = handle
    lim = rate // 2 - 6000
    offsets = np.linspace(-lim, lim, CHANNELS).astype(np.int32)
    n_out = 5184 + 2 * 2592
    raw, _ = wg.plant_scene(n_out, rate, offsets, [3, 32], np.random.default_rng(rate % 1000 + 7), snr_db=20.0)
    parts = wc.split_pushes(raw, rate, 3)
    for extras in (False, True):
        together = _run(d, rate, offsets, parts, OPTIONS, extras)
        for option in OPTIONS:
            alone = _run(d, rate, offsets, parts, (option,), extras)
            what = f"{option} at {rate} Hz" + (", blanker and AGC on" if extras else "")
            for i in range(len(parts)):
                assert alone[option][i] == together[option][i], f"{what}: push {i} differs from the run with every option on"
                assert alone["hops"][i] == together["hops"][i], f"{what}: the hops of push {i} differ from the run with every option on"
