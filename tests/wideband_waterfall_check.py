"""What the tests of the per-channel waterfall share (CPU: test_wideband_waterfall_model.py, test_wideband_waterfall_cli.py; GPU:
test_gpu_wideband_waterfall.py): the error bound of the contract (include/msk144hip.h), the ctypes view of the C++ rules in
libmsk144host.so, and the comparison of a device push with the float64 model.

The bound, per row.  With T = sum_k P[k] of the row, u the relative l2 error of one f32 transform and v = 4 x 2^-24 the rounding of
re^2 + im^2,

    |rows[b][j] - P[k]| <= 2 u sqrt(P[k] T) + u^2 T + v P[k]

(|dX[k]| <= ||dX||_2 <= u ||X||_2).  U is the contract's value of u, MSK144_WATERFALL_U: 4 x the largest u any row of the GPU
tests needed on an MI355X (needed_u below; the figure is beside U, in the header and in DESIGN 4.4), rounded up to one significant
digit.  The margin covers other seeds and another compiler's summation order, not another algorithm, and U must lie below CEILING,
the worst case of a 96-term f32 sum with rounded twiddles and window."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from msk144cudecoder_amd import wideband as wb

V = 4.0 * 2.0 ** -24
U = 3e-6     # largest needed: 6.9e-7 (24 125 sps x 33 channels, cu8, all-ones window)
CEILING = 98.0 * 2.0 ** -24
assert U < CEILING


def bound(P: np.ndarray, u: float) -> np.ndarray:
    """[..., 96] -> the bound of every value, T taken per row."""
    T = np.sum(P, axis=-1, keepdims=True)
    return 2.0 * u * np.sqrt(P * T) + u * u * T + V * P


def needed_u(got: np.ndarray, want: np.ndarray) -> float:
    """The smallest u for which every value of `got` [..., 96] satisfies its row's bound against the exact `want`."""
    T = np.sum(want, axis=-1, keepdims=True)
    d = np.maximum(np.abs(got - want) - V * want, 0.0)
    den = np.sqrt(want * T + T * d) + np.sqrt(want * T)   # the positive root of u^2 T + 2 u sqrt(P T) - d = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(den > 0.0, d / den, np.where(d > 0.0, np.inf, 0.0))
    return float(np.max(u)) if u.size else 0.0


def assert_rows(got, want, u: float, what: str) -> float:
    """Print what the comparison needs, then hold every value of every row to the bound with u."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: {got.shape} against {want.shape}"
    assert np.all(np.isfinite(got)), f"{what}: a value is not finite"
    need = needed_u(got, want)
    print(f"{what}: needs u = {need:.3e} (bound with u = {u:.1e})")
    over = np.abs(got - want) - bound(want, u)
    worst = np.unravel_index(int(np.argmax(over)), over.shape)
    assert np.all(over <= 0.0), f"{what}: {worst} reads {got[worst]!r}, the model {want[worst]!r}; needs u = {need:.3e}"
    return need


def random_window(seed: int) -> np.ndarray:
    """A seeded positive window: uniform in 0.1 .. 1."""
    return np.random.default_rng([96, seed]).uniform(0.1, 1.0, wb.WATERFALL_BINS)


def assert_rows_past_n_are_zero(d, what: str):
    """The raw entry, into buffers filled with ones: rows[54][96] of a channel and rows[channels][54][96] of all are 0 past *n."""
    for channel, count in ((d.channels - 1, 1), (-1, d.channels)):
        out = np.ones((count, wb.WATERFALL_ROWS, wb.WATERFALL_BINS), dtype=np.float32)
        n = C.c_int32()
        assert d.L.msk144_wideband_waterfall(d.h, channel, out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n)) == 0, what
        assert n.value in (27, 54) and not out[:, n.value:].any(), f"{what}: rows past {n.value} of channel {channel}"


def assert_push(d, model: wb.Waterfall, u: float, what: str):
    """The last push of handle d against the model fed d's own hops: every row within the bound, the single-channel reads equal
    to the read of all, and the sums the sequential double sum of the device's own rows, exactly.  Returns (rows, needed u)."""
    hops = np.stack([d.dump_wideband_hop(c) for c in range(d.channels)])
    want = model.push(hops)
    rows = d.wideband_waterfall()
    assert rows.dtype == np.float32 and rows.shape == want.shape, f"{what}: {rows.shape} against {want.shape}"
    need = assert_rows(rows, want, u, what)
    assert_rows_past_n_are_zero(d, what)
    for c in sorted({0, d.channels // 2, d.channels - 1}):
        assert np.array_equal(d.wideband_waterfall(c), rows[c]), f"{what}: the rows of ch={c} read alone"
    sums = d.wideband_waterfall_sums()
    assert sums.dtype == np.float64 and sums.tobytes() == wb.waterfall_sums(rows).tobytes(), f"{what}: sums"
    return rows, need


# ---- the C++ rules (csrc/wideband.h through libmsk144host.so) ----

@functools.lru_cache(maxsize=None)
def host():
    L = C.CDLL(wb.HOST_LIB)
    vp, i32 = C.c_void_p, C.c_int32
    L.msk144host_wideband_waterfall_window.argtypes, L.msk144host_wideband_waterfall_window.restype = [vp], C.c_int
    L.msk144host_wideband_waterfall_check.argtypes, L.msk144host_wideband_waterfall_check.restype = [vp, C.c_char_p, C.c_int], C.c_int
    L.msk144host_wideband_waterfall_full.argtypes, L.msk144host_wideband_waterfall_full.restype = [vp], C.c_double
    L.msk144host_wideband_waterfall_db.argtypes, L.msk144host_wideband_waterfall_db.restype = [C.c_double, C.c_double], C.c_double
    L.msk144host_wideband_waterfall_line.argtypes, L.msk144host_wideband_waterfall_line.restype = [i32, i32, C.c_int64, vp, C.c_double, C.c_char_p, C.c_int], None
    L.msk144host_wideband_waterfall_parse.argtypes, L.msk144host_wideband_waterfall_parse.restype = [C.c_char_p, vp], C.c_int
    L.msk144host_wideband_ping_spectra_new.argtypes, L.msk144host_wideband_ping_spectra_new.restype = [C.c_int, C.c_int], vp
    L.msk144host_wideband_ping_spectra_free.argtypes, L.msk144host_wideband_ping_spectra_free.restype = [vp], None
    L.msk144host_wideband_ping_spectra_push.argtypes, L.msk144host_wideband_ping_spectra_push.restype = [vp, vp, vp, vp, C.c_int], C.c_int
    L.msk144host_wideband_ping_spectra_close.argtypes, L.msk144host_wideband_ping_spectra_close.restype = [vp, vp, C.c_int], C.c_int
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_window() -> np.ndarray:
    out = np.zeros(wb.WATERFALL_BINS, dtype=np.float64)
    assert host().msk144host_wideband_waterfall_window(_p(out)) == wb.WATERFALL_BINS
    return out


def host_check(window) -> str:
    """'' when msk144_set_wideband_waterfall takes the window (None: the default), else the refusal text."""
    why = C.create_string_buffer(256)
    w = None if window is None else np.ascontiguousarray(window, dtype=np.float64)
    return "" if host().msk144host_wideband_waterfall_check(None if w is None else _p(w), why, len(why)) == 0 else why.value.decode()


def host_full(window=None) -> float:
    w = None if window is None else np.ascontiguousarray(window, dtype=np.float64)
    return float(host().msk144host_wideband_waterfall_full(None if w is None else _p(w)))


def host_line(channel: int, offset_hz: int, block: int, row, full: float) -> str:
    r = np.ascontiguousarray(row, dtype=np.float32)
    buf = C.create_string_buffer(2048)
    host().msk144host_wideband_waterfall_line(channel, offset_hz, block, _p(r), full, buf, len(buf))
    return buf.value.decode()


def host_parse(arg: str):
    """(by pings, the listed channels, len(FILE)) as the program parses --wideband-waterfall=arg, None when it refuses it."""
    out = np.zeros(19, dtype=np.int32)
    if host().msk144host_wideband_waterfall_parse(arg.encode(), _p(out)) != 0:
        return None
    return bool(out[0]), [int(v) for v in out[3:3 + int(out[1])]], int(out[2])


def padded(rows) -> np.ndarray:
    """float32 [channel][54][96] from rows [channel][nb][96]."""
    r = np.asarray(rows, dtype=np.float32)
    out = np.zeros((r.shape[0], wb.WATERFALL_ROWS, wb.WATERFALL_BINS), dtype=np.float32)
    out[:, :r.shape[1]] = r
    return out


class HostSpectra:
    """The C++ frequency rule (csrc/wideband.h PingSpectra, the one the program runs) with the interface of wideband.PingSpectra."""
    CAP = 4096

    def __init__(self, channels: int, min_blocks: int = wb.PING_MIN_BLOCKS):
        self.s = host().msk144host_wideband_ping_spectra_new(channels, min_blocks)
        assert self.s, "parameters refused"

    def push(self, records, rows) -> list:
        out = np.zeros(self.CAP, dtype=np.int32)
        rec, r = np.ascontiguousarray(records), padded(rows)
        n = host().msk144host_wideband_ping_spectra_push(self.s, _p(rec), _p(r), _p(out), self.CAP)
        assert n <= self.CAP
        return [int(v) for v in out[:n]]

    def close(self) -> list:
        out = np.zeros(self.CAP, dtype=np.int32)
        n = host().msk144host_wideband_ping_spectra_close(self.s, _p(out), self.CAP)
        assert n <= self.CAP
        return [int(v) for v in out[:n]]

    def __del__(self):
        if getattr(self, "s", None):
            host().msk144host_wideband_ping_spectra_free(self.s)
            self.s = None


def parse_line(line: str) -> dict:
    """The fields of one line of the waterfall log."""
    head, *fields = line.split()
    assert head == "wf", line
    d = dict(f.split("=", 1) for f in fields)
    assert list(d) == ["ch", "offset", "block", "t", "db"] and len(d["db"].split(",")) == wb.WATERFALL_BINS, line
    return d


def tone_hop(f_hz: float, nb: int = 27, amplitude: float = 100.0) -> np.ndarray:
    """int8 [96 nb][2]: a tone of `amplitude` LSB at f_hz from the channel's offset, rounded."""
    n = np.arange(96 * nb)
    x = amplitude * np.exp(2j * np.pi * f_hz * n / 12000.0)
    return np.stack([np.rint(x.real), np.rint(x.imag)], axis=1).astype(np.int8)
