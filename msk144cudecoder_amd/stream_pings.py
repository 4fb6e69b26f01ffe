"""Per-stream levels and ping detection on the audio hops of the stream path, in Python integers: the model of
msk144_set_stream_pings (include/msk144hip.h "Stream levels and pings"; csrc/stream_pings.h).

The rule and the event rule are wideband.Pings and wideband.PingEvents, reused - one of each per stream - and not restated here;
only the block energies of int16 audio, the levels and the per-stream bookkeeping are this module's.
"""
from __future__ import annotations

import math

import numpy as np

from .wideband import PING_BLOCK, PING_DTYPE, PING_MAX_BLOCKS, PING_MIN_BLOCKS, PingEvents, Pings

HOP_SAMPLES = 2592
FIRST_SAMPLES = 5184
ENERGY_CAP = (1 << 22) - 1
MAX_SHIFT = 24
# the defaults of msk144_stream_pings_params (csrc/stream_pings.h Params); the ratio is the table's in that header
STREAM_PINGS_DEFAULTS = dict(ratio_q4=56, memory=8, min_ref=96, shift=12)
# msk144_stream_level; HipDecoder.stream_pings() returns the same records
LEVEL_DTYPE = np.dtype([("sum", "<i8"), ("sum_sq", "<i8"), ("peak", "<i4"), ("full_scale", "<i4"), ("samples", "<i4"), ("saturated_blocks", "<i4")])
assert LEVEL_DTYPE.itemsize == 32


def _samples(x) -> np.ndarray:
    x = np.asarray(x)
    if x.ndim != 1 or x.size % PING_BLOCK or not np.issubdtype(x.dtype, np.integer) or np.any(x < -32768) or np.any(x > 32767):
        raise ValueError("samples must be a row of int16 values, a multiple of 96 long")
    return x.astype(np.int64)


def _shift(shift) -> int:
    if not 0 <= int(shift) <= MAX_SHIFT:
        raise ValueError("shift must lie within 0..24")
    return int(shift)


def block_energies(x, shift: int = STREAM_PINGS_DEFAULTS["shift"]) -> np.ndarray:
    """int64 [nb]: E[b] = min(2^22 - 1, (the sum of x^2 over samples 96b .. 96b+95) >> shift), the sum exact."""
    sq = np.sum(_samples(x).reshape(-1, PING_BLOCK) ** 2, axis=1)
    return np.minimum(sq >> _shift(shift), ENERGY_CAP)


def levels(x, shift: int = STREAM_PINGS_DEFAULTS["shift"]) -> np.ndarray:
    """LEVEL_DTYPE scalar of one position's samples: exact sum and sum of squares, peak |x|, full-scale samples, the sample count and
    the blocks whose E is the cap at this shift."""
    v = _samples(x)
    out = np.zeros((), dtype=LEVEL_DTYPE)
    out["sum"], out["sum_sq"] = int(v.sum()), int((v * v).sum())
    out["peak"] = int(np.abs(v).max()) if v.size else 0
    out["full_scale"] = int(np.count_nonzero((v == 32767) | (v == -32768)))
    out["samples"] = v.size
    out["saturated_blocks"] = int(np.count_nonzero(block_energies(x, shift) == ENERGY_CAP))
    return out


class StreamPings:
    """The detector of a handle, push by push.  Per stream one wideband.Pings(1) - its history restarts on the stream's is_first hop
    and on its first listed hop, as after msk144_set_stream_pings - and one wideband.PingEvents, so that an event's start counts the
    blocks of that stream alone.  Streams a push does not list keep their state."""

    def __init__(self, streams: int, min_blocks: int = PING_MIN_BLOCKS, **params):
        p = dict(STREAM_PINGS_DEFAULTS)
        unknown = set(params) - set(p)
        if unknown:
            raise TypeError(f"unknown stream ping parameters {sorted(unknown)}")
        p.update({k: int(v) for k, v in params.items()})
        self.shift = _shift(p.pop("shift"))
        self.streams = int(streams)
        self.pings = [Pings(1, **p) for _ in range(self.streams)]
        self.events = [PingEvents(min_blocks) for _ in range(self.streams)]
        self.seen = [False] * self.streams

    def push(self, ids, is_first, rows):
        """ids: ascending stream numbers; is_first[j]; rows[j]: int16 samples of position j, 5184 when is_first[j] else 2592.
        Returns (records PING_DTYPE [n], levels LEVEL_DTYPE [n], energies int64 [n][54] with zeros behind nb, events): the events
        that closed in this push, dicts as PingEvents reports them with `channel` the stream."""
        ids = [int(s) for s in ids]
        if any(not 0 <= s < self.streams for s in ids) or any(b <= a for a, b in zip(ids, ids[1:])):
            raise ValueError("streams must be ascending stream numbers below the stream count")
        n = len(ids)
        records, lev = np.zeros(n, dtype=PING_DTYPE), np.zeros(n, dtype=LEVEL_DTYPE)
        energies = np.zeros((n, PING_MAX_BLOCKS), dtype=np.int64)
        out = []
        for j, s in enumerate(ids):
            x = np.asarray(rows[j])
            if x.shape != ((FIRST_SAMPLES if is_first[j] else HOP_SAMPLES),):
                raise ValueError("a first hop has 5184 samples, a later one 2592")
            E = block_energies(x, self.shift)
            if is_first[j] or not self.seen[s]:
                self.pings[s].reset()
            self.seen[s] = True
            records[j] = self.pings[s].push(None, 1.0, energies=E[None, :])[0]
            lev[j] = levels(x, self.shift)
            energies[j, :E.size] = E
            for e in self.events[s].push(records[j:j + 1], E[None, :]):
                out.append(dict(e, channel=s))
        return records, lev, energies, out

    def close(self) -> list:
        """The end of every stream: the events still open, by stream."""
        return [dict(e, channel=s) for s in range(self.streams) for e in self.events[s].close()]

    def up_blocks(self, s: int) -> int:
        return self.events[s].up_blocks

    def total_blocks(self, s: int) -> int:
        return self.events[s].total_blocks


def stream_ping_line(event: dict) -> str:
    """One line of the event log of msk144hipdecoder --stream-pings=FILE; start and dur are block counts x 0.008 s."""
    s, d = event["start"] * 8, event["blocks"] * 8
    return (f"ping ch={event['channel']} start={s // 1000}.{s % 1000:03d} dur={d // 1000}.{d % 1000:03d} blocks={event['blocks']} "
            f"peak={event['peak']} ref={event['reference']} peak_db={10.0 * math.log10(event['peak'] / event['reference']):.1f}")


class StreamReport:
    """The end-of-run lines of msk144hipdecoder --stream-pings and --stream-levels from what a StreamPings run reported: feed it
    every push's (ids, levels, events) and the events of close()."""

    def __init__(self, streams: int):
        self.streams = int(streams)
        self.sum_sq = [0] * self.streams
        self.samples = [0] * self.streams
        self.full_scale = [0] * self.streams
        self.peak = [0] * self.streams
        self.hops = [0] * self.streams
        self.zero_hops = [0] * self.streams
        self.events = [0] * self.streams

    def add(self, ids, levels, events):
        for s, l in zip(ids, levels):
            s = int(s)
            self.sum_sq[s] += int(l["sum_sq"])
            self.samples[s] += int(l["samples"])
            self.full_scale[s] += int(l["full_scale"])
            self.peak[s] = max(self.peak[s], int(l["peak"]))
            self.hops[s] += 1
            self.zero_hops[s] += int(l["peak"]) == 0
        self.add_events(events)

    def add_events(self, events):
        for e in events:
            self.events[e["channel"]] += 1

    def rms(self, s: int) -> float:
        return math.sqrt(self.sum_sq[s] / self.samples[s]) if self.samples[s] else 0.0

    def _three(self, key, take, smallest=False):
        order = sorted((s for s in range(self.streams) if take(s)), key=lambda s: (key(s) if smallest else -key(s), s))
        return order[:3]

    def pings_line(self, model: StreamPings, params: dict) -> str:
        """params: ratio_q4, memory, shift, min_blocks as the run had them."""
        up = [model.up_blocks(s) for s in range(self.streams)]
        total = sum(model.total_blocks(s) for s in range(self.streams))
        line = (f"msk144hipdecoder: stream pings: {sum(self.events)} events on {sum(1 for n in self.events if n)} of {self.streams} streams, {sum(up)} of {total} blocks up "
                f"(ratio {params['ratio_q4'] / 16.0:g}, min blocks {params['min_blocks']}, memory {params['memory']}, shift {params['shift']})")
        for i, s in enumerate(self._three(lambda s: self.events[s], lambda s: self.events[s] > 0)):
            line += ("," if i else "; most active") + f" ch={s} ({self.events[s]} events, {up[s]} blocks up)"
        return line

    def levels_lines(self) -> list:
        out = [f"msk144hipdecoder: stream levels: ch={s} rms={self.rms(s):.1f} peak={self.peak[s]} full_scale={self.full_scale[s]} hops={self.hops[s]} zero_hops={self.zero_hops[s]}"
               for s in range(self.streams)]
        seen = lambda s: self.hops[s] > 0
        full = self._three(lambda s: self.full_scale[s], lambda s: self.full_scale[s] > 0)
        line = "msk144hipdecoder: stream levels: most full-scale" + ("".join(f" ch={s} ({self.full_scale[s]})" for s in full) or " none")
        line += "; quietest" + "".join(f" ch={s} ({self.rms(s):.1f})" for s in self._three(self.rms, seen, smallest=True))
        zero = [s for s in range(self.streams) if seen(s) and self.zero_hops[s] == self.hops[s]]
        line += "; all hops zero" + ("".join(f" ch={s}" for s in zero) or " none")
        return out + [line]


# ---- the same contract as libmsk144host.so holds it (csrc/stream_pings.h), for the CPU tests ----

def _host():
    import ctypes as C
    from .wideband import HOST_LIB
    L = C.CDLL(HOST_LIB)
    L.msk144host_stream_pings_check.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.msk144host_stream_pings_new.argtypes = [C.c_int, C.c_void_p]
    L.msk144host_stream_pings_new.restype = C.c_void_p
    L.msk144host_stream_pings_free.argtypes = [C.c_void_p]
    L.msk144host_stream_pings_push.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.msk144host_stream_pings_defaults.argtypes = [C.c_void_p]
    L.msk144host_stream_ping_line.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.msk144host_stream_pings_parse.argtypes = [C.c_char_p, C.c_void_p]
    return L


def _params4(params: dict) -> np.ndarray:
    p = dict(STREAM_PINGS_DEFAULTS)
    p.update(params)
    return np.array([p["ratio_q4"], p["memory"], p["min_ref"], p["shift"]], dtype=np.int32)


def host_defaults() -> dict:
    """The defaults of msk144_stream_pings_params as the C++ header has them."""
    out = np.zeros(4, dtype=np.int32)
    _host().msk144host_stream_pings_defaults(out.ctypes.data)
    return dict(zip(("ratio_q4", "memory", "min_ref", "shift"), (int(v) for v in out)))


def host_check(**params) -> str:
    """'' when msk144_set_stream_pings takes the parameters, else its refusal."""
    import ctypes as C
    why = C.create_string_buffer(256)
    _host().msk144host_stream_pings_check(_params4(params).ctypes.data, why, len(why))
    return why.value.decode()


def host_parse(arg: str):
    """"FILE[:RATIO[:MIN_BLOCKS[:MEMORY[:SHIFT]]]]" as the program parses it: dict(ratio_q4, min_blocks, memory, shift, file_len), or None."""
    out = np.zeros(5, dtype=np.int32)
    if _host().msk144host_stream_pings_parse(arg.encode(), out.ctypes.data) != 0:
        return None
    return dict(zip(("ratio_q4", "min_blocks", "memory", "shift", "file_len"), (int(v) for v in out)))


def host_ping_line(event: dict) -> str:
    import ctypes as C
    e = np.zeros((), dtype=np.dtype([("channel", "<i4"), ("pad", "<i4"), ("start", "<i8"), ("blocks", "<i8"), ("peak", "<i4"), ("reference", "<i4")]))
    for k in ("channel", "start", "blocks", "peak", "reference"):
        e[k] = event[k]
    out = C.create_string_buffer(256)
    _host().msk144host_stream_ping_line(e.ctypes.data, out, len(out))
    return out.value.decode()


class HostStreamPings:
    """msk144sp::Model of libmsk144host.so: push(ids, is_first, rows) -> (records, levels, energies) as StreamPings.push."""

    def __init__(self, streams: int, **params):
        self.L = _host()
        self.m = self.L.msk144host_stream_pings_new(int(streams), _params4(params).ctypes.data)
        if not self.m:
            raise ValueError("the host library refuses these parameters")

    def __del__(self):
        if getattr(self, "m", None):
            self.L.msk144host_stream_pings_free(self.m)
            self.m = None

    def push(self, ids, is_first, rows):
        n = len(ids)
        records, lev = np.zeros(n, dtype=PING_DTYPE), np.zeros(n, dtype=LEVEL_DTYPE)
        energies = np.zeros((n, PING_MAX_BLOCKS), dtype=np.int32)
        for j, s in enumerate(ids):
            x = np.ascontiguousarray(rows[j], dtype=np.int16)
            if x.shape != ((FIRST_SAMPLES if is_first[j] else HOP_SAMPLES),):
                raise ValueError("a first hop has 5184 samples, a later one 2592")
            if self.L.msk144host_stream_pings_push(self.m, int(s), 1 if is_first[j] else 0, x.ctypes.data, records[j:j + 1].ctypes.data, lev[j:j + 1].ctypes.data, energies[j].ctypes.data) != 0:
                raise ValueError(f"no stream {s}")
        return records, lev, energies
