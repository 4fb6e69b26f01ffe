"""Per-stream levels and ping detection on the audio hops of the stream path, in Python integers: the model of
msk144_set_stream_pings (include/msk144hip.h "Stream levels and pings"; csrc/stream_pings.h).

The rule and the event rule are wideband.Pings and wideband.PingEvents, reused - one of each per stream - and not restated here;
only the block energies of int16 audio, the levels and the per-stream bookkeeping are this module's.
"""
from __future__ import annotations

import math

import numpy as np

from .wideband import GATE_MAX_HOLD, HOP_BLOCKS, PING_BLOCK, PING_DTYPE, PING_MAX_BLOCKS, PING_MIN_BLOCKS, SINCE_QUIET, PingEvents, Pings, since_next

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


# ---- the stream gate: only the streams with activity are decoded (msk144_set_stream_gate; csrc/stream_gate.h) ----

def stream_gate_check(streams: int, hold: int = 1, min_up: int = 1, max_streams: int = 0, ratio_q4: int = 0) -> str:
    """'' when msk144_set_stream_gate takes the parameters on a handle of `streams` streams, else why not."""
    if not 0 <= int(hold) <= GATE_MAX_HOLD:
        return "hold must lie within 0..16 hops"
    if not 1 <= int(min_up) <= HOP_BLOCKS:
        return "min_up must lie within 1..27 blocks"
    if not 0 <= int(max_streams) <= int(streams):
        return "max_streams must lie within 1..streams, or be 0 for all"
    if int(ratio_q4) != 0 and not 16 <= int(ratio_q4) <= 65535:
        return "ratio_q4 must be 0 or lie within 16..65535"
    return ""


class StreamGate:
    """The stream gate rule of the contract (include/msk144hip.h "Stream gate") in Python integers, push by push.  Per STREAM
    `since`, the hops since its last active one, saturating at SINCE_QUIET; a stream's first listed hop since the gate was made, and
    every is_first hop, start from SINCE_QUIET; streams a push does not list keep theirs.  push() is fed what StreamPings.push
    returns for the same hops and gives (positions int32, total): the listed POSITIONS j, ascending, at most max_streams of them,
    and the number that qualified.  A new StreamGate stands for msk144_set_stream_gate."""

    def __init__(self, streams: int, hold: int = 1, min_up: int = 1, max_streams=None, ratio_q4: int = 0, always=()):
        streams = int(streams)
        max_streams = 0 if not max_streams else int(max_streams)
        why = stream_gate_check(streams, hold, min_up, max_streams, ratio_q4)
        if why:
            raise ValueError(why)
        always = [int(s) for s in always]
        if any(not 0 <= s < streams for s in always):
            raise ValueError("an always stream is out of range")
        self.streams, self.hold, self.min_up, self.ratio_q4 = streams, int(hold), int(min_up), int(ratio_q4)
        self.max_streams = max_streams or streams
        self.always = frozenset(always)
        self.since = [SINCE_QUIET] * streams
        self.seen = [False] * streams

    def mask(self, record, energies) -> int:
        """The up mask of one position: the record's, or with a ratio of the gate's own bit b < blocks set iff
        E[b] x 16 > reference x ratio_q4."""
        if self.ratio_q4 == 0:
            return int(record["up_mask"])
        R = int(record["reference"])
        return sum(1 << b for b in range(int(record["blocks"])) if int(energies[b]) * 16 > R * self.ratio_q4)

    def push(self, ids, is_first, records=None, energies=None):
        """ids: ascending stream numbers; is_first[j]; records PING_DTYPE [n] and energies [n][54] of the detector for this push, or
        None: the detector is off, every mask is 0."""
        ids = [int(s) for s in ids]
        if any(not 0 <= s < self.streams for s in ids) or any(b <= a for a, b in zip(ids, ids[1:])):
            raise ValueError("streams must be ascending stream numbers below the stream count")
        hop = (1 << HOP_BLOCKS) - 1
        chosen = []
        for j, s in enumerate(ids):
            first = bool(is_first[j])
            m = 0 if records is None else self.mask(records[j], energies[j])
            since = SINCE_QUIET if first or not self.seen[s] else self.since[s]
            self.seen[s] = True
            for bits in ([m & hop, (m >> HOP_BLOCKS) & hop] if first else [m & hop]):
                since = since_next(since, bin(bits).count("1") >= self.min_up)
            self.since[s] = since
            if s in self.always or since <= self.hold:
                chosen.append(j)
        return np.array(chosen[:self.max_streams], dtype=np.int32), len(chosen)


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


def host_gate_check(streams: int, hold: int = 1, min_up: int = 1, max_streams: int = 0, ratio_q4: int = 0) -> str:
    """'' when msk144_set_stream_gate takes the parameters (csrc/stream_gate.h check_params), else its refusal."""
    import ctypes as C
    L = _host()
    L.msk144host_stream_gate_check.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    why = C.create_string_buffer(256)
    L.msk144host_stream_gate_check(int(streams), np.array([hold, min_up, max_streams, ratio_q4], dtype=np.int32).ctypes.data, why, len(why))
    return why.value.decode()


def host_gate_parse(arg: str):
    """"[HOLD[:MIN_UP[:MAX[:RATIO[:ALWAYS]]]]]" as the program parses it: dict(hold, min_up, max_streams, ratio_q4, always), or None."""
    import ctypes as C
    L = _host()
    L.msk144host_stream_gate_parse.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int]
    out, always = np.zeros(4, dtype=np.int32), np.zeros(4096, dtype=np.int32)
    n = L.msk144host_stream_gate_parse(arg.encode(), out.ctypes.data, always.ctypes.data, len(always))
    if n < 0:
        return None
    return dict(zip(("hold", "min_up", "max_streams", "ratio_q4"), (int(v) for v in out)), always=[int(v) for v in always[:n]])


class HostStreamGate:
    """msk144sg::Model of libmsk144host.so: push(ids, is_first, records, energies) -> (positions, total) as StreamGate.push; `since`
    is the model's state behind the last push."""

    def __init__(self, streams: int, hold: int = 1, min_up: int = 1, max_streams=None, ratio_q4: int = 0, always=()):
        import ctypes as C
        self.L = _host()
        self.L.msk144host_stream_gate_new.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        self.L.msk144host_stream_gate_new.restype = C.c_void_p
        self.L.msk144host_stream_gate_free.argtypes = [C.c_void_p]
        self.L.msk144host_stream_gate_push.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        self.streams = int(streams)
        flags = np.zeros(max(self.streams, 1), dtype=np.uint8)
        if any(not 0 <= int(s) < self.streams for s in always):
            raise ValueError("an always stream is out of range")
        for s in always:
            flags[int(s)] = 1
        p = np.array([hold, min_up, max_streams or 0, ratio_q4], dtype=np.int32)
        self.m = self.L.msk144host_stream_gate_new(self.streams, p.ctypes.data, flags.ctypes.data)
        if not self.m:
            raise ValueError("the host library refuses these parameters")
        self.since = [SINCE_QUIET] * self.streams

    def __del__(self):
        if getattr(self, "m", None):
            self.L.msk144host_stream_gate_free(self.m)
            self.m = None

    def push(self, ids, is_first, records=None, energies=None):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        first = np.ascontiguousarray([1 if f else 0 for f in is_first], dtype=np.uint8)
        n = len(ids)
        rec = None if records is None else np.ascontiguousarray(records, dtype=PING_DTYPE)
        en = None if records is None else np.ascontiguousarray(energies, dtype=np.int32).reshape(n, PING_MAX_BLOCKS)
        out, count, since = np.zeros(max(n, 1), dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(self.streams, dtype=np.int32)
        total = self.L.msk144host_stream_gate_push(self.m, n, ids.ctypes.data, first.ctypes.data, None if rec is None else rec.ctypes.data, None if en is None else en.ctypes.data,
                                                    out.ctypes.data, count.ctypes.data, since.ctypes.data)
        if total < 0:
            raise ValueError("streams must be ascending stream numbers below the stream count")
        self.since = [int(v) for v in since]
        return out[:int(count[0])].copy(), int(total)
