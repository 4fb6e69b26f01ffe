"""ctypes view of libmsk144hip.so (include/msk144hip.h), one method per ABI entry point.

No CPU fallback: if the library is missing or no HIP device is present the constructor raises.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys
from typing import Optional

import numpy as np

from .protocol import ITEM_BYTES
from .wideband import AGC_DEFAULTS, BLANKER_DEFAULTS, LEVEL_DTYPE    # the defaults of msk144_wideband_agc and _blanker; msk144_wideband_level
from .wideband import PING_DTYPE, PING_MAX_BLOCKS, PINGS_DEFAULTS    # msk144_wideband_ping; the defaults of msk144_wideband_pings_params
from .wideband import CAPTURE_DTYPE, CAPTURE_UNIT_BYTES, capture_default_max_units   # msk144_wideband_capture_unit
from .wideband import WATERFALL_BINS, WATERFALL_ROWS                 # the shape of msk144_wideband_waterfall's rows

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libmsk144hip.so")

STAGE_SCAN, STAGE_SOFTBITS, STAGE_INDEX, STAGE_LDPC, STAGE_COLLECT, STAGE_ALL = 1, 2, 4, 8, 16, 31
T_NAMES = ("frontend", "scan", "softbits", "index", "ldpc", "collect", "h2d", "d2h")

WB_FORMATS = {"cu8": 0, "cs8": 1, "cs16": 2}   # msk144_wideband_params.format


class WidebandParams(C.Structure):
    _fields_ = [("rate_hz", C.c_int64), ("format", C.c_int32), ("taps_per_phase", C.c_int32), ("gain", C.c_float), ("num_taps", C.c_int32),
                ("taps", C.POINTER(C.c_double)), ("offsets_hz", C.POINTER(C.c_int32)), ("num_offsets", C.c_int32)]


class WidebandAgc(C.Structure):
    """msk144_wideband_agc; AGC_DEFAULTS holds the defaults of include/msk144hip.h."""
    _fields_ = [("lo_sq", C.c_int32), ("hi_sq", C.c_int32), ("clip_ppm", C.c_int32), ("hold", C.c_int32), ("min_exp", C.c_int32), ("max_exp", C.c_int32)]


class WidebandSpectrum(C.Structure):
    """msk144_wideband_spectrum_params: bins and the window (NULL: periodic Hann)."""
    _fields_ = [("bins", C.c_int32), ("window", C.POINTER(C.c_double))]


class WidebandWaterfall(C.Structure):
    """msk144_wideband_waterfall_params: the window (NULL: periodic Hann)."""
    _fields_ = [("window", C.POINTER(C.c_double))]


class WidebandBlanker(C.Structure):
    """msk144_wideband_blanker; BLANKER_DEFAULTS holds the defaults of include/msk144hip.h."""
    _fields_ = [("threshold_q4", C.c_int32), ("pre", C.c_int32), ("post", C.c_int32)]


class WidebandPing(C.Structure):
    """msk144_wideband_ping; wideband.PING_DTYPE is the same record for numpy."""
    _fields_ = [("up_mask", C.c_uint64), ("blocks", C.c_int32), ("history", C.c_int32), ("quiet", C.c_int32), ("reference", C.c_int32), ("peak", C.c_int32),
                ("peak_block", C.c_int32)]


class WidebandPingsParams(C.Structure):
    """msk144_wideband_pings_params; PINGS_DEFAULTS holds the defaults of include/msk144hip.h."""
    _fields_ = [("ratio_q4", C.c_int32), ("memory", C.c_int32), ("min_ref", C.c_int32)]


class WidebandPingBandParams(C.Structure):
    """msk144_wideband_ping_band_params."""
    _fields_ = [("taps", (C.c_int8 * 2) * 64), ("shift", C.c_int32)]


class WidebandNotchParams(C.Structure):
    """msk144_wideband_notch_params."""
    _fields_ = [("taps", (C.c_int8 * 2) * 64), ("shift", C.c_int32)]


class WidebandNotchCount(C.Structure):
    """msk144_wideband_notch_count; NOTCH_COUNT_DTYPE is the same record for numpy."""
    _fields_ = [("on", C.c_int32), ("clipped", C.c_int32)]


NOTCH_COUNT_DTYPE = np.dtype([("on", "<i4"), ("clipped", "<i4")])
assert C.sizeof(WidebandNotchParams) == 132 and C.sizeof(WidebandNotchCount) == NOTCH_COUNT_DTYPE.itemsize == 8


class WidebandCaptureParams(C.Structure):
    """msk144_wideband_capture_params."""
    _fields_ = [("pre", C.c_int32), ("post", C.c_int32), ("max_units", C.c_int32), ("num_listed", C.c_int32), ("listed", C.c_int32 * 16)]


class WidebandCaptureUnit(C.Structure):
    """msk144_wideband_capture_unit; wideband.CAPTURE_DTYPE is the same record for numpy."""
    _fields_ = [("channel", C.c_int32), ("flags", C.c_int32), ("hop", C.c_int64)]


class WidebandAudioParams(C.Structure):
    """msk144_wideband_audio_params."""
    _fields_ = [("taps", (C.c_int8 * 2) * 64), ("phasor", (C.c_int16 * 2) * 96), ("shift", C.c_int32)]


class WidebandGateParams(C.Structure):
    """msk144_wideband_gate_params."""
    _fields_ = [("hold", C.c_int32), ("min_up", C.c_int32), ("max_channels", C.c_int32)]


assert C.sizeof(WidebandPing) == PING_DTYPE.itemsize == 32
assert C.sizeof(WidebandCaptureUnit) == CAPTURE_DTYPE.itemsize == 16
assert C.sizeof(WidebandAudioParams) == 516

BLANKER_STATS = ("samples", "sum_power", "threshold", "hits", "blanked", "carry_out", "total_samples", "total_hits", "total_blanked")


class WidebandBlankerCounts(C.Structure):
    """msk144_wideband_blanker_counts."""
    _fields_ = [(n, C.c_int64) for n in BLANKER_STATS]


class InputRateParams(C.Structure):
    _fields_ = [("rate_hz", C.c_int64), ("shift", C.c_int32), ("num_taps", C.c_int32), ("taps", C.POINTER(C.c_int16))]


class StreamPingsParams(C.Structure):
    """msk144_stream_pings_params."""
    _fields_ = [("ratio_q4", C.c_int32), ("memory", C.c_int32), ("min_ref", C.c_int32), ("shift", C.c_int32)]


class StreamGateParams(C.Structure):
    """msk144_stream_gate_params."""
    _fields_ = [("hold", C.c_int32), ("min_up", C.c_int32), ("max_streams", C.c_int32), ("ratio_q4", C.c_int32)]


class Params(C.Structure):
    _fields_ = [("center_hz", C.c_float), ("width_hz", C.c_float), ("step_hz", C.c_float), ("scan_depth", C.c_int32),
                ("nbadsync_threshold", C.c_int32), ("read_mode", C.c_int32), ("analytic_method", C.c_int32), ("channels", C.c_int32),
                ("device", C.c_int32), ("max_results", C.c_int32), ("llr_block_channels", C.c_int32)]


_vp, _i32, _P = C.c_void_p, C.c_int32, C.POINTER
# name -> (argtypes, restype) of every symbol include/msk144hip.h declares (tests check the library exports each of them)
PROTOTYPES = {
    "msk144_default_params": ([_P(Params)], None),
    "msk144_create": ([_P(Params), _P(_vp)], C.c_int),
    "msk144_destroy": ([_vp], None),
    "msk144_last_error": ([_vp], C.c_char_p),
    "msk144_geometry": ([_vp, _P(_i32), _P(_i32), _P(_i32)], C.c_int),
    "msk144_frequency": ([_vp, _i32, _P(C.c_float)], C.c_int),
    "msk144_set_stream": ([_vp, _vp], C.c_int),
    "msk144_submit_audio": ([_vp, _vp], C.c_int),
    "msk144_submit_iq": ([_vp, _vp], C.c_int),
    "msk144_submit_audio_device": ([_vp, _vp], C.c_int),
    "msk144_submit_iq_device": ([_vp, _vp], C.c_int),
    "msk144_submit_analytic": ([_vp, _vp], C.c_int),
    "msk144_decode": ([_vp], C.c_int),
    "msk144_decode_stages": ([_vp, C.c_uint32], C.c_int),
    "msk144_synchronize": ([_vp], C.c_int),
    "msk144_results": ([_vp, _vp, _i32, _P(_i32)], C.c_int),
    "msk144_result_count": ([_vp, _P(_i32)], C.c_int),
    "msk144_results_device": ([_vp, _P(_vp), _P(_vp)], C.c_int),
    "msk144_set_channel_base": ([_vp, _i32], C.c_int),
    "msk144_segment_power": ([_vp, _vp], C.c_int),
    "msk144_dump_analytic": ([_vp, _i32, _vp], C.c_int),
    "msk144_dump_mix_table": ([_vp, _i32, _vp], C.c_int),
    "msk144_dump_candidates": ([_vp, _i32, _vp], C.c_int),
    "msk144_dump_indexes": ([_vp, _i32, _vp, _P(_i32)], C.c_int),
    "msk144_load_candidates": ([_vp, _i32, _vp], C.c_int),
    "msk144_set_profiling": ([_vp, _i32], C.c_int),
    "msk144_stage_times": ([_vp, _vp, _vp, _i32], C.c_int),
    "msk144_input_slot": ([_vp, _i32, _P(_vp), _P(C.c_size_t)], C.c_int),
    "msk144_submit_slot": ([_vp, _i32], C.c_int),
    "msk144_submit_slot_n": ([_vp, _i32, _i32], C.c_int),
    "msk144_fetch_async": ([_vp, _i32], C.c_int),
    "msk144_fetch_wait": ([_vp, _i32, _P(_vp), _P(_i32), _P(_vp)], C.c_int),
    "msk144_hop_slot": ([_vp, _i32, _P(_vp), _P(_vp), _P(_vp), _P(_vp)], C.c_int),
    "msk144_push_hops": ([_vp, _i32, _i32], C.c_int),
    "msk144_device_count": ([_P(_i32)], C.c_int),
    "msk144_clock_probe": ([_vp, _i32, _P(C.c_float)], C.c_int),
    "msk144_set_copy_handover": ([_vp, _i32], C.c_int),
    "msk144_copy_handover": ([_vp, _P(_i32)], C.c_int),
    "msk144_copy_count": ([_vp, _P(C.c_int64)], C.c_int),
    "msk144_set_llr_retention": ([_vp, _i32], C.c_int),
    "msk144_llr_block_channels": ([_vp, _P(_i32)], C.c_int),
    "msk144_set_wideband": ([_vp, _P(WidebandParams)], C.c_int),
    "msk144_wideband_slot": ([_vp, _i32, _P(_vp), _P(C.c_size_t)], C.c_int),
    "msk144_push_wideband": ([_vp, _i32, _i32], C.c_int),
    "msk144_dump_wideband_hop": ([_vp, _i32, _vp], C.c_int),
    "msk144_wideband_clip_count": ([_vp, _P(C.c_int64)], C.c_int),
    "msk144_set_wideband_ex": ([_vp, _P(WidebandParams), _P(C.c_double), _i32], C.c_int),
    "msk144_dump_wideband_band": ([_vp, _i32, _vp], C.c_int),
    "msk144_wideband_levels": ([_vp, _vp], C.c_int),
    "msk144_set_wideband_gains": ([_vp, _P(C.c_float)], C.c_int),
    "msk144_set_wideband_agc": ([_vp, _P(WidebandAgc)], C.c_int),
    "msk144_set_wideband_blanker": ([_vp, _P(WidebandBlanker)], C.c_int),
    "msk144_wideband_blanker_stats": ([_vp, _P(WidebandBlankerCounts)], C.c_int),
    "msk144_dump_wideband_blanked": ([_vp, _vp], C.c_int),
    "msk144_set_wideband_spectrum": ([_vp, _P(WidebandSpectrum)], C.c_int),
    "msk144_wideband_spectrum": ([_vp, _P(C.c_double), _P(C.c_int64)], C.c_int),
    "msk144_set_wideband_pings": ([_vp, _P(WidebandPingsParams)], C.c_int),
    "msk144_wideband_pings": ([_vp, _P(WidebandPing)], C.c_int),
    "msk144_wideband_ping_blocks": ([_vp, _i32, _P(_i32), _P(_i32)], C.c_int),
    "msk144_set_wideband_ping_band": ([_vp, _P(WidebandPingBandParams)], C.c_int),
    "msk144_set_wideband_notch": ([_vp, _P(_i32), _i32, _P(WidebandNotchParams)], C.c_int),
    "msk144_wideband_notch_stats": ([_vp, _P(WidebandNotchCount)], C.c_int),
    "msk144_set_wideband_waterfall": ([_vp, _P(WidebandWaterfall)], C.c_int),
    "msk144_wideband_waterfall": ([_vp, _i32, _P(C.c_float), _P(_i32)], C.c_int),
    "msk144_wideband_waterfall_sums": ([_vp, _P(C.c_double)], C.c_int),
    "msk144_set_wideband_capture": ([_vp, _P(WidebandCaptureParams)], C.c_int),
    "msk144_wideband_capture": ([_vp, _P(WidebandCaptureUnit), _P(C.c_int8), _P(_i32), _P(_i32)], C.c_int),
    "msk144_set_wideband_audio": ([_vp, _P(WidebandAudioParams)], C.c_int),
    "msk144_wideband_capture_audio": ([_vp, _P(C.c_int16), _P(_i32), _P(_i32)], C.c_int),
    "msk144_set_wideband_gate": ([_vp, _P(WidebandGateParams), _P(C.c_uint8)], C.c_int),
    "msk144_wideband_gate": ([_vp, _P(_i32), _P(_i32), _P(_i32)], C.c_int),
    "msk144_set_input_rate": ([_vp, _P(InputRateParams)], C.c_int),
    "msk144_rate_hop_slot": ([_vp, _i32, _P(_vp), _P(_vp), _P(_vp), _P(_vp), _P(_i32)], C.c_int),
    "msk144_push_rate_hops": ([_vp, _i32, _i32], C.c_int),
    "msk144_dump_rate_hop": ([_vp, _i32, _vp, _P(_i32)], C.c_int),
    "msk144_input_rate_clamped": ([_vp, _P(_i32)], C.c_int),
    "msk144_input_rate_slot_clamped": ([_vp, _i32, _P(_vp), _P(_i32)], C.c_int),
    "msk144_set_stream_pings": ([_vp, _P(StreamPingsParams)], C.c_int),
    "msk144_stream_pings": ([_vp, _P(WidebandPing), _vp, _P(_i32)], C.c_int),
    "msk144_stream_ping_blocks": ([_vp, _i32, _P(_i32), _P(_i32)], C.c_int),
    "msk144_stream_pings_slot": ([_vp, _i32, _P(_vp), _P(_vp), _P(_vp), _P(_i32)], C.c_int),
    "msk144_set_stream_gate": ([_vp, _P(StreamGateParams), _P(C.c_uint8)], C.c_int),
    "msk144_stream_gate": ([_vp, _P(_i32), _P(_i32), _P(_i32)], C.c_int),
    "msk144_stream_gate_slot": ([_vp, _i32, _P(_vp), _P(_i32), _P(_i32)], C.c_int),
}
ABI_SYMBOLS = tuple(PROTOTYPES)

RESULT_DTYPE = np.dtype([
    ("channel", "<i4"), ("item", "<i4"), ("f0", "<f4"), ("pattern_idx", "<i4"), ("num_avg", "<i4"), ("pos", "<u4"), ("xb", "<f4"),
    ("nbadsync", "<i4"), ("ldpc_iterations", "<i4"), ("ldpc_hard_errors", "<i4"), ("message", "u1", (10,)), ("reserved", "u1", (2,)),
])
assert RESULT_DTYPE.itemsize == 52

CANDIDATE_DTYPE = np.dtype([
    ("block_idx", "<u4"), ("pattern_idx", "<u4"), ("pos", "<u4"), ("f0", "<f4"), ("nbadsync", "<i4"), ("xb", "<f4"),
    ("num_avg", "<i4"), ("softbits_wo_sync", "<f4", (128,)), ("is_message_present", "u1"), ("_pad0", "u1", (3,)),
    ("ldpc_num_iterations", "<i4"), ("ldpc_num_hard_errors", "<i4"), ("message", "i1", (77,)), ("_pad1", "u1", (3,)),
])
assert CANDIDATE_DTYPE.itemsize == ITEM_BYTES


class Msk144Error(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__(f"msk144hip error {code}: {text}")
        self.code = code


_lib = None


def load_library(path: Optional[str] = None):
    """dlopen libmsk144hip.so and declare prototypes.  Raises if it is absent - there is no fallback."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("MSK144HIP_LIBRARY") or LIB_PATH      # MSK144HIP_LIBRARY: same-box A/B of two builds (tools/)
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7.  If torch were
    # imported AFTER this library, two runtimes would be live and the second finds no GPU.  Importing
    # torch first makes the dynamic linker bind libmsk144hip.so to the runtime torch already loaded.
    if "torch" not in sys.modules and not os.environ.get("MSK144_NO_TORCH_PRELOAD") and importlib.util.find_spec("torch"):
        import torch  # noqa: F401
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} not found: build it with `python -m msk144cudecoder_amd.build` (hipcc, gfx950)")
    L = C.CDLL(p)
    for name, (argtypes, restype) in PROTOTYPES.items():
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes, restype
    if path is None:
        _lib = L
    return L


def default_params() -> Params:
    p = Params()
    load_library().msk144_default_params(C.byref(p))
    return p


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class HipDecoder:
    """One msk144_handle: `channels` independent windows per decode on one MI355X."""

    def __init__(self, center=1500.0, width=200.0, step=2.0, depth=4, nbadsync_threshold=1, read_mode=1, analytic_method=2,
                 channels=1, device=0, max_results=0, llr_block_channels=0):
        self.L = load_library()
        p = Params(center, width, step, depth, nbadsync_threshold, read_mode, analytic_method, channels, device, max_results, llr_block_channels)
        self.params = p
        self.h = C.c_void_p()
        rc = self.L.msk144_create(C.byref(p), C.byref(self.h))
        if rc != 0:
            raise Msk144Error(rc, (self.L.msk144_last_error(None) or b"").decode())
        f, d, k = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self.L.msk144_geometry(self.h, C.byref(f), C.byref(d), C.byref(k)))
        self.F, self.D, self.K = f.value, d.value, k.value
        self.channels = channels
        self.read_mode = read_mode
        self._ir_taps, self._ir_last_n = None, 0   # the resampler's taps (kept alive for the library's call) and n of its last push
        self._wb_spectrum_bins = self._wb_spectrum_last = 0   # bins of the next wideband push and of the last one; 0: no spectrum
        b = C.c_int32()
        self._chk(self.L.msk144_llr_block_channels(self.h, C.byref(b)))
        self.llr_block = b.value            # channels per softbits -> index -> LDPC block (the library's choice when llr_block_channels = 0)

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.msk144_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, allow=()):
        if rc != 0 and rc not in allow:
            raise Msk144Error(rc, (self.L.msk144_last_error(self.h) or b"").decode())
        return rc

    def frequency(self, b: int) -> float:
        v = C.c_float()
        self._chk(self.L.msk144_frequency(self.h, b, C.byref(v)))
        return v.value

    def set_stream(self, hip_stream: int):
        self._chk(self.L.msk144_set_stream(self.h, C.c_void_p(hip_stream)))

    # ---- front end ----
    def submit_audio(self, windows: np.ndarray):
        w = np.ascontiguousarray(windows, dtype=np.int16).reshape(self.channels, 5184)
        self._chk(self.L.msk144_submit_audio(self.h, _ptr(w)))

    def submit_iq(self, windows: np.ndarray):
        w = np.ascontiguousarray(windows, dtype=np.int8).reshape(self.channels, 2 * 5184)
        self._chk(self.L.msk144_submit_iq(self.h, _ptr(w)))

    def submit_audio_device(self, dev_ptr: int):
        self._chk(self.L.msk144_submit_audio_device(self.h, C.c_void_p(dev_ptr)))

    def submit_iq_device(self, dev_ptr: int):
        self._chk(self.L.msk144_submit_iq_device(self.h, C.c_void_p(dev_ptr)))

    def submit_analytic(self, windows: np.ndarray):
        w = np.ascontiguousarray(windows, dtype=np.complex64).reshape(self.channels, 5184)
        self._chk(self.L.msk144_submit_analytic(self.h, _ptr(w)))

    # ---- decode ----
    def decode(self, stages: int = STAGE_ALL):
        self._chk(self.L.msk144_decode_stages(self.h, stages))

    def synchronize(self):
        self._chk(self.L.msk144_synchronize(self.h))

    def result_count(self) -> int:
        n = C.c_int32()
        self._chk(self.L.msk144_result_count(self.h, C.byref(n)))
        return n.value

    def results(self) -> np.ndarray:
        n = self.result_count()
        out = np.zeros(max(n, 1), dtype=RESULT_DTYPE)
        got = C.c_int32()
        self._chk(self.L.msk144_results(self.h, _ptr(out), len(out), C.byref(got)), allow=(-5,))
        return out[:min(n, len(out))]

    def results_device(self):
        rec, cnt = C.c_void_p(), C.c_void_p()
        self._chk(self.L.msk144_results_device(self.h, C.byref(rec), C.byref(cnt)))
        return rec.value, cnt.value

    def set_channel_base(self, base: int):
        """Result records carry channel = base + local channel (global ids for the multi-GPU gather)."""
        self._chk(self.L.msk144_set_channel_base(self.h, base))

    def set_llr_retention(self, retain: bool):
        """A one-block handle (llr_block_channels = channels) keeps every LLR row readable (dumps).  retain=False: behave like a
        blocked handle - early nbadsync gate, copies handed over, dumps refused (what msk144hipdecoder asks for)."""
        self._chk(self.L.msk144_set_llr_retention(self.h, 1 if retain else 0))

    def set_copy_handover(self, on: bool):
        """Blocked staging only: whether a slot that folds the same frames as a lower slot of its group reports that slot's result
        (default) or is demodulated and decoded on its own, as the reference does."""
        self._chk(self.L.msk144_set_copy_handover(self.h, 1 if on else 0))

    def copy_handover(self) -> bool:
        v = C.c_int32()
        self._chk(self.L.msk144_copy_handover(self.h, C.byref(v)))
        return bool(v.value)

    def copy_count(self) -> int:
        """Slots of the last decode that were handed to a lower slot of their group."""
        v = C.c_int64()
        self._chk(self.L.msk144_copy_count(self.h, C.byref(v)))
        return int(v.value)

    def segment_power(self) -> np.ndarray:
        out = np.empty((self.channels, 8), dtype=np.float32)
        self._chk(self.L.msk144_segment_power(self.h, _ptr(out)))
        return out

    # ---- pinned staging slots (pipelined hops) ----
    def input_slot(self, slot: int) -> np.ndarray:
        """The slot's pinned window buffer as a numpy view: int16 [channels][5184] or int8 [channels][2*5184]."""
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._chk(self.L.msk144_input_slot(self.h, slot, C.byref(ptr), C.byref(nbytes)))
        raw = (C.c_uint8 * nbytes.value).from_address(ptr.value)
        a = np.frombuffer(raw, dtype=np.int8 if self.read_mode == 2 else np.int16)
        return a.reshape(self.channels, -1)

    def submit_slot(self, slot: int, n_channels: int = 0):
        """n_channels > 0: the hop covers only the first n_channels windows of the slot."""
        self._chk(self.L.msk144_submit_slot_n(self.h, slot, n_channels) if n_channels else self.L.msk144_submit_slot(self.h, slot))

    def hop_slot(self, slot: int):
        """(hops, first_halves, streams, is_first): numpy views of the slot's pinned hop-ring inputs - hops and first_halves as
        [channels][2592] int16 or [channels][2*2592] int8, streams int32[channels], is_first uint8[channels]."""
        p = [C.c_void_p() for _ in range(4)]
        self._chk(self.L.msk144_hop_slot(self.h, slot, *[C.byref(x) for x in p]))
        half = 5184  # bytes of half a window in both read modes
        dt = np.int8 if self.read_mode == 2 else np.int16
        hops = np.frombuffer((C.c_uint8 * (half * self.channels)).from_address(p[0].value), dtype=dt).reshape(self.channels, -1)
        first = np.frombuffer((C.c_uint8 * (half * self.channels)).from_address(p[1].value), dtype=dt).reshape(self.channels, -1)
        streams = np.frombuffer((C.c_int32 * self.channels).from_address(p[2].value), dtype=np.int32)
        is_first = np.frombuffer((C.c_uint8 * self.channels).from_address(p[3].value), dtype=np.uint8)
        return hops, first, streams, is_first

    def push_hops(self, slot: int, n: int):
        self._chk(self.L.msk144_push_hops(self.h, slot, n))

    def fetch_async(self, slot: int):
        self._chk(self.L.msk144_fetch_async(self.h, slot))

    def fetch_wait(self, slot: int):
        """(records, segment powers [channels][8]) of the slot, copied out of its pinned output."""
        rec, seg, n = C.c_void_p(), C.c_void_p(), C.c_int32()
        self._chk(self.L.msk144_fetch_wait(self.h, slot, C.byref(rec), C.byref(n), C.byref(seg)))
        records = np.frombuffer((C.c_uint8 * (n.value * RESULT_DTYPE.itemsize)).from_address(rec.value), dtype=RESULT_DTYPE).copy() if n.value else np.zeros(0, dtype=RESULT_DTYPE)
        powers = np.frombuffer((C.c_float * (8 * self.channels)).from_address(seg.value), dtype=np.float32).reshape(self.channels, 8).copy()
        return records, powers

    # ---- audio input at 24 to 192 kHz (read_mode 1 handles) ----
    def set_input_rate(self, rate_hz, taps=None, taps_per_phase: int = 16, shift: Optional[int] = None):
        """Resample every stream's hops from rate_hz to 12 kHz on the device (include/msk144hip.h).  taps=None: the default design of
        libmsk144host.so, input_rate.default_taps(rate_hz, taps_per_phase), with shift 14; otherwise int16 taps, K x P of them, and
        their shift.  rate_hz None switches the resampler off."""
        self._ir_last_n = 0
        if rate_hz is None:
            self._chk(self.L.msk144_set_input_rate(self.h, None))
            self._ir_taps = None
            return
        from .input_rate import DEFAULT_SHIFT, default_taps
        if taps is None:
            taps = default_taps(int(rate_hz), taps_per_phase)
        t = np.asarray(taps)
        if t.ndim != 1 or not np.issubdtype(t.dtype, np.integer) or np.any(t < -32768) or np.any(t > 32767):
            raise ValueError("taps must be a row of int16 values")
        self._ir_taps = np.ascontiguousarray(t, dtype=np.int16)
        p = InputRateParams(int(rate_hz), DEFAULT_SHIFT if shift is None else int(shift), len(self._ir_taps), self._ir_taps.ctypes.data_as(C.POINTER(C.c_int16)))
        self._chk(self.L.msk144_set_input_rate(self.h, C.byref(p)))

    def rate_hop_slot(self, slot: int):
        """(hops, first_halves, streams, is_first): numpy views of the slot's pinned inputs at the input rate - hops and first_halves as
        int16 [channels][2592 P/Q], streams int32[channels], is_first uint8[channels]."""
        p = [C.c_void_p() for _ in range(4)]
        row = C.c_int32()
        self._chk(self.L.msk144_rate_hop_slot(self.h, slot, *[C.byref(x) for x in p], C.byref(row)))
        n = row.value * self.channels
        hops = np.frombuffer((C.c_int16 * n).from_address(p[0].value), dtype=np.int16).reshape(self.channels, row.value)
        first = np.frombuffer((C.c_int16 * n).from_address(p[1].value), dtype=np.int16).reshape(self.channels, row.value)
        streams = np.frombuffer((C.c_int32 * self.channels).from_address(p[2].value), dtype=np.int32)
        is_first = np.frombuffer((C.c_uint8 * self.channels).from_address(p[3].value), dtype=np.uint8)
        return hops, first, streams, is_first

    def push_rate_hops(self, slot: int, n: int):
        self._chk(self.L.msk144_push_rate_hops(self.h, slot, n))
        self._ir_last_n = int(n)

    def dump_rate_hop(self, j: int) -> np.ndarray:
        """int16 resampled samples of position j of the last push: 5184 for a first hop, else 2592."""
        out = np.empty(5184, dtype=np.int16)
        n = C.c_int32()
        self._chk(self.L.msk144_dump_rate_hop(self.h, j, _ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def input_rate_clamped(self) -> np.ndarray:
        """int32 [n of the last push]: clamped output samples by position."""
        out = np.zeros(max(self._ir_last_n, 1), dtype=np.int32)   # one spare element: before any push the library answers ESTATE
        self._chk(self.L.msk144_input_rate_clamped(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out[:self._ir_last_n]

    def input_rate_slot_clamped(self, slot: int) -> np.ndarray:
        """The same for the slot's last push, without a wait: valid once fetch_wait(slot) of that hop has returned."""
        p, n = C.c_void_p(), C.c_int32()
        self._chk(self.L.msk144_input_rate_slot_clamped(self.h, slot, C.byref(p), C.byref(n)))
        return np.frombuffer((C.c_int32 * n.value).from_address(p.value), dtype=np.int32).copy()

    # ---- per-stream levels and pings of the audio hops (read_mode 1 handles) ----
    def set_stream_pings(self, params=True, **kw):
        """Levels and a ping record per listed stream from the next push_hops / push_rate_hops on (include/msk144hip.h):
        set_stream_pings() takes the defaults (stream_pings.STREAM_PINGS_DEFAULTS), keywords replace single ones (ratio_q4, memory,
        min_ref, shift); set_stream_pings(None) switches it off."""
        if params is None:
            self._chk(self.L.msk144_set_stream_pings(self.h, None))
            return
        from .stream_pings import STREAM_PINGS_DEFAULTS
        p = dict(STREAM_PINGS_DEFAULTS)
        if isinstance(params, dict):
            p.update(params)
        p.update(kw)
        a = StreamPingsParams(**{k: int(v) for k, v in p.items()})
        self._chk(self.L.msk144_set_stream_pings(self.h, C.byref(a)))

    def stream_pings(self):
        """(records PING_DTYPE [n], levels stream_pings.LEVEL_DTYPE [n]) of the last push, by position; waits for it."""
        from .stream_pings import LEVEL_DTYPE as STREAM_LEVEL_DTYPE
        rec, lev, n = np.zeros(self.channels, dtype=PING_DTYPE), np.zeros(self.channels, dtype=STREAM_LEVEL_DTYPE), C.c_int32()
        self._chk(self.L.msk144_stream_pings(self.h, rec.ctypes.data_as(C.POINTER(WidebandPing)), _ptr(lev), C.byref(n)))
        return rec[:n.value].copy(), lev[:n.value].copy()

    def stream_ping_blocks(self, j: int) -> np.ndarray:
        """int32 [nb] block energies of position j of the last push: nb = 54 for a first hop, else 27."""
        out, nb = np.zeros(PING_MAX_BLOCKS, dtype=np.int32), C.c_int32()
        self._chk(self.L.msk144_stream_ping_blocks(self.h, int(j), out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nb)))
        return out[:nb.value].copy()

    def stream_pings_slot(self, slot: int):
        """(records [n], levels [n], energies int32 [n][54]) of the slot's last push, without a wait: valid once fetch_wait(slot) of
        that hop has returned."""
        from .stream_pings import LEVEL_DTYPE as STREAM_LEVEL_DTYPE
        r, l, e, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
        self._chk(self.L.msk144_stream_pings_slot(self.h, slot, C.byref(r), C.byref(l), C.byref(e), C.byref(n)))
        k = n.value
        rec = np.frombuffer((C.c_uint8 * (k * PING_DTYPE.itemsize)).from_address(r.value), dtype=PING_DTYPE).copy()
        lev = np.frombuffer((C.c_uint8 * (k * STREAM_LEVEL_DTYPE.itemsize)).from_address(l.value), dtype=STREAM_LEVEL_DTYPE).copy()
        en = np.frombuffer((C.c_int32 * (k * PING_MAX_BLOCKS)).from_address(e.value), dtype=np.int32).reshape(k, PING_MAX_BLOCKS).copy()
        return rec, lev, en

    # ---- the stream gate: only the streams with activity are decoded (read_mode 1 handles) ----
    def set_stream_gate(self, hold=1, min_up=1, max_streams=None, ratio_q4=0, always=()):
        """The stream gate from the next push_hops / push_rate_hops on (include/msk144hip.h "Stream gate"): a listed stream's window
        is decoded while the stream had a hop with at least `min_up` up blocks within its last `hold` hops, or is one of the `always`
        streams (stream numbers); at most `max_streams` per push (None: all); ratio_q4 0 takes the stream-ping records' up masks,
        another value the gate's own ratio on their energies.  set_stream_gate(None) switches it off.  Either ends the last push's
        list: stream_gate() raises (MSK144_ESTATE) until the next gated push.  Records of a gated decode carry list indices as
        channel."""
        if hold is None:
            self._chk(self.L.msk144_set_stream_gate(self.h, None, None))
            return
        flags = np.zeros(self.channels, dtype=np.uint8)
        for s in always:
            if not 0 <= int(s) < self.channels:
                raise ValueError(f"always stream {s} is out of range")
            flags[int(s)] = 1
        p = StreamGateParams(int(hold), int(min_up), 0 if max_streams is None else int(max_streams), int(ratio_q4))
        self._chk(self.L.msk144_set_stream_gate(self.h, C.byref(p), flags.ctypes.data_as(C.POINTER(C.c_uint8))))

    def stream_gate(self):
        """(positions, total) of the last push: the int32 positions j whose window it decodes, ascending - index i of the list is
        what the decode's records carry as channel - and the number that qualified, of which total - len(positions) were dropped.
        Waits for the gate's event only."""
        out = np.zeros(self.channels, dtype=np.int32)
        count, total = C.c_int32(), C.c_int32()
        self._chk(self.L.msk144_stream_gate(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(count), C.byref(total)))
        return out[:count.value].copy(), total.value

    def stream_gate_slot(self, slot: int):
        """The same for the slot's last push, without a wait: valid once fetch_wait(slot) of that hop has returned."""
        p, count, total = C.c_void_p(), C.c_int32(), C.c_int32()
        self._chk(self.L.msk144_stream_gate_slot(self.h, slot, C.byref(p), C.byref(count), C.byref(total)))
        k = count.value
        return (np.frombuffer((C.c_int32 * k).from_address(p.value), dtype=np.int32).copy() if k else np.zeros(0, dtype=np.int32)), total.value

    # ---- wideband channeliser (read_mode 2 handles) ----
    def set_wideband(self, rate_hz: int, offsets_hz, fmt: str = "cu8", taps=None, taps_per_phase: int = 16, gain: float = 100.0, bank_taps=None):
        """Configure the down-converter bank: one channel per offset (len == channels).  taps=None: the default design of
        libmsk144host.so, wideband.default_taps_for_rate (rate_hz = 12000 x P/Q: K*P taps summing to Q).  Above 6.144 Msps the taps are the channeliser's at rate_hz/32 (the default: the same
        design at that rate) and bank_taps the analysis bank's (64 K1 taps; None: the default bank)."""
        from .wideband import default_taps_for_rate, rate_ratio, stage2_rate
        rate2 = stage2_rate(int(rate_hz)) if int(rate_hz) > 0 else 0
        P, Q = rate_ratio(int(rate_hz)) if int(rate_hz) > 0 else (0, 1)
        P2, Q2 = rate_ratio(rate2) if rate2 > 0 else (0, 1)
        if taps is None:
            taps = default_taps_for_rate(rate2, taps_per_phase)
        self._wb_taps = np.ascontiguousarray(taps, dtype=np.float64)
        self._wb_offsets = np.ascontiguousarray(offsets_hz, dtype=np.int32)
        self._wb_format = fmt
        self._wb_P, self._wb_Q = P, Q
        self._wb_bank_ratio = (P2, Q2)
        self._wb_bank_taps = None if bank_taps is None else np.ascontiguousarray(bank_taps, dtype=np.float64)
        self._wb_spectrum_bins = self._wb_spectrum_last = 0   # a new configuration has no spectrum
        wp = WidebandParams(int(rate_hz), WB_FORMATS[fmt], int(taps_per_phase), float(gain), len(self._wb_taps),
                            self._wb_taps.ctypes.data_as(C.POINTER(C.c_double)), self._wb_offsets.ctypes.data_as(C.POINTER(C.c_int32)),
                            len(self._wb_offsets))
        if self._wb_bank_taps is None:
            self._chk(self.L.msk144_set_wideband_ex(self.h, C.byref(wp), None, 0))
        else:
            self._chk(self.L.msk144_set_wideband_ex(self.h, C.byref(wp), self._wb_bank_taps.ctypes.data_as(C.POINTER(C.c_double)), len(self._wb_bank_taps)))

    def wideband_slot(self, slot: int) -> np.ndarray:
        """The slot's pinned wideband buffer as a numpy view of raw sample components (uint8 / int8 / int16, I,Q interleaved)."""
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._chk(self.L.msk144_wideband_slot(self.h, slot, C.byref(ptr), C.byref(nbytes)))
        dt = {"cu8": np.uint8, "cs8": np.int8, "cs16": np.int16}[self._wb_format]
        return np.frombuffer((C.c_uint8 * nbytes.value).from_address(ptr.value), dtype=dt)

    def push_wideband(self, slot: int, samples: Optional[np.ndarray] = None, first: bool = False):
        """samples (raw components, 2*5184*P/Q for a first push, else 2*2592*P/Q; P/Q = D at an integer rate) are copied into the
        slot first when given."""
        if samples is not None:
            buf = self.wideband_slot(slot)
            a = np.asarray(samples).reshape(-1)
            want = 2 * (5184 if first else 2592) // self._wb_Q * self._wb_P
            if a.size != want:
                raise ValueError(f"a {'first' if first else 'later'} push carries {want} components, got {a.size}")
            buf[:want] = a
        self._chk(self.L.msk144_push_wideband(self.h, slot, 1 if first else 0))
        self._wb_last_first = bool(first)
        self._wb_spectrum_last = self._wb_spectrum_bins

    def dump_wideband_hop(self, channel: int) -> np.ndarray:
        """int8 [n][2] I/Q of the channel's last push (n = 5184 after a first push, else 2592)."""
        out = np.empty((5184 if getattr(self, "_wb_last_first", True) else 2592, 2), dtype=np.int8)
        self._chk(self.L.msk144_dump_wideband_hop(self.h, channel, _ptr(out)))
        return out

    def dump_wideband_band(self, band: int) -> np.ndarray:
        """complex64 s_k[n] of band k (-32..32) from the last push at a bank rate: 5184 or 2592 x P/Q samples, P/Q = (rate/32)/12000."""
        P2, Q2 = self._wb_bank_ratio
        out = np.empty((5184 if getattr(self, "_wb_last_first", True) else 2592) * P2 // Q2, dtype=np.complex64)
        self._chk(self.L.msk144_dump_wideband_band(self.h, int(band), _ptr(out)))
        return out

    def wideband_clip_count(self) -> int:
        v = C.c_int64()
        self._chk(self.L.msk144_wideband_clip_count(self.h, C.byref(v)))
        return int(v.value)

    def set_wideband_gains(self, gains=None):
        """One gain per channel from the next push on (None: back to the scalar gain of set_wideband); zeroes the AGC exponents."""
        if gains is None:
            self._chk(self.L.msk144_set_wideband_gains(self.h, None))
            return
        g = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        if g.size != self.channels:
            raise ValueError(f"one gain per channel: {self.channels}, got {g.size}")
        self._chk(self.L.msk144_set_wideband_gains(self.h, g.ctypes.data_as(C.POINTER(C.c_float))))

    def set_wideband_agc(self, params=True, **kw):
        """The stepped AGC from the next push on: set_wideband_agc() takes the defaults (AGC_DEFAULTS), keywords replace single ones
        (lo_sq, hi_sq, clip_ppm, hold, min_exp, max_exp); set_wideband_agc(None) switches it off."""
        if params is None:
            self._chk(self.L.msk144_set_wideband_agc(self.h, None))
            return
        p = dict(AGC_DEFAULTS)
        if isinstance(params, dict):
            p.update(params)
        p.update(kw)
        a = WidebandAgc(**{k: int(v) for k, v in p.items()})
        self._chk(self.L.msk144_set_wideband_agc(self.h, C.byref(a)))

    def wideband_levels(self) -> np.ndarray:
        """LEVEL_DTYPE [channels]: samples, sum_sq, clipped, gain and AGC exponent of the last push."""
        out = np.zeros(self.channels, dtype=LEVEL_DTYPE)
        self._chk(self.L.msk144_wideband_levels(self.h, _ptr(out)))
        return out

    def set_wideband_blanker(self, params=True, **kw):
        """The impulse-noise blanker from the next first push on: set_wideband_blanker() takes the defaults (BLANKER_DEFAULTS),
        keywords replace single ones (threshold_q4, pre, post); set_wideband_blanker(None) switches it off."""
        if params is None:
            self._chk(self.L.msk144_set_wideband_blanker(self.h, None))
            return
        p = dict(BLANKER_DEFAULTS)
        if isinstance(params, dict):
            p.update(params)
        p.update(kw)
        b = WidebandBlanker(**{k: int(v) for k, v in p.items()})
        self._chk(self.L.msk144_set_wideband_blanker(self.h, C.byref(b)))

    def wideband_blanker_stats(self) -> dict:
        """The blanker's statistics of the last push and its totals since the first push (BLANKER_STATS), as Python integers."""
        st = WidebandBlankerCounts()
        self._chk(self.L.msk144_wideband_blanker_stats(self.h, C.byref(st)))
        return {n: int(getattr(st, n)) for n in BLANKER_STATS}

    def dump_wideband_blanked(self) -> np.ndarray:
        """int16 [n][2] I/Q: the new samples of the last push as the channeliser saw them (n = 5184 P/Q after a first push, else 2592 P/Q)."""
        out = np.empty(((5184 if getattr(self, "_wb_last_first", True) else 2592) // self._wb_Q * self._wb_P, 2), dtype=np.int16)
        self._chk(self.L.msk144_dump_wideband_blanked(self.h, _ptr(out)))
        return out

    def set_wideband_spectrum(self, bins=1024, window=None):
        """The power spectrum of every push's input samples from the next push on (include/msk144hip.h): bins a power of two within
        256..8192 and no longer than a later push, window `bins` finite values (None: periodic Hann).
        set_wideband_spectrum(None) switches it off."""
        if bins is None:
            self._chk(self.L.msk144_set_wideband_spectrum(self.h, None))
            self._wb_spectrum_bins = 0
            return
        w = None if window is None else np.ascontiguousarray(window, dtype=np.float64)
        if w is not None and w.shape != (int(bins),):
            raise ValueError("the window must hold `bins` values")
        p = WidebandSpectrum(int(bins), None if w is None else w.ctypes.data_as(C.POINTER(C.c_double)))
        self._chk(self.L.msk144_set_wideband_spectrum(self.h, C.byref(p)))
        self._wb_spectrum_bins = int(bins)

    def wideband_spectrum(self):
        """(float64 [bins] in ascending frequency - power[j] at (j - bins/2) Fs / bins -, segments) of the last push."""
        out = np.zeros(max(self._wb_spectrum_last, 1), dtype=np.float64)   # no spectrum in the last push: the library writes nothing
        seg = C.c_int64()
        self._chk(self.L.msk144_wideband_spectrum(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(seg)))
        return out, int(seg.value)

    def set_wideband_pings(self, params=True, **kw):
        """The ping detector from the next push on (include/msk144hip.h): set_wideband_pings() takes the defaults (PINGS_DEFAULTS),
        keywords replace single ones (ratio_q4, memory, min_ref); set_wideband_pings(None) switches it off."""
        if params is None:
            self._chk(self.L.msk144_set_wideband_pings(self.h, None))
            return
        p = dict(PINGS_DEFAULTS)
        if isinstance(params, dict):
            p.update(params)
        p.update(kw)
        a = WidebandPingsParams(**{k: int(v) for k, v in p.items()})
        self._chk(self.L.msk144_set_wideband_pings(self.h, C.byref(a)))

    def set_wideband_ping_band(self, centre_hz=0, halfwidth_hz: int = 1500, taps=None, shift: Optional[int] = None):
        """The ping band from the next push on (include/msk144hip.h): the detector then runs on in-band energies.
        set_wideband_ping_band() takes the default design around centre_hz +- halfwidth_hz (wideband.ping_band_taps);
        taps (int8 [k][2], k <= 64) and shift give a filter of one's own; set_wideband_ping_band(None) switches it off."""
        if centre_hz is None:
            self._chk(self.L.msk144_set_wideband_ping_band(self.h, None))
            return
        if taps is None:
            from .wideband import ping_band_taps
            t, s = ping_band_taps(centre_hz, halfwidth_hz)
            shift = s if shift is None else shift
        else:
            if shift is None:
                raise ValueError("taps need a shift")
            t = np.asarray(taps)
            if t.ndim != 2 or t.shape[1] != 2 or not 1 <= t.shape[0] <= 64 or np.any(t != t.astype(np.int8)):
                raise ValueError("taps must be int8 [k][2] with 1 <= k <= 64")
        a = WidebandPingBandParams()
        full = np.zeros((64, 2), dtype=np.int8)
        full[:t.shape[0]] = t
        C.memmove(a.taps, full.ctypes.data, full.nbytes)
        a.shift = int(shift)
        self._chk(self.L.msk144_set_wideband_ping_band(self.h, C.byref(a)))

    def wideband_pings(self) -> np.ndarray:
        """PING_DTYPE [channels]: up mask, blocks, history, quiet level, reference, peak and peak block of the last push."""
        out = np.zeros(self.channels, dtype=PING_DTYPE)
        self._chk(self.L.msk144_wideband_pings(self.h, out.ctypes.data_as(C.POINTER(WidebandPing))))
        return out

    def wideband_ping_blocks(self, channel: Optional[int] = None) -> np.ndarray:
        """int32 [nb] block energies of the channel's last push (nb = 54 after a first push, else 27); channel None: every channel's,
        int32 [channels][nb]."""
        out = np.zeros((self.channels if channel is None else 1, PING_MAX_BLOCKS), dtype=np.int32)
        n = C.c_int32()
        self._chk(self.L.msk144_wideband_ping_blocks(self.h, -1 if channel is None else int(channel), out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)))
        return out[:, :n.value].copy() if channel is None else out[0, :n.value].copy()

    def set_wideband_notch(self, table=None):
        """The notch table from the next push on (include/msk144hip.h): {channel: [f_hz, ...]} takes the default design for 1 or 2
        frequencies relative to the channel's offset (wideband.notch_taps, halfwidth_hz = 100), {channel: (taps, shift)} a filter of
        one's own (taps int8 [k][2], k <= 64).  The table replaces the one before it: a channel whose entry is unchanged keeps its
        tail, a new or changed one starts from silence.  set_wideband_notch(None), or an empty table, switches the notch off."""
        if not table:
            self._chk(self.L.msk144_set_wideband_notch(self.h, None, 0, None))
            return
        from .wideband import notch_entry
        chans = sorted(int(c) for c in table)
        if len(set(chans)) != len(table):
            raise ValueError("a channel is listed twice")
        arr = (WidebandNotchParams * len(chans))()
        for a, c in zip(arr, chans):
            t, s = notch_entry(table[c])
            C.memmove(a.taps, t.ctypes.data, t.nbytes)
            a.shift = int(s)
        self._chk(self.L.msk144_set_wideband_notch(self.h, (C.c_int32 * len(chans))(*chans), len(chans), arr))

    def wideband_notch_stats(self) -> np.ndarray:
        """NOTCH_COUNT_DTYPE [channels]: whether the channel was notched in the last push, and the components of it that sat8 clamped."""
        out = np.zeros(self.channels, dtype=NOTCH_COUNT_DTYPE)
        self._chk(self.L.msk144_wideband_notch_stats(self.h, out.ctypes.data_as(C.POINTER(WidebandNotchCount))))
        return out

    def set_wideband_waterfall(self, window="hann"):
        """The per-channel waterfall from the next push on (include/msk144hip.h): set_wideband_waterfall() takes the periodic Hann
        window, set_wideband_waterfall(w) 96 finite values; set_wideband_waterfall(None) switches it off."""
        if window is None:
            self._chk(self.L.msk144_set_wideband_waterfall(self.h, None))
            return
        w = None if isinstance(window, str) and window == "hann" else np.ascontiguousarray(window, dtype=np.float64)
        if w is not None and w.shape != (WATERFALL_BINS,):
            raise ValueError("the window must hold 96 values")
        p = WidebandWaterfall(None if w is None else w.ctypes.data_as(C.POINTER(C.c_double)))
        self._chk(self.L.msk144_set_wideband_waterfall(self.h, C.byref(p)))

    def wideband_waterfall(self, channel: Optional[int] = None) -> np.ndarray:
        """float32 [nb][96] of the channel's last push - rows[b][j] the power of block b at (j - 48) x 125 Hz from the channel's
        offset, nb = 54 after a first push, else 27; channel None: every channel's, float32 [channels][nb][96]."""
        out = np.zeros((self.channels if channel is None else 1, WATERFALL_ROWS, WATERFALL_BINS), dtype=np.float32)
        n = C.c_int32()
        self._chk(self.L.msk144_wideband_waterfall(self.h, -1 if channel is None else int(channel), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n)))
        return out[:, :n.value].copy() if channel is None else out[0, :n.value].copy()

    def wideband_waterfall_sums(self) -> np.ndarray:
        """float64 [channels][96]: every channel's rows of the last push added in double, block by block."""
        out = np.zeros((self.channels, WATERFALL_BINS), dtype=np.float64)
        self._chk(self.L.msk144_wideband_waterfall_sums(self.h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def set_wideband_capture(self, pre=1, post=1, max_units=None, channels=()):
        """The per-ping capture from the next push on (include/msk144hip.h): `pre` 0 or 1 hops of pre-roll, `post` hops kept after the
        last active one, at most `max_units` units stored per push (None: min(2 x channels, 512)), `channels` up to 16 listed channels
        that are kept whether active or not; set_wideband_capture(None) switches it off.  Either ends the last push's units:
        wideband_capture() raises (MSK144_ESTATE) until the next push made with capture on."""
        if pre is None:
            self._chk(self.L.msk144_set_wideband_capture(self.h, None))
            return
        listed = [int(c) for c in channels]
        if len(listed) > 16:
            raise ValueError("capture lists at most 16 channels")
        n = capture_default_max_units(self.channels) if max_units is None else int(max_units)
        p = WidebandCaptureParams(int(pre), int(post), n, len(listed), (C.c_int32 * 16)(*listed))
        self._chk(self.L.msk144_set_wideband_capture(self.h, C.byref(p)))
        self._capture_units = n   # what a push made from now on stores at the most; `set` ends the units of the push before it

    def wideband_capture(self):
        """(units, data, total) of the last push: CAPTURE_DTYPE [count] by channel then by hop, their int8 I/Q [count][2592][2] - the
        bytes dump_wideband_hop returned for that hop in the push that carried it - and the number of units the push had, of which
        total - count were dropped."""
        cap = max(getattr(self, "_capture_units", 0), 1)
        units = np.zeros(cap, dtype=CAPTURE_DTYPE)
        data = np.zeros((cap, CAPTURE_UNIT_BYTES // 2, 2), dtype=np.int8)
        count, total = C.c_int32(), C.c_int32()
        self._chk(self.L.msk144_wideband_capture(self.h, units.ctypes.data_as(C.POINTER(WidebandCaptureUnit)), data.ctypes.data_as(C.POINTER(C.c_int8)), C.byref(count),
                                                 C.byref(total)))
        return units[:count.value].copy(), data[:count.value].copy(), total.value

    def set_wideband_audio(self, centre_hz=0, halfwidth_hz: int = 1250, tone_hz: int = 1500, taps=None, phasor=None, shift: Optional[int] = None):
        """The audio from the next push on (include/msk144hip.h): every channel's hops as real int16 audio at 12000 samples per second.
        set_wideband_audio() takes the default design - centre_hz +- halfwidth_hz comes out around tone_hz (wideband.audio_design);
        taps (int8 [k][2], k <= 64), phasor (int16 [96][2]) and shift give a filter and a table of one's own;
        set_wideband_audio(None) switches it off.  Either ends the last push's rows: wideband_capture_audio() raises (MSK144_ESTATE)
        until the next push made with the audio and the capture on."""
        if centre_hz is None:
            self._chk(self.L.msk144_set_wideband_audio(self.h, None))
            return
        if taps is None and phasor is None:
            from .wideband import audio_design
            t, w, s = audio_design(centre_hz, halfwidth_hz, tone_hz)
            shift = s if shift is None else shift
        else:
            if taps is None or phasor is None or shift is None:
                raise ValueError("taps, phasor and shift come together")
            t, w = np.asarray(taps), np.asarray(phasor)
            if t.ndim != 2 or t.shape[1] != 2 or not 1 <= t.shape[0] <= 64 or np.any(t != t.astype(np.int8)):
                raise ValueError("taps must be int8 [k][2] with 1 <= k <= 64")
            if w.shape != (96, 2) or np.any(w != w.astype(np.int16)):
                raise ValueError("phasor must be int16 [96][2]")
        a = WidebandAudioParams()
        full = np.zeros((64, 2), dtype=np.int8)
        full[:t.shape[0]] = t
        w16 = np.ascontiguousarray(w, dtype=np.int16)
        C.memmove(a.taps, full.ctypes.data, full.nbytes)
        C.memmove(a.phasor, w16.ctypes.data, w16.nbytes)
        a.shift = int(shift)
        self._chk(self.L.msk144_set_wideband_audio(self.h, C.byref(a)))

    def wideband_capture_audio(self):
        """(audio, clamped) of the last push: int16 [count][2592], row u the audio of unit u of wideband_capture(), and int32 [count],
        the samples of that hop that the clamp to int16 changed."""
        cap = max(getattr(self, "_capture_units", 0), 1)
        audio = np.zeros((cap, CAPTURE_UNIT_BYTES // 2), dtype=np.int16)
        clamped = np.zeros(cap, dtype=np.int32)
        count = C.c_int32()
        self._chk(self.L.msk144_wideband_capture_audio(self.h, audio.ctypes.data_as(C.POINTER(C.c_int16)), clamped.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(count)))
        return audio[:count.value].copy(), clamped[:count.value].copy()

    def set_wideband_gate(self, hold=1, min_up=1, max_channels=None, always=()):
        """The gate from the next push on (include/msk144hip.h): a channel's window is decoded while the channel had a hop with at
        least `min_up` up blocks within the last `hold` hops, or is one of the `always` channels; at most `max_channels` per push
        (None: all).  set_wideband_gate(None) switches it off.  Either ends the last push's list: wideband_gate() raises
        (MSK144_ESTATE) until the next push made with the gate on.  Records of a gated decode carry list positions as channel."""
        if hold is None:
            self._chk(self.L.msk144_set_wideband_gate(self.h, None, None))
            return
        flags = np.zeros(self.channels, dtype=np.uint8)
        for c in always:
            if not 0 <= int(c) < self.channels:
                raise ValueError(f"always channel {c} is out of range")
            flags[int(c)] = 1
        p = WidebandGateParams(int(hold), int(min_up), 0 if max_channels is None else int(max_channels))
        self._chk(self.L.msk144_set_wideband_gate(self.h, C.byref(p), flags.ctypes.data_as(C.POINTER(C.c_uint8))))

    def wideband_gate(self):
        """(list, total) of the last push: the int32 channels whose window it decodes, ascending - position j of the list is what
        the decode's records carry as channel - and the number of channels that qualified, of which total - len(list) were dropped."""
        out = np.zeros(self.channels, dtype=np.int32)
        count, total = C.c_int32(), C.c_int32()
        self._chk(self.L.msk144_wideband_gate(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(count), C.byref(total)))
        return out[:count.value].copy(), total.value

    # ---- parity / debug ----
    def dump_analytic(self, channel=0) -> np.ndarray:
        out = np.empty(5184, dtype=np.complex64)
        self._chk(self.L.msk144_dump_analytic(self.h, channel, _ptr(out)))
        return out

    def dump_mix_table(self, b=0) -> np.ndarray:
        """Row b of the handle's phasor table as float32 [5184][2]: (cos, sin) of the mixers' phase at frequency hypothesis b."""
        out = np.empty((5184, 2), dtype=np.float32)
        self._chk(self.L.msk144_dump_mix_table(self.h, b, _ptr(out)))
        return out

    def dump_candidates(self, channel=0) -> np.ndarray:
        out = np.zeros(self.K, dtype=CANDIDATE_DTYPE)
        self._chk(self.L.msk144_dump_candidates(self.h, channel, _ptr(out)))
        return out

    def dump_indexes(self, channel=0) -> np.ndarray:
        out = np.empty(self.K, dtype=np.int32)
        n = C.c_int32()
        self._chk(self.L.msk144_dump_indexes(self.h, channel, _ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def load_candidates(self, items: np.ndarray, channel=0):
        a = np.ascontiguousarray(items)
        assert a.dtype.itemsize == ITEM_BYTES and len(a) == self.K
        self._chk(self.L.msk144_load_candidates(self.h, channel, _ptr(a)))

    def set_profiling(self, on: bool):
        self._chk(self.L.msk144_set_profiling(self.h, 1 if on else 0))

    def stage_times(self, reset=False):
        """{stage: (avg_ms, launches)} measured with HIP events on the decode stream."""
        ms = np.zeros(len(T_NAMES), dtype=np.float32)
        cnt = np.zeros(len(T_NAMES), dtype=np.int32)
        self._chk(self.L.msk144_stage_times(self.h, _ptr(ms), _ptr(cnt), 1 if reset else 0))
        return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(T_NAMES)}

    def clock_probe(self, spin_us: int = 1000) -> float:
        """Shader clock in MHz read by a one-wave kernel beside whatever the decode stream is running (blocks ~spin_us)."""
        mhz = C.c_float(0.0)
        self._chk(self.L.msk144_clock_probe(self.h, int(spin_us), C.byref(mhz)))
        return float(mhz.value)


def device_count() -> int:
    """HIP devices the library sees (raises without one: there is no CPU fallback)."""
    n = C.c_int32(0)
    L = load_library()
    rc = L.msk144_device_count(C.byref(n))
    if rc != 0:
        raise Msk144Error(rc, (L.msk144_last_error(None) or b"").decode())
    return int(n.value)


def unpack_message(msg10: np.ndarray) -> np.ndarray:
    """10 packed bytes (MSB first) -> 77 bits."""
    return np.unpackbits(np.asarray(msg10, dtype=np.uint8))[:77]
