"""The scene the input-rate decode tests share (test_input_rate_cli.py decodes it on the CPU from the model's output,
test_gpu_input_rate.py on the GPU through msk144_push_rate_hops): five 12 kHz audio streams with one +6 dB ping each, taken to a
higher rate by sample-hold (48000 Hz) or by linear interpolation (32000 Hz)."""
import functools

import numpy as np

from msk144cudecoder_amd import input_rate as ir
from msk144cudecoder_amd import synth
from msk144cudecoder_amd.wideband import rate_ratio

CHANNELS = 5
HOPS = 4                                  # a first hop and three later ones
CFG = dict(center=1500.0, width=20.0, step=2.0, depth=2)
TOTAL = 5184 + (HOPS - 1) * 2592


@functools.lru_cache(maxsize=None)
def streams_12k():
    rng = np.random.default_rng(20241)
    out = []
    for c in range(CHANNELS):
        start = 600 + 1700 * c
        ping = synth.Ping(synth.random_message(rng), start, 6, 1500.0 + float(rng.integers(-4, 5)) * 2.0, 6.0, float(rng.uniform(0, 6)))
        out.append(synth.synth_audio(TOTAL, [ping], 1000.0, rng))
    return tuple(out)


def upsample(x: np.ndarray, rate: int) -> np.ndarray:
    """48000: every sample held four times; 32000: linear interpolation between the 12 kHz samples.  len(x) P/Q samples."""
    P, Q = rate_ratio(rate)
    if rate == 48000:
        return np.repeat(x, 4)
    assert rate == 32000
    n = len(x) // Q * P
    t = np.arange(n, dtype=np.float64) * Q / P
    xe = np.concatenate([x.astype(np.float64), [float(x[-1])]])
    return np.clip(np.rint(np.interp(t, np.arange(len(xe)), xe)), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def scene(rate: int):
    """(inputs, hops): inputs[c] the stream at `rate`; hops[k][c] the model's 12 kHz output of hop k (5184 samples for k = 0)."""
    inputs = tuple(upsample(x, rate) for x in streams_12k())
    row = ir.row_samples(rate)
    model = ir.Resampler(CHANNELS, rate)
    hops = []
    for k in range(HOPS):
        rows = [x[:2 * row] if k == 0 else x[(k + 1) * row:(k + 2) * row] for x in inputs]
        y, _ = model.push(rows, list(range(CHANNELS)), [k == 0] * CHANNELS)
        hops.append(tuple(y))
    return inputs, tuple(hops)


def windows(rate: int):
    """windows[k][c]: the 5184-sample window the decoder sees at hop k, from the model's output."""
    _, hops = scene(rate)
    out = [list(hops[0])]
    for k in range(1, HOPS):
        out.append([np.concatenate([out[-1][c][2592:], hops[k][c]]) for c in range(CHANNELS)])
    return out
