"""What the tests of the wideband audio (msk144_set_wideband_audio, include/msk144hip.h) share: the host rule of libmsk144host.so,
the extreme parameter set, streams of int8 hops and the measurement of a tone in the audio."""
import ctypes as C

import numpy as np

from msk144cudecoder_amd import wideband as wb

HOP = wb.HOP_OUT
LEVEL = 256                      # the design's: amplitude A comes out near 256 A (a design parameter, not a measurement)
EXTREME_TAPS = np.full((64, 2), -128, dtype=np.int8)
EXTREME_PHASOR = np.full((96, 2), -32768, dtype=np.int16)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class HostAudio:
    """msk144host_wideband_audio_push behind the interface of wideband.Audio: the tails are kept here, zeroed for a restart."""

    def __init__(self, channels, taps, phasor, shift):
        self.L = wb._host_lib()
        self.taps = np.ascontiguousarray(taps, dtype=np.int8)
        self.phasor = np.ascontiguousarray(phasor, dtype=np.int16)
        assert self.taps.shape == (64, 2) and self.phasor.shape == (96, 2)
        self.shift, self.channels = int(shift), int(channels)
        self.tails = np.zeros((channels, 63, 2), dtype=np.int8)

    def push(self, rows, restart=False):
        x = np.ascontiguousarray(rows, dtype=np.int8)
        n = x.shape[1]
        if restart:
            self.tails[:] = 0
        y = np.zeros((self.channels, n), dtype=np.int16)
        clamped = np.zeros((self.channels, n // HOP), dtype=np.int32)
        rc = self.L.msk144host_wideband_audio_push(_p(self.taps), _p(self.phasor), C.c_int32(self.shift), self.channels, _p(x), n, _p(self.tails), _p(y), _p(clamped))
        assert rc == 0
        return y, clamped


def host_check(shift):
    """'' when msk144_set_wideband_audio takes the shift, else the refusal text (csrc/wideband.h check_audio)."""
    why = C.create_string_buffer(256)
    rc = wb._host_lib().msk144host_wideband_audio_check(C.c_int32(int(shift)), why, len(why))
    return "" if rc == 0 else why.value.decode()


def tone_hops(f_hz, amplitude, hops, phase=0.3):
    """int8 [1][hops x 2592][2]: a complex tone at f_hz from the channel's offset, rounded to the stored integers."""
    n = np.arange(hops * HOP)
    z = amplitude * np.exp(1j * (2 * np.pi * f_hz * n / wb.OUT_RATE + phase))
    return np.stack([np.rint(z.real), np.rint(z.imag)], axis=-1).astype(np.int8)[None]


def model_audio(design, x):
    """The model's audio of a whole stream x [1][hops x 2592][2], pushed as a first push of two hops and later pushes of one."""
    a = wb.Audio(1, *design)
    out = [a.push(x[:, :2 * HOP], restart=True)[0]]
    for k in range(2, x.shape[1] // HOP):
        out.append(a.push(x[:, k * HOP:(k + 1) * HOP])[0])
    return np.concatenate(out, axis=1)[0]


def strongest_line(y):
    """(frequency in Hz, amplitude) of the strongest line of the real signal y under a Hann window, the amplitude that of a tone on
    the bin's centre; the frequency is good to the bin, 12000 / len(y) Hz."""
    w = np.hanning(len(y) + 1)[:-1]
    Y = np.abs(np.fft.rfft(y.astype(np.float64) * w)) * 2.0 / w.sum()
    k = int(np.argmax(Y))
    return k * wb.OUT_RATE / len(y), float(Y[k])


def tone_amplitude(y, f_hz):
    """The amplitude of the component of y at f_hz, by projection under a Hann window."""
    w = np.hanning(len(y) + 1)[:-1]
    n = np.arange(len(y))
    return float(np.abs(np.sum(y * w * np.exp(-2j * np.pi * f_hz * n / wb.OUT_RATE))) * 2.0 / w.sum())
