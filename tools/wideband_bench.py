"""Wideband channeliser cost per push (msk144_push_wideband), measured with the library's HIP-event stage times.

For every (channels, rate) the handle is pushed `--pushes` later pushes of random cu8 samples.  In wideband mode the front-end stage
time covers the channeliser and the IQ front end; the same handle is then fed the same number of plain msk144_push_hops calls,
whose front-end time is the IQ front end alone, and the difference is the channeliser.  FLOP count: channels x 2592 x K x
(Fs/12000) x 8 (= channels x 2592 x K*D x 8 at Fs = D x 12000); above 6.144 Msps (the two-stage bank) the bank's work per push
plus the channeliser's at Fs/32.  push_host_us is the median host time of one msk144_push_wideband call (the call returns before
the device has run it; profiling is on, so the HIP events of the stage times are part of it).  One JSON line per configuration on
stdout.  --agc: the stepped AGC is on (msk144_set_wideband_agc with the defaults), so the time includes its step kernel after
every push.  --blanker: the impulse-noise blanker is on
(msk144_set_wideband_blanker with the defaults), so the time includes its two kernels ahead of the channeliser, which then reads cs16;
blanker_bytes is what they move per push (the raw push read twice, its cs16 form written once).  --spectrum[=BINS]: the input
spectrum is on (msk144_set_wideband_spectrum, BINS default 1024, the default window), so the time includes its two kernels ahead of the
channeliser; spectrum_bytes is the push they read once.  --pings: the ping detector is on (msk144_set_wideband_pings with the
defaults), so the time includes its kernel behind the channeliser; pings_bytes is the staged hops it reads once.  --pings-band: the
ping band is on as well (msk144_set_wideband_ping_band with the default design; implies --pings), so the time includes its kernel
ahead of the detector's; pings_band_dot4 is the int8 dot products of a push (channels x 2592 x 99).  --waterfall: the
per-channel waterfall is on (msk144_set_wideband_waterfall, the default window), so the time includes its two kernels behind the
channeliser; waterfall_mfma is the f32 MFMA instructions of a push (576 per channel) and waterfall_bytes the rows it writes.
--capture: the capture is on (msk144_set_wideband_capture with the defaults) with every 8th channel listed, up to the 16 the list
holds, so that the units are non-trivial without a detector; the time includes its two kernels behind the hop ring, capture_units is
the units of a push and capture_bytes what the copy kernel moves for them.  --notch N: the first N channels are notched
(msk144_set_wideband_notch with the default design at +300 Hz), so the time includes the notch kernel behind the channeliser, one
workgroup per notched channel; notch_dot4 is its int8 dot products of a push (N x 2592 x 99).  Every line of such a run is also
appended to profiles/wideband_bench_notch.jsonl; run it with --notch 0 as well, on the same box, and compare the two.

Then one msk144hipdecoder run over a pre-written cu8 file (1024 channels at --program-rate, default 1.92 Msps, the program's
default decode configuration): hops per second of the whole program against the real-time rate of 4.63 hops/s (one hop = 2592
samples at 12 kHz).

--gate SHARES is a leg of its own: 1024 channels at D = 160 and the deep options (width 500, step 1, depth 6), the detector off,
and for each share an always list (msk144_set_wideband_gate) of round(share x 1024) evenly spread channels.  It measures the host
milliseconds of push + decode + fetch per share, and the same for an ungated handle in the same run, then runs the program three
times with the detector on - ungated, with every channel always decoded, and with the bare --wideband-gate - and appends every line
to profiles/wideband_bench_gate.jsonl.  Nothing is asserted on these times.

--audio is a leg of its own as well: 1024 channels at D = 160 with the capture on (every 8th channel listed, up to 16), once with
the audio off and once with it on (msk144_set_wideband_audio, the default design), two handles in one run.  It measures the host
milliseconds of one later push that ends in msk144_synchronize - the whole push: channeliser, hop ring, the audio kernel and its
copy, the capture, the IQ front end - in `--rounds` rounds of `--pushes` pushes that alternate between the two handles, and gives
the median of every round, so that the spread from round to round stands beside the difference.  audio_dot4 is the audio kernel's
int8 dot products of a push (channels x 2592 x 99), audio_bytes the int16 rows it writes (channels x 5184).  The lines are
appended to profiles/wideband_bench_audio.jsonl.  Nothing is asserted on these times.

    python tools/wideband_bench.py [--channels 256,1024,4096] [--decimations 80,160,200] [--rates 2048000,2500000]
                                   [--audio [--rounds 5]]
                                   [--pushes 20] [--program-hops 40] [--program-rate 1920000] [--agc] [--blanker] [--spectrum[=BINS]] [--pings] [--pings-band] [--waterfall] [--capture] [--notch N]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from msk144cudecoder_amd import hipdecoder, wideband  # noqa: E402

FP32_PEAK_TFLOPS = 157.3   # MI355X, vector and f32-input MFMA (spec)


def measure(C: int, rate: int, pushes: int, K: int = 16, agc: bool = False, blanker: bool = False, spectrum: int = 0, pings: bool = False, waterfall: bool = False,
            capture: bool = False, pings_band: bool = False, notch: int = None) -> dict:
    D = rate // 12000
    rng = np.random.default_rng(C + D)
    g = math.gcd(rate, 12000)
    P, Q = rate // g, 12000 // g
    lim = rate // 2 - 6000
    offsets = np.linspace(-lim, lim, C).astype(np.int32)
    with hipdecoder.HipDecoder(center=0.0, width=0.0, step=1.0, depth=1, read_mode=2, channels=C) as d:
        d.set_wideband(rate, offsets, "cu8", taps_per_phase=K)
        if agc:
            d.set_wideband_agc()
        if blanker:
            d.set_wideband_blanker()
        if spectrum:
            d.set_wideband_spectrum(spectrum)
        if pings or pings_band:
            d.set_wideband_pings()
        if pings_band:
            d.set_wideband_ping_band()
        if notch:
            d.set_wideband_notch({c: [300] for c in range(min(notch, C))})
        if waterfall:
            d.set_wideband_waterfall()
        listed = list(range(0, C, 8))[:wideband.CAPTURE_MAX_LISTED]
        if capture:
            d.set_wideband_capture(channels=listed)
        for s in range(2):
            d.wideband_slot(s)[:] = rng.integers(120, 136, size=d.wideband_slot(s).size, dtype=np.uint8)
        d.push_wideband(0, first=True)
        d.synchronize()
        d.set_profiling(True)
        d.stage_times(reset=True)
        host = []
        for i in range(pushes):
            t0 = time.perf_counter()
            d.push_wideband(i % 2, first=False)
            host.append(time.perf_counter() - t0)
        wide = d.stage_times(reset=True)
        for s in range(2):
            hops, _, streams, is_first = d.hop_slot(s)
            hops[:] = rng.integers(-8, 8, size=hops.shape, dtype=np.int8)
            streams[:] = np.arange(C)
            is_first[:] = 0
        for i in range(pushes):
            d.push_hops(i % 2, C)
        plain = d.stage_times(reset=True)
    ms = wide["frontend"][0] - plain["frontend"][0]
    flop = C * 2592 * K * P * 8 // Q
    ratio = dict(D=D) if Q == 1 else dict(rate_hz=rate, P=P, Q=Q)
    target = 2.0 if C == 1024 and rate in (1920000, 2048000, 2500000) else None
    if wideband.is_bank_rate(rate):
        # two stages: the bank's 64 K1 real-by-complex MACs (4 flop) per frame plus 64 complex MACs (8 flop) per occupied band and
        # frame, then the channeliser at Fs/32 (P2/Q2 = Fs/32/12000), channels x 2592 x K P2/Q2 x 8
        P2, Q2 = wideband.rate_ratio(rate // 32)
        frames = 2592 * P2 // Q2
        bands = len({int(k) % 64 for k in wideband.bank_band(rate, offsets)})
        flop1 = frames * (64 * 8 * 4 + bands * 64 * 8)
        flop = flop1 + C * 2592 * K * P2 * 8 // Q2
        ratio = dict(rate_hz=rate, stage1_bands=bands, stage1_gflop=round(flop1 / 1e9, 3), stage2_P=P2, stage2_Q=Q2)
        target = {10000000: 2.0, 20000000: 2.0, 61440000: 3.0}.get(rate) if C == 1024 else None
    if blanker:
        ratio["blanker_bytes"] = 2592 * P // Q * (2 * 2 + 4)   # cu8 in, cs16 out
    if spectrum:
        ratio["spectrum_bins"] = spectrum
        ratio["spectrum_bytes"] = 2592 * P // Q * (4 if blanker else 2)   # the push read once: cu8, or the blanker's cs16
    if pings_band:
        ratio["pings_band"] = True
        ratio["pings_band_dot4"] = C * 2592 * 99   # 33 tap dwords x 3 sums per output
    if pings or pings_band:
        ratio["pings"] = True
        ratio["pings_bytes"] = C * 2592 * 2   # every channel's int8 hop read once
    if notch is not None:
        ratio["notch_channels"] = min(notch, C)
        ratio["notch_dot4"] = min(notch, C) * 2592 * 99   # 33 tap dwords x 3 sums per output
    if waterfall:
        ratio["waterfall"] = True
        ratio["waterfall_mfma"] = C * 576               # 3 waves x 96 steps x 2 per channel and hop
        ratio["waterfall_bytes"] = C * 27 * 96 * 4      # the rows of a hop, written once
    if capture:
        ratio["capture"] = True
        ratio["capture_units"] = len(listed)
        ratio["capture_bytes"] = len(listed) * wideband.CAPTURE_UNIT_BYTES
    return dict(channels=C, **ratio, K=K, agc=agc, blanker=blanker, pushes=pushes, push_frontend_ms=round(wide["frontend"][0], 4), iq_frontend_ms=round(plain["frontend"][0], 4),
                channeliser_ms=round(ms, 4), h2d_ms=round(wide["h2d"][0], 4), push_host_us=round(float(np.median(host)) * 1e6, 1), gflop=round(flop / 1e9, 2),
                tflops=round(flop / (ms * 1e-3) / 1e12, 1) if ms > 0 else None,
                fraction_of_fp32_peak=round(flop / (ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 3) if ms > 0 else None,
                target_ms=target)


GATE_CFG = dict(center=0.0, width=500.0, step=1.0, depth=6, nbadsync_threshold=1, read_mode=2)   # the deep options


def gate_channels(share: float, C: int) -> list:
    """round(share x C) channels spread evenly over the C, so that the share is exact."""
    n = int(round(share * C))
    return sorted({i * C // n for i in range(n)}) if n else []


def step_ms(d, pushes: int, warmup: int = 3) -> list:
    """Host milliseconds of push + decode + fetch, one value per later push, behind `warmup` unmeasured ones."""
    out = []
    for i in range(warmup + pushes):
        s = i % 2
        t0 = time.perf_counter()
        d.push_wideband(s, first=False)
        d.decode()
        d.fetch_async(s)
        d.fetch_wait(s)
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def measure_gate(shares, pushes: int, C: int = 1024, rate: int = 1920000) -> list:
    """--gate: ms per push + decode + fetch at the deep options with the detector off and an always list of each share of the
    channels, and the same for an ungated handle in the same run.  Nothing is asserted."""
    lim = rate // 2 - 6000
    offsets = np.linspace(-lim, lim, C).astype(np.int32)
    rng = np.random.default_rng(C)
    out = []
    with hipdecoder.HipDecoder(channels=C, **GATE_CFG) as plain, hipdecoder.HipDecoder(channels=C, **GATE_CFG) as gated:
        for d in (plain, gated):
            d.set_wideband(rate, offsets, "cu8")
            for s in range(2):
                d.wideband_slot(s)[:] = rng.integers(120, 136, size=d.wideband_slot(s).size, dtype=np.uint8)
            d.push_wideband(0, first=True)
            d.synchronize()
        for share in shares:
            listed = gate_channels(share, C)
            gated.set_wideband_gate(always=listed)
            a, b = step_ms(plain, pushes), step_ms(gated, pushes)
            lst, total = gated.wideband_gate()
            assert list(lst) == listed and total == len(listed)
            out.append(dict(gate_share=share, channels=C, D=rate // 12000, config="width 500 step 1 depth 6", detector=False, listed=len(listed), pushes=pushes,
                            gated_ms_median=round(float(np.median(b)), 3), gated_ms_mean=round(float(np.mean(b)), 3), ungated_ms_median=round(float(np.median(a)), 3),
                            ungated_ms_mean=round(float(np.mean(a)), 3), gather_bytes=len(listed) * 5184 * 8 * 2))
    return out


def push_ms(d, pushes: int) -> list:
    """Host milliseconds of one later push that ends in a synchronise, one value per push."""
    out = []
    for i in range(pushes):
        t0 = time.perf_counter()
        d.push_wideband(i % 2, first=False)
        d.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def measure_audio(pushes: int, rounds: int, C: int = 1024, rate: int = 1920000) -> list:
    """--audio: ms per push with the audio off and on, the capture on in both, in alternating rounds of one run.  Nothing is asserted."""
    lim = rate // 2 - 6000
    offsets = np.linspace(-lim, lim, C).astype(np.int32)
    rng = np.random.default_rng(C)
    listed = list(range(0, C, 8))[:wideband.CAPTURE_MAX_LISTED]
    cfg = dict(center=0.0, width=0.0, step=1.0, depth=1, read_mode=2, channels=C)
    with hipdecoder.HipDecoder(**cfg) as off, hipdecoder.HipDecoder(**cfg) as on:
        for d in (off, on):
            d.set_wideband(rate, offsets, "cu8")
            d.set_wideband_capture(channels=listed)
            for s in range(2):
                d.wideband_slot(s)[:] = rng.integers(120, 136, size=d.wideband_slot(s).size, dtype=np.uint8)
        on.set_wideband_audio()
        for d in (off, on):
            d.push_wideband(0, first=True)
            push_ms(d, 5)                      # warm-up: every kernel of a later push has run
        medians = {False: [], True: []}
        for _ in range(rounds):
            for audio, d in ((False, off), (True, on)):
                medians[audio].append(float(np.median(push_ms(d, pushes))))
        rows, clamped = on.wideband_capture_audio()
        assert rows.shape == (len(listed), wideband.HOP_OUT)
    out = []
    for audio in (False, True):
        m = medians[audio]
        line = dict(audio=audio, channels=C, D=rate // 12000, capture_units=len(listed), pushes=pushes, rounds=rounds, push_ms=round(float(np.median(m)), 4),
                    round_medians_ms=[round(v, 4) for v in m], spread_ms=round(max(m) - min(m), 4), timing="host clock around msk144_push_wideband + msk144_synchronize")
        if audio:
            line.update(audio_dot4=C * 2592 * 99, audio_bytes=C * 2 * wideband.HOP_OUT)
        out.append(line)
    return out


def program_run(hops: int, C: int = 1024, rate: int = 1920000, gate: str = None, pings: bool = False) -> dict:
    """Wall time of one msk144hipdecoder run over a file of 1 first + (hops - 1) later pushes of cu8 noise.  gate: the value of
    --wideband-gate ("" the bare option, "all": every channel always decoded); pings: with --wideband-pings (the events to /dev/null)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "msk144cudecoder_amd", "msk144hipdecoder")
    g = math.gcd(rate, 12000)
    P, Q = rate // g, 12000 // g
    lim = rate // 2 - 6000
    offsets = np.linspace(-lim, lim, C).astype(np.int64)
    rng = np.random.default_rng(5)
    n = 2 * (5184 + (hops - 1) * 2592) * P // Q
    with tempfile.NamedTemporaryFile(suffix=".cu8") as f:
        f.write(np.clip(np.rint(127.5 + 6.0 * rng.standard_normal(n)), 0, 255).astype(np.uint8).tobytes())
        f.flush()
        args = [exe, f"--wideband-rate={rate}", "--wideband-format=cu8", "--channel-offsets=" + ",".join(str(int(v)) for v in offsets), "--wideband-gain=20"]
        if pings:
            args.append("--wideband-pings=/dev/null")
        if gate is not None:
            args.append("--wideband-gate" + ("=1:1:0:" + ",".join(str(c) for c in range(C)) if gate == "all" else "=" + gate if gate else ""))
        with open(f.name, "rb") as src:
            t0 = time.perf_counter()
            p = subprocess.run(args, stdin=src, capture_output=True, timeout=600)
            wall = time.perf_counter() - t0
    if p.returncode != 0:
        raise RuntimeError(p.stderr.decode()[-2000:])
    err = p.stderr.decode()
    m = re.search(r"msk144hipdecoder: (\d+) batches", err)
    batches = int(m.group(1)) if m else None
    ratio = dict(D=P) if Q == 1 else dict(rate_hz=rate, P=P, Q=Q)
    if gate is not None:
        m = re.search(r"wideband gate: (\d+) of (\d+) channel windows decoded", err)
        ratio.update(gate=gate, gate_windows=[int(m.group(1)), int(m.group(2))] if m else None)
    if pings:
        ratio["pings"] = True
    return dict(program="msk144hipdecoder", channels=C, **ratio, hops=batches, wall_s=round(wall, 3), hops_per_s=round(batches / wall, 2) if batches else None,
                realtime_hops_per_s=4.63, note="wall time of the whole process, handle creation and file reading included")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--channels", default="256,1024,4096")
    ap.add_argument("--decimations", default="80,160,200", help="integer rates D x 12000; empty: none")
    ap.add_argument("--rates", default="", help="any further rates in Hz (multiples of 125, e.g. 2048000,2500000,96125)")
    ap.add_argument("--pushes", type=int, default=20)
    ap.add_argument("--program-hops", type=int, default=40, help="0: skip the program run")
    ap.add_argument("--program-rate", type=int, default=1920000)
    ap.add_argument("--agc", action="store_true", help="measure with the stepped AGC on")
    ap.add_argument("--blanker", action="store_true", help="measure with the impulse-noise blanker on")
    ap.add_argument("--spectrum", type=int, nargs="?", const=1024, default=0, metavar="BINS", help="measure with the input spectrum on (BINS default 1024)")
    ap.add_argument("--pings", action="store_true", help="measure with the ping detector on")
    ap.add_argument("--pings-band", action="store_true", help="measure with the ping detector and its in-band filter on")
    ap.add_argument("--waterfall", action="store_true", help="measure with the per-channel waterfall on")
    ap.add_argument("--capture", action="store_true", help="measure with the capture on, every 8th channel (up to 16) listed")
    ap.add_argument("--notch", type=int, default=None, metavar="N", help="measure with the first N channels notched (0: none, for the comparison); appends to profiles/wideband_bench_notch.jsonl")
    ap.add_argument("--gate", default=None, metavar="SHARES", help="only the gate leg: ms per push + decode + fetch at 1024 channels, D = 160 and the deep options with each share "
                    "(e.g. 0,0.1,0.5,1) of the channels always decoded and the detector off, against an ungated handle in the same run; then the program ungated, with every channel "
                    "always decoded and behind the detector; appends to profiles/wideband_bench_gate.jsonl")
    ap.add_argument("--audio", action="store_true", help="only the audio leg: ms per push at 1024 channels and D = 160 with the capture on, the audio off and on, in alternating "
                    "rounds of one run; appends to profiles/wideband_bench_audio.jsonl")
    ap.add_argument("--rounds", type=int, default=5, help="--audio: rounds of --pushes pushes per handle")
    a = ap.parse_args()
    if a.audio:
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wideband_bench_audio.jsonl"), "a") as log:
            for line in measure_audio(a.pushes, a.rounds):
                print(json.dumps(line), flush=True)
                log.write(json.dumps(line) + "\n")
        return
    if a.gate is not None:
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wideband_bench_gate.jsonl"), "a") as log:
            lines = measure_gate([float(v) for v in a.gate.split(",") if v], a.pushes)
            if a.program_hops:
                lines += [program_run(a.program_hops, rate=a.program_rate, pings=True), program_run(a.program_hops, rate=a.program_rate, pings=True, gate="all"),
                          program_run(a.program_hops, rate=a.program_rate, pings=True, gate="")]
            for line in lines:
                print(json.dumps(line), flush=True)
                log.write(json.dumps(line) + "\n")
        return
    log = None
    if a.notch is not None:
        log = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wideband_bench_notch.jsonl"), "a")
    rates = [int(v) * 12000 for v in a.decimations.split(",") if v] + [int(v) for v in a.rates.split(",") if v]
    for C in [int(v) for v in a.channels.split(",")]:
        for rate in rates:
            line = json.dumps(measure(C, rate, a.pushes, agc=a.agc, blanker=a.blanker, spectrum=a.spectrum, pings=a.pings, waterfall=a.waterfall, capture=a.capture,
                                      pings_band=a.pings_band, notch=a.notch))
            print(line, flush=True)
            if log:
                log.write(line + "\n")
                log.flush()
    if a.program_hops:
        print(json.dumps(program_run(a.program_hops, rate=a.program_rate)), flush=True)


if __name__ == "__main__":
    main()
