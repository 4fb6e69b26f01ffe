"""What the three CPU test files of msk144hipdecoder --wideband-rate share (test_wideband_cli.py: integer rates and the options,
test_wideband_rational_cli.py: 12000 P/Q, test_wideband_bank_cli.py: above 6.144 Msps): the program against the stand-in library
with the wideband entries, the refused rates with every message each must show, the run of the wideband loop, the help text."""
import re
from math import gcd

from host_stub import run, shared_program, windows_seen

FORMAT_CODE = {"cu8": 0, "cs8": 1, "cs16": 2}

# every substring a refused rate's message must hold, whichever file names the rate
REFUSED_RATES = {
    1920001: ["multiple of 12000", "multiple of 125"],
    2048001: ["multiple of 12000", "multiple of 125"],
    44100: ["multiple of 12000", "multiple of 125"],     # the 44.1 kHz family
    6152001: ["multiple of 125"],                        # above 6.144 Msps and not a multiple of 125
    12000: ["2 <= D <= 512"],
    23875: ["2 <= D <= 512"],                            # a multiple of 125 below 24000
    6144125: ["2 <= D <= 512"],                          # ... above 6144000, not of 8000
    6156000: ["2 <= D <= 512"],
    12500000: ["2 <= D <= 512"],                         # a multiple of 125, not of 8000
    61448000: ["2 <= D <= 512"],                         # a multiple of 8000 above 61.44 Msps
}
HELP = ("--wideband-rate=HZ", "--wideband-format=FMT", "--channel-offsets=", "--channel-grid=", "--wideband-gain=G", "--taps-per-phase=K",
        "multiple of 125", "2048000", "multiple of 8000 up to 61440000", "HZ/32")


def program():
    return shared_program(("msk144hip_stub.cpp", "wideband_stub.cpp"))


def check_refused(exe, args, messages):
    """Exit 2 with every one of `messages`, before the library was asked for anything."""
    r = run(exe, args)
    err = r.stderr.decode()
    assert r.returncode == 2, (args, err)
    for message in messages:
        assert message in err
    assert b"stub:" not in r.stderr


def check_refused_rate(exe, rate, message):
    check_refused(exe, [f"--wideband-rate={rate}", "--channel-offsets=0"], [message] + REFUSED_RATES[int(rate)])


def check_help(exe):
    out = run(exe, ["--help"]).stdout.decode()
    for text in HELP:
        assert text in out


def ratio(rate):
    return rate // gcd(rate, 12000), 12000 // gcd(rate, 12000)


def check_loop(exe, rate, fmt, sample_bytes, pushes, offsets, channels, summary, options=(), K=16, gain="100", within=1e-6):
    """One run over `pushes` pushes of silence: `channels` is the option that asks for `offsets`.  The library is handed K x P taps
    summing to Q (+-within) for the rate's P/Q - behind the bank, the sub-band rate's -, stderr holds `summary` and every channel's
    offset, every channel decodes every push once, in order, and the clip counts are summed."""
    n, n_out = len(offsets), 5184 + (pushes - 1) * 2592
    data = bytes(n_out * rate // 12000 * sample_bytes + 100)     # a short tail: the reference's end-of-input message
    r = run(exe, [f"--wideband-rate={rate}", f"--wideband-format={fmt}", channels, *options], data, timeout=300)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert r.stdout.decode().strip().endswith("Done")
    P, Q = ratio(rate // 32 if rate > 6144000 else rate)
    taps = re.search(rf"stub: msk144_set_wideband\(rate {rate}, format {FORMAT_CODE[fmt]}, K {K}, gain {gain}, (\d+) taps summing to ([0-9.]+), "
                     rf"{n} offsets, first {offsets[0]}, last {offsets[-1]}\)", err)
    assert taps and int(taps.group(1)) == K * P and abs(float(taps.group(2)) - Q) <= within
    for c in range(n):
        assert f"ch={c} offset {offsets[c]} Hz" in err
    assert summary in err
    seen = windows_seen(r.stdout.decode(), n)
    for c in range(n):
        assert seen[c] == [(100 * c + k, 100 * c + k + 1) for k in range(pushes)], c
    assert "Incomplete read error. rc=" in err
    assert re.search(rf"wideband: {7 * pushes} of {2 * n * n_out} channel I/Q components clipped", err)
