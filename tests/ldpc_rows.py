"""Synthetic LLR rows for the BP kernel, the index list and the collect stage (tests/test_ldpc_rows_model.py on the CPU,
tests/test_gpu_ldpc_rows.py on the GPU).

Every row is a float32 [128] LLR vector in the kernel's sign convention (a bit is 1 where LLR > 0), built from codewords of
synth.encode_message / synth.ldpc_encode with plain numpy and fixed seeds.  The families aim at what LLR rows demodulated from
audio or IQ windows reach rarely or never:

  clean         a codeword times 1e-42 (a denormal) .. 1e30, the all-zero row and an all-negative row (both: the zero codeword)
  noisy         (+-1 + N(0, sigma)) * amp near the decoding threshold: accepts at every iteration 0..9 and rejects; at amp 8 and
                on the strong rows below the leave-one-out products reach the three upper atanh pieces and the +-1 saturation
  erasures      a codeword at amplitude 3 with 1..38 positions exactly 0.0: tanh products that are exactly 0
  strong_flips  1, 2 or 4 positions of the wrong sign at magnitude 3, 30 or 1e6: saturated messages against a wrong bit
  gate          16..19 positions of the wrong sign at magnitude 0.05 among 3.0: BP corrects them, the hard-error gate (< 18)
                decides
  bad_crc       a codeword of the LDPC code whose CRC-13 has one bit flipped: zero syndrome, never accepted
  nonfinite     rows of the families above with NaN, +inf or -inf in 1, 2 or 64 positions, and an all-NaN row

A kernel outcome that differs from the oracle's on one of them is judged by parity.verify_marginal_bp(absolute=True): the
perturbation then has an absolute term, because a relative one cannot move an exact zero.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from msk144cudecoder_amd import synth

import parity

FINITE_FAMILIES = ("clean", "noisy", "erasures", "strong_flips", "gate", "bad_crc")

CLEAN_AMPLITUDES = (1e-42, 1e-30, 1e-3, 1.0, 20.0, 1e4, 1e30)
NOISY_SIGMAS = (0.45, 0.6, 0.7, 0.8)
NOISY_AMPLITUDES = (1.0, 3.0, 8.0)
# rows per (sigma, amplitude): most where the oracle's accepts spread over iterations 2..9 (sigma 0.6 and 0.7 at amplitudes 3 and 8);
# amplitude 1 under-weights the channel so far that nearly every row is rejected, sigma 0.45 converges at once, 0.8 hardly ever
NOISY_ROWS = {0.45: (60, 100, 100), 0.6: (60, 500, 500), 0.7: (60, 300, 600), 0.8: (60, 100, 100)}     # 2540 rows
NOISY_SEED = 9100       # chosen: every accept iteration at least 20 times, and no row on which the oracle is undecided at a relative 1e-5
ERASURE_COUNTS = (1, 4, 8, 16, 24, 38)
FLIP_COUNTS = (1, 2, 4)
FLIP_MAGNITUDES = (3.0, 30.0, 1e6)
GATE_COUNTS = (16, 17, 18, 19)
GATE_ROWS_PER_COUNT = 20
BAD_CRC_AMPLITUDES = (0.5, 3.0, 40.0)

OUTCOME_DTYPE = np.dtype([("ok", "u1"), ("it", "<i4"), ("nh", "<i4"), ("msg", "i1", (77,))])


@dataclasses.dataclass
class RowSet:
    rows: np.ndarray        # float32 [n][128]
    family: np.ndarray      # str [n]
    tag: np.ndarray         # int32 [n]: the family's own parameter (amplitude index, erasures, flips, ...), see each builder
    msg: np.ndarray         # uint8 [n][77]: the message the row was built from

    def __len__(self):
        return len(self.rows)

    def of(self, family: str) -> np.ndarray:
        return np.nonzero(self.family == family)[0]


def _signs(cw) -> np.ndarray:
    return 2.0 * np.asarray(cw, dtype=np.float64) - 1.0


def _codeword(rng):
    msg = synth.random_message(rng)
    return msg, synth.encode_message(msg)


def _clean(out):
    rng = np.random.default_rng(7001)
    for m in range(8):
        msg, cw = _codeword(rng)
        for a, amp in enumerate(CLEAN_AMPLITUDES):
            out("clean", a, msg, (_signs(cw) * np.float64(np.float32(amp))).astype(np.float32))
    zero = np.zeros(77, dtype=np.uint8)
    out("clean", len(CLEAN_AMPLITUDES), zero, np.zeros(128, dtype=np.float32))                # zn = 0 is the bit 0: the zero codeword, CRC 0
    out("clean", len(CLEAN_AMPLITUDES) + 1, zero, np.full(128, -3.0, dtype=np.float32))


def _noisy(out):
    for s, sigma in enumerate(NOISY_SIGMAS):
        for a, amp in enumerate(NOISY_AMPLITUDES):
            rng = np.random.default_rng(NOISY_SEED + 10 * s + a)
            for _ in range(NOISY_ROWS[sigma][a]):
                msg, cw = _codeword(rng)
                out("noisy", 10 * s + a, msg, ((_signs(cw) + rng.normal(0.0, sigma, 128)) * amp).astype(np.float32))


def _erasures(out):
    rng = np.random.default_rng(7200)
    for e in ERASURE_COUNTS:
        for _ in range(16):
            msg, cw = _codeword(rng)
            llr = (_signs(cw) * 3.0).astype(np.float32)
            llr[rng.choice(128, size=e, replace=False)] = 0.0
            out("erasures", e, msg, llr)


def _strong_flips(out):
    rng = np.random.default_rng(7300)
    for e in FLIP_COUNTS:
        for m, mag in enumerate(FLIP_MAGNITUDES):
            for _ in range(12):
                msg, cw = _codeword(rng)
                llr = (_signs(cw) * 3.0).astype(np.float32)
                at = rng.choice(128, size=e, replace=False)
                llr[at] = (-_signs(cw)[at] * mag).astype(np.float32)
                out("strong_flips", 10 * e + m, msg, llr)


def _gate(out):
    rng = np.random.default_rng(7400)
    for e in GATE_COUNTS:
        for _ in range(GATE_ROWS_PER_COUNT):
            msg, cw = _codeword(rng)
            llr = (_signs(cw) * 3.0).astype(np.float32)
            at = rng.choice(128, size=e, replace=False)
            llr[at] = (-_signs(cw)[at] * 0.05).astype(np.float32)
            out("gate", e, msg, llr)


def _bad_crc(out):
    rng = np.random.default_rng(7500)
    for a, amp in enumerate(BAD_CRC_AMPLITUDES):
        for bit in range(13):
            msg = synth.random_message(rng)
            crc = synth.crc13_bits(msg).copy()
            crc[bit] ^= 1
            cw = synth.ldpc_encode(np.concatenate([msg, crc]))
            out("bad_crc", a, msg, (_signs(cw) * amp).astype(np.float32))


def finite_rows() -> RowSet:
    """Every finite family, in FINITE_FAMILIES order; rows are unique."""
    rows, family, tag, msgs = [], [], [], []

    def out(fam, t, msg, llr):
        assert llr.dtype == np.float32 and llr.shape == (128,) and np.isfinite(llr).all()
        rows.append(llr)
        family.append(fam)
        tag.append(t)
        msgs.append(np.asarray(msg, dtype=np.uint8))

    for build in (_clean, _noisy, _erasures, _strong_flips, _gate, _bad_crc):
        build(out)
    rs = RowSet(np.stack(rows), np.array(family), np.array(tag, dtype=np.int32), np.stack(msgs))
    assert len({r.tobytes() for r in rs.rows}) == len(rs), "rows must be unique"
    return rs


def nonfinite_rows(finite: RowSet):
    """(rows float32 [n][128], description [n]): rows of every finite family with NaN, +inf or -inf in 1, 2 or 64 positions - at
    a position whose bit agrees with the value (NaN decides 0 like a non-positive LLR) where the row should still be accepted at
    iteration 0, at any position otherwise -, a row whose inf has the wrong sign, and an all-NaN row."""
    rng = np.random.default_rng(7600)
    rows, desc = [], []
    for fam in FINITE_FAMILIES:
        members = finite.of(fam)
        for name, value in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            for n in (1, 2, 64):
                for agree in (True, False):
                    base = finite.rows[members[rng.integers(len(members))]].copy()
                    want_positive = value > 0                                    # NaN and -inf decide the bit 0
                    fits = np.nonzero((base > 0) == want_positive)[0]
                    pool = fits if agree and len(fits) >= n else np.arange(128)
                    base[rng.choice(pool, size=n, replace=False)] = value
                    rows.append(base)
                    desc.append(f"{fam}:{name}x{n}:{'agreeing' if agree and len(fits) >= n else 'anywhere'}")
    clean = finite.rows[finite.of("clean")[3]].copy()                            # amplitude 1
    k = int(np.nonzero(clean > 0)[0][0])
    clean[k] = -np.inf
    rows.append(clean)
    desc.append("clean:-inf on a 1 bit")
    rows.append(np.full(128, np.nan, dtype=np.float32))
    desc.append("all NaN")
    rows = np.stack(rows).astype(np.float32)
    assert not np.isfinite(rows).all(axis=1).any()
    return rows, desc


def oracle_outcomes(orc_mod, rows) -> np.ndarray:
    """OUTCOME_DTYPE [n]: the oracle's BP on every row (it, nh and msg are 0 where the row is not accepted)."""
    from concurrent.futures import ThreadPoolExecutor
    out = np.zeros(len(rows), dtype=OUTCOME_DTYPE)
    with ThreadPoolExecutor(max_workers=8) as pool:                    # the oracle call releases the interpreter lock
        for k, (ok, msg, it, nh) in enumerate(pool.map(orc_mod.ldpc_one, rows)):
            if ok:
                out[k] = (1, it, nh, msg)
    return out


def oracle_unstable_rows(orc_mod, rows, outcomes, scale=1e-6, trials=8, seed=7700):
    """Indexes of the rows whose (accept, iteration) the oracle itself changes under a relative perturbation of `scale`.  Every row
    draws from a generator of its own, so the answer does not depend on how the rows are spread over the threads (the oracle
    call releases the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor

    def unstable(k):
        rng = np.random.default_rng([seed, k])
        base = (bool(outcomes["ok"][k]), int(outcomes["it"][k]) if outcomes["ok"][k] else -1)
        return any(parity.bp_outcome(orc_mod, parity.perturbed_llr(rows[k], scale, rng))[:2] != base for _ in range(trials))

    with ThreadPoolExecutor(max_workers=8) as pool:
        flags = list(pool.map(unstable, range(len(rows))))
    return [k for k, f in enumerate(flags) if f]


def tolerated_cap(compared: int) -> int:
    """0.1 % of the compared rows, rounded up: near-threshold rows are marginal far more often than the noise-dominated
    windows parity.bp_marginal_limit was measured on, so this file states its own cap; the model test shows with the oracle
    alone that at most half of it is spent by rows the oracle itself cannot decide."""
    return -(-compared // 1000)
