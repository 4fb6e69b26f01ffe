"""The softbits kernel's sync pass (csrc/softbits.hip), checked in numpy against tests/numpy_model.py and the plane model of
tests/test_softbits_plane_model.py.

Once per wave, lane 8 i + j serves candidate c = wave + 8 i (pattern i, valid when i < D) and sync bit j.  It folds two entries of
the filtered plane over the pattern's frames, F(j - 1) for softbit j (lane j = 0 takes the wrap sum W instead) and F(55 + j) for
softbit 56 + j; lanes j = 1..6 put both into the carrier-phase sum with sync bit S8[j] (odd j on the real part, even j as -i F),
the eight lanes of the octet are summed as ((v0 + v1) + (v2 + v3)) + ((v7 + v6) + (v5 + v4)) and the edge term
s7 (u1[6] + u1[62]) - i s0 (u2[0] + u2[56]) is added.  The 16 de-rotated softbits are compared with the sync word in two ballots.
CPU only: this pins the lane map, the octet association and the sign rule of the pass, not the compiled kernel."""
import numpy as np
import pytest

import numpy_model as M
import test_softbits_plane_model as PM

N, FRAME, RING, STRIDE = PM.N, PM.FRAME, PM.RING, PM.STRIDE
S8 = M.S8
SCAN_POSITIONS = 5376
EPS32 = 2.0 ** -24                 # unit roundoff of float32


def positions(D, seed):
    """Scan positions of one tile, one per lane (lane = 8 pattern + slot): position 0, one of each residue mod 6, positions whose folded
    frames wrap the sub-ring (base + group beyond entry 863), positions >= 5184 (the scan walks 5376 positions of a 5184 ring)."""
    fixed = [0, 1, 2, 3, 4, 5, 863 * 6, 863 * 6 + 5, 5183, 5184, 5185, 5375, 4319, 4320, 5178, 5184 + 95]
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, SCAN_POSITIONS, 8 * D)
    where = rng.permutation(8 * D)[:min(len(fixed), 8 * D)]
    pos[where] = fixed[:len(where)]
    if D == 1:
        pos[:] = [0, 5183, 5185, 5375, 863 * 6, 2, 3, 4]
    return pos.astype(np.int64)


def lane_entries(pos_of_lane, D, wave, mask_of):
    """For every lane 8 i + j with i < D: (i, j, [LDS entries of read A per frame], [LDS entries of read B per frame]) - the index algebra
    of the pass: sub-ring pos mod 6, base (pos / 6 + 144 m) mod 864, group max(j - 1, 0) for A and 55 + j for B."""
    out = []
    for lane in range(64):
        i, j = lane >> 3, lane & 7
        if i >= D:
            continue
        pos = int(pos_of_lane[wave + 8 * i])
        if pos >= N:
            pos -= N
        q, r = pos // 6, pos % 6
        ea, eb = [], []
        for m in range(6):
            if not mask_of[i][m]:
                continue
            base = (q + 144 * m) % RING
            ea.append(r * STRIDE + base + max(j - 1, 0))
            eb.append(r * STRIDE + base + 55 + j)
        out.append((i, j, pos, ea, eb))
    return out


def oct_sum(v):
    """oct_sum2_f32: quad xor 1, quad xor 2, half mirror; every lane of the octet ends with the same bits."""
    v = v + v[np.arange(8) ^ 1]
    v = v + v[np.arange(8) ^ 2]
    v = v + v[7 - np.arange(8)]
    assert (v == v[0]).all()
    return v[0]


def wave_sum(v):
    """wave_sum2_f32 (the parent's phase sum): four in-row steps, then (row0 + row1) + (row2 + row3), read in lane 63."""
    l = np.arange(64)
    for src in (l ^ 1, l ^ 2, (l & ~7) | (7 - (l & 7)), (l & ~15) | (15 - (l & 15))):
        v = v + v[src]
    r = v[15::16]
    return (r[3] + r[2]) + (r[1] + r[0])


def side_sums(x, mask, pos, dtype):
    """W and the edge term of one candidate from its five half-pulse sums, combined as the kernel combines them."""
    u2_0, u1_143, u1_6, u2_56, u1_62 = [PM.half_pulse(x, mask, pos, g, rising) for g, rising in ((0, True), (143, False), (6, False), (56, True), (62, False))]
    re = lambda z: dtype(z.real)
    im = lambda z: dtype(z.imag)
    s0, s7 = dtype(S8[0]), dtype(S8[7])
    w = (re(u1_143) + re(u2_0), im(u1_143) + im(u2_0))
    edge = (s7 * (re(u1_6) + re(u1_62)) + s0 * (im(u2_0) + im(u2_56)), s7 * (im(u1_6) + im(u1_62)) - s0 * (re(u2_0) + re(u2_56)))
    return w, edge


def sync_pass(x, lds_r, lds_i, pos_of_lane, D, wave, dtype, parent_association=False):
    """The pass in `dtype` arithmetic: per candidate i < D the phase sum (re, im), the sum of the terms' magnitudes, the unit phasor and
    nbadsync.  parent_association: the phase sum as the per-candidate loop formed it (one term per lane, whole-wave sum)."""
    masks = PM._masks()
    res = {}
    lanes = lane_entries(pos_of_lane, D, wave, masks)
    for i in range(D):
        mine = [e for e in lanes if e[0] == i]
        pos = mine[0][2]
        fa_r, fa_i, fb_r, fb_i = (np.zeros(8, dtype) for _ in range(4))
        for _, j, _, ea, eb in mine:
            for dst, src, ent in ((fa_r, lds_r, ea), (fa_i, lds_i, ea), (fb_r, lds_r, eb), (fb_i, lds_i, eb)):
                acc = src[ent[0]]
                for e in ent[1:]:
                    acc = dtype(acc + src[e])         # fold_plane's order: frame 0, then the pattern's frames ascending
                dst[j] = acc
        k_x = np.array([S8[j] if 1 <= j <= 6 and j % 2 == 1 else 0 for j in range(8)], dtype)
        k_y = np.array([S8[j] if 1 <= j <= 6 and j % 2 == 0 else 0 for j in range(8)], dtype)
        w, edge = side_sums(x, masks[i], pos, dtype)
        ta_r, ta_i = k_x * fa_r + k_y * fa_i, k_x * fa_i - k_y * fa_r       # +-1 and 0 factors: exact
        tb_r, tb_i = k_x * fb_r + k_y * fb_i, k_x * fb_i - k_y * fb_r
        if parent_association:
            vr, vi = np.zeros(64, dtype), np.zeros(64, dtype)
            vr[0:8], vi[0:8], vr[56:64], vi[56:64] = ta_r, ta_i, tb_r, tb_i
            pr, pi = wave_sum(vr), wave_sum(vi)
        else:
            pr, pi = oct_sum((ta_r + tb_r).astype(dtype)), oct_sum((ta_i + tb_i).astype(dtype))
        sre, sim = dtype(pr + edge[0]), dtype(pi + edge[1])
        mag = float(np.abs(np.concatenate([ta_r, ta_i, tb_r, tb_i]).astype(np.float64)).sum() + abs(float(edge[0])) + abs(float(edge[1])))
        inv = dtype(1.0) / np.sqrt(dtype(sre * sre + sim * sim))
        cr, ci = dtype(sre * inv), dtype(-sim * inv)
        odd = np.arange(8) % 2 == 1
        b_r, b_i = np.where(odd, cr, ci).astype(dtype), np.where(odd, -ci, cr).astype(dtype)
        ga_r, ga_i = fa_r.copy(), fa_i.copy()
        ga_r[0], ga_i[0] = w                                                 # softbit 0: the wrap sum
        soft_a = (ga_r * b_r + ga_i * b_i).astype(dtype)
        soft_b = (fb_r * b_r + fb_i * b_i).astype(dtype)
        bad = lambda s: int((np.where(s < 0, -1, 1) != S8).sum())            # popcount of the candidate's ballot byte
        res[i] = dict(pos=pos, s=complex(float(sre), float(sim)), mag=mag, rot=complex(float(cr), float(ci)), nbad=bad(soft_a) + bad(soft_b),
                      soft=np.concatenate([soft_a, soft_b]).astype(np.float64))
    return res


@pytest.mark.parametrize("D", [1, 6, 8])
def test_lane_map_reads_the_plane_entries_of_the_sync_softbits(D):
    """Lane 8 i + j reads, per frame of pattern i, exactly P[pos + 864 m + 6 (j - 1)] (softbit j, j >= 1) and P[pos + 864 m + 6 (55 + j)]
    (softbit 56 + j) of candidate wave + 8 i, inside the sub-ring and its wrap pad, for every slot."""
    Pn = np.arange(N, dtype=np.float64)
    lds = PM.residue_major(Pn)
    masks = PM._masks()
    pos_of_lane = positions(D, 10 + D)
    assert (pos_of_lane == 0).any() and (pos_of_lane >= N).any() and set(pos_of_lane % N % 6) == set(range(6))
    wrapped = 0
    for wave in range(8):
        lanes = lane_entries(pos_of_lane, D, wave, masks)
        assert len(lanes) == 8 * D
        for i, j, pos, ea, eb in lanes:
            assert pos == int(pos_of_lane[wave + 8 * i]) % N
            frames = [m for m in range(6) if masks[i][m]]
            assert len(ea) == len(eb) == len(frames)
            for m, a, b in zip(frames, ea, eb):
                assert 0 <= a < 6 * STRIDE and 0 <= b < 6 * STRIDE
                if j >= 1:
                    assert lds[a] == (pos + FRAME * m + 6 * (j - 1)) % N          # G[u] = F(u - 1), u = j
                else:
                    assert not np.isnan(lds[a])                                   # lane j = 0: a valid entry, replaced by W
                assert lds[b] == (pos + FRAME * m + 6 * (55 + j)) % N             # u = 56 + j
                wrapped += int(b % STRIDE >= RING)
    assert wrapped > 0          # some reads went through the wrap pad


@pytest.mark.parametrize("D", [1, 6, 8])
def test_octet_sums_and_signs_equal_the_float64_model(D):
    x = PM._window(300 + D)
    lds = PM.residue_major(PM.plane(x))
    pos_of_lane = positions(D, 20 + D)
    masks = PM._masks()
    for wave in range(8):
        got = sync_pass(x, lds.real.copy(), lds.imag.copy(), pos_of_lane, D, wave, np.float64)
        for i in range(D):
            pos = int(pos_of_lane[wave + 8 * i]) % N
            soft_ref, _, nbad_ref = M.softbits(x, masks[i], pos)
            s_ref = PM._reference_phase_sum(x, masks[i], pos)
            assert abs(got[i]["s"] - s_ref) <= 1e-12 * abs(s_ref), (wave, i, pos)
            scale = np.abs(soft_ref).max()
            assert np.abs(got[i]["soft"] - np.concatenate([soft_ref[0:8], soft_ref[56:64]])).max() <= 1e-12 * scale, (wave, i, pos)
            assert got[i]["nbad"] == nbad_ref, (wave, i, pos)


def test_phasor_float32_octet_association_against_the_parents():
    """float32 emulation of the phase sum in both associations - the parent's (one term per lane, whole-wave sum) and the pass's (two
    terms per lane, octet sum) - from the same float32 plane and side values, against the float64 model.

    Bound, from the format: either order is 15 float32 adds of the same 14 terms (12 plane entries, the edge term's two halves),
    so either sum is within 15 eps x sum|term| of the exact sum of its float32 terms (eps = 2^-24), the two differ by at most twice
    that, and the unit phasors by at most that over |s| plus 3 eps for the rsq and the two multiplies (a unit vector moves by no
    more than the relative change of the vector it normalises).  Against float64 the plane's own float32 error comes on top, the
    1e-5 of the largest softbit that test_softbits_plane_model.py records; here it is taken relative to |s|.
    Measured over the 46 candidates below: the two float32 phasors differ by at most 1.7e-7, and either differs from the float64
    model's by at most 4.6e-7 - next to the 1e-5 the plane file records for a softbit."""
    f32 = np.float32
    masks = PM._masks()
    worst_pair = worst_model = 0.0
    for D, wave in ((8, 0), (8, 5), (6, 7), (1, 3)):
        x = PM._window(400 + D + wave)
        Pr, Pi = PM.plane(x, f32)
        lr, li = PM.residue_major(Pr), PM.residue_major(Pi)
        x32 = x.real.astype(f32).astype(np.float64) + 1j * x.imag.astype(f32).astype(np.float64)
        pos_of_lane = positions(D, 30 + D + wave)
        for w in (wave, (wave + 3) % 8):
            new = sync_pass(x32, lr, li, pos_of_lane, D, w, f32)
            old = sync_pass(x32, lr, li, pos_of_lane, D, w, f32, parent_association=True)
            for i in range(D):
                s_ref = PM._reference_phase_sum(x, masks[i], new[i]["pos"])
                rot_ref = np.conj(s_ref) / abs(s_ref)
                bound = 2 * 15 * EPS32 * new[i]["mag"] / abs(s_ref) + 2 * 3 * EPS32
                pair = abs(new[i]["rot"] - old[i]["rot"])
                assert pair <= bound, (D, w, i, pair, bound)
                worst_pair = max(worst_pair, pair)
                for rot in (new[i]["rot"], old[i]["rot"]):
                    dev = abs(rot - rot_ref)
                    assert dev <= bound + 1e-5 * new[i]["mag"] / abs(s_ref), (D, w, i, dev)
                    worst_model = max(worst_model, dev)
    print(f"float32 phasor: octet against whole-wave association {worst_pair:.2e}, against the float64 model {worst_model:.2e}")
