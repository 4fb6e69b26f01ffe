// softbits: matched-filter plane per tile, per-candidate frame fold, carrier-phase estimate, LLR scaling, sync check.
//
// Replaces softbits_kernel (softbits_kernel.cuh:9-249).  The reference launches one
// 160-thread block per candidate and every block re-mixes the whole 5184-sample window; here one
// workgroup (8 waves) serves all D*8 candidates of a (channel, frequency) pair and mixes the window ONCE
// into LDS (same float phase as the scan).
//
// Filtering and folding are both linear, so they commute.  The workgroup applies the 11-tap half-sine pulse ONCE to the
// whole ring, P[n] = sum_{s=1..11} pp[s] x[(n + s) mod 5184], and writes P over the mixed window.  Softbit u = 1..143 of a
// candidate at `pos` with frame mask M is then one component of rot * F(u-1) (Re for odd u, Im for even u), where
//     F(g) = sum_{m in M} P[pos + 864 m + 6 g]
// and rot is the carrier phasor: a candidate costs one LDS read and one complex add per frame and 64 softbits, then a rotation.
// (softbits_kernel.cuh:157-180 sums I bits 12j..12j+11 and Q bits 12j-6..12j+5 of the rotated folded frame: softbit u is the
// 12-tap sum over groups u-1 and u, i.e. u1[u-1] + u2[u] with u1[g] = sum_{t<6} pp[t] c[6g+t], u2[g] = sum_{t<6} pp[6+t] c[6g+t],
// and u1[g] + u2[g+1] is the folded P at group g.)  Five half-pulse sums per candidate cannot come from P and are folded from the
// mixed window before P replaces it: u2[0] and u1[143] (softbit 0 wraps round the folded frame, group 143 -> group 0) and u1[6],
// u2[56], u1[62] (the sync template covers half a pulse at the edges of each sync word).  Every result is the reference's linear
// form, associated differently (~1e-7 relative, as filtering before rotating already was).
//
// Plane layout, residue-major: P_r[k] = P[6 k + r] in six sub-rings of 864 entries plus a 142-entry wrap pad (kPlaneStride apart),
// so lane l of a candidate reads group g = l + 64 s - 1 at the wave-uniform base ((pos - r)/6 + 144 m) mod 864 of sub-ring
// r = pos mod 6: one lane-contiguous, conflict-free ds_read_b64 per slot and frame.  The plane overwrites the 48.4 KB window in
// place (workgroup barriers between the last read of x and the first write of P), so three workgroups (24 waves) still fit a CU.
//
// A wave demodulates its D candidates (slot `wave` of every pattern) in two steps.  The sync pass runs ONCE per wave, one candidate
// per 8-lane octet (lane 8 i + j: candidate wave + 8 i, sync bit j): it folds the 16 sync softbits (u = 0..7 and 56..63) of every
// candidate, forms the carrier phase per octet and stores nbadsync.  The candidate loop then holds part two only: all three slots,
// the normalisation and the LLR row.  In blocked staging (no LLR row outlives its channel block) a candidate the index stage will
// drop (nbadsync > threshold) has no part two; with the LLR store retained every candidate is demodulated in full.  In part two
// softbit u lives in lane u % 64 of slot u / 64.
// From there the two 144-term sums (softbits_kernel.cuh:186-194) are one per-lane add over the three slots plus a
// single cross-lane reduction carrying both sums (sum_reduction.cuh:14-44 replaced by two interleaved DPP chains).
// The phase rotation uses conj(s)/|s| instead of atan2f + sincosf (same unit vector to ~1 ulp); the
// 84-term phase sum is accumulated per lane and then across the lanes of an octet (order differs from the reference's
// 42->32->16 tree: ~1e-7 relative on a rotation angle).
#include "msk144_kernels.h"
#include "mix.h"
#include "phase_stamps.h"
#include "tile_map.h"
#include "wave64.h"

namespace msk144
{

namespace
{

constexpr int kSbThreads = 512;
constexpr int kSbWaves = kSbThreads / 64;
constexpr int kGroup = 6;                                  // samples per half-bit group
constexpr int kGroups = kFrameSamples / kGroup;            // 144
constexpr int kSlots = (kGroups + 63) / 64;                // 3
// The mixed window is a ring of exactly six frames.  LDS carries one more frame (+ one run of samples) behind it, so a frame
// starting anywhere in the ring is 864 CONTIGUOUS samples (the side values below) and a filter run never wraps.
constexpr int kRingPad = kFrameSamples + kGroup - 1;
constexpr int kWindowLds = kWindowSamples + kRingPad + 3;  // float2 entries of the LDS buffer (48.4 KB)

// The filtered plane, in the same buffer: sub-ring r (r = 0..5) holds P[6 k + r] at entry r * kPlaneStride + k, k < 864, and
// repeats its first kPlanePad entries behind it, so groups 0..142 of a folded frame starting at any k are contiguous.
constexpr int kPlaneRing = kWindowSamples / kGroup;        // 864
constexpr int kPlanePad = kGroups - 2;                     // 142: groups 0..142 come from P (143 wraps into softbit 0)
// 1009 (not 1006): the eleven-output runs of the plane build then write with at most 2-way bank conflicts (1010: 6-way)
constexpr int kPlaneStride = 1009;
static_assert(kPlaneStride >= kPlaneRing + kPlanePad, "sub-ring and its wrap pad");
static_assert(kGroup * kPlaneStride <= kWindowLds, "the plane fits the window's LDS");
// P build: thread t filters outputs 11 t .. 11 t + 10 (an odd run: the 88-byte lane stride of its x reads is conflict-free)
constexpr int kPlaneRun = 11;
static_assert(kPlaneRun * kSbThreads >= kWindowSamples, "one run per thread covers the ring");
static_assert((kWindowSamples + kPlaneRun - 1) / kPlaneRun * kPlaneRun - kWindowSamples <= kGroup * kPlanePad,
              "the last run's outputs past the ring land on wrap-pad entries");
constexpr int kSideValues = 5;                             // u2[0], u1[143], u1[6], u2[56], u1[62]

struct SoftbitsArgs
{
    DeviceStore st;
    SyncTemplate tpl;
    int total_tiles;
    MSK144_STAMP_ARG
};

typedef float v2f __attribute__((ext_vector_type(2)));
typedef const volatile __attribute__((address_space(3))) v2f* lds_v2f_ptr;  // volatile: adjacent reads stay single ds_read_b64

__device__ __forceinline__ v2f fma2(v2f x, float w, v2f acc)
{
    return v2f{fmaf(x.x, w, acc.x), fmaf(x.y, w, acc.y)};
}

__device__ __forceinline__ v2f readlane2(v2f v, int lane)
{
    return v2f{readlane_f32(v.x, lane), readlane_f32(v.y, lane)};
}

// bit 8 p + m: frame m takes part in pattern p (kPatternMask as one word, for a per-lane pattern)
constexpr uint64_t pattern_bits()
{
    uint64_t b = 0;
    for(int p = 0; p < kScanDepthMax; p++)
        for(int m = 0; m < kPatternBits; m++)
            if(kPatternMask[p][m]) b |= uint64_t{1} << (8 * p + m);
    return b;
}
constexpr uint64_t kPatternWord = pattern_bits();

// Fold of the filtered plane over the frames of pattern p (softbits_kernel.cuh:59-82 after the filter) for the slots in kSlotMask.
// pbytes = this candidate's sub-ring, q = its base entry; frame m starts 144 m entries further round the 864-entry sub-ring.
// Frame 0 is part of every pattern (msk_context.cuh:231-238): its values ARE the initial sums.
template<int kSlotMask>
__device__ __forceinline__ void fold_plane(v2f (&f)[kSlots], const char* pbytes, const uint32_t (&lane_g8)[kSlots], uint32_t q, int p)
{
#pragma unroll
    for(int s = 0; s < kSlots; s++)
        if((kSlotMask >> s) & 1) f[s] = *(lds_v2f_ptr)(pbytes + (lane_g8[s] + q * 8u));
    for(int m = 1; m < kPatternBits; m++)
    {
        if(!kPatternMask[p][m]) continue;  // wave-uniform
        uint32_t b = q + static_cast<uint32_t>(kGroups * m);
        if(b >= static_cast<uint32_t>(kPlaneRing)) b -= kPlaneRing;
#pragma unroll
        for(int s = 0; s < kSlots; s++)
            if((kSlotMask >> s) & 1) f[s] += *(lds_v2f_ptr)(pbytes + (lane_g8[s] + b * 8u));
    }
}

// kGateEarly: blocked staging keeps no LLR row of a candidate the index stage will drop (nbadsync > threshold), so such a
// candidate stops after its sync check - a third of the noise candidates at threshold 3.  With the LLR store retained
// (llr_block_channels = channels: dumps, parity tests) every candidate is demodulated in full, as in the reference.
// kHandOver (only with kGateEarly): slots that fold the same frames as a lower slot of their group are handed to it (below).
template<bool kGateEarly, bool kHandOver>
__global__ __launch_bounds__(kSbThreads, 6) void softbits_kernel(const SoftbitsArgs a)
{
    __shared__ __attribute__((aligned(16))) float2 s_x[kWindowLds];
    static_assert(sizeof(s_x) <= 53248, "three workgroups per CU");

    const int tile = tile_index(blockIdx.x, a.total_tiles);  // tile_map.h
    if(tile < 0) return;
    const Tile tl = tile_of(tile, a.st.nch, a.st.F);
    const int ch_rel = tl.ch_rel, b = tl.b;  // channel inside the block [ch0, ch0 + nch), frequency hypothesis
    const int ch = a.st.ch0 + ch_rel;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    MSK144_STAMP_ROW(tile);
    MSK144_STAMP(0);
    MSK144_STAMP(11);  // two stamps back to back: the stamp's own cost

    static_assert(kSbWaves == kSlotsPerPattern, "wave w owns slot w of every pattern: candidate c = w + 8 i is (pattern i, slot w)");
    // Candidates of this wave: c = wave + 8 i, i < D.  The scan positions of all the tile's candidates are fetched once, one per lane
    // (the latency hides under the mix phase), and handed out by readlane: the position is a scalar in the candidate loop.
    const int D = a.st.D;
    const int ncand = D * kSlotsPerPattern;
    const size_t item0 = static_cast<size_t>(ch) * a.st.K + static_cast<size_t>(b) * ncand;
    uint32_t pos_of_lane = 0u;  // lane l: scan position of the tile's candidate l (pattern l / 8, slot l % 8)
    if(lane < ncand) pos_of_lane = a.st.pos[item0 + lane];
    // ---- mix (softbits_kernel.cuh:27-52): each sample rotated by its phasor from the handle's table (mix.h) ----
    const float2* __restrict__ cdat = a.st.analytic + static_cast<size_t>(ch) * kWindowSamples;
    const float2* __restrict__ phasor = a.st.mix_table + static_cast<size_t>(b) * kWindowSamples;
    {
        constexpr int kPerThread = (kWindowSamples + kSbThreads - 1) / kSbThreads;  // 11 (10.125)
        float2 xin[kPerThread], ph[kPerThread];  // all loads in flight before any arithmetic
#pragma unroll
        for(int i = 0; i < kPerThread; i++)
        {
            const int n = tid + i * kSbThreads;
            xin[i] = n < kWindowSamples ? cdat[n] : make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for(int i = 0; i < kPerThread; i++)
        {
            const int n = tid + i * kSbThreads;
            ph[i] = n < kWindowSamples ? phasor[n] : make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for(int i = 0; i < kPerThread; i++)
        {
            const int n = tid + i * kSbThreads;
            if(n < kWindowSamples)
            {
                // the tail (mix.h): the last two samples, n >= 4608; i is a constant once the loop is unrolled
                const float2 y = i >= kPerThread - 2 ? rotate<true>(xin[i], ph[i].x, ph[i].y) : rotate<false>(xin[i], ph[i].x, ph[i].y);
                s_x[n] = y;
                if(n < kRingPad) s_x[kWindowSamples + n] = y;
            }
        }
    }
    MSK144_STAMP(1);
    __syncthreads();
    MSK144_STAMP(2);
#ifdef MSK144_PHASE_STAMPS
    uint64_t st_sync = 0, st_part2 = 0, st_n2 = 0;  // wave 0: cycles in the sync pass / part two of its kept candidates, part-two runs
#endif

    float pp[12];
#pragma unroll
    for(int i = 0; i < 12; i++) pp[i] = a.tpl.pp[i];
    const char* __restrict__ xbytes = reinterpret_cast<const char*>(s_x);

    // Octet layout of the side values and of the sync pass: lane 8 i + j works for this wave's candidate of pattern i, c = wave + 8 i
    // (the `8 p + slot` idiom of the scan's slot rule).  cpos: that candidate's position on the ring.
    const int oct_i = lane >> 3, oct_j = lane & 7;
    uint32_t cpos = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(4 * (wave + kSbWaves * oct_i), static_cast<int>(pos_of_lane)));
    if(cpos >= static_cast<uint32_t>(kWindowSamples)) cpos -= kWindowSamples;  // scanned positions reach 5375
    const uint32_t cmask = static_cast<uint32_t>(kPatternWord >> (8 * oct_i));  // frames of pattern i

    // ---- side values: the five half-pulse sums of each of this wave's candidates that P cannot give ----
    // Lane 8 i + v: candidate wave + 8 i (pattern i), value v = u2[0], u1[143], u1[6], u2[56], u1[62] of its folded frame, folded
    // and filtered exactly as a whole group's fold + matched filter would be (same frames in the same order, same operations).
    // pp[0] = sin 0 = 0 and pp[6] = sin pi/2 = 1 exactly (checked at create): u1 has no tap on sample 0, u2's is the sample.
    v2f side = v2f{0.0f, 0.0f};
    {
        const int si = oct_i, sv = oct_j;
        if(sv < kSideValues && si < D)
        {
            const uint32_t spos = cpos;
            const bool rising = sv == 0 || sv == 3;  // u2: taps pp[6..11]; else u1: taps pp[0..5]
            const uint32_t group = sv == 0 ? 0u : sv == 1 ? static_cast<uint32_t>(kGroups - 1) : sv == 2 ? 6u : sv == 3 ? 56u : 62u;
            const uint32_t mbits = cmask;
            v2f acc[kGroup];
#pragma unroll
            for(int m = 0; m < kPatternBits; m++)
            {
                if(m > 0 && !((mbits >> m) & 1u)) continue;  // per lane; frame 0 is in every pattern
                uint32_t fb = spos + static_cast<uint32_t>(kFrameSamples * m);
                if(fb >= static_cast<uint32_t>(kWindowSamples)) fb -= kWindowSamples;
                lds_v2f_ptr xr = (lds_v2f_ptr)(xbytes + (fb + kGroup * group) * 8u);
#pragma unroll
                for(int t = 0; t < kGroup; t++)
                {
                    const v2f xt = xr[t];
                    acc[t] = m == 0 ? xt : acc[t] + xt;
                }
            }
            if(rising)
            {
                side = acc[0];
#pragma unroll
                for(int t = 1; t < kGroup; t++) side = fma2(acc[t], pp[kGroup + t], side);
            }
            else
            {
                side = acc[1] * pp[1];
#pragma unroll
                for(int t = 2; t < kGroup; t++) side = fma2(acc[t], pp[t], side);
            }
        }
    }

    // Per candidate i only two sums are needed: W = u1[143] + u2[0] (softbit 0), left in lane 8 i (side_w), and the sync words' edge
    // term s7 (u1[6] + u1[62]) - i s0 (u2[0] + u2[56]) of the phase sum, formed in lane 8 i + 1 and spread over the octet (side_edge).
    v2f side_w, side_edge;
    {
        const v2f a1 = v2f{__shfl(side.x, lane + 1), __shfl(side.y, lane + 1)};  // lane 8 i: u1[143]; lane 8 i + 1: u1[6]
        const v2f a2 = v2f{__shfl(side.x, lane + 2), __shfl(side.y, lane + 2)};  // lane 8 i + 1: u2[56]
        const v2f a3 = v2f{__shfl(side.x, lane + 3), __shfl(side.y, lane + 3)};  // lane 8 i + 1: u1[62]
        const v2f m1 = v2f{__shfl(side.x, lane - 1), __shfl(side.y, lane - 1)};  // lane 8 i + 1: u2[0]
        constexpr float s0 = static_cast<float>(kSync8Pm[0]), s7 = static_cast<float>(kSync8Pm[7]);
        const v2f edge = v2f{s7 * (a1.x + a3.x) + s0 * (m1.y + a2.y), s7 * (a1.y + a3.y) - s0 * (m1.x + a2.x)};
        side_w = a1 + side;
        side_edge = v2f{__shfl(edge.x, (lane & ~7) + 1), __shfl(edge.y, (lane & ~7) + 1)};
    }

    // ---- P build: thread t filters outputs n = 11 t .. 11 t + 10 of the ring from x[n + 1 .. n + 11] (softbits_kernel.cuh:157-180
    // before the rotation and the fold), held in registers across the barrier, then writes them over x ----
    {
        const uint32_t n0 = static_cast<uint32_t>(tid) * kPlaneRun;
        v2f pv[kPlaneRun];
        if(n0 < static_cast<uint32_t>(kWindowSamples))
        {
            lds_v2f_ptr xr = (lds_v2f_ptr)(xbytes + (n0 + 1u) * 8u);  // x[n0 + 1 + k]: at most x[5202], inside the ring pad
            v2f w[kPlaneRun + 2 * kGroup - 2];
#pragma unroll
            for(int k = 0; k < kPlaneRun + 2 * kGroup - 2; k++) w[k] = xr[k];
#pragma unroll
            for(int j = 0; j < kPlaneRun; j++)
            {
                // u1 = taps 1..5 on x[n+1..n+5], u2 = taps 6..11 on x[n+6..n+11] (pp[6] = 1): the half-pulse sums of the old
                // per-group filter, added
                v2f u1 = w[j] * pp[1];
#pragma unroll
                for(int t = 2; t < kGroup; t++) u1 = fma2(w[j + t - 1], pp[t], u1);
                v2f u2 = w[j + kGroup - 1];
#pragma unroll
                for(int t = 1; t < kGroup; t++) u2 = fma2(w[j + kGroup - 1 + t], pp[kGroup + t], u2);
                pv[j] = u1 + u2;
            }
        }
        __syncthreads();  // every read of x (side values and plane build) is done
        // The last run (thread 471) ends 8 outputs past the ring: P[5184 + j] is filtered from the ring pad, x[5185 + ...] =
        // x[1 + ...], so it IS P[j] and lands on P[j]'s wrap-pad entry (sub-ring j mod 6, entry 864 + j / 6) with the same bits.
        if(n0 < static_cast<uint32_t>(kWindowSamples))
        {
            const uint32_t r0 = n0 % kGroup, k0 = n0 / kGroup;
            uint32_t r = r0, k = k0;
#pragma unroll
            for(int j = 0; j < kPlaneRun; j++)
            {
                s_x[r * kPlaneStride + k] = make_float2(pv[j].x, pv[j].y);
                if(++r == static_cast<uint32_t>(kGroup))
                {
                    r = 0;
                    ++k;
                }
            }
            if(n0 < static_cast<uint32_t>(kGroup * kPlanePad))  // waves 0 and 1 only: the wrap pad
            {
                r = r0;
                k = k0;
#pragma unroll
                for(int j = 0; j < kPlaneRun; j++)
                {
                    if(k < static_cast<uint32_t>(kPlanePad)) s_x[r * kPlaneStride + k + kPlaneRing] = make_float2(pv[j].x, pv[j].y);
                    if(++r == static_cast<uint32_t>(kGroup))
                    {
                        r = 0;
                        ++k;
                    }
                }
            }
        }
        __syncthreads();
    }
    MSK144_STAMP(7);

    // Slots that fold the same frames.  The scan walks 5376 positions of a 5184-sample ring, so positions p and p + 5184 are one
    // place (2.9 % of the slots of a noise window hold such a pair); masks 111111 and 100100 moreover sum the same frames at pos
    // and pos + 864 (+ 2592), so the eight slots of those patterns are mostly the copies of two or three peaks, one per period
    // (exact ties in exact arithmetic: 73 % of the slots of pattern 5 on the bench workload).  The reference demodulates and decodes
    // every copy (softbits_kernel.cuh:56-83 folds the frames of a periodic copy in another order: the same sums up to float
    // association; a wrapped copy is the same computation).  Here, when no LLR row outlives its block, a slot whose position is
    // congruent to a LOWER slot's of its group hands its work to that slot: it stores -1 - slot as its nbadsync, the index stage
    // leaves it out and the collect stage gives it the nbadsync and the decode of the slot it names (index.hip).  With the store
    // retained every slot is computed on its own, as in the reference.
    // Bit 8 i + s of same_frames: slot s of pattern i is congruent to THIS wave's slot of pattern i.
    static_assert(kGateEarly || !kHandOver, "a retained LLR store keeps every slot's own row");
    uint64_t same_frames = 0;
    if(kHandOver)
    {
        uint32_t r = pos_of_lane >= static_cast<uint32_t>(kWindowSamples) ? pos_of_lane - kWindowSamples : pos_of_lane;
        const int pattern_of_lane = lane >> 3;
        if(pattern_of_lane == kFirstPeriodicPattern) r %= static_cast<uint32_t>(kPatternPeriod[0]);
        if(pattern_of_lane == kFirstPeriodicPattern + 1) r %= static_cast<uint32_t>(kPatternPeriod[1]);
        const uint32_t mine = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(4 * ((lane & ~(kSlotsPerPattern - 1)) + wave), static_cast<int>(r)));
        same_frames = __ballot(lane < ncand && r == mine);
    }

    // ---- sync pass: the 16 sync softbits, the carrier phase and nbadsync of all this wave's candidates at once ----
    // Lane 8 i + j folds two plane entries of candidate i over its pattern's frames (order m = 0..5, the adds of fold_plane: the same
    // bits part two folds later): F(j - 1) for softbit j (lane j = 0: softbit 0 is the wrap sum W instead) and F(55 + j) for softbit
    // 56 + j.  The 8 lanes of an octet read consecutive entries of one sub-ring; octets may meet in a bank.
    // Phase estimate = sum over the two sync words of folded sample x conj(template) (softbits_kernel.cuh:88-137).  Inside a group
    // the template is one half of the half-sine pulse on each rail, signed by a sync bit (msk_context.cuh:188-196: I carries bits
    // 1,1,3,3,5,5,7 and Q bits 0,2,2,4,4,6,6 over the seven groups), so the sum over the first sync word is
    //     s1 F(0) + s3 F(2) + s5 F(4) + s7 u1[6] - i (s0 u2[0] + s2 F(1) + s4 F(3) + s6 F(5))
    // and the second the same at groups 56..62.  Lanes j = 1..6 take both their F with their own sync bit, on the real part for odd j
    // (k_x) and as -i F for even j (k_y); lanes 0 and 7 add nothing: their bits sit in the edge term, added after the octet sum.
#ifdef MSK144_PHASE_STAMPS
    const uint64_t st_s0 = (stamp_row_ && tid < 64) ? stamp_now() : 0;
#endif
    float cr_v = 1.0f, ci_v = 0.0f;  // lane 8 i + j: unit phasor of candidate i
    uint64_t keep;                   // bit 8 i: candidate i goes through part two
    {
        const uint32_t q = cpos / kGroup;
        const uint32_t ga8 = static_cast<uint32_t>(oct_j > 0 ? oct_j - 1 : 0) * 8u;  // lane j = 0 re-reads group 0; W replaces it
        const uint32_t gb8 = static_cast<uint32_t>(kSecondSyncBit - 1 + oct_j) * 8u;
        const uint32_t a0 = (cpos - q * kGroup) * (kPlaneStride * 8u) + q * 8u + ga8;  // sub-ring pos mod 6, per lane: byte offset of read A, frame 0
        const uint32_t a_to_b = gb8 - ga8;
        // every frame is read (the address is inside the sub-ring whatever the pattern), all twelve loads in flight; a lane adds the
        // frames of its own pattern only
        v2f va[kPatternBits], vb[kPatternBits];
#pragma unroll
        for(int m = 0; m < kPatternBits; m++)
        {
            // base (q + 144 m) mod 864, as a byte offset from frame 0's
            uint32_t oa = a0 + static_cast<uint32_t>(kGroups * m) * 8u;
            if(m > 0 && q >= static_cast<uint32_t>(kPlaneRing - kGroups * m)) oa -= kPlaneRing * 8u;
            va[m] = *(lds_v2f_ptr)(xbytes + oa);
            vb[m] = *(lds_v2f_ptr)(xbytes + (oa + a_to_b));
        }
        v2f fa = va[0], fb = vb[0];  // frame 0 is in every pattern
#pragma unroll
        for(int m = 1; m < kPatternBits; m++)
        {
            const bool in = ((cmask >> m) & 1u) != 0u;  // per lane
            const v2f ta = fa + va[m], tb = fb + vb[m];
            fa = in ? ta : fa;
            fb = in ? tb : fb;
        }

        constexpr uint32_t kSyncBits = []() { uint32_t b = 0; for(int k = 0; k < 8; k++) b |= static_cast<uint32_t>(kSync8[k]) << k; return b; }();
        const int sync_pm = static_cast<int>((kSyncBits >> oct_j) & 1u) * 2 - 1;  // sync bit j as +-1
        // pr = k_x F.x + k_y F.y, pi = k_x F.y - k_y F.x: the lane's sync bit on one of the two, j = 1..6 only
        const bool inner = static_cast<uint32_t>(oct_j - 1) < 6u;
        const float k_x = inner && (oct_j & 1) ? static_cast<float>(sync_pm) : 0.0f;
        const float k_y = inner && !(oct_j & 1) ? static_cast<float>(sync_pm) : 0.0f;
        // carrier phase from the two sync words (softbits_kernel.cuh:88-137): sum c3[k]*conj(cb[k])
        float pr = f32_add(fmaf(k_y, fa.y, k_x * fa.x), fmaf(k_y, fb.y, k_x * fb.x));
        float pi = f32_add(fmaf(-k_y, fa.x, k_x * fa.y), fmaf(-k_y, fb.x, k_x * fb.y));
        oct_sum2_f32(pr, pi);
        const float sre = pr + side_edge.x;
        const float sim = pi + side_edge.y;
        // cfac = conj(exp(i*atan2(im,re))) = (re, -im)/|s|
        {
            const float m2 = fmaf(sre, sre, sim * sim);
            if(m2 > 0.0f)
            {
                const float inv = __builtin_amdgcn_rsqf(m2);  // 1 ulp: the unit phasor only needs ~1e-7
                cr_v = sre * inv;
                ci_v = -sim * inv;
            }
            else if(!(m2 == 0.0f))
            {
                cr_v = m2;  // NaN propagates like the reference's atan2f/sincosf chain
                ci_v = m2;
            }
        }

        // de-rotate (softbits_kernel.cuh:146-153): softbit u = Re(rot F) for odd u (I bit), Im(rot F) for even u (Q bit), rot = cr + i ci;
        // u = j and u = 56 + j have the parity of j.  The same expression as part two's, so the same bits.
        const bool odd = (oct_j & 1) != 0;
        const float b_r = odd ? cr_v : ci_v, b_i = odd ? -ci_v : cr_v;
        const v2f f0 = oct_j == 0 ? side_w : fa;  // softbit 0: group 143 of the folded frame wraps into group 0
        const float soft_a = fmaf(f0.y, b_i, f0.x * b_r);
        const float soft_b = fmaf(fb.y, b_i, fb.x * b_r);

        // ---- sync-word disagreements (softbits_kernel.cuh:214-241): bits 0..7 and 56..63; byte i of each ballot is candidate i's ----
        const uint64_t bad_a = __ballot(((soft_a < 0.0f) ? -1 : 1) != sync_pm);
        const uint64_t bad_b = __ballot(((soft_b < 0.0f) ? -1 : 1) != sync_pm);
        const int nbad = __popc(static_cast<uint32_t>(bad_a >> (8 * oct_i)) & 0xffu) + __popc(static_cast<uint32_t>(bad_b >> (8 * oct_i)) & 0xffu);

        // Slots that fold the same frames as a lower slot of their (frequency, pattern) group: that slot does the work, this one names it
        uint32_t lower = 0u;
        if(kHandOver) lower = static_cast<uint32_t>(same_frames >> (kSlotsPerPattern * oct_i)) & ((1u << wave) - 1u);
        const bool owner = oct_j == 0 && oct_i < D;
        if(owner) a.st.nbadsync[item0 + wave + kSbWaves * oct_i] = lower != 0u ? -1 - __builtin_ctz(lower) : nbad;
        // the gate is wave-uniform per candidate: the index stage drops a candidate with nbadsync > threshold
        keep = __ballot(owner && lower == 0u && !(kGateEarly && nbad > a.st.nbadsync_threshold));
    }
#ifdef MSK144_PHASE_STAMPS
    if(stamp_row_ && tid < 64) st_sync = stamp_now() - st_s0;
#endif

    // byte offset inside a sub-ring of the group this lane reads per slot: softbit u = lane + 64 s needs F(u - 1).  Lane 0 of slot 0
    // (softbit 0 wraps: it takes the side values) and lanes >= 16 of slot 2 (no softbit) re-read a neighbouring group so the reads
    // stay in the sub-ring and convergent; their values are replaced or discarded.
    uint32_t lane_g8[kSlots];
#pragma unroll
    for(int s = 0; s < kSlots; s++)
    {
        int g = lane + 64 * s - 1;
        g = g < 0 ? 0 : g > kPlanePad ? kPlanePad : g;
        lane_g8[s] = static_cast<uint32_t>(g) * 8u;
    }
    const bool odd = (lane & 1) != 0;

    // ---- part two, per kept candidate: all three slots and the rest of the demodulation ----
    for(int i = 0; i < D; i++)
    {
        if(!((keep >> (kSlotsPerPattern * i)) & 1u)) continue;  // handed over, or gated: wave-uniform
        const int p = i, slot = wave;  // wave w owns slot w of every pattern
        const int c = slot + kSbWaves * p;
        const size_t item = item0 + c;
#ifdef MSK144_PHASE_STAMPS
        const uint64_t st_t1 = (stamp_row_ && tid < 64) ? stamp_now() : 0;
#endif
        const uint32_t pos = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cpos), kSlotsPerPattern * i));
        const uint32_t q = pos / kGroup;
        const char* pbytes = xbytes + (pos - q * kGroup) * (kPlaneStride * 8u);  // sub-ring pos mod 6
        v2f f[kSlots];
        fold_plane<0b111>(f, pbytes, lane_g8, q, p);
        const float cr = readlane_f32(cr_v, kSlotsPerPattern * i), ci = readlane_f32(ci_v, kSlotsPerPattern * i);
        const v2f wrap = readlane2(side_w, kSlotsPerPattern * i);

        // de-rotate (softbits_kernel.cuh:146-153): softbit u = Re(rot F) for odd u (I bit), Im(rot F) for even u (Q bit), rot = cr + i ci.
        // re = fr*cr - fi*ci, im = fr*ci + fi*cr: pick the coefficient pair per lane once instead of selecting per value.
        const float b_r = odd ? cr : ci, b_i = odd ? -ci : cr;
        float soft[kSlots];
        {
            const v2f f0 = lane == 0 ? wrap : f[0];  // softbit 0: group 143 of the folded frame wraps into group 0
            soft[0] = fmaf(f0.y, b_i, f0.x * b_r);
        }
        soft[1] = fmaf(f[1].y, b_i, f[1].x * b_r);
        soft[2] = lane < kGroups - 64 * (kSlots - 1) ? fmaf(f[2].y, b_i, f[2].x * b_r) : 0.0f;

        // ---- normalisation (softbits_kernel.cuh:186-201) ----
        // sum and sum of squares of the 144 softbits: per lane over its three slots first, then ONE cross-lane reduction
        // for both (two interleaved DPP chains, row sums combined as ((r0+r1)+(r2+r3))).  The reference's
        // sum_reduction_two_cycles order (five 32-lane warp sums) was reproduced term by term until round 2 at the price of
        // six separate reductions; a different association moves sav/s2av by ~1e-7 relative, i.e. every LLR by ~1e-7 of
        // itself - four orders inside the 1e-3 tolerance and below what sincos/sqrt differences already contribute (8e-6).
        float sum_sav, sum_s2av;
        {
            float t = f32_add(f32_add(soft[0], soft[1]), soft[2]);
            float q2 = fmaf(soft[2], soft[2], fmaf(soft[1], soft[1], f32_mul(soft[0], soft[0])));
            wave_sum2_f32(t, q2);
            sum_sav = t;
            sum_s2av = q2;
        }
        // sav, s2av, ssig and the scale are wave-uniform numbers formed from two 144-term sums that already differ from the
        // reference's by ~1e-7 relative (different association): rounding them correctly on top (a Markstein division by 144,
        // the library's 15-instruction sqrt, a Newton step on the reciprocal) bought nothing measurable and cost ~35 uniform
        // VALU instructions per candidate.  One-ulp hardware forms: x * (1/144), v_sqrt_f32, 2 * v_rcp_f32.
        const float sav = sum_sav * (1.0f / 144.0f);
        const float s2av = sum_s2av * (1.0f / 144.0f);
        const float ssig = __builtin_amdgcn_sqrtf(fmaf(-sav, sav, s2av));
        const float sigma = 0.60f;
        const float scale = 2.0f * __builtin_amdgcn_rcpf(ssig * (sigma * sigma));

        // ---- store (softbits_kernel.cuh:204-211,244-247) ----
        float* __restrict__ llr = a.st.llr + (item - static_cast<size_t>(a.st.ch0) * a.st.K) * kCodeBits;
        if(lane >= 8 && lane < 56) llr[lane - 8] = f32_mul(scale, soft[0]);      // u = 8..55    -> 0..47
        llr[48 + lane] = f32_mul(scale, soft[1]);                                // u = 64..127  -> 48..111
        if(lane < 16) llr[112 + lane] = f32_mul(scale, soft[2]);                 // u = 128..143 -> 112..127
#ifdef MSK144_PHASE_STAMPS
        if(stamp_row_ && tid < 64)
        {
            st_part2 += stamp_now() - st_t1;
            st_n2++;
        }
#endif
    }
#ifdef MSK144_PHASE_STAMPS
    if(stamp_row_ && tid == 0)
    {
        stamp_row_[3] = st_sync;
        stamp_row_[4] = st_part2;
        stamp_row_[5] = st_n2;
    }
#endif
    MSK144_STAMP(6);
    MSK144_STAMP_WAVE_END();
}

}  // namespace

void launch_softbits(const DeviceStore& st, const SyncTemplate& tpl, hipStream_t stream)
{
    SoftbitsArgs a;
    a.st = st;
    a.tpl = tpl;
    a.total_tiles = st.nch * st.F;
#ifdef MSK144_PHASE_STAMPS
    a.stamps = stamp_buffer(1);
#endif
    const int grid = tiles_per_xcd(a.total_tiles) * 8;
    // LLR rows are retained only when one block covers every channel of the handle (msk144_api.cpp: dumps, parity tests)
    if(st.gate_early && st.handover) hipLaunchKernelGGL((softbits_kernel<true, true>), dim3(grid), dim3(kSbThreads), 0, stream, a);
    else if(st.gate_early) hipLaunchKernelGGL((softbits_kernel<true, false>), dim3(grid), dim3(kSbThreads), 0, stream, a);
    else hipLaunchKernelGGL((softbits_kernel<false, false>), dim3(grid), dim3(kSbThreads), 0, stream, a);
}

}  // namespace msk144
