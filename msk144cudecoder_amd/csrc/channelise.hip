// channelise: the wideband down-converter bank (msk144_push_wideband), one kernel for every rate Fs = 12000 P/Q, Q >= 1.
//
// For channel c with offset f_c and the prototype low-pass h[0..L), L = K*P taps at the upsampled rate Q Fs, every output sample is
//     y_c[m] = e^{-j2pi (f_c n_m mod Fs)/Fs} * sum_k h[r_m + kQ] e^{+j2pi (f_c k mod Fs)/Fs} x[n_m - k],   n_m = floor(mP/Q), r_m = mP mod Q
// (include/msk144hip.h).  Output m = mr + Q a reads n_m = n0 + a P with n0 = floor(mr P/Q) and the taps h[r + kQ], r = mr P mod Q,
// k < K_r = ceil((L - r)/Q): each of the Q residues mr is a decimate-by-P branch of its own (blockIdx.z = mr, WidebandBranch) whose
// outputs land Q apart in the same staging.  An integer rate Fs = D x 12000 is the case Q = 1: one branch with r = 0, n0 = 0 and all
// L taps, D = P.
//
// A branch is a complex GEMM over a Hankel view of the input, computed only at the output rate.  With k = p + P*q (phase p < P),
// x[n0 + aP - k] = xp[p][a - q] where xp[p][n] = x[n0 + nP - p]: stored phase by phase in LDS, the operand a wave reads for one tap
// is 32 consecutive floats, so the Hankel view costs no bank conflicts.  The loop walks exactly the K_r taps of the branch: phases
// p < s carry Kq = ceil(K_r/P) taps, the others one fewer (Q = 1: every phase carries K).
//
// Tiling: one workgroup = 4 waves = 128 channels x 64 output samples of one branch.  Each wave owns 32 channels and two 32-sample
// halves of the output tile and runs v_mfma_f32_32x32x2_f32 with the two k-slots of the instruction carrying the real and the
// imaginary part:
//     Re: A[c][0] = Re G, A[c][1] = -Im G;   Im: A[c][0] = Im G, A[c][1] = Re G;   B[0][m] = Re x, B[1][m] = Im x
// so 4 MFMAs per tap and wave (Re/Im x two halves), accumulating in f32.  The input span of the tile is converted to f32 once,
// 32 phases at a time, and shared by the 4 waves; the taps stream from L2 (a branch's G block is stored [channel/32][p][q][32], the
// order the loop walks, so a wave reads 256 contiguous bytes per tap) and are reused across the 64 samples of the tile.
//
// Output: q = clamp(rint(scale_c * y), -128, 127) for I and Q with scale_c = 128 * gain of the channel's slot (times 2^e under the
// AGC), written as int8 pairs straight into the hop ring's staging (first push: samples 0..2591 into first_halves, 2592..5183 into
// hops; later pushes: hops).  A component counts as clipped when its rounded value lies outside [-128, 127].  Every channel's
// sum of I^2 + Q^2 over the stored values and its clipped components are added to levels[channel], in integers.
//
// Rates above 6.144 Msps (format kSubbandFormat): the kernel runs at the sub-band rate Fs/32 on the complex-f32 streams of the
// analysis bank (bank.hip), each wave on the band of its 32 channel slots; see channelise_kernel.
#include "msk144_kernels.h"
#include "wideband_samples.h"

namespace msk144
{

namespace
{

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kTileChannels = 128;  // 4 waves x 32
constexpr int kTileSamples = 64;    // 2 x 32 per wave
constexpr int kPhaseChunk = 32;     // phases staged in LDS at a time
constexpr int kMaxK = 64;
constexpr int kMaxSpan = kTileSamples + kMaxK - 1;
constexpr int kHalf = kWindowSamples / 2;  // 2592 samples per hop
constexpr int kChannelRate = 12000;

// FMT 3 (the two-stage bank): raw holds one complex-f32 sub-band stream per occupied band, bands.stride apart, and channel slot c
// (channels grouped by band, each band's group padded to whole waves) belongs to channel bands.slot_channel[c] (-1: padding).  Every
// wave stages its own band's input in its own quarter of the LDS image (kPhaseChunk/4 phases at a time), so the slots of one tile
// may lie in four different bands; the taps, branches and loop structure are the same for every band.
template<int FMT>
__global__ __launch_bounds__(kThreads) void channelise_kernel(const void* __restrict__ raw, const float2* __restrict__ G, const WidebandBranch* __restrict__ branches,
                                                              const int32_t* __restrict__ fmod, const float2* __restrict__ rot, int8_t* __restrict__ first_halves,
                                                              int8_t* __restrict__ hops, unsigned long long* __restrict__ clip_count, int channels, int P, int Q,
                                                              int hist, int M, int first, long long m_base, const float* __restrict__ scale,
                                                              unsigned long long* __restrict__ levels, WidebandBands bands)
{
    __shared__ float xs[2][kPhaseChunk][kMaxSpan];
    constexpr bool kBank = FMT == kSubbandFormat;
    constexpr int kChunk = kBank ? kPhaseChunk / 4 : kPhaseChunk;

    const int mr = blockIdx.z;
    const WidebandBranch br = branches[mr];
    const int Kr = br.taps;
    const int Kq = (Kr + P - 1) / P;         // taps of the longest phases
    const int s_full = Kr - (Kq - 1) * P;    // phases 0 .. s_full-1 have Kq taps, the others Kq-1
    const int phases = min(P, Kr);
    const int A = M / Q;                     // outputs of this branch in the push
    const int n_in = hist + A * P;           // samples in raw: `hist` before this push, then the new ones
    const int span = kTileSamples + Kq - 1;
    const int at0 = blockIdx.x * kTileSamples;
    const int base = hist + br.n0 + (at0 - Kq + 1) * P;  // raw index of xp[0][0]
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int j = lane & 31;
    const int hsel = lane >> 5;              // k-slot of the MFMA: 0 = real part, 1 = imaginary part
    const int cb32 = blockIdx.y * (kTileChannels / 32) + wave;
    const bool active = cb32 * 32 < channels;
    const float2* __restrict__ g = G + br.g_off + static_cast<size_t>(cb32) * Kr * 32 + j;

    // who stages what: all 256 threads one image of raw, or (bank) the 64 lanes of each active wave an image of the wave's own band
    const int e0 = kBank ? lane : threadIdx.x;
    constexpr int kStageStride = kBank ? 64 : kThreads;
    const bool stages = !kBank || active;
    const int prow = kBank ? wave * kChunk : 0;  // the image's first phase row in LDS
    const void* src = raw;
    if(kBank && active) src = static_cast<const float2*>(raw) + bands.stride * bands.wave_band[cb32];

    f32x16 acc_re0 = {}, acc_im0 = {}, acc_re1 = {}, acc_im1 = {};

    for(int p0 = 0; p0 < phases; p0 += kChunk)
    {
        const int pc = min(kChunk, phases - p0);
        __syncthreads();
        // xp[p][n] = raw[base + n P - p]: output at0 + n - (Kq-1), tap p (+ P q for the q-th tap of the phase, read at n - q);
        // consecutive threads take consecutive phases, i.e. consecutive (descending) input samples
        for(int e = e0; stages && e < pc * span; e += kStageStride)
        {
            const int pl = e % pc;
            const int n = e / pc;
            const int i = base + n * P - (p0 + pl);
            float2 v = make_float2(0.0f, 0.0f);
            if(i >= 0 && i < n_in && !(first && i < hist)) v = load_sample<FMT>(src, i);
            xs[0][prow + pl][n] = v.x;
            xs[1][prow + pl][n] = v.y;
        }
        __syncthreads();
        if(!active) continue;
        const int t0 = p0 * Kq - max(0, p0 - s_full);
        const int T = (p0 + pc) * Kq - max(0, p0 + pc - s_full) - t0;
        const float2* __restrict__ gp = g + static_cast<size_t>(t0) * 32;
        const float* __restrict__ xrow = &xs[hsel][prow][j + Kq - 1];
        float2 gnext = gp[0];
        int pl = 0, q = 0;
        int kp = p0 < s_full ? Kq : Kq - 1;
        for(int t = 0; t < T; t++)
        {
            const float2 gv = gnext;
            if(t + 1 < T) gnext = gp[static_cast<size_t>(t + 1) * 32];
            const float a_re = hsel ? -gv.y : gv.x;
            const float a_im = hsel ? gv.x : gv.y;
            const float* xr = xrow + pl * kMaxSpan - q;
            const float b0 = xr[0];
            const float b1 = xr[32];
            acc_re0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re, b0, acc_re0, 0, 0, 0);
            acc_im0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_im, b0, acc_im0, 0, 0, 0);
            acc_re1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re, b1, acc_re1, 0, 0, 0);
            acc_im1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_im, b1, acc_im1, 0, 0, 0);
            if(++q == kp)
            {
                q = 0;
                pl++;
                kp = p0 + pl < s_full ? Kq : Kq - 1;
            }
        }
    }
    if(!active) return;

    // D[row][col]: col = lane & 31 = output sample, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = channel within the wave.
    // The two samples of a lane: where they go, and the phase index of their rotation.
    // f_c n_m / Fs = f_c (m - mr) / 12000 + f_c n0 / Fs; the second term is in G
    const int half = kHalf;
    bool live[2];
    int mm[2];
    char2* dst[2];
#pragma unroll
    for(int s = 0; s < 2; s++)
    {
        const int a = at0 + s * 32 + j;
        const int mo = mr + Q * a;
        live[s] = a < A;
        mm[s] = static_cast<int>((m_base + static_cast<long long>(Q) * a) % kChannelRate);
        int8_t* base_s = hops;
        int idx = mo;
        if(first && mo < half) base_s = first_halves;
        else if(first) idx = mo - half;
        dst[s] = reinterpret_cast<char2*>(base_s) + idx;
    }
    // Row by row: quantise and store the lane's two samples, then sum the row's statistics over the 32 lanes of the half-wave that
    // share its channel - sum of I^2 + Q^2 of the stored values in bits 0..23 (<= 2 x 2 x 128^2 a lane, 2^21 a row), clipped
    // components from bit 24 (<= 4 a lane, 128 a row) - and leave the sum with lane j = r.  Integer sums: any order, same result.
    unsigned int mine = 0;
#pragma unroll
    for(int r = 0; r < 16; r++)
    {
        const int c = cb32 * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
        int ch = -1;
        if(c < channels) ch = kBank ? bands.slot_channel[c] : c;  // the channel of slot c; -1: padding
        unsigned int v = 0;
        if(ch >= 0)
        {
            const int f = fmod[c];
            const float scale_c = scale[c];
#pragma unroll
            for(int s = 0; s < 2; s++)
            {
                if(!live[s]) continue;
                const float yr = s ? acc_re1[r] : acc_re0[r];
                const float yi = s ? acc_im1[r] : acc_im0[r];
                const int ph = (f * mm[s]) % kChannelRate;
                const float2 e = rot[ph];
                const float vr = rintf(scale_c * (yr * e.x - yi * e.y));
                const float vi = rintf(scale_c * (yr * e.y + yi * e.x));
                const unsigned int over = (vr < -128.0f || vr > 127.0f) + (vi < -128.0f || vi > 127.0f);
                char2 o;
                o.x = static_cast<signed char>(fminf(fmaxf(vr, -128.0f), 127.0f));
                o.y = static_cast<signed char>(fminf(fmaxf(vi, -128.0f), 127.0f));
                dst[s][static_cast<size_t>(ch) * half] = o;
                v += static_cast<unsigned int>(o.x * o.x + o.y * o.y) + (over << 24);
            }
        }
        for(int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if(j == r) mine = v;
    }
    // one atomic instruction per wave and tile: lane j < 16 of each half adds row j's sums to its channel's word (pack_level)
    if(j < 16 && mine)
    {
        const int c = cb32 * 32 + (j & 3) + 8 * (j >> 2) + 4 * hsel;  // < channels and no padding slot, as mine != 0
        const int ch = kBank ? bands.slot_channel[c] : c;
        atomicAdd(&levels[ch], msk144wb::pack_level(mine & 0xffffffu, mine >> 24));
    }
    unsigned int clipped = j < 16 ? mine >> 24 : 0;
    for(int off = 32; off > 0; off >>= 1) clipped += __shfl_xor(clipped, off);
    if(lane == 0 && clipped) atomicAdd(clip_count, static_cast<unsigned long long>(clipped));
}

// The AGC step after a push (msk144_set_wideband_agc), one thread per channel slot: record the exponent the push was quantised
// with, apply msk144wb::agc_step to the push's statistics, and write the slot's scale for the next push.
__global__ void agc_step_kernel(const unsigned long long* __restrict__ levels, const int32_t* __restrict__ slot_channel, const float* __restrict__ gains,
                                int32_t* __restrict__ exps, int32_t* __restrict__ quiet, int32_t* __restrict__ used_exps, float* __restrict__ scale, int slots,
                                int samples, msk144wb::AgcParams p)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if(c >= slots) return;
    const int ch = slot_channel ? slot_channel[c] : c;
    if(ch < 0) return;
    const unsigned long long w = levels[ch];
    int32_t e = exps[ch], q = quiet[ch];
    used_exps[ch] = e;
    msk144wb::agc_step(p, samples, msk144wb::level_sum_sq(w), msk144wb::level_clipped(w), e, q);
    exps[ch] = e;
    quiet[ch] = q;
    scale[c] = msk144wb::agc_scale(gains[ch], e);
}

}  // namespace

void launch_channelise(const void* raw, int format, const float2* G, const WidebandBranch* branches, const int32_t* fmod, const float2* rot, int8_t* first_halves,
                       int8_t* hops, unsigned long long* clip_count, int channels, int P, int Q, int hist, int M, int first, long long m_base,
                       const float* scale, unsigned long long* levels, hipStream_t stream, WidebandBands bands)
{
    const dim3 grid((M / Q + kTileSamples - 1) / kTileSamples, (channels + kTileChannels - 1) / kTileChannels, Q);
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, raw, G, branches, fmod, rot, first_halves, hops, clip_count, channels, P, Q, hist, M, first, m_base,
                           scale, levels, bands);
    };
    switch(format)
    {
    case 0: launch(channelise_kernel<0>); break;
    case 1: launch(channelise_kernel<1>); break;
    case 2: launch(channelise_kernel<2>); break;
    default: launch(channelise_kernel<kSubbandFormat>); break;
    }
}

void launch_agc_step(const unsigned long long* levels, const int32_t* slot_channel, const float* gains, int32_t* exps, int32_t* quiet, int32_t* used_exps, float* scale,
                     int slots, int samples, const msk144wb::AgcParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(agc_step_kernel, dim3((slots + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, levels, slot_channel, gains, exps, quiet, used_exps, scale,
                       slots, samples, p);
}

}  // namespace msk144
