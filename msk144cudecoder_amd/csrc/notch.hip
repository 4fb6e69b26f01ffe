// notch: steady carriers taken out of a channel's staged hops, in place (msk144_set_wideband_notch, include/msk144hip.h).
//
// One workgroup of four waves per notched channel: the grid runs over the compact list of the table's channels, and with an empty
// list there is no launch.  The shape is pingband.hip's.  The workgroup stages the channel's 63-sample raw tail and the push's row
// (two rows on a first push) in LDS with 16-byte loads, so that stored sample m of the push lies at byte 128 + 2m and the tail in
// bytes 2..127 in front of it (bytes 0..1, "sample -64", are zero), and packs the channel's own 64 complex int8 taps once into 33
// dwords per sum for the int8 dot product.
//
// A work item is 12 consecutive outputs y[n0] .. y[n0 + 11], n0 = 12 x item; a lane takes one item per pass (216 items of a later
// push, 432 of a first one).  A dword of the row holds two samples (I0, Q0, I1, Q1), and the window x[n - 63 .. n] of an odd n starts
// on a dword, that of an even n two bytes behind one.  So the taps are packed twice:
//
//   even n   dword j of the window that starts at sample n - 64 meets taps (64 - 2j, 63 - 2j): 33 dwords, tap 64 and tap -1 are 0;
//   odd n    the same dword - the window of n - 1 - meets taps (65 - 2j, 64 - 2j): dword 0 is all zero;
//
// and a pair of outputs (n, n + 1), n even, runs over the same 33 dwords.  The 38 dwords that an item's six pairs cover are read
// once, with 8-byte LDS loads, and stay in registers; x[n - 31] of every output is among them.  Per dword and output there are three
// dot products: Re z = sum br I - sum bi Q as two of them, with packings (br, 0) and (0, bi) - a single packing (br, -bi) cannot hold
// bi = -128, and any int8 tap is valid - and Im z as one with (bi, br).  y = sat8(((x[n - 31] << s) - z + r) >> s) is formed in
// int32 (msk144wb::notch_out) and an item's 24 bytes go back over the staged row with three 8-byte stores.  The clamped components
// are counted per lane, summed over a wave with shuffles and over the four waves through LDS into one store per channel: exact in
// any order, no atomics, the same hops give the same bytes.
//
// The update is in place.  Every global read of the rows and of the tail happens before the workgroup's barrier - the rows and the
// tail are complete in LDS behind it - and every global write, of y over the rows and of the raw tail from LDS, behind it.  This
// workgroup is the only one that touches the channel, so the in-place update needs no order between workgroups.
#include "msk144_kernels.h"

namespace msk144
{

namespace
{

constexpr int kThreads = 256;
constexpr int kRowBytes = 2 * kHopSamples;                          // 5184
constexpr int kRowVecs = kRowBytes / 16;                            // 324
constexpr int kTailBytes = 128;                                     // 2 zero bytes + 63 samples
constexpr int kTailVecs = kTailBytes / 16;
constexpr int kItemOutputs = 12;
constexpr int kPairs = kItemOutputs / 2;
constexpr int kRowItems = kHopSamples / kItemOutputs;               // 216
constexpr int kTapDwords = msk144wb::kNotchTaps / 2 + 1;            // 33
constexpr int kWindowDwords = kTapDwords + kPairs - 1;              // 38
constexpr int kDelaySample = msk144wb::kNotchTaps - msk144wb::kNotchDelay;  // x[n0 + o - 31] is sample o + 33 of the item's window
static_assert(kRowBytes % 16 == 0 && kHopSamples % kItemOutputs == 0 && kWindowDwords % 2 == 0 && (2 * kItemOutputs) % 8 == 0, "whole vectors, whole items");
static_assert(kTailBytes == 2 * (msk144wb::kNotchTail + 1), "the tail row is 64 samples, the oldest one zero");
static_assert((kDelaySample + kItemOutputs - 1) / 2 < kWindowDwords, "the delayed samples lie inside the window");

__device__ __forceinline__ int32_t dot4(uint32_t a, uint32_t b, int32_t acc)
{
#if __has_builtin(__builtin_amdgcn_sdot4)
    return __builtin_amdgcn_sdot4(static_cast<int>(a), static_cast<int>(b), acc, false);
#else
#pragma unroll
    for(int k = 0; k < 4; k++) acc += static_cast<int32_t>(static_cast<int8_t>(a >> (8 * k))) * static_cast<int32_t>(static_cast<int8_t>(b >> (8 * k)));
    return acc;
#endif
}

// first_halves, hops: [channels][5184] bytes; list[gridDim.x]; taps[channels][64][2]; shifts[channels]; tails[channels][128] bytes
__global__ __launch_bounds__(kThreads) void notch_kernel(uint4* first_halves, uint4* hops, int first, const int32_t* __restrict__ list, const int8_t* __restrict__ all_taps,
                                                         const int32_t* __restrict__ shifts, uint4* tails, int32_t* __restrict__ clipped)
{
    __shared__ uint4 s_x[kTailVecs + 2 * kRowVecs];
    __shared__ uint4 s_t[kTapDwords][2];  // even n: (br, 0), (0, bi), (bi, br); odd n: the same three; two dwords unused
    __shared__ int32_t s_count[kThreads / 64];
    const int tid = threadIdx.x;
    const size_t ch = static_cast<size_t>(list[blockIdx.x]);
    const int nvec = first ? 2 * kRowVecs : kRowVecs;
    const int8_t* taps = all_taps + ch * (2 * msk144wb::kNotchTaps);
    const int shift = shifts[ch];

    if(tid < kTailVecs) s_x[tid] = tails[ch * kTailVecs + tid];
    for(int i = tid; i < nvec; i += kThreads)
    {
        const bool head = first && i < kRowVecs;
        s_x[kTailVecs + i] = (head ? first_halves : hops)[ch * kRowVecs + (first && !head ? i - kRowVecs : i)];
    }
    if(tid < kTapDwords)
    {
        // tap k as unsigned bytes, zero outside 0..63
        auto re = [&](int k) -> uint32_t { return k >= 0 && k < msk144wb::kNotchTaps ? static_cast<uint8_t>(taps[2 * k]) : 0u; };
        auto im = [&](int k) -> uint32_t { return k >= 0 && k < msk144wb::kNotchTaps ? static_cast<uint8_t>(taps[2 * k + 1]) : 0u; };
        const int e1 = 64 - 2 * tid, e2 = e1 - 1, o1 = e1 + 1, o2 = e1;
        uint4 a, b;
        a.x = re(e1) | (re(e2) << 16);
        a.y = (im(e1) << 8) | (im(e2) << 24);
        a.z = im(e1) | (re(e1) << 8) | (im(e2) << 16) | (re(e2) << 24);
        a.w = re(o1) | (re(o2) << 16);
        b.x = (im(o1) << 8) | (im(o2) << 24);
        b.y = im(o1) | (re(o1) << 8) | (im(o2) << 16) | (re(o2) << 24);
        b.z = b.w = 0;
        s_t[tid][0] = a;
        s_t[tid][1] = b;
    }
    __syncthreads();

    // the last 63 raw samples of the push, as the next push finds them
    if(tid < kTailVecs)
    {
        uint4 v = s_x[nvec + tid];
        if(tid == 0) v.x &= 0xffff0000u;
        tails[ch * kTailVecs + tid] = v;
    }

    const uint2* xw = reinterpret_cast<const uint2*>(s_x);
    const int items = first ? 2 * kRowItems : kRowItems;
    int32_t count = 0;
    for(int base = 0; base < items; base += kThreads)
    {
        const int item = base + tid;
        const int it = item < items ? item : items - 1;  // lanes past the end redo the last item and write nothing
        // the item's window starts at sample 12 it - 64: byte 24 it, dwords 6 it .. 6 it + 37 (the last one of the last item ends the row)
        uint32_t d[kWindowDwords];
#pragma unroll
        for(int i = 0; i < kWindowDwords / 2; i++)
        {
            const uint2 v = xw[it * (kPairs / 2) + i];
            d[2 * i] = v.x;
            d[2 * i + 1] = v.y;
        }
        int32_t ra[kItemOutputs] = {}, rb[kItemOutputs] = {}, zi[kItemOutputs] = {};
#pragma unroll
        for(int j = 0; j < kTapDwords; j++)
        {
            const uint4 t0 = s_t[j][0], t1 = s_t[j][1];
#pragma unroll
            for(int p = 0; p < kPairs; p++)
            {
                const uint32_t x = d[j + p];
                ra[2 * p] = dot4(t0.x, x, ra[2 * p]);
                rb[2 * p] = dot4(t0.y, x, rb[2 * p]);
                zi[2 * p] = dot4(t0.z, x, zi[2 * p]);
                ra[2 * p + 1] = dot4(t0.w, x, ra[2 * p + 1]);
                rb[2 * p + 1] = dot4(t1.x, x, rb[2 * p + 1]);
                zi[2 * p + 1] = dot4(t1.y, x, zi[2 * p + 1]);
            }
        }
        uint32_t y[kPairs] = {};
        int32_t over = 0;
#pragma unroll
        for(int o = 0; o < kItemOutputs; o++)
        {
            const uint32_t x = d[(kDelaySample + o) / 2] >> (16 * ((kDelaySample + o) & 1));
            const int32_t vr = msk144wb::notch_out(static_cast<int8_t>(x), ra[o] - rb[o], shift);
            const int32_t vq = msk144wb::notch_out(static_cast<int8_t>(x >> 8), zi[o], shift);
            const int32_t yr = msk144wb::notch_sat8(vr), yq = msk144wb::notch_sat8(vq);
            over += (yr != vr) + (yq != vq);
            y[o / 2] |= ((static_cast<uint32_t>(yr) & 0xffu) | ((static_cast<uint32_t>(yq) & 0xffu) << 8)) << (16 * (o & 1));
        }
        if(item < items)
        {
            count += over;
            const bool head = first && item < kRowItems;
            uint2* row = reinterpret_cast<uint2*>((head ? first_halves : hops) + ch * kRowVecs) + (first && !head ? item - kRowItems : item) * (kPairs / 2);
#pragma unroll
            for(int i = 0; i < kPairs / 2; i++) row[i] = uint2{y[2 * i], y[2 * i + 1]};
        }
    }
#pragma unroll
    for(int m = 1; m < 64; m <<= 1) count += __shfl_xor(count, m);
    if((tid & 63) == 0) s_count[tid >> 6] = count;
    __syncthreads();
    if(tid == 0) clipped[ch] = s_count[0] + s_count[1] + s_count[2] + s_count[3];
}

}  // namespace

void launch_notch(int8_t* first_halves, int8_t* hops, int first, const int32_t* list, int count, const int8_t* taps, const int32_t* shifts, uint8_t* tails, int32_t* clipped,
                  hipStream_t stream)
{
    hipLaunchKernelGGL(notch_kernel, dim3(count), dim3(kThreads), 0, stream, reinterpret_cast<uint4*>(first_halves), reinterpret_cast<uint4*>(hops), first, list, taps, shifts,
                       reinterpret_cast<uint4*>(tails), clipped);
}

}  // namespace msk144
