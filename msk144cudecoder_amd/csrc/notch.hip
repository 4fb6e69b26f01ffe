// notch: steady carriers taken out of a channel's staged hops, in place (msk144_set_wideband_notch, include/msk144hip.h).
//
// The filter, its LDS layout and the raw tail are fir64.h's, with one workgroup per notched channel: the grid runs over the compact
// list of the table's channels, and with an empty list there is no launch.  This file's own is the ending: x[n - 31] of every
// output is among the item's 38 window dwords, y = sat8(((x[n - 31] << s) - z + r) >> s) is formed in int32 (msk144wb::notch_out)
// and an item's 24 bytes go back over the staged row with three 8-byte stores - behind fir64::stage's barrier, as the in-place
// update needs.  The clamped components are counted per lane, summed over a wave with shuffles and over the four waves through
// LDS into one store per channel: exact in any order, no atomics, the same hops give the same bytes.
#include "fir64.h"

namespace msk144
{

namespace
{

using namespace fir64;

constexpr int kDelaySample = msk144wb::kFirTaps - msk144wb::kNotchDelay;  // x[n0 + o - 31] is sample o + 33 of the item's window
static_assert((kDelaySample + kItemOutputs - 1) / 2 < kWindowDwords, "the delayed samples lie inside the window");

// first_halves, hops: [channels][5184] bytes; list[gridDim.x]; taps[channels][64][2]; shifts[channels]; tails[channels][128] bytes
__global__ __launch_bounds__(kThreads) void notch_kernel(uint4* first_halves, uint4* hops, int first, const int32_t* __restrict__ list, const int8_t* __restrict__ all_taps,
                                                         const int32_t* __restrict__ shifts, uint4* tails, int32_t* __restrict__ clipped)
{
    __shared__ Lds s;
    __shared__ int32_t s_count[kThreads / 64];
    const int tid = threadIdx.x;
    const size_t ch = static_cast<size_t>(list[blockIdx.x]);
    const int shift = shifts[ch];
    stage(s, first_halves, hops, first, ch, all_taps + ch * (2 * msk144wb::kFirTaps), 0, tails);

    const int items = first ? 2 * kRowItems : kRowItems;
    int32_t count = 0;
    for(int base = 0; base < items; base += kThreads)
    {
        const int n = base + tid;
        uint32_t d[kWindowDwords];
        int32_t ra[kItemOutputs], rb[kItemOutputs], zi[kItemOutputs];
        item(s, n < items ? n : items - 1, d, ra, rb, zi);  // lanes past the end redo the last item and write nothing
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
        if(n < items)
        {
            count += over;
            const bool head = first && n < kRowItems;
            uint2* row = reinterpret_cast<uint2*>((head ? first_halves : hops) + ch * kRowVecs) + (first && !head ? n - kRowItems : n) * (kPairs / 2);
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
