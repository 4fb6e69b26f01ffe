// pingband: the in-band filter ahead of the ping detector's block energies (msk144_set_wideband_ping_band, include/msk144hip.h).
//
// The filter, its LDS layout and the tail are fir64.h's.  This file's own is the ending: eight items to a block of 96 outputs, the
// squares and the block sum in 64-bit integers, summed over an item's 12 outputs in the lane and over a block's eight lanes with
// three wave shuffles - exact in any order, no atomics, the same hops give the same bytes - then the shift and the clamp to 22 bits.
#include "fir64.h"

namespace msk144
{

namespace
{

using namespace fir64;

constexpr int kBlockItems = msk144wb::kPingBlock / kItemOutputs;    // 8 lanes to a block
static_assert(msk144wb::kPingBlock % kItemOutputs == 0 && kThreads % kBlockItems == 0, "whole items to a block, whole blocks to a wave");
static_assert(kBlockItems == 8, "three shuffles sum a block");

// first_halves, hops: [channels][5184] bytes; taps[64][2]; tails[channels][128] bytes; energies[channels][54]
__global__ __launch_bounds__(kThreads) void pingband_kernel(const uint4* __restrict__ first_halves, const uint4* __restrict__ hops, int first, const int8_t* __restrict__ taps,
                                                            int shift, int restart, uint4* __restrict__ tails, int32_t* __restrict__ energies)
{
    __shared__ Lds s;
    const int tid = threadIdx.x;
    const size_t ch = blockIdx.x;
    stage(s, first_halves, hops, first, ch, taps, restart, tails);

    const int items = first ? 2 * kRowItems : kRowItems;  // nb x 8
    for(int base = 0; base < items; base += kThreads)    // the same trips in every lane: the shuffles meet whole waves
    {
        const int n = base + tid;
        uint32_t d[kWindowDwords];
        int32_t ra[kItemOutputs], rb[kItemOutputs], zi[kItemOutputs];
        item(s, n < items ? n : items - 1, d, ra, rb, zi);  // lanes past the end redo the last item and write nothing
        unsigned long long sum = 0;
#pragma unroll
        for(int o = 0; o < kItemOutputs; o++)
        {
            const long long zr = ra[o] - rb[o], zq = zi[o];
            sum += static_cast<unsigned long long>(zr * zr) + static_cast<unsigned long long>(zq * zq);
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        sum += __shfl_xor(sum, 4);
        if(n < items && (tid & (kBlockItems - 1)) == 0)
        {
            const unsigned long long e = sum >> shift;
            energies[ch * msk144wb::kPingMaxBlocks + n / kBlockItems] = e > static_cast<unsigned long long>(msk144wb::kPingBandMaxEnergy) ? msk144wb::kPingBandMaxEnergy : static_cast<int32_t>(e);
        }
    }
}

}  // namespace

void launch_pingband(const int8_t* first_halves, const int8_t* hops, int first, int channels, const int8_t* taps, int shift, int restart, uint8_t* tails, int32_t* energies,
                     hipStream_t stream)
{
    hipLaunchKernelGGL(pingband_kernel, dim3(channels), dim3(kThreads), 0, stream, reinterpret_cast<const uint4*>(first_halves), reinterpret_cast<const uint4*>(hops), first, taps,
                       shift, restart, reinterpret_cast<uint4*>(tails), energies);
}

}  // namespace msk144
