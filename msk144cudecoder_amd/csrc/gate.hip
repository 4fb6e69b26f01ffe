// gate: picks the channels of a push whose window is worth decoding and packs their analytic windows densely, so that scan,
// softbits, index, LDPC and collect run on `count` channels and not on all of them (msk144_set_wideband_gate, include/msk144hip.h).
// The plan kernel runs behind the ping detector and only reads its records; the gather runs behind the IQ front end, which has
// written every channel's analytic window and segment powers as without the gate.
//
//   plan    one workgroup walks the channels in chunks of kPlanThreads, one channel per lane.  A lane applies msk144wb::gate_step to
//           its channel - the ping record's up mask, the always flag, the channel's `since` - and is in or out.  The exclusive prefix
//           in ascending channel order: within a wave one ballot and the popcount of the lanes below; across the waves their totals
//           through LDS; across chunks a running base every lane keeps.  The first max_channels channels go into the list, the
//           header gets {count, total, newest hop}.  No atomics, one order.
//   gather  one workgroup per list position, the grid fixed by the channels: a workgroup at or past the header's count leaves at
//           once, the others move row list[j] of the analytic store, 2592 16-byte words, to row j of the gate's own store.
#include "msk144_kernels.h"

namespace msk144
{

namespace
{

constexpr int kPlanWaves = 4;
constexpr int kPlanThreads = kPlanWaves * 64;  // the chunk: one channel per lane
constexpr int kGatherThreads = 256;
constexpr int kRowWords = kWindowSamples * static_cast<int>(sizeof(float2)) / 16;  // 2592
static_assert(kWindowSamples * sizeof(float2) % 16 == 0, "an analytic window is a whole number of 16-byte words");

__global__ __launch_bounds__(kPlanThreads) void gate_plan_kernel(const msk144wb::PingRecord* __restrict__ records, const uint8_t* __restrict__ always,
                                                                 int32_t* __restrict__ since, int channels, int first, int clear, msk144wb::GateParams p, int max_channels,
                                                                 long long newest, msk144wb::GateHeader* __restrict__ header, int32_t* __restrict__ list)
{
    __shared__ int s_total[2][kPlanWaves];  // by chunk parity: a wave writes a chunk's total only after every wave has read the one two before
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0;
    for(int c0 = 0, parity = 0; c0 < channels; c0 += kPlanThreads, parity ^= 1)
    {
        const int c = c0 + static_cast<int>(threadIdx.x);
        bool in = false;
        if(c < channels)
        {
            int32_t s = since[c];
            in = msk144wb::gate_step(s, first != 0, clear != 0, records ? records[c].up_mask : 0ull, always[c] != 0, p.hold, p.min_up);
            since[c] = s;
        }
        const unsigned long long mask = __ballot(in);
        if(lane == 0) s_total[parity][wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for(int w = 0; w < kPlanWaves; w++)
        {
            const int t = s_total[parity][w];
            all += t;
            before += w < wave ? t : 0;
        }
        const int idx = base + before + __popcll(mask & below);
        if(in && idx < max_channels) list[idx] = c;
        base += all;
    }
    if(threadIdx.x == 0) *header = msk144wb::GateHeader{base < max_channels ? base : max_channels, base, newest};
}

__global__ __launch_bounds__(kGatherThreads) void gate_gather_kernel(const uint4* __restrict__ analytic, const msk144wb::GateHeader* __restrict__ header,
                                                                     const int32_t* __restrict__ list, uint4* __restrict__ packed)
{
    const int j = static_cast<int>(blockIdx.x);
    if(j >= header->count) return;  // the whole workgroup leaves
    const uint4* __restrict__ src = analytic + static_cast<size_t>(list[j]) * kRowWords;
    uint4* __restrict__ dst = packed + static_cast<size_t>(j) * kRowWords;
    for(int i = static_cast<int>(threadIdx.x); i < kRowWords; i += kGatherThreads) dst[i] = src[i];
}

}  // namespace

void launch_gate_plan(const msk144wb::PingRecord* records, const uint8_t* always, int32_t* since, int channels, int first, int clear, const msk144wb::GateParams& p,
                      long long newest, msk144wb::GateHeader* header, int32_t* list, hipStream_t stream)
{
    hipLaunchKernelGGL(gate_plan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, records, always, since, channels, first, clear, p, msk144wb::gate_max_channels(p, channels), newest,
                       header, list);
}

void launch_gate_gather(const float2* analytic, const msk144wb::GateHeader* header, const int32_t* list, int channels, float2* packed, hipStream_t stream)
{
    hipLaunchKernelGGL(gate_gather_kernel, dim3(channels), dim3(kGatherThreads), 0, stream, reinterpret_cast<const uint4*>(analytic), header, list,
                       reinterpret_cast<uint4*>(packed));
}

}  // namespace msk144
