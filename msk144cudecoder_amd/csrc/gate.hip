// gate: picks the channels of a push whose window is worth decoding and packs their analytic windows densely, so that scan,
// softbits, index, LDPC and collect run on `count` channels and not on all of them (msk144_set_wideband_gate, include/msk144hip.h).
// The plan kernel runs behind the ping detector and only reads its records; the gather runs behind the IQ front end, which has
// written every channel's analytic window and segment powers as without the gate.
//
//   plan    the walk of plan.h with msk144wb::gate_step as a lane's step: the ping record's up mask, the always flag and the
//           channel's `since` say whether the channel is in.  The first max_channels channels go into the list, the header gets
//           {count, total, newest hop}.
//   gather  one workgroup per list position, the grid fixed by the channels: a workgroup at or past the header's count leaves at
//           once, the others move row list[j] of the analytic store, 2592 16-byte words, to row j of the gate's own store.
#include "msk144_kernels.h"
#include "plan.h"

namespace msk144
{

namespace
{

constexpr int kGatherThreads = 256;
constexpr int kRowWords = kWindowSamples * static_cast<int>(sizeof(float2)) / 16;  // 2592
static_assert(kWindowSamples * sizeof(float2) % 16 == 0, "an analytic window is a whole number of 16-byte words");

__global__ __launch_bounds__(kPlanThreads) void gate_plan_kernel(const msk144wb::PingRecord* __restrict__ records, const uint8_t* __restrict__ always,
                                                                 int32_t* __restrict__ since, int channels, int first, int clear, msk144wb::GateParams p, int max_channels,
                                                                 long long newest, msk144wb::PlanHeader* __restrict__ header, int32_t* __restrict__ list)
{
    PlanWalk walk;
    for(int c0 = 0; c0 < channels; c0 += kPlanThreads)
    {
        const int c = c0 + static_cast<int>(threadIdx.x);
        const bool in = c < channels && msk144wb::gate_step(since[c], first != 0, clear != 0, records ? records[c].up_mask : 0ull, always[c] != 0, p.hold, p.min_up);
        const int idx = walk.place<1>(in ? 1 : 0);
        if(in && idx < max_channels) list[idx] = c;
    }
    walk.finish(header, max_channels, newest);
}

__global__ __launch_bounds__(kGatherThreads) void gate_gather_kernel(const uint4* __restrict__ analytic, const msk144wb::PlanHeader* __restrict__ header,
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
                      long long newest, msk144wb::PlanHeader* header, int32_t* list, hipStream_t stream)
{
    hipLaunchKernelGGL(gate_plan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, records, always, since, channels, first, clear, p, msk144wb::gate_max_channels(p, channels), newest,
                       header, list);
}

void launch_gate_gather(const float2* analytic, const msk144wb::PlanHeader* header, const int32_t* list, int channels, float2* packed, hipStream_t stream)
{
    hipLaunchKernelGGL(gate_gather_kernel, dim3(channels), dim3(kGatherThreads), 0, stream, reinterpret_cast<const uint4*>(analytic), header, list,
                       reinterpret_cast<uint4*>(packed));
}

}  // namespace msk144
