// stream_gate: picks the listed positions of a push of audio hops whose window is worth decoding (msk144_set_stream_gate,
// include/msk144hip.h; the rule is csrc/stream_gate.h, which takes it from csrc/wideband.h).  Both kernels run behind the
// stream-pings kernel and only read what it left; the gather behind the front end is gate.hip's, launched with the push's n.
//
//   mask    only when the gate has a ratio of its own.  One wave per listed position j, kMaskWaves waves per workgroup; a whole
//           wave leaves when j is past n.  Lane b reads energies[j][b]; one ballot of msk144wb::ping_up against the record's
//           reference, over the lanes below the record's block count, is masks[j].  No LDS, no atomics.
//   plan    the walk of plan.h, one position per lane: stream s = streams[j], the mask (the gate's own, the record's, or 0 while
//           the detector is off), always[s] and since[s] go through msk144wb::gate_step, which moves since[s].  The first `cap`
//           positions that are in go into the list, the header gets {count, total, hop}.  A push lists a stream once, so no two
//           lanes share a `since`: no atomics, and the same hops give the same bytes.
#include "msk144_kernels.h"
#include "plan.h"

namespace msk144
{

namespace
{

constexpr int kMaskWaves = 4;
static_assert(msk144sg::kMaxBlocks <= 64, "one lane per block of a position");

// records[n], energies[n][54] by position, as the stream-pings kernel left them; masks[n]
__global__ __launch_bounds__(kMaskWaves * 64) void stream_gate_mask_kernel(const msk144wb::PingRecord* __restrict__ records, const int32_t* __restrict__ energies, int n, int ratio_q4,
                                                                          unsigned long long* __restrict__ masks)
{
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * kMaskWaves + threadIdx.x / 64));
    if(j >= n) return;  // whole waves leave
    const int nb = __builtin_amdgcn_readfirstlane(records[j].blocks);
    const int32_t R = __builtin_amdgcn_readfirstlane(records[j].reference);
    const int32_t E = lane < msk144sg::kMaxBlocks ? energies[static_cast<size_t>(j) * msk144sg::kMaxBlocks + lane] : 0;
    const unsigned long long up = __ballot(lane < nb && lane < msk144sg::kMaxBlocks && msk144wb::ping_up(E, R, ratio_q4));
    if(lane == 0) masks[j] = up;
}

// streams[n], is_first[n], restart[n] by position; records[n] or nullptr (the detector is off); masks[n] or nullptr (no ratio of
// the gate's own); always[channels], since[channels] by stream; list[cap]
__global__ __launch_bounds__(kPlanThreads) void stream_gate_plan_kernel(const int32_t* __restrict__ streams, const uint8_t* __restrict__ is_first, const uint8_t* __restrict__ restart,
                                                                        const msk144wb::PingRecord* __restrict__ records, const unsigned long long* __restrict__ masks,
                                                                        const uint8_t* __restrict__ always, int32_t* __restrict__ since, int n, int hold, int min_up, int cap,
                                                                        long long hop, msk144wb::PlanHeader* __restrict__ header, int32_t* __restrict__ list)
{
    PlanWalk walk;
    for(int j0 = 0; j0 < n; j0 += kPlanThreads)
    {
        const int j = j0 + static_cast<int>(threadIdx.x);
        bool in = false;
        if(j < n)
        {
            const int s = streams[j];
            const bool first = is_first[j] != 0;
            const uint64_t mask = masks ? masks[j] : records ? records[j].up_mask : 0ull;
            in = msk144wb::gate_step(since[s], first, first || restart[j] != 0, mask, always[s] != 0, hold, min_up);
        }
        const int idx = walk.place<1>(in ? 1 : 0);
        if(in && idx < cap) list[idx] = j;
    }
    walk.finish(header, cap, hop);
}

}  // namespace

void launch_stream_gate_mask(const msk144wb::PingRecord* records, const int32_t* energies, int n, int ratio_q4, unsigned long long* masks, hipStream_t stream)
{
    hipLaunchKernelGGL(stream_gate_mask_kernel, dim3((n + kMaskWaves - 1) / kMaskWaves), dim3(kMaskWaves * 64), 0, stream, records, energies, n, ratio_q4, masks);
}

void launch_stream_gate_plan(const int32_t* streams, const uint8_t* is_first, const uint8_t* restart, const msk144wb::PingRecord* records, const unsigned long long* masks,
                             const uint8_t* always, int32_t* since, int n, const msk144sg::Params& p, int cap, long long hop, msk144wb::PlanHeader* header, int32_t* list,
                             hipStream_t stream)
{
    hipLaunchKernelGGL(stream_gate_plan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, streams, is_first, restart, records, masks, always, since, n, p.hold, p.min_up, cap, hop, header,
                       list);
}

}  // namespace msk144
