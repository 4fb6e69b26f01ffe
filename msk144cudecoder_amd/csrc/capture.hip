// capture: picks the (channel, hop) pairs of a push that are worth keeping and packs their int8 I/Q densely, so that the host
// reads a 16-byte header when the band is quiet and 5184 bytes per kept hop when it is not (msk144_set_wideband_capture,
// include/msk144hip.h).  Both kernels run behind the hop ring kernel: ring[c] then holds the hop before the newest in its first
// 5184 bytes and the newest in its second (hops 0 and 1 after a first push), so every unit is one half of a ring window.
//
//   plan   the walk of plan.h with msk144wb::capture_step as a lane's step: the ping record's up mask, the list flag and the
//          channel's state give 0, 1 or 2 units.  The first max_units units get a descriptor, the header gets {count, total,
//          newest hop}.
//   copy   one wave per unit slot, the grid fixed by max_units: a wave at or past the header's count leaves at once, the others move
//          their unit's 324 16-byte words from the ring window to row u of the dense buffer.
#include "msk144_kernels.h"
#include "plan.h"

namespace msk144
{

namespace
{

constexpr int kCopyWaves = 4;
constexpr int kUnitWords = msk144wb::kCaptureUnitBytes / 16;  // 324
static_assert(2 * kHopSamples == msk144wb::kCaptureUnitBytes && 2 * kWindowSamples == 2 * msk144wb::kCaptureUnitBytes, "a unit is a hop of int8 I/Q: half a ring window");

__global__ __launch_bounds__(kPlanThreads) void capture_plan_kernel(const msk144wb::PingRecord* __restrict__ records, const uint8_t* __restrict__ listed,
                                                                    msk144wb::CaptureState* __restrict__ state, int channels, int first, int clear,
                                                                    msk144wb::CaptureParams p, long long newest, msk144wb::PlanHeader* __restrict__ header,
                                                                    msk144wb::CaptureUnit* __restrict__ units)
{
    PlanWalk walk;
    for(int c0 = 0; c0 < channels; c0 += kPlanThreads)
    {
        const int c = c0 + static_cast<int>(threadIdx.x);
        int32_t flags[2] = {0, 0}, half[2] = {0, 0};
        const int n = c < channels ? msk144wb::capture_step(state[c], first != 0, clear != 0, records ? records[c].up_mask : 0ull, listed[c] != 0, p.pre, p.post, flags, half) : 0;
        const int idx = walk.place<2>(n);
        for(int i = 0; i < n; i++)
            if(idx + i < p.max_units) units[idx + i] = msk144wb::CaptureUnit{c, flags[i], newest - 1 + half[i]};
    }
    walk.finish(header, p.max_units, newest);
}

__global__ __launch_bounds__(kCopyWaves * 64) void capture_copy_kernel(const uint4* __restrict__ ring, const msk144wb::PlanHeader* __restrict__ header,
                                                                       const msk144wb::CaptureUnit* __restrict__ units, int max_units, uint4* __restrict__ data)
{
    const int lane = threadIdx.x & 63;
    const int u = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * kCopyWaves + threadIdx.x / 64));
    if(u >= max_units || u >= header->count) return;  // whole waves leave
    const msk144wb::CaptureUnit x = units[u];
    const int half = static_cast<int>(x.hop - (header->hop - 1));  // 0 or 1, as the plan kernel wrote it
    const uint4* __restrict__ src = ring + (static_cast<size_t>(x.channel) * 2 + static_cast<size_t>(half)) * kUnitWords;
    uint4* __restrict__ dst = data + static_cast<size_t>(u) * kUnitWords;
    for(int i = lane; i < kUnitWords; i += 64) dst[i] = src[i];
}

}  // namespace

void launch_capture(const void* ring, const msk144wb::PingRecord* records, const uint8_t* listed, msk144wb::CaptureState* state, int channels, int first, int clear,
                    const msk144wb::CaptureParams& p, long long newest, msk144wb::PlanHeader* header, msk144wb::CaptureUnit* units, void* data, hipStream_t stream)
{
    hipLaunchKernelGGL(capture_plan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, records, listed, state, channels, first, clear, p, newest, header, units);
    hipLaunchKernelGGL(capture_copy_kernel, dim3((p.max_units + kCopyWaves - 1) / kCopyWaves), dim3(kCopyWaves * 64), 0, stream, static_cast<const uint4*>(ring), header, units,
                       p.max_units, static_cast<uint4*>(data));
}

}  // namespace msk144
