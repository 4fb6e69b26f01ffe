// plan: the walk behind the plan kernels of the capture and the gate (capture.hip, gate.hip).  One workgroup of kPlanThreads walks
// the channels in chunks of kPlanThreads, one channel per lane: a lane finds the entries its channel has in this push, 0 .. kMax,
// place() gives it the position of the first of them among all entries in ascending channel order, and the lane stores those
// below its cap.  Within a wave the position is one ballot per possible entry and the popcounts of the lanes below; across the
// waves cross_wave_prefix (wave64.h), on two LDS rows taken in turn, so one barrier per chunk; across chunks the running base
// every lane keeps.  finish() writes the header {count, total, newest hop}.  No atomics, one order.
//
// The chunk loop stays in the kernel, so that what a lane keeps of its entries between step and store are locals of that loop.
// Handed in as functors, step and store cost capture_plan_kernel 4 KiB of LDS (the compiler moved the lane's flags there) or,
// with the entries kept by the walk, a VGPR granule more.
#pragma once

#include "wave64.h"
#include "wideband.h"

namespace msk144
{

constexpr int kPlanWaves = 4;
constexpr int kPlanThreads = kPlanWaves * 64;  // the chunk: one channel per lane

struct PlanWalk
{
    int base = 0, parity = 0;  // entries of the chunks before; the LDS row of this chunk

    // n: this lane's entries of the chunk, 0 .. kMax (0 for a lane past the last channel).  All threads call it, once per chunk.
    template<int kMax>
    __device__ __forceinline__ int place(int n)
    {
        static_assert(kMax == 1 || kMax == 2, "one ballot per possible entry of a lane");
        __shared__ int s_total[2][kPlanWaves];
        const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull;
        const unsigned long long one = __ballot(n >= 1);
        int count = __popcll(one), idx = __popcll(one & below);
        if constexpr(kMax == 2)
        {
            const unsigned long long two = __ballot(n == 2);
            count += __popcll(two);
            idx += __popcll(two & below);
        }
        int before, all;
        cross_wave_prefix<kPlanWaves>(count, s_total[parity], before, all);
        idx += base + before;
        base += all;
        parity ^= 1;
        return idx;
    }

    // behind the last chunk; cap: the most entries the kernel stores
    __device__ __forceinline__ void finish(msk144wb::PlanHeader* __restrict__ header, int cap, long long newest) const
    {
        if(threadIdx.x == 0) *header = msk144wb::PlanHeader{base < cap ? base : cap, base, newest};
    }
};

}  // namespace msk144
