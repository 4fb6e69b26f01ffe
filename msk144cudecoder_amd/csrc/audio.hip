// audio: every channel's stored int8 hops as real 12 kHz int16 audio (msk144_set_wideband_audio, include/msk144hip.h), and the audio
// of the capture's units packed densely beside their I/Q (msk144_wideband_capture_audio).  Both kernels run behind the hop ring
// kernel: ring[c] then holds the hop before the newest in its first 5184 bytes and the newest in its second.
//
//   audio  the filter, its LDS layout and the tail are fir64.h's, read from the ring's windows (row stride 648 words).  This file's
//          own is the ending: y = clamp((Re z pr - Im z pi + 2^(shift - 1)) >> shift) in int64 (msk144wb::audio_out) with the
//          96-entry phasor table in LDS - an item's 12 outputs start at entry 12 (item mod 8) - and an item's 12 int16 go to byte
//          24 x item of the hop's row as three 8-byte stores, so that a wave writes one contiguous run.  The audio of hop k lies in
//          row k & 1 of the channel.  The clamped samples are counted per lane and hop, summed over a wave with shuffles and over
//          the four waves through LDS into one store per hop: exact in any order, no atomics, the same hops give the same bytes.
//   copy   capture.hip's copy again, one wave per unit slot: a wave at or past the header's count leaves at once, the others move
//          row (channel, hop & 1) of the audio, 324 16-byte words, to row u of the dense buffer, and its clamp count to clamped[u].
#include "fir64.h"

namespace msk144
{

namespace
{

using namespace fir64;

constexpr int kItemWords = 2 * kItemOutputs / 8;                   // an item's int16 outputs as 8-byte words: 3
constexpr int kAudioRowWords = kRowItems * kItemWords;             // 648: a hop of int16
constexpr int kTableItems = msk144wb::kAudioPhasors / kItemOutputs;  // the table's turn, in items: 8
constexpr int kCopyWaves = 4;
constexpr int kUnitVecs = 2 * msk144wb::kAudioHopSamples / 16;     // 324
static_assert(kHopSamples == msk144wb::kAudioHopSamples && kRowItems % kTableItems == 0 && msk144wb::kAudioPhasors % kItemOutputs == 0,
              "a hop is whole turns of the table, a turn whole items");
static_assert(kItemWords * 8 == 2 * kItemOutputs && kAudioRowWords * 8 == 2 * kHopSamples && kUnitVecs * 16 == 2 * kHopSamples, "whole words");
static_assert(msk144wb::kAudioPhasors <= kThreads, "one lane per table entry");

// ring[channels][2][5184] bytes; taps[64][2]; phasor[96]; tails[channels][128] bytes; audio[channels][2][2592] int16; clamped[channels][2]
__global__ __launch_bounds__(kThreads) void audio_kernel(const uint4* __restrict__ ring, int both, int newest_row, const int8_t* __restrict__ taps,
                                                         const short2* __restrict__ phasor, int shift, uint4* __restrict__ tails, uint2* __restrict__ audio,
                                                         int32_t* __restrict__ clamped)
{
    __shared__ Lds s;
    __shared__ short2 s_w[msk144wb::kAudioPhasors];
    __shared__ int32_t s_count[2][kThreads / 64];
    const int tid = threadIdx.x;
    const size_t ch = blockIdx.x;
    if(tid < msk144wb::kAudioPhasors) s_w[tid] = phasor[tid];  // complete behind stage's barrier
    stage(s, ring, ring + kRowVecs, both, ch, taps, both, tails, 2 * kRowVecs);

    const int items = both ? 2 * kRowItems : kRowItems;
    int32_t older = 0, newest = 0;
    for(int base = 0; base < items; base += kThreads)
    {
        const int n = base + tid, it = n < items ? n : items - 1;  // lanes past the end redo the last item and write nothing
        uint32_t d[kWindowDwords];
        int32_t ra[kItemOutputs], rb[kItemOutputs], zi[kItemOutputs];
        item(s, it, d, ra, rb, zi);
        const short2* w = s_w + (it % kTableItems) * kItemOutputs;
        uint32_t y[kPairs] = {};
        int32_t over = 0;
#pragma unroll
        for(int o = 0; o < kItemOutputs; o++)
        {
            const short2 p = w[o];
            const int32_t v = msk144wb::audio_out(ra[o] - rb[o], zi[o], p.x, p.y, shift, over);
            y[o / 2] |= (static_cast<uint32_t>(v) & 0xffffu) << (16 * (o & 1));
        }
        if(n < items)
        {
            const bool head = both && n < kRowItems;  // the hop before the newest
            if(head) older += over;
            else newest += over;
            uint2* row = audio + (ch * 2 + static_cast<size_t>(head ? newest_row ^ 1 : newest_row)) * kAudioRowWords + (both && !head ? n - kRowItems : n) * kItemWords;
#pragma unroll
            for(int i = 0; i < kItemWords; i++) row[i] = uint2{y[2 * i], y[2 * i + 1]};
        }
    }
#pragma unroll
    for(int m = 1; m < 64; m <<= 1)
    {
        older += __shfl_xor(older, m);
        newest += __shfl_xor(newest, m);
    }
    if((tid & 63) == 0)
    {
        s_count[0][tid >> 6] = older;
        s_count[1][tid >> 6] = newest;
    }
    __syncthreads();
    if(tid == 0)
    {
        clamped[ch * 2 + static_cast<size_t>(newest_row)] = s_count[1][0] + s_count[1][1] + s_count[1][2] + s_count[1][3];
        if(both) clamped[ch * 2 + static_cast<size_t>(newest_row ^ 1)] = s_count[0][0] + s_count[0][1] + s_count[0][2] + s_count[0][3];
    }
}

__global__ __launch_bounds__(kCopyWaves * 64) void audio_copy_kernel(const uint4* __restrict__ audio, const int32_t* __restrict__ clamped,
                                                                     const msk144wb::PlanHeader* __restrict__ header, const msk144wb::CaptureUnit* __restrict__ units,
                                                                     int max_units, uint4* __restrict__ rows, int32_t* __restrict__ row_clamped)
{
    const int lane = threadIdx.x & 63;
    const int u = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * kCopyWaves + threadIdx.x / 64));
    if(u >= max_units || u >= header->count) return;  // whole waves leave
    const msk144wb::CaptureUnit x = units[u];
    const size_t r = static_cast<size_t>(x.channel) * 2 + static_cast<size_t>(x.hop & 1);
    const uint4* __restrict__ src = audio + r * kUnitVecs;
    uint4* __restrict__ dst = rows + static_cast<size_t>(u) * kUnitVecs;
    for(int i = lane; i < kUnitVecs; i += 64) dst[i] = src[i];
    if(lane == 0) row_clamped[u] = clamped[r];
}

}  // namespace

void launch_audio(const void* ring, int channels, int both, long long newest, const int8_t* taps, const int16_t* phasor, int shift, uint8_t* tails, int16_t* audio,
                  int32_t* clamped, hipStream_t stream)
{
    hipLaunchKernelGGL(audio_kernel, dim3(channels), dim3(kThreads), 0, stream, static_cast<const uint4*>(ring), both, static_cast<int>(newest & 1), taps,
                       reinterpret_cast<const short2*>(phasor), shift, reinterpret_cast<uint4*>(tails), reinterpret_cast<uint2*>(audio), clamped);
}

void launch_audio_copy(const int16_t* audio, const int32_t* clamped, const msk144wb::PlanHeader* header, const msk144wb::CaptureUnit* units, int max_units, int16_t* rows,
                       int32_t* row_clamped, hipStream_t stream)
{
    hipLaunchKernelGGL(audio_copy_kernel, dim3((max_units + kCopyWaves - 1) / kCopyWaves), dim3(kCopyWaves * 64), 0, stream, reinterpret_cast<const uint4*>(audio), clamped, header,
                       units, max_units, reinterpret_cast<uint4*>(rows), row_clamped);
}

}  // namespace msk144
