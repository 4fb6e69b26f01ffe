// pings: per-channel ping detection on the staged hops of a push (msk144_set_wideband_pings, include/msk144hip.h).
//
// One wave per channel, kWaves waves per workgroup.  Lane b < nb (nb = 27, or 54 after a first push) owns block b of the channel's
// push: it reads its 96 int8 I/Q pairs with twelve 16-byte loads and sums I^2 + Q^2 in int32 with the int8 dot product.  The rest
// stays in registers and in wave-uniform values:
//
//   quiet level   an MSB-first radix select over the 22 bits of E: per bit one ballot of the candidates whose bit is 0 and one
//                 popcount decide whether the rank lies among them - 22 steps whatever nb is, no LDS and no sorted copy;
//   reference     msk144wb::ping_history_min / ping_reference on the channel's history (every lane reads the same words);
//   up mask       one ballot of msk144wb::ping_up;
//   peak          one wave max (wave64.h) of (E << 6) | (63 - b): the largest E, and the lowest b that has it.
//
// With the ping band on (msk144_set_wideband_ping_band) pingband.hip has left the in-band energies Ef of the push in the debug array,
// and the second instantiation of the kernel takes its E from there instead of the hops; everything behind that is the same code.
//
// Lane 0 then moves the history (msk144wb::ping_history_put) and writes the record; every lane writes its E (0 past nb) to the
// channel's row of the debug array.  No atomics and no order between waves: the same hops give the same bytes.
//
// The scale a push was quantised with is formed as msk144_wideband_levels reports it, ldexpf(gains[ch], used_exps[ch]) (exponent
// 0 without the AGC), from the per-channel arrays: the hop rows, the records and these are all indexed by channel, so the padded
// slots of a bank rate do not enter here.
#include "msk144_kernels.h"
#include "wave64.h"

namespace msk144
{

namespace
{

constexpr int kWaves = 4;
constexpr int kBlockBytes = 2 * msk144wb::kPingBlock;        // 192: a multiple of 16, as the 5184-byte rows are
constexpr int kRowBytes = 2 * kHopSamples;
using msk144wb::kHopBlocks;
static_assert(kHopSamples == kHopBlocks * msk144wb::kPingBlock && 2 * kHopBlocks == msk144wb::kPingMaxBlocks, "a hop is 27 whole blocks");
static_assert(kBlockBytes % 16 == 0 && kRowBytes % 16 == 0, "16-byte loads");
static_assert(msk144wb::kPingEnergyBits + 6 <= 28, "the peak key keeps clear of the exponent bits that bias it");

// first_halves, hops: [channels][5184] bytes, the hop ring's staging; records[channels]; energies[channels][54]; state[channels].
// kBand: the energies of the push are already in `energies` (pingband.hip wrote the in-band Ef there, ahead on the same stream) and
// the hops are not read; every other step is the same code.
template<bool kBand>
__global__ __launch_bounds__(kWaves * 64) void pings_kernel(const int8_t* __restrict__ first_halves, const int8_t* __restrict__ hops, int first, int channels,
                                                            const float* __restrict__ gains, const int32_t* __restrict__ used_exps, msk144wb::PingParams p, int restart,
                                                            msk144wb::PingHistory* __restrict__ state, msk144wb::PingRecord* __restrict__ records,
                                                            int32_t* __restrict__ energies)
{
    const int lane = threadIdx.x & 63;
    const int ch = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * kWaves + threadIdx.x / 64));
    if(ch >= channels) return;  // whole waves leave
    const int nb = first ? 2 * kHopBlocks : kHopBlocks;

    int32_t E = 0;
    if constexpr(kBand)
    {
        if(lane < nb) E = energies[static_cast<size_t>(ch) * msk144wb::kPingMaxBlocks + lane];
    }
    else if(lane < nb)
    {
        const bool head = first && lane < kHopBlocks;
        const int8_t* row = (head ? first_halves : hops) + static_cast<size_t>(ch) * kRowBytes;
        const uint4* src = reinterpret_cast<const uint4*>(row + (first && !head ? lane - kHopBlocks : lane) * kBlockBytes);
#pragma unroll
        for(int j = 0; j < kBlockBytes / 16; j++)
        {
            const uint4 v = src[j];
            E = dot4(v.x, v.x, E);
            E = dot4(v.y, v.y, E);
            E = dot4(v.z, v.z, E);
            E = dot4(v.w, v.w, E);
        }
    }

    // ---- the value at rank nb/4 of the nb energies: MSB first, the candidates narrowed by one bit per step ----
    unsigned long long cand = (1ull << nb) - 1;
    int rank = msk144wb::ping_rank(nb);
    int32_t q = 0;
#pragma unroll
    for(int bit = msk144wb::kPingEnergyBits - 1; bit >= 0; bit--)
    {
        const unsigned long long zero = cand & __ballot(((E >> bit) & 1) == 0);
        const int n0 = __popcll(zero);
        if(rank < n0) cand = zero;
        else
        {
            rank -= n0;
            cand &= ~zero;
            q |= 1 << bit;
        }
    }

    // ---- reference, up mask, peak ----
    const float scale = ldexpf(gains[ch], used_exps ? used_exps[ch] : 0);
    msk144wb::PingHistory& s = state[ch];
    int32_t h = 0;
    const int32_t R = msk144wb::ping_reference(msk144wb::ping_history_min(s, restart != 0, scale, p.memory, q, h), p.min_ref);
    const unsigned long long up = __ballot(lane < nb && msk144wb::ping_up(E, R, p.ratio_q4));
    // positive floats order as their bit patterns do; bit 30 makes every key a normal number
    const uint32_t key = lane < nb ? (static_cast<uint32_t>(E) << 6) | static_cast<uint32_t>(63 - lane) : 0u;
    const uint32_t top = __builtin_bit_cast(uint32_t, wave_max_f32(__builtin_bit_cast(float, key | 0x40000000u))) & 0x0fffffffu;

    if(lane < msk144wb::kPingMaxBlocks) energies[static_cast<size_t>(ch) * msk144wb::kPingMaxBlocks + lane] = E;
    if(lane == 0)
    {
        msk144wb::ping_history_put(s, restart != 0, scale, q);
        msk144wb::PingRecord r;
        r.up_mask = up;
        r.blocks = nb;
        r.history = h;
        r.quiet = q;
        r.reference = R;
        r.peak = static_cast<int32_t>(top >> 6);
        r.peak_block = 63 - static_cast<int32_t>(top & 63);
        records[ch] = r;
    }
}

}  // namespace

void launch_pings(const int8_t* first_halves, const int8_t* hops, int first, int channels, const float* gains, const int32_t* used_exps, const msk144wb::PingParams& p,
                  int restart, msk144wb::PingHistory* state, msk144wb::PingRecord* records, int32_t* energies, bool band, hipStream_t stream)
{
    hipLaunchKernelGGL(band ? pings_kernel<true> : pings_kernel<false>, dim3((channels + kWaves - 1) / kWaves), dim3(kWaves * 64), 0, stream, first_halves, hops, first, channels, gains, used_exps, p, restart,
                       state, records, energies);
}

}  // namespace msk144
