// stream_pings: per-stream levels and ping detection on the staged audio hops of a push (msk144_set_stream_pings,
// include/msk144hip.h; the arithmetic is csrc/stream_pings.h, the rule csrc/wideband.h).
//
// One wave per listed position j, kWaves waves per workgroup; a whole wave leaves when j is past n.  The stream s = streams[j] and
// the restart flag is_first[j] | restart[j] are wave-uniform.  Lane b < nb (nb = 27, or 54 on the stream's first hop) owns block b:
// it reads its 96 int16 samples with twelve 16-byte loads - lanes 0..26 of a first hop from first_halves[j], lanes 27..53 from
// hops[j] - and keeps, per dword of two samples, the unsigned sum of the two squares (at most 2^31: it fits a dword where a block
// does not) added into a 64-bit block sum, the plain sum, the largest magnitude and the full-scale count.
//
// Behind that it is pings.hip's code on E = min(2^22 - 1, block sum >> shift): the 22-step ballot radix select for the quiet level,
// msk144wb::ping_history_min / ping_reference on state[s] with the scale fixed at 1.0f, one ballot for the up mask, one wave max of
// (E << 6) | (63 - b) for the peak and its lowest block.  The levels come from the same registers: integer butterfly sums over the
// wave, a butterfly max, and the popcount of one ballot for the saturated blocks.
//
// Lane 0 moves state[s] and writes records[j] and levels[j]; every lane below 54 writes its E (0 past nb) to energies[j].  A push lists
// a stream once, so no two waves share a state; no atomics and no order between waves: the same hops give the same bytes.
#include "msk144_kernels.h"
#include "wave64.h"

namespace msk144
{

namespace
{

constexpr int kWaves = 4;
constexpr int kBlockBytes = 2 * msk144sp::kBlock;   // 192: a multiple of 16, as the 5184-byte rows are
constexpr int kRowBytes = 2 * kHopSamples;
static_assert(kHopSamples == msk144sp::kHopSamples && kBlockBytes % 16 == 0 && kRowBytes % 16 == 0 && kRowBytes == msk144sp::kHopBlocks * kBlockBytes, "a row is 27 whole blocks of 16-byte loads");
static_assert(msk144wb::kPingEnergyBits + 6 <= 28, "the peak key keeps clear of the exponent bits that bias it");

// sum and max over the 64 lanes, the same value in every lane
template<typename T>
__device__ __forceinline__ T wave_sum_int(T v)
{
#pragma unroll
    for(int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ int32_t wave_max_i32(int32_t v)
{
#pragma unroll
    for(int m = 1; m < 64; m <<= 1)
    {
        const int32_t o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

// two int16 samples of a dword into the lane's sums
__device__ __forceinline__ void take(uint32_t w, uint64_t& sq, int32_t& sum, int32_t& peak, int32_t& full)
{
    const int32_t a = static_cast<int16_t>(w & 0xffffu), b = static_cast<int16_t>(w >> 16);
    sq += static_cast<uint32_t>(a * a) + static_cast<uint32_t>(b * b);   // <= 2^31, in unsigned 32 bits
    sum += a + b;
    const int32_t ma = a < 0 ? -a : a, mb = b < 0 ? -b : b;
    peak = ma > peak ? ma : peak;
    peak = mb > peak ? mb : peak;
    full += (a == 32767 || a == -32768 ? 1 : 0) + (b == 32767 || b == -32768 ? 1 : 0);
}

// first_halves, hops: [n][5184] bytes, the hop ring's staging by position; streams[n], is_first[n], restart[n]; state[channels] by
// stream; records[n], levels[n], energies[n][54] by position
__global__ __launch_bounds__(kWaves * 64) void stream_pings_kernel(const uint8_t* __restrict__ first_halves, const uint8_t* __restrict__ hops, const int32_t* __restrict__ streams,
                                                                   const uint8_t* __restrict__ is_first, const uint8_t* __restrict__ restart, int n, msk144sp::Params p,
                                                                   msk144wb::PingHistory* __restrict__ state, msk144wb::PingRecord* __restrict__ records,
                                                                   msk144sp::Level* __restrict__ levels, int32_t* __restrict__ energies)
{
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * kWaves + threadIdx.x / 64));
    if(j >= n) return;  // whole waves leave
    const int s = __builtin_amdgcn_readfirstlane(streams[j]);
    const bool first = __builtin_amdgcn_readfirstlane(static_cast<int>(is_first[j])) != 0;
    const bool again = first || __builtin_amdgcn_readfirstlane(static_cast<int>(restart[j])) != 0;
    const int nb = first ? msk144sp::kMaxBlocks : msk144sp::kHopBlocks;

    uint64_t sq = 0;
    int32_t sum = 0, peak = 0, full = 0;
    if(lane < nb)
    {
        const bool head = first && lane < msk144sp::kHopBlocks;
        const uint8_t* row = (head ? first_halves : hops) + static_cast<size_t>(j) * kRowBytes;
        const uint4* src = reinterpret_cast<const uint4*>(row + (first && !head ? lane - msk144sp::kHopBlocks : lane) * kBlockBytes);
#pragma unroll
        for(int k = 0; k < kBlockBytes / 16; k++)
        {
            const uint4 v = src[k];
            take(v.x, sq, sum, peak, full);
            take(v.y, sq, sum, peak, full);
            take(v.z, sq, sum, peak, full);
            take(v.w, sq, sum, peak, full);
        }
    }
    const int32_t E = lane < nb ? msk144sp::block_energy(sq, p.shift) : 0;

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
    msk144wb::PingHistory& st = state[s];
    int32_t h = 0;
    const int32_t R = msk144wb::ping_reference(msk144wb::ping_history_min(st, again, 1.0f, p.memory, q, h), p.min_ref);
    const unsigned long long up = __ballot(lane < nb && msk144wb::ping_up(E, R, p.ratio_q4));
    // positive floats order as their bit patterns do; bit 30 makes every key a normal number
    const uint32_t key = lane < nb ? (static_cast<uint32_t>(E) << 6) | static_cast<uint32_t>(63 - lane) : 0u;
    const uint32_t top = __builtin_bit_cast(uint32_t, wave_max_f32(__builtin_bit_cast(float, key | 0x40000000u))) & 0x0fffffffu;

    // ---- levels: every lane past nb holds zeros ----
    const int64_t all_sq = static_cast<int64_t>(wave_sum_int(static_cast<unsigned long long>(sq)));
    const int32_t all_sum = wave_sum_int(sum);
    const int32_t all_full = wave_sum_int(full);
    const int32_t all_peak = wave_max_i32(peak);
    const int saturated = __popcll(__ballot(lane < nb && E == msk144sp::kEnergyCap));

    if(lane < msk144sp::kMaxBlocks) energies[static_cast<size_t>(j) * msk144sp::kMaxBlocks + lane] = E;
    if(lane == 0)
    {
        msk144wb::ping_history_put(st, again, 1.0f, q);
        msk144wb::PingRecord r;
        r.up_mask = up;
        r.blocks = nb;
        r.history = h;
        r.quiet = q;
        r.reference = R;
        r.peak = static_cast<int32_t>(top >> 6);
        r.peak_block = 63 - static_cast<int32_t>(top & 63);
        records[j] = r;
        msk144sp::Level l;
        l.sum = all_sum;
        l.sum_sq = all_sq;
        l.peak = all_peak;
        l.full_scale = all_full;
        l.samples = nb * msk144sp::kBlock;
        l.saturated_blocks = saturated;
        levels[j] = l;
    }
}

}  // namespace

void launch_stream_pings(const void* first_halves, const void* hops, const int32_t* streams, const uint8_t* is_first, const uint8_t* restart, int n, const msk144sp::Params& p,
                         msk144wb::PingHistory* state, msk144wb::PingRecord* records, msk144sp::Level* levels, int32_t* energies, hipStream_t stream)
{
    hipLaunchKernelGGL(stream_pings_kernel, dim3((n + kWaves - 1) / kWaves), dim3(kWaves * 64), 0, stream, static_cast<const uint8_t*>(first_halves), static_cast<const uint8_t*>(hops),
                       streams, is_first, restart, n, p, state, records, levels, energies);
}

}  // namespace msk144
