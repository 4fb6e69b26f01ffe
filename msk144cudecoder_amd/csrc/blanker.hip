// blanker: the impulse-noise blanker ahead of the channeliser and the bank (msk144_set_wideband_blanker, include/msk144hip.h).
//
// Per push of N raw samples, in integers only: p[n] = cI^2 + cQ^2 in component units of the input format (cu8: c = 2u - 255, cs8 and
// cs16: c = s), S = sum p[n], T = msk144wb::blanker_threshold(S, N, threshold_q4); sample n is a hit iff p[n] > T and is blanked iff
// a hit h of this push has h - pre <= n <= h + post, or n < carry_in (what the previous push's last hit still owes).  The output
// is the push as cs16 - cu8 (2u - 255) x 128, cs8 s x 256, the same real numbers - with every blanked sample 0 + 0j: cu8 has no
// byte that means zero.
//
// Two launches.  blanker_power_kernel sums the squared components with 16-byte loads, a wave reduction and one 64-bit atomic per
// workgroup: integer adds, so exact in any order.  blanker_apply_kernel takes one tile of 4096 samples per workgroup: lane i of a
// wave owns sample i of a 64-sample word, so __ballot(p > T) is the word's hit mask and loads and stores stay coalesced.  The hit
// words of the tile and of ceil(post/64) words before it and ceil(pre/64) behind it (re-read from the raw push: out of place, no
// tile reads what another writes) go to LDS, one wave scans them for the last hit at or before the end of each word, and
// "blanked" is then one question per sample: does the last hit at or before n + pre lie at or after n - post?
#include "msk144_kernels.h"

#include <algorithm>

namespace msk144
{

namespace
{

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileWords = 64;                      // 64-sample words per workgroup: a tile of 4096 samples
constexpr int kTileSamples = 64 * kTileWords;
constexpr int kOwnWords = kTileWords / kWaves;      // tile words per wave, kept in registers between the two passes
constexpr int kHaloWords = msk144wb::kBlankerMaxGuard / 64;
constexpr int kWindowWords = kTileWords + 2 * kHaloWords;
constexpr int kNoHit = -(1 << 30);                  // "no hit in reach": below n - post for every n
constexpr int kMaxPowerBlocks = 2048;

// the integer components of sample i, and the same sample as cs16
template<int FMT>
__device__ inline int2 load_components(const void* __restrict__ raw, int i)
{
    if(FMT == 0)
    {
        const uchar2 v = static_cast<const uchar2*>(raw)[i];
        return make_int2(2 * v.x - 255, 2 * v.y - 255);
    }
    else if(FMT == 1)
    {
        const char2 v = static_cast<const char2*>(raw)[i];
        return make_int2(v.x, v.y);
    }
    else
    {
        const short2 v = static_cast<const short2*>(raw)[i];
        return make_int2(v.x, v.y);
    }
}

template<int FMT>
__device__ inline short2 as_cs16(int2 c)
{
    constexpr int kUnit = FMT == 0 ? 128 : FMT == 1 ? 256 : 1;
    return make_short2(static_cast<short>(c.x * kUnit), static_cast<short>(c.y * kUnit));
}

// sum of the squared components of one 32-bit word of raw input (4 components at 8 bits, 2 at 16); at most 2^31
template<int FMT>
__device__ inline unsigned int word_power(unsigned int w)
{
    unsigned int s = 0;
    if(FMT == 2)
    {
        const int a = static_cast<short>(w & 0xffffu), b = static_cast<short>(w >> 16);
        s = static_cast<unsigned int>(a * a) + static_cast<unsigned int>(b * b);
    }
    else
    {
#pragma unroll
        for(int k = 0; k < 4; k++)
        {
            const unsigned int u = (w >> (8 * k)) & 0xffu;
            const int c = FMT == 0 ? 2 * static_cast<int>(u) - 255 : static_cast<signed char>(u);
            s += static_cast<unsigned int>(c * c);
        }
    }
    return s;
}

__device__ inline unsigned long long wave_sum_u64(unsigned long long v)
{
    for(int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// S over the push's `bytes` of raw input: 16 bytes at a time, then the last 0..14 bytes component by component (a push of an odd
// number of 8-bit samples is no whole number of words)
template<int FMT>
__global__ __launch_bounds__(kThreads) void blanker_power_kernel(const void* __restrict__ raw, long long bytes, BlankerCounters* __restrict__ ctr)
{
    __shared__ unsigned long long part[kWaves];
    const long long vecs = bytes / 16;
    unsigned long long sum = 0;
    for(long long v = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; v < vecs; v += static_cast<long long>(gridDim.x) * kThreads)
    {
        const uint4 q = static_cast<const uint4*>(raw)[v];
        sum += word_power<FMT>(q.x);
        sum += word_power<FMT>(q.y);
        sum += word_power<FMT>(q.z);
        sum += word_power<FMT>(q.w);
    }
    constexpr int kComponentBytes = FMT == 2 ? 2 : 1;
    const long long c = 16 / kComponentBytes * vecs + threadIdx.x;
    if(blockIdx.x == 0 && c * kComponentBytes < bytes)
    {
        const int v = FMT == 0 ? 2 * static_cast<const unsigned char*>(raw)[c] - 255 : FMT == 1 ? static_cast<const signed char*>(raw)[c] : static_cast<const short*>(raw)[c];
        sum += static_cast<unsigned int>(v * v);
    }
    sum = wave_sum_u64(sum);
    if((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if(threadIdx.x == 0)
    {
        unsigned long long s = 0;
        for(int w = 0; w < kWaves; w++) s += part[w];
        if(s) atomicAdd(&ctr->sum_power, s);
    }
}

// out[n] = blanked ? 0 : raw[n] as cs16, n < N; counts hits and blanked samples; the last tile leaves carry[parity] for the next push
template<int FMT>
__global__ __launch_bounds__(kThreads) void blanker_apply_kernel(const void* __restrict__ raw, short2* __restrict__ out, int N, msk144wb::BlankerParams p, int parity,
                                                                 BlankerCounters* __restrict__ ctr)
{
    __shared__ unsigned long long hit_words[kWindowWords];
    __shared__ int last_hit[kWindowWords + 1];  // last_hit[k]: the last hit in window words < k, or kNoHit
    __shared__ unsigned long long threshold;
    __shared__ unsigned int counts[kWaves][2];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int halo_l = (p.post + 63) >> 6, halo_r = (p.pre + 63) >> 6;  // <= kHaloWords each (check_blanker)
    const int window = halo_l + kTileWords + halo_r;
    const int word0 = blockIdx.x * kTileWords - halo_l;                 // the 64-sample word of window word 0; negative: before the push
    if(threadIdx.x == 0) threshold = msk144wb::blanker_threshold(ctr->sum_power, static_cast<uint64_t>(N), static_cast<uint32_t>(p.threshold_q4));
    __syncthreads();
    const unsigned long long T = threshold;

    // pass 1: the hit word of every window word; a wave keeps the cs16 samples of its own tile words
    short2 own[kOwnWords];
    unsigned int hits = 0;
#pragma unroll
    for(int i = 0; i < kOwnWords; i++)
    {
        const int k = halo_l + wave + kWaves * i;
        const int n = (word0 + k) * 64 + lane;
        bool hit = false;
        own[i] = make_short2(0, 0);
        if(n < N)
        {
            const int2 c = load_components<FMT>(raw, n);
            hit = static_cast<unsigned long long>(static_cast<unsigned int>(c.x * c.x) + static_cast<unsigned int>(c.y * c.y)) > T;
            own[i] = as_cs16<FMT>(c);
        }
        const unsigned long long w = __ballot(hit);
        hits += __popcll(w);
        if(lane == 0) hit_words[k] = w;
    }
    for(int j = wave; j < halo_l + halo_r; j += kWaves)
    {
        const int k = j < halo_l ? j : j + kTileWords;
        const int n = (word0 + k) * 64 + lane;
        bool hit = false;
        if(n >= 0 && n < N)
        {
            const int2 c = load_components<FMT>(raw, n);
            hit = static_cast<unsigned long long>(static_cast<unsigned int>(c.x * c.x) + static_cast<unsigned int>(c.y * c.y)) > T;
        }
        const unsigned long long w = __ballot(hit);
        if(lane == 0) hit_words[k] = w;
    }
    __syncthreads();

    // one wave: last_hit[k + 1] = the last hit in window words <= k, a running maximum over the words, 64 at a time
    if(wave == 0)
    {
        int carry = kNoHit;
        if(lane == 0) last_hit[0] = kNoHit;
        for(int k0 = 0; k0 < window; k0 += 64)
        {
            const int k = k0 + lane;
            const unsigned long long w = k < window ? hit_words[k] : 0;
            int v = w ? (word0 + k) * 64 + 63 - __clzll(static_cast<long long>(w)) : kNoHit;
            for(int off = 1; off < 64; off <<= 1)
            {
                const int u = __shfl_up(v, off);
                if(lane >= off) v = max(v, u);
            }
            v = max(v, carry);
            if(k < window) last_hit[k + 1] = v;
            carry = __shfl(v, 63);
        }
    }
    __syncthreads();

    // pass 2: sample n is blanked iff the last hit at or before n + pre lies at or after n - post, or the previous push owes it
    const int carry_in = blockIdx.x == 0 ? static_cast<int>(ctr->carry[parity ^ 1]) : 0;  // <= post <= a tile
    unsigned int blanked = 0;
#pragma unroll
    for(int i = 0; i < kOwnWords; i++)
    {
        const int n = (blockIdx.x * kTileWords + wave + kWaves * i) * 64 + lane;
        const int q = n + p.pre;
        const int kq = (q >> 6) - word0;          // < window, as q < (tile end) + pre
        const int bq = q & 63;
        const unsigned long long m = hit_words[kq] & (bq == 63 ? ~0ull : (2ull << bq) - 1);
        const int h = m ? (q & ~63) + 63 - __clzll(static_cast<long long>(m)) : last_hit[kq];
        const bool blank = n < N && (h >= n - p.post || n < carry_in);
        if(n < N) out[n] = blank ? make_short2(0, 0) : own[i];
        blanked += __popcll(__ballot(blank));
    }
    if(lane == 0)
    {
        counts[wave][0] = hits;
        counts[wave][1] = blanked;
    }
    __syncthreads();
    if(threadIdx.x == 0)
    {
        unsigned long long h = 0, b = 0;
        for(int w = 0; w < kWaves; w++)
        {
            h += counts[w][0];
            b += counts[w][1];
        }
        if(h)
        {
            atomicAdd(&ctr->hits, h);
            atomicAdd(&ctr->total_hits, h);
        }
        if(b)
        {
            atomicAdd(&ctr->blanked, b);
            atomicAdd(&ctr->total_blanked, b);
        }
        // the last tile: a hit further back than its window owes nothing (it lies more than post before the tile)
        if(blockIdx.x == gridDim.x - 1)
        {
            const int owed = last_hit[window] + p.post - (N - 1);
            ctr->carry[parity] = owed > 0 ? static_cast<unsigned long long>(owed) : 0;
        }
    }
}

}  // namespace

void launch_blanker(const void* raw, int format, short2* out, int N, const msk144wb::BlankerParams& p, int parity, BlankerCounters* counters, hipStream_t stream)
{
    const long long bytes = static_cast<long long>(N) * msk144wb::sample_bytes(format);
    const int power_blocks = static_cast<int>(std::min<long long>(kMaxPowerBlocks, bytes / (16 * kThreads) + 1));
    const dim3 tiles((N + kTileSamples - 1) / kTileSamples);
    const auto launch = [&](auto power, auto apply) {
        hipLaunchKernelGGL(power, dim3(power_blocks), dim3(kThreads), 0, stream, raw, bytes, counters);
        hipLaunchKernelGGL(apply, tiles, dim3(kThreads), 0, stream, raw, out, N, p, parity, counters);
    };
    switch(format)
    {
    case 0: launch(blanker_power_kernel<0>, blanker_apply_kernel<0>); break;
    case 1: launch(blanker_power_kernel<1>, blanker_apply_kernel<1>); break;
    default: launch(blanker_power_kernel<2>, blanker_apply_kernel<2>); break;
    }
}

}  // namespace msk144
