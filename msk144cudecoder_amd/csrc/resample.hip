// resample: real int16 audio at Fs = 12000 P/Q (24 to 192 kHz) to the 12 kHz hops the hop ring takes, per stream, in exact integers
// (contract in include/msk144hip.h; the same rule on the host is csrc/input_rate.h Resampler).
//
//   y[m] = clamp((sum_k h[r_m + kQ] x[n_m - k] + 2^(s-1)) >> s),   n_m = floor(mP/Q), r_m = (mP) mod Q
//
// One workgroup per (listed stream j, tile of 288 outputs): Q divides 288, so a tile starts on branch 0 at input sample
// n0 = tile x 288 P/Q of the push, and r_m, n_m - n0 depend only on the position inside the tile - 32-bit indices throughout.  A hop
// is nine tiles, a first hop eighteen (the first nine write the first half).
//
// A tile stages its 288 P/Q inputs and the H = ceil(L/Q) - 1 samples in front of them in LDS as int16, input n0 - H at index 0, from
// the stream's history (tile 0 of a later hop), zeros (tile 0 of a first hop), the first-half row or the hop row; two zero samples
// follow.  Output i of the tile then reads the window that starts at LDS sample w = floor(iP/Q), H + 1 samples long, with the packed
// int16 dot product (v_dot2c_i32_i16) one dword = two samples at a time.  w is odd for some outputs and a dword starts on an even
// sample, so the taps come packed twice (msk144ir::pack_taps): for an even w as they are, for an odd w behind one zero, read from
// dword (w - 1) / 2.  Either packing is `dwords` long and zero-padded; the zero taps meet the sample in front of the window or the
// one or two behind it, which are staged (the zeros behind the last window are what the two extra samples are for).
//
// The taps stay in global memory, [Q][2][dwords] dwords: 96 branches of 64 taps per phase (96125 Hz, 197 KB packed) do not fit in
// LDS, every workgroup reads the same table, and a wave's lanes read at most Q rows of it, so the table lives in L2 and the vector L1.
//
// The history is read-only here: tile 0 reads the stream's old history while tiles 1.. of the same stream run, so the new one is
// written by resample_history_kernel, a second launch behind this one on the same stream.
#include "input_rate.h"
#include "msk144_kernels.h"

namespace msk144
{

namespace
{

constexpr int kTile = 288;            // outputs per workgroup; every Q that divides 96 divides it
constexpr int kThreads = 320;         // five waves, 288 lanes of them with an output
constexpr int kTilesPerHop = kHopSamples / kTile;  // 9
constexpr int kMaxTileIn = kTile * 16;             // P/Q <= 16 (192 kHz)
constexpr int kStageSamples = kMaxTileIn + msk144ir::kMaxHistory + 8;
static_assert(kHopSamples % kTile == 0 && kTile % 96 == 0 && kThreads % 64 == 0 && kThreads >= kTile && kStageSamples % 2 == 0, "whole tiles, whole waves");

typedef short short2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int32_t dot2(uint32_t a, uint32_t b, int32_t acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), acc, false);
}

__global__ __launch_bounds__(kThreads) void resample_kernel(ResampleArgs a)
{
    __shared__ uint32_t xs[kStageSamples / 2];
    int16_t* x16 = reinterpret_cast<int16_t*>(xs);

    const int tile = blockIdx.x;
    const int j = blockIdx.y;
    const bool first = a.is_first[j] != 0;
    if(!first && tile >= kTilesPerHop) return;  // the whole workgroup, ahead of the barrier
    const int s = a.streams[j];
    const int tid = threadIdx.x;
    const int tile_in = kTile / a.Q * a.P;
    const int n0 = tile * tile_in;              // of the push: a first push starts at the first-half row
    const int staged = tile_in + a.H;           // <= kMaxTileIn + kMaxHistory
    const int16_t* __restrict__ head = a.in_first + static_cast<size_t>(j) * a.row;
    const int16_t* __restrict__ hop = a.in_hops + static_cast<size_t>(j) * a.row;
    const int16_t* __restrict__ hist = a.hist + static_cast<size_t>(s) * a.hist_stride;

    // staged sample i is input n0 - H + i of the push; n0 + tile_in <= row (two rows on a first push), and only tile 0 reaches below 0
    for(int i = tid; i < staged + 2; i += kThreads)
    {
        const int n = n0 - a.H + i;
        int16_t v = 0;
        if(i >= staged) v = 0;
        else if(n < 0) v = first ? static_cast<int16_t>(0) : hist[a.H + n];
        else if(first) v = n < a.row ? head[n] : hop[n - a.row];
        else v = hop[n];
        x16[i] = v;
    }
    __syncthreads();

    bool clamped = false;
    if(tid < kTile)
    {
        const int mp = tid * a.P;
        const int w = mp / a.Q, r = mp - w * a.Q;
        const uint32_t* __restrict__ g = a.taps + (static_cast<size_t>(r) * 2 + (w & 1)) * a.dwords;
        const uint32_t* xw = xs + (w >> 1);     // (w >> 1) + dwords <= (tile_in - 1 + H + 3) / 2 < (staged + 2) / 2 + 1
        int32_t acc = 0;
        for(int d = 0; d < a.dwords; d++) acc = dot2(g[d], xw[d], acc);
        int32_t y = (acc + (1 << (a.shift - 1))) >> a.shift;
        clamped = y > 32767 || y < -32768;
        y = y > 32767 ? 32767 : (y < -32768 ? -32768 : y);
        const int m = tile * kTile + tid;       // of the push
        int16_t* out = first && tile < kTilesPerHop ? a.out_first + static_cast<size_t>(j) * kHopSamples + m
                                                    : a.out_hops + static_cast<size_t>(j) * kHopSamples + (first ? m - kHopSamples : m);
        *out = static_cast<int16_t>(y);
    }
    const unsigned long long mask = __ballot(clamped);
    if((tid & 63) == 0 && mask) atomicAdd(a.clamped + j, __popcll(mask));
}

// the stream's new history: the last H inputs of the push, which lie in the hop row (H is shorter than a row)
__global__ __launch_bounds__(256) void resample_history_kernel(const int16_t* __restrict__ in_hops, const int32_t* __restrict__ streams, int16_t* __restrict__ hist, int H,
                                                               int hist_stride, int row)
{
    const int j = blockIdx.x;
    const int16_t* __restrict__ src = in_hops + static_cast<size_t>(j) * row + (row - H);
    int16_t* __restrict__ dst = hist + static_cast<size_t>(streams[j]) * hist_stride;
    for(int i = threadIdx.x; i < H; i += 256) dst[i] = src[i];
}

}  // namespace

void launch_resample(const ResampleArgs& a, int n, bool any_first, hipStream_t stream)
{
    hipLaunchKernelGGL(resample_kernel, dim3(any_first ? 2 * kTilesPerHop : kTilesPerHop, n), dim3(kThreads), 0, stream, a);
    if(a.H > 0) hipLaunchKernelGGL(resample_history_kernel, dim3(n), dim3(256), 0, stream, a.in_hops, a.streams, const_cast<int16_t*>(a.hist), a.H, a.hist_stride, a.row);
}

}  // namespace msk144
