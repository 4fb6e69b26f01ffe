// spectrum: the power spectrum of a push's input samples at Fs (msk144_set_wideband_spectrum, include/msk144hip.h).
//
// The N new samples of a push, as the channeliser or the bank reads them, are cut into S = floor(N / B) segments of B samples, not
// overlapped; X_s[k] = sum_i w[i] x[sB + i] e^{-j2pi ik/B} in f32, and P[k] = sum_s |X_s[k]|^2 with the sum over s in double.
//
// Two launches.  spectrum_kernel: a workgroup transforms a round of 8192 consecutive samples at a time - 8192 / B whole segments side
// by side, so that every B from 256 to 8192 gives its 256 threads the same work - and takes the rounds g, g + G, g + 2G, ...  A
// transform is the mixed-radix decimation in frequency of frontend.hip's FFT section, B = R1 x R2 x 32 (R2 = 1 at B = 256 and 512: two passes):
//
//   n = (32 R2) n1 + 32 n2 + n3,   k = k1 + R1 k2 + R1 R2 k3,   W = exp(-2 pi i / B):
//   W^(nk) = W_R1^(n1 k1) . W^((32 n2 + n3) k1) . W_R2^(n2 k2) . W^(R1 n3 k2) . W_32^(n3 k3)
//
// with the butterflies in registers (fft_reg.h), every pass in place in LDS behind one barrier, the same one pad cell per 32 as the
// front end's (the radix-32 columns of the last pass are 33 cells apart, the other passes walk 32 contiguous cells per half wave)
// and twiddles from an f32 table of B entries computed in double at `set`.  The last pass leaves bin k1 + R1 k2 + R1 R2 k3 of its
// (segment, k1, k2) column in register k3 of one thread, in every round the same bins: |X|^2 is formed there in f32 and added to 32
// double accumulators that stay in registers across the rounds.  After its last round the workgroup adds its 8192 / B segment
// columns in segment order through LDS and writes one row of B sums to partials[g].  spectrum_reduce_kernel adds the G rows in row
// order and writes them in ascending frequency.  G and the round a segment falls into are functions of S alone, no atomics: the
// same samples give the same bytes.
#include "msk144_kernels.h"

#include <algorithm>

#include "fft_reg.h"
#include "wideband_samples.h"

namespace msk144
{

namespace
{

constexpr int kThreads = 256;
constexpr int kRound = 8192;                  // samples a workgroup transforms at a time: kRound / B whole segments
constexpr int kCells = kRound + kRound / 32;  // padded: fft_cell(i) = i + i / 32
static_assert(kRound / 32 == kThreads, "one radix-32 column per thread in the last pass");
static_assert(kRound == msk144wb::kSpectrumMaxBins, "the largest B is one round");

// window x sample p of the round that starts at sample `base` of the push, 0 + 0j from sample `live` on; kPer consecutive ones
template<int FMT, int B, int kPer>
__device__ __forceinline__ void store_windowed(float2* __restrict__ s, const void* chunk, int p, bool live, const float* __restrict__ window)
{
    float w[kPer];
#pragma unroll
    for(int j = 0; j < kPer; j += 4)
    {
        const float4 v = *reinterpret_cast<const float4*>(window + ((p + j) & (B - 1)));
        w[j] = v.x, w[j + 1] = v.y, w[j + 2] = v.z, w[j + 3] = v.w;
    }
#pragma unroll
    for(int j = 0; j < kPer; j++)
    {
        const float2 x = load_sample<FMT>(chunk, j);
        s[fft_cell(p + j)] = live ? make_float2(w[j] * x.x, w[j] * x.y) : make_float2(0.0f, 0.0f);
    }
}

// raw = the N new samples of a push, S = floor(N / B); window[B], tw[m] = exp(-2 pi i m / B), m < B; partials[gridDim.x][B].
// vec: raw is 16-byte aligned (a round starts a multiple of 16 bytes behind it).
// Registers: 64 hold the accumulators and 64 the radix-32 column, and two workgroups per CU (what LDS admits) leave a lane 256.  The
// twiddles of a thread are the same in every round, and left to itself the compiler loads those of all passes once and pins them
// across the rounds: 266 - 352 registers, one workgroup per CU.  So the table of round r is addressed as tables[r x table_stride] with
// table_stride a kernel argument - the launcher passes 0, there is one table - which makes the loads part of the round (they hit L1),
// and the second launch bound holds the kernel to 256 registers: 226 - 247 VGPR, no scratch, occupancy 2 at every size.
template<int FMT, int R1, int R2>
__global__ __launch_bounds__(kThreads, 2) void spectrum_kernel(const void* __restrict__ raw, int S, int vec, const float* __restrict__ window,
                                                               const float2* __restrict__ tables, int table_stride, double* __restrict__ partials)
{
    constexpr int B = R1 * R2 * 32;
    constexpr int kSeg = kRound / B;
    constexpr int kPer = FMT == 2 ? 4 : 8;  // samples per 16 bytes
    __shared__ __align__(16) float2 s[kCells];

    const int tid = threadIdx.x;
    const int live = S * B;  // samples of the push that belong to a segment (< 2^31: a push has at most 5184 x 5120 samples)
    const int rounds = (S + kSeg - 1) / kSeg;
    double acc[32];
#pragma unroll
    for(int k3 = 0; k3 < 32; k3++) acc[k3] = 0.0;

    for(int round = blockIdx.x; round < rounds; round += gridDim.x)
    {
        // ---- the round's samples, windowed, into LDS; the slots of segments past S hold zeros ----
        const int base = round * kRound;
        const float2* __restrict__ tw = tables + round * table_stride;
        if(vec)
        {
#pragma unroll 1
            for(int r = 0; r < kRound / kPer / kThreads; r++)
            {
                const int p = (tid + r * kThreads) * kPer;
                const bool in = base + p < live;  // live is a multiple of 256: a 16-byte chunk lies on one side
                const uint4 chunk = in ? static_cast<const uint4*>(raw)[(base + p) / kPer] : make_uint4(0, 0, 0, 0);
                store_windowed<FMT, B, kPer>(s, &chunk, p, in, window);
            }
        }
        else
        {
#pragma unroll 4
            for(int p = tid; p < kRound; p += kThreads)
            {
                const float w = window[p & (B - 1)];
                const float2 x = base + p < live ? load_sample<FMT>(raw, base + p) : make_float2(0.0f, 0.0f);
                s[fft_cell(p)] = make_float2(w * x.x, w * x.y);
            }
        }
        __syncthreads();

        // ---- radix R1 over n1 (stride B / R1), twiddle W^(t k1), in place ----
        constexpr int kN1 = B / R1;
#pragma unroll 1
        for(int r = 0; r < kRound / R1 / kThreads; r++)
        {
            const int b = tid + r * kThreads, t = b & (kN1 - 1), cell = (b / kN1) * B + t;
            float2 a[R1];
#pragma unroll
            for(int n1 = 0; n1 < R1; n1++) a[n1] = s[fft_cell(cell + n1 * kN1)];
            fft_reg<R1, false>(a);
            s[fft_cell(cell)] = a[0];
#pragma unroll
            for(int k1 = 1; k1 < R1; k1++) s[fft_cell(cell + k1 * kN1)] = cmul_fma(a[k1], tw[t * k1]);
        }
        __syncthreads();

        // ---- radix R2 over n2 (stride 32 inside the block of k1), twiddle W^(R1 n3 k2), in place ----
        if constexpr(R2 > 1)
        {
            constexpr int kN2 = B / R2;
#pragma unroll 1
            for(int r = 0; r < kRound / R2 / kThreads; r++)
            {
                const int b = tid + r * kThreads, c = b & (kN2 - 1), n3 = c & 31, cell = (b / kN2) * B + (c >> 5) * (R2 * 32) + n3;
                float2 a[R2];
#pragma unroll
                for(int n2 = 0; n2 < R2; n2++) a[n2] = s[fft_cell(cell + n2 * 32)];
                fft_reg<R2, false>(a);
                s[fft_cell(cell)] = a[0];
#pragma unroll
                for(int k2 = 1; k2 < R2; k2++) s[fft_cell(cell + k2 * 32)] = cmul_fma(a[k2], tw[R1 * n3 * k2]);
            }
            __syncthreads();
        }

        // ---- radix 32 over n3: one thread per (segment, k1, k2) column; |X|^2 in f32, summed over the rounds in double ----
        {
            float2 a[32];
#pragma unroll
            for(int n3 = 0; n3 < 32; n3++) a[n3] = s[tid * 33 + n3];
            fft_reg<32, false>(a);
#pragma unroll
            for(int k3 = 0; k3 < 32; k3++) acc[k3] += static_cast<double>(a[k3].x * a[k3].x + a[k3].y * a[k3].y);
        }
        __syncthreads();  // the next round, or the sums below, overwrite the buffer
    }

    // ---- this workgroup's row: its kSeg segment columns added in segment order ----
    double* sums = reinterpret_cast<double*>(s);  // kRound doubles: kSeg x B
    {
        const int col = tid & (B / 32 - 1), k = col / R2 + R1 * (col & (R2 - 1));
#pragma unroll
        for(int k3 = 0; k3 < 32; k3++) sums[(tid / (B / 32)) * B + k + R1 * R2 * k3] = acc[k3];
    }
    __syncthreads();
    for(int k = tid; k < B; k += kThreads)
    {
        double sum = sums[k];
#pragma unroll
        for(int q = 1; q < kSeg; q++) sum += sums[q * B + k];
        partials[static_cast<size_t>(blockIdx.x) * B + k] = sum;
    }
}

// out[j] = sum over the G rows, in row order, of bin k = (j - B/2) mod B: ascending frequency
__global__ __launch_bounds__(kThreads) void spectrum_reduce_kernel(const double* __restrict__ partials, int G, int B, double* __restrict__ out)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if(j >= B) return;
    const int k = (j + B / 2) & (B - 1);
    double sum = 0.0;
    for(int g = 0; g < G; g++) sum += partials[static_cast<size_t>(g) * B + k];
    out[j] = sum;
}

template<int FMT>
void launch_spectrum_format(const void* raw, int S, int G, int vec, int B, const float* window, const float2* tw, double* partials, hipStream_t stream)
{
    const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(G), dim3(kThreads), 0, stream, raw, S, vec, window, tw, 0, partials); };
    switch(B)
    {
    case 256: launch(spectrum_kernel<FMT, 8, 1>); break;
    case 512: launch(spectrum_kernel<FMT, 16, 1>); break;
    case 1024: launch(spectrum_kernel<FMT, 8, 4>); break;
    case 2048: launch(spectrum_kernel<FMT, 8, 8>); break;
    case 4096: launch(spectrum_kernel<FMT, 16, 8>); break;
    default: launch(spectrum_kernel<FMT, 16, 16>); break;
    }
}

}  // namespace

void launch_spectrum(const void* raw, int format, int N, int B, const float* window, const float2* twiddles, double* partials, double* out, hipStream_t stream)
{
    const int S = N / B;
    const int rounds = (S + kRound / B - 1) / (kRound / B);
    const int G = std::min(rounds, kSpectrumMaxGroups);
    const int vec = reinterpret_cast<uintptr_t>(raw) % 16 == 0 ? 1 : 0;
    if(G > 0)
    {
        switch(format)
        {
        case 0: launch_spectrum_format<0>(raw, S, G, vec, B, window, twiddles, partials, stream); break;
        case 1: launch_spectrum_format<1>(raw, S, G, vec, B, window, twiddles, partials, stream); break;
        default: launch_spectrum_format<2>(raw, S, G, vec, B, window, twiddles, partials, stream); break;
        }
    }
    hipLaunchKernelGGL(spectrum_reduce_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, partials, G, B, out);
}

}  // namespace msk144
