// bank: the 64-band, 2x oversampled analysis bank in front of the channeliser at rates above 6.144 Msps (msk144_push_wideband).
//
// For every occupied band b = k mod 64 and frame n (32 input samples), with the real prototype h1[0..L1), L1 = 64 K1:
//     s_b[n] = (-1)^{b n} sum_{l<L1} h1[l] e^{+j2pi (b l mod 64)/64} x[32n - l]          (include/msk144hip.h)
//            = (-1)^{b n} sum_{p<64} e^{+j2pi b p/64} u_p[n],   u_p[n] = sum_{q<K1} h1[p + 64q] x[32n - p - 64q]
// so a frame costs 64 K1 real-by-complex MACs for the 64 polyphase sums and 64 complex MACs per occupied band for the DFT; the
// DFT is evaluated only for the occupied bands.
//
// One workgroup = 64 frames: the input span (32 x 63 + L1 samples) is converted to f32 into LDS once; lane p of each wave forms
// u_p for 16 of the frames (consecutive lanes read consecutive, descending samples) into an LDS tile u[p][f]; then each wave takes
// every 4th occupied band, lane f = frame, and sums the 64 phases against a broadcast twiddle - u[p][f] is read by 64 consecutive
// lanes at once, so neither pass has bank conflicts beyond the 2-way of the u stores.  f32 throughout; the output stays f32 on the
// device and is never quantised.
#include "msk144_kernels.h"
#include "wideband_samples.h"

namespace msk144
{

namespace
{

constexpr int kThreads = 256;
constexpr int kFrames = 64;     // frames per workgroup
constexpr int kBands = 64;
constexpr int kDecim = 32;
constexpr int kMaxK1 = 16;
constexpr int kMaxSpan = kDecim * (kFrames - 1) + kBands * kMaxK1;

template<int FMT>
__global__ __launch_bounds__(kThreads) void bank_kernel(const void* __restrict__ raw, const float* __restrict__ h1, const int32_t* __restrict__ bands,
                                                        const float2* __restrict__ tw, float2* __restrict__ sub, int n_bands, int K1, int frames,
                                                        long long stride, int off, int first, long long n_base)
{
    __shared__ float2 xs[kMaxSpan];
    __shared__ float2 us[kBands][kFrames + 1];
    __shared__ float hs[kBands * kMaxK1];
    __shared__ float2 tws[kBands];

    const int L1 = kBands * K1;
    const int hist = L1 - 1;                 // raw[0 .. hist) = the L1-1 samples before this push
    const int n_in = hist + frames * kDecim;
    const int f0 = blockIdx.x * kFrames;
    const int span = kDecim * (kFrames - 1) + L1;
    // xs[t] = raw[32 f0 + t]: frame f0 + f, tap l reads xs[32 f + hist - l]
    for(int t = threadIdx.x; t < span; t += kThreads)
    {
        const int i = kDecim * f0 + t;
        float2 v = make_float2(0.0f, 0.0f);
        if(i < n_in && !(first && i < hist)) v = load_sample<FMT>(raw, i);
        xs[t] = v;
    }
    for(int t = threadIdx.x; t < L1; t += kThreads) hs[t] = h1[t];
    if(threadIdx.x < kBands) tws[threadIdx.x] = tw[threadIdx.x];
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for(int f = wave; f < kFrames; f += kThreads / 64)
    {
        const int p = lane;
        float2 acc = make_float2(0.0f, 0.0f);
        for(int q = 0; q < K1; q++)
        {
            const float hq = hs[p + kBands * q];
            const float2 v = xs[kDecim * f + hist - p - kBands * q];
            acc.x = fmaf(hq, v.x, acc.x);
            acc.y = fmaf(hq, v.y, acc.y);
        }
        us[p][f] = acc;
    }
    __syncthreads();

    const int f = lane;
    if(f0 + f >= frames) return;
    const long long n = n_base + f0 + f;
    for(int jb = wave; jb < n_bands; jb += kThreads / 64)
    {
        const int b = bands[jb];
        float re = 0.0f, im = 0.0f;
        for(int p = 0; p < kBands; p++)
        {
            const float2 w = tws[(b * p) & (kBands - 1)];
            const float2 u = us[p][f];
            re = fmaf(w.x, u.x, re);
            re = fmaf(-w.y, u.y, re);
            im = fmaf(w.x, u.y, im);
            im = fmaf(w.y, u.x, im);
        }
        if(b & n & 1)
        {
            re = -re;
            im = -im;
        }
        sub[stride * jb + off + f0 + f] = make_float2(re, im);
    }
}

}  // namespace

void launch_bank(const void* raw, int format, const float* h1, const int32_t* bands, const float2* tw, float2* sub, int n_bands, int K1, int frames,
                 long long stride, int off, int first, long long n_base, hipStream_t stream)
{
    const dim3 grid((frames + kFrames - 1) / kFrames);
    if(format == 0)
        hipLaunchKernelGGL(bank_kernel<0>, grid, dim3(kThreads), 0, stream, raw, h1, bands, tw, sub, n_bands, K1, frames, stride, off, first, n_base);
    else if(format == 1)
        hipLaunchKernelGGL(bank_kernel<1>, grid, dim3(kThreads), 0, stream, raw, h1, bands, tw, sub, n_bands, K1, frames, stride, off, first, n_base);
    else
        hipLaunchKernelGGL(bank_kernel<2>, grid, dim3(kThreads), 0, stream, raw, h1, bands, tw, sub, n_bands, K1, frames, stride, off, first, n_base);
}

}  // namespace msk144
