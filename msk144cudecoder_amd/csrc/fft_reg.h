// Register-resident DFT butterflies and the LDS cell padding shared by the transforms in frontend.hip (the 8192-point analytic
// signal) and spectrum.hip (the wideband power spectrum).
#pragma once

#include <hip/hip_runtime.h>

namespace msk144
{

// one pad cell per 32: columns of 32 cells lie 33 apart
__device__ __forceinline__ int fft_cell(int i)
{
    return i + (i >> 5);
}

// cos(k pi / 16), k = 0..16: after full unrolling k is a constant and the switch folds to a literal
__device__ __forceinline__ float cos_pi16(int k)
{
    switch(k)
    {
    case 0: return 1.0f;
    case 1: return 0.980785280403230449f;
    case 2: return 0.923879532511286756f;
    case 3: return 0.831469612302545237f;
    case 4: return 0.707106781186547524f;
    case 5: return 0.555570233019602225f;
    case 6: return 0.382683432365089772f;
    case 7: return 0.195090322016128268f;
    case 8: return 0.0f;
    case 9: return -0.195090322016128268f;
    case 10: return -0.382683432365089772f;
    case 11: return -0.555570233019602225f;
    case 12: return -0.707106781186547524f;
    case 13: return -0.831469612302545237f;
    case 14: return -0.923879532511286756f;
    case 15: return -0.980785280403230449f;
    default: return -1.0f;
    }
}

// x . W32^k (forward) or x . conj(W32^k) (inverse), k = 0..15 a compile-time constant after unrolling
template<bool kInverse>
__device__ __forceinline__ float2 mul_w32(float2 x, int k)
{
    if(k == 0) return x;
    if(k == 8) return kInverse ? make_float2(-x.y, x.x) : make_float2(x.y, -x.x);
    const float c = cos_pi16(k);
    const float sn = cos_pi16(k < 8 ? 8 - k : k - 8);  // sin(k pi / 16) = cos(|8 - k| pi / 16) > 0
    const float s = kInverse ? sn : -sn;
    return make_float2(fmaf(x.x, c, -(x.y * s)), fmaf(x.x, s, x.y * c));
}

__device__ __forceinline__ float2 cmul_fma(float2 x, float2 w)
{
    return make_float2(fmaf(x.x, w.x, -(x.y * w.y)), fmaf(x.x, w.y, x.y * w.x));
}

// R-point DFT (R = 4, 8, 16 or 32) of a register array, natural order in and out: log2(R) radix-2 decimation-in-frequency stages and
// the bit reversal, all indices compile-time constants
template<int R, bool kInverse>
__device__ __forceinline__ void fft_reg(float2 (&a)[R])
{
    constexpr int kLog = R == 32 ? 5 : R == 16 ? 4 : R == 8 ? 3 : 2;
    static_assert(R == 1 << kLog, "R must be 4, 8, 16 or 32");
#pragma unroll
    for(int stage = 0; stage < kLog; stage++)
    {
        const int len = R >> stage, half = len >> 1;
#pragma unroll
        for(int b = 0; b < R; b += len)
        {
#pragma unroll
            for(int j = 0; j < half; j++)
            {
                const float2 u = a[b + j], v = a[b + j + half];
                a[b + j] = make_float2(u.x + v.x, u.y + v.y);
                a[b + j + half] = mul_w32<kInverse>(make_float2(u.x - v.x, u.y - v.y), j * (32 / len));
            }
        }
    }
#pragma unroll
    for(int i = 0; i < R; i++)
    {
        int r = 0;
#pragma unroll
        for(int bit = 0; bit < kLog; bit++) r |= ((i >> bit) & 1) << (kLog - 1 - bit);
        if(i < r)
        {
            const float2 t = a[i];
            a[i] = a[r];
            a[r] = t;
        }
    }
}

}  // namespace msk144
