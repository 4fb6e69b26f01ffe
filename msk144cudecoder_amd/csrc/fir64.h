// fir64: z[n] = sum_k b[k] x[n - k], 64 complex int8 taps over a channel's staged int8 hops, for the kernels that end it their own
// way (pingband.hip: block energies; notch.hip: x[n - 31] - z, in place; audio.hip: mixed to real int16 audio).  What
// msk144wb::fir_push computes on the host.
//
// One workgroup of four waves per channel.  stage() puts the channel's 63-sample tail and the push's row (two rows on a first push)
// in LDS with 16-byte loads, so that stored sample m of the push lies at byte 128 + 2m and the tail in bytes 2..127 in front of it
// (bytes 0..1, "sample -64", are zero), and packs the 64 taps once into 33 dwords per sum for the int8 dot product.
//
// A work item is 12 consecutive outputs z[n0] .. z[n0 + 11], n0 = 12 x item; a lane takes one item per pass (216 items of a later
// push, 432 of a first one).  A dword of the row holds two samples (I0, Q0, I1, Q1), and the window x[n - 63 .. n] of an odd n starts
// on a dword, that of an even n two bytes behind one.  So the taps are packed twice:
//
//   even n   dword j of the window that starts at sample n - 64 meets taps (64 - 2j, 63 - 2j): 33 dwords, tap 64 and tap -1 are 0;
//   odd n    the same dword - the window of n - 1 - meets taps (65 - 2j, 64 - 2j): dword 0 is all zero;
//
// and a pair of outputs (n, n + 1), n even, runs over the same 33 dwords.  item() reads the 38 dwords that an item's six pairs
// cover once, with 8-byte LDS loads, into registers; the tap dwords are the same address in every lane (LDS broadcasts).  Per dword
// and output there are three dot products: Re z = sum br I - sum bi Q as two of them, with packings (br, 0) and (0, bi) - a single
// packing (br, -bi) cannot hold bi = -128, and any int8 tap is valid - and Im z as one with (bi, br).
//
// Every global read, of the rows and of the tail, happens before the workgroup's barrier - the rows and the tail are complete in LDS
// behind it - and every global write, the new tail from LDS among them, behind it.  The workgroup is the only one that touches the
// channel, so neither the tail nor an in-place update of the rows needs an order between workgroups.
#pragma once

#include "msk144_kernels.h"
#include "wave64.h"

namespace msk144
{
namespace fir64
{

constexpr int kThreads = 256;
constexpr int kRowBytes = 2 * kHopSamples;                          // 5184
constexpr int kRowVecs = kRowBytes / 16;                            // 324
constexpr int kTailBytes = 128;                                     // 2 zero bytes + 63 samples
constexpr int kTailVecs = kTailBytes / 16;
constexpr int kItemOutputs = 12;
constexpr int kPairs = kItemOutputs / 2;
constexpr int kRowItems = kHopSamples / kItemOutputs;               // 216
constexpr int kTapDwords = msk144wb::kFirTaps / 2 + 1;              // 33
constexpr int kWindowDwords = kTapDwords + kPairs - 1;              // 38
static_assert(kRowBytes % 16 == 0 && kHopSamples % kItemOutputs == 0 && kWindowDwords % 2 == 0 && (2 * kItemOutputs) % 8 == 0, "whole vectors, whole items");
static_assert(kTailBytes == 2 * (msk144wb::kFirTail + 1), "the tail row is 64 samples, the oldest one zero");

struct Lds
{
    uint4 x[kTailVecs + 2 * kRowVecs];  // the tail, then the row or rows
    uint4 t[kTapDwords][2];             // even n: (br, 0), (0, bi), (bi, br); odd n: the same three; two dwords unused
};

// Everything up to the new tail.  first_halves, hops: [channels][5184] bytes; taps[64][2]; tails[channels][128] bytes, taken as all
// zero with `restart`.  The workgroup's barrier is in here: what the caller writes to global memory it writes behind this call.
// row_vecs: the 16-byte words from one channel's row to the next in first_halves and in hops - 324 for the staged hops, 648 where
// the two are the halves of the hop ring's windows (audio.hip).
__device__ __forceinline__ void stage(Lds& s, const uint4* first_halves, const uint4* hops, int first, size_t ch, const int8_t* taps, int restart, uint4* tails,
                                      size_t row_vecs = kRowVecs)
{
    const int tid = threadIdx.x;
    const int nvec = first ? 2 * kRowVecs : kRowVecs;

    if(tid < kTailVecs) s.x[tid] = restart ? uint4{0, 0, 0, 0} : tails[ch * kTailVecs + tid];
    for(int i = tid; i < nvec; i += kThreads)
    {
        const bool head = first && i < kRowVecs;
        s.x[kTailVecs + i] = (head ? first_halves : hops)[ch * row_vecs + (first && !head ? i - kRowVecs : i)];
    }
    if(tid < kTapDwords)
    {
        // tap k as unsigned bytes, zero outside 0..63
        auto re = [&](int k) -> uint32_t { return k >= 0 && k < msk144wb::kFirTaps ? static_cast<uint8_t>(taps[2 * k]) : 0u; };
        auto im = [&](int k) -> uint32_t { return k >= 0 && k < msk144wb::kFirTaps ? static_cast<uint8_t>(taps[2 * k + 1]) : 0u; };
        const int e1 = 64 - 2 * tid, e2 = e1 - 1, o1 = e1 + 1, o2 = e1;
        uint4 a, b;
        a.x = re(e1) | (re(e2) << 16);
        a.y = (im(e1) << 8) | (im(e2) << 24);
        a.z = im(e1) | (re(e1) << 8) | (im(e2) << 16) | (re(e2) << 24);
        a.w = re(o1) | (re(o2) << 16);
        b.x = (im(o1) << 8) | (im(o2) << 24);
        b.y = im(o1) | (re(o1) << 8) | (im(o2) << 16) | (re(o2) << 24);
        b.z = b.w = 0;
        s.t[tid][0] = a;
        s.t[tid][1] = b;
    }
    __syncthreads();

    // the last 63 samples of the push, as the next push finds them
    if(tid < kTailVecs)
    {
        uint4 v = s.x[nvec + tid];
        if(tid == 0) v.x &= 0xffff0000u;
        tails[ch * kTailVecs + tid] = v;
    }
}

// Item `it`: its window d[], which starts at sample 12 it - 64 - byte 24 it, dwords 6 it .. 6 it + 37 (the last one of the last item
// ends the row) - and its 12 outputs, Re z[n0 + o] = ra[o] - rb[o], Im z[n0 + o] = zi[o].
__device__ __forceinline__ void item(const Lds& s, int it, uint32_t (&d)[kWindowDwords], int32_t (&ra)[kItemOutputs], int32_t (&rb)[kItemOutputs], int32_t (&zi)[kItemOutputs])
{
    const uint2* xw = reinterpret_cast<const uint2*>(s.x);
#pragma unroll
    for(int i = 0; i < kWindowDwords / 2; i++)
    {
        const uint2 v = xw[it * (kPairs / 2) + i];
        d[2 * i] = v.x;
        d[2 * i + 1] = v.y;
    }
#pragma unroll
    for(int o = 0; o < kItemOutputs; o++) ra[o] = rb[o] = zi[o] = 0;
#pragma unroll
    for(int j = 0; j < kTapDwords; j++)
    {
        const uint4 t0 = s.t[j][0], t1 = s.t[j][1];
#pragma unroll
        for(int p = 0; p < kPairs; p++)
        {
            const uint32_t x = d[j + p];
            ra[2 * p] = dot4(t0.x, x, ra[2 * p]);
            rb[2 * p] = dot4(t0.y, x, rb[2 * p]);
            zi[2 * p] = dot4(t0.z, x, zi[2 * p]);
            ra[2 * p + 1] = dot4(t0.w, x, ra[2 * p + 1]);
            rb[2 * p + 1] = dot4(t1.x, x, rb[2 * p + 1]);
            zi[2 * p + 1] = dot4(t1.y, x, zi[2 * p + 1]);
        }
    }
}

}  // namespace fir64
}  // namespace msk144
