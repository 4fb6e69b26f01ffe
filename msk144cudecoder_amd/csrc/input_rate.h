// Input-rate contract (include/msk144hip.h, "Audio input at 24 to 192 kHz") shared by the library (msk144_input_rate_api.cpp,
// resample.hip), the stream program and the host test library (host_capi.cpp): the rules a configuration must meet, the default
// integer taps, the tap packing the kernel reads, and the resampler itself in plain integers.  Header-only, plain C++ (no HIP).
#pragma once

#include "wideband.h"

namespace msk144ir
{

constexpr int64_t kMinRateHz = 24000;
constexpr int64_t kMaxRateHz = 192000;
constexpr int kDefaultShift = 14;
constexpr int kMinShift = 1, kMaxShift = 15;
constexpr int kMaxTapsPerPhase = msk144wb::kMaxTapsPerPhase;
constexpr int kDefaultTapsPerPhase = msk144wb::kDefaultTapsPerPhase;
constexpr int kBranchSumMax = 65535;  // sum over k of |h[r + kQ]|: then |acc| <= 65535 x 32768 = 2^31 - 32768, and the rounding term fits
constexpr int kHopOut = 2592, kFirstOut = 5184;
constexpr int kMaxHistory = kMaxTapsPerPhase * 16;  // H = ceil(K P / Q) - 1 < K x 16, as P/Q <= 16

// '' for a rate the resampler takes, else the refusal
inline std::string check_rate(int64_t rate_hz)
{
    char buf[200];
    if(rate_hz == msk144wb::kOutRate) return "input rate 12000 Hz needs no resampler: switch the option off";
    if(rate_hz < kMinRateHz || rate_hz > kMaxRateHz)
    {
        snprintf(buf, sizeof(buf), "input rate %lld Hz is outside %lld..%lld Hz", static_cast<long long>(rate_hz), static_cast<long long>(kMinRateHz), static_cast<long long>(kMaxRateHz));
        return buf;
    }
    if(rate_hz % msk144wb::kRateStepHz != 0)
    {
        snprintf(buf, sizeof(buf), "input rate %lld Hz is not a multiple of %d Hz (the 44.1 kHz family is not supported)", static_cast<long long>(rate_hz), msk144wb::kRateStepHz);
        return buf;
    }
    return "";
}

// The whole configuration: rate, shift, L = K P taps with 1 <= K <= 64, and the headroom rule on every polyphase branch
inline std::string check_config(int64_t rate_hz, int shift, int num_taps, const int16_t* taps)
{
    char buf[200];
    std::string why = check_rate(rate_hz);
    if(!why.empty()) return why;
    if(shift < kMinShift || shift > kMaxShift)
    {
        snprintf(buf, sizeof(buf), "shift %d is outside %d..%d", shift, kMinShift, kMaxShift);
        return buf;
    }
    const msk144wb::RateRatio rr = msk144wb::rate_ratio(rate_hz);
    if(num_taps < rr.P || num_taps % rr.P != 0 || num_taps / rr.P > kMaxTapsPerPhase)
    {
        snprintf(buf, sizeof(buf), "num_taps %d is not K x P with P = %d and 1 <= K <= %d", num_taps, rr.P, kMaxTapsPerPhase);
        return buf;
    }
    if(!taps) return "taps missing";
    for(int r = 0; r < rr.Q && r < num_taps; r++)
    {
        long long sum = 0;
        for(int k = r; k < num_taps; k += rr.Q) sum += std::abs(static_cast<int>(taps[k]));
        if(sum > kBranchSumMax)
        {
            snprintf(buf, sizeof(buf), "polyphase branch %d has sum |h| = %lld > %d: a 32-bit accumulator could overflow", r, sum, kBranchSumMax);
            return buf;
        }
    }
    return "";
}

// h[k] = rint(2^14 d[k]), d = msk144wb::design_taps_rate(rate, K); used with shift 14
inline std::vector<int16_t> default_taps(int64_t rate_hz, int K)
{
    const std::vector<double> d = msk144wb::design_taps_rate(rate_hz, K);
    std::vector<int16_t> h(d.size());
    for(size_t k = 0; k < d.size(); k++) h[k] = static_cast<int16_t>(std::rint(std::ldexp(d[k], kDefaultShift)));
    return h;
}

// The shape of a configuration
struct Shape
{
    int P = 0, Q = 0, L = 0;
    int H = 0;        // input samples kept per stream between hops: ceil(L/Q) - 1
    int row = 0;      // input samples of a hop: 2592 P/Q (a first hop has two rows)
    int dwords = 0;   // tap dwords per branch and packing: floor((H + 1) / 2) + 1
};

inline Shape shape(int64_t rate_hz, int num_taps)
{
    const msk144wb::RateRatio rr = msk144wb::rate_ratio(rate_hz);
    Shape s;
    s.P = rr.P;
    s.Q = rr.Q;
    s.L = num_taps;
    s.H = (num_taps + rr.Q - 1) / rr.Q - 1;
    s.row = kHopOut / rr.Q * rr.P;
    s.dwords = (s.H + 1) / 2 + 1;
    return s;
}

// The taps as resample.hip reads them: [Q][2][dwords] dwords of two int16 each (low half first).  Branch r's taps in the order of
// ascending input sample, c[j] = h[r + (H - j) Q] (0 beyond L) meets x[n - H + j], j = 0..H.  Packing 0 is c[0], c[1], ... for a
// window that starts on a dword of the staged samples; packing 1 is 0, c[0], c[1], ... for one that starts on the odd half of a dword.
// Both are padded with zeros to 2 x dwords entries.
inline std::vector<uint32_t> pack_taps(const Shape& s, const int16_t* h)
{
    std::vector<uint32_t> g(static_cast<size_t>(s.Q) * 2 * s.dwords, 0u);
    for(int r = 0; r < s.Q; r++)
        for(int odd = 0; odd < 2; odd++)
        {
            uint32_t* out = g.data() + (static_cast<size_t>(r) * 2 + odd) * s.dwords;
            for(int j = 0; j <= s.H; j++)
            {
                const int k = r + (s.H - j) * s.Q;
                const uint32_t c = k < s.L ? static_cast<uint16_t>(h[k]) : 0u;
                const int e = j + odd;
                out[e / 2] |= c << (16 * (e & 1));
            }
        }
    return g;
}

// One output from its accumulator: (acc + 2^(s-1)) >> s, floor, clamped to int16
inline int16_t round_clamp(int32_t acc, int shift, int32_t* clamped)
{
    int32_t v = (acc + (1 << (shift - 1))) >> shift;
    if(v > 32767 || v < -32768)
    {
        v = v > 32767 ? 32767 : -32768;
        ++*clamped;
    }
    return static_cast<int16_t>(v);
}

// The resampler of every stream of a handle, in the integers of the contract (what input_rate.Resampler computes in int64 numpy)
struct Resampler
{
    Shape s;
    int shift = kDefaultShift;
    std::vector<int16_t> h;
    std::vector<int16_t> hist;  // [channels][H]: the last H input samples, oldest first
    std::vector<uint8_t> started;

    Resampler(int channels, int64_t rate_hz, const int16_t* taps, int num_taps, int shift_) : s(shape(rate_hz, num_taps)), shift(shift_), h(taps, taps + num_taps)
    {
        hist.assign(static_cast<size_t>(channels) * std::max(s.H, 1), 0);
        started.assign(static_cast<size_t>(channels), 0);
    }

    // One stream's hop: x holds 2 rows for a first hop (the stream restarts from zero history), else one; y gets 5184 or 2592
    // samples.  Returns the number of clamped outputs, or -1 for a later hop before a first one.
    int push(int stream, const int16_t* x, bool first, int16_t* y)
    {
        if(!first && !started[static_cast<size_t>(stream)]) return -1;
        int16_t* hs = hist.data() + static_cast<size_t>(stream) * std::max(s.H, 1);
        if(first) std::fill(hs, hs + s.H, 0);
        started[static_cast<size_t>(stream)] = 1;
        const int M = first ? kFirstOut : kHopOut;
        const int N = first ? 2 * s.row : s.row;
        int32_t clamped = 0;
        for(int m = 0; m < M; m++)
        {
            const long long mp = static_cast<long long>(m) * s.P;
            const int n = static_cast<int>(mp / s.Q), r = static_cast<int>(mp % s.Q);
            int32_t acc = 0;
            for(int k = 0; r + k * s.Q < s.L; k++)
            {
                const int i = n - k;
                const int32_t xv = i >= 0 ? x[i] : hs[s.H + i];
                acc += static_cast<int32_t>(h[static_cast<size_t>(r + k * s.Q)]) * xv;
            }
            y[m] = round_clamp(acc, shift, &clamped);
        }
        for(int i = 0; i < s.H; i++) hs[i] = x[N - s.H + i];  // H is shorter than a row
        return clamped;
    }
};

}  // namespace msk144ir
