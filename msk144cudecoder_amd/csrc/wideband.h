// Wideband channeliser contract shared by the library (msk144_wideband_api.cpp, channelise.hip), the stream program (main.cpp) and the
// host test library (host_capi.cpp): the rules a wideband configuration must meet and the default prototype filter.
// Header-only, plain C++ (no HIP), so that every one of those builds gets the same taps and the same checks.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

namespace msk144wb
{

constexpr int kOutRate = 12000;        // channel output rate, samples per second
constexpr int kMinDecimation = 2;
constexpr int kMaxDecimation = 512;
constexpr int kRateStepHz = 125;       // Fs = 12000 P/Q: a multiple of 125 Hz, so that a 2592-sample hop is 27 Fs/125 inputs
constexpr int64_t kMinRateHz = static_cast<int64_t>(kMinDecimation) * 12000;
constexpr int64_t kMaxRateHz = static_cast<int64_t>(kMaxDecimation) * 12000;
constexpr int kMaxTapsPerPhase = 64;   // K; L = K*D taps
constexpr int kDefaultTapsPerPhase = 16;
constexpr float kDefaultGain = 100.0f; // the `csdr gain_ff 100` stage of a CPU decimation chain
constexpr float kMaxGain = 1e36f;      // the device scales by 128 x gain in f32: finite up to about 2.66e38 / 128
constexpr int kGuardHz = 6000;         // |f_c| <= Fs/2 - 6000
constexpr double kPassHz = 4000.0;     // design band edges of the default filter
constexpr double kStopHz = 8000.0;
constexpr double kKaiserBeta = 7.0;    // about 70 dB side lobes

// Two-stage bank above 6.144 Msps: a 64-band, 2x oversampled analysis bank (decimation 32) in front of the channeliser, which then
// runs at the sub-band rate Fs/32 on each channel's band
constexpr int kBankBands = 64;
constexpr int kBankDecimation = 32;
constexpr int kBankRateStepHz = 8000;  // Fs/64 a multiple of 125, Fs/32 a multiple of 250 with Q dividing 96
constexpr int64_t kMaxBankRateHz = 61440000;
constexpr int kDefaultBankTapsPerBand = 8;  // K1; L1 = 64 K1 taps
constexpr int kMaxBankTapsPerBand = 16;
constexpr double kBankKaiserBeta = 8.0;     // about 80 dB side lobes

enum Format
{
    kCu8 = 0,   // rtl_sdr: (u - 127.5) / 128
    kCs8 = 1,   // s / 128
    kCs16 = 2   // s / 32768
};

inline int sample_bytes(int format) { return format == kCs16 ? 4 : 2; }

inline double bessel_i0(double x)
{
    double sum = 1.0, term = 1.0;
    const double q = 0.25 * x * x;
    for(int k = 1; k < 200; k++)
    {
        term *= q / (static_cast<double>(k) * k);
        sum += term;
        if(term < 1e-17 * sum) break;
    }
    return sum;
}

// Kaiser-windowed sinc of L taps with its cut-off at fc cycles per sample, scaled to unit DC gain.  Symmetric about (L-1)/2.
inline std::vector<double> kaiser_sinc(int L, double fc, double beta)
{
    const double mid = 0.5 * (L - 1);
    const double i0b = bessel_i0(beta);
    std::vector<double> h(static_cast<size_t>(L));
    double sum = 0.0;
    for(int k = 0; k < L; k++)
    {
        const double t = k - mid;
        const double arg = 2.0 * fc * t;
        const double sinc = std::fabs(arg) < 1e-12 ? 1.0 : std::sin(M_PI * arg) / (M_PI * arg);
        const double r = L > 1 ? t / mid : 0.0;
        const double w = bessel_i0(beta * std::sqrt(std::fmax(0.0, 1.0 - r * r))) / i0b;
        h[static_cast<size_t>(k)] = sinc * w;
        sum += h[static_cast<size_t>(k)];
    }
    for(double& v : h) v /= sum;
    return h;
}

// Default prototype low-pass, L = K*D taps at Fs = D*12000 (for a rational rate 12000 P/Q: D = P, at the upsampled rate; see
// design_taps_rate): a Kaiser-windowed sinc (beta 7) with its cut-off half way between the 4 kHz pass edge and the 8 kHz stop edge.
inline std::vector<double> design_taps(int D, int K)
{
    const double fs = static_cast<double>(D) * kOutRate;
    return kaiser_sinc(K * D, 0.5 * (kPassHz + kStopHz) / fs, kKaiserBeta);
}

// Fs / 12000 = P/Q in lowest terms (Q = 1: the integer decimation D = P).  Q divides 96 for every rate that check_config accepts.
struct RateRatio
{
    int P = 0, Q = 0;
};

inline RateRatio rate_ratio(int64_t rate_hz)
{
    const int64_t g = std::gcd(rate_hz, static_cast<int64_t>(kOutRate));
    return RateRatio{static_cast<int>(rate_hz / g), static_cast<int>(kOutRate / g)};
}

// The default prototype for Fs = 12000 P/Q: design_taps(P, K) - the same Kaiser-sinc at the upsampled rate Q Fs = 12000 P, L = K P
// taps - scaled to sum to Q, so that each of the Q polyphase branches h[r], h[r + Q], ... has about unit DC gain.  Q = 1 is
// design_taps(D, K) exactly.
inline std::vector<double> design_taps_rate(int64_t rate_hz, int K)
{
    const RateRatio rr = rate_ratio(rate_hz);
    std::vector<double> h = design_taps(rr.P, K);
    if(rr.Q > 1)
        for(double& v : h) v *= rr.Q;
    return h;
}

// A rate above 6.144 Msps that the two-stage bank takes: a multiple of 8000 Hz up to 61.44 Msps
inline bool is_bank_rate(int64_t rate_hz)
{
    return rate_hz > kMaxRateHz && rate_hz <= kMaxBankRateHz && rate_hz % kBankRateStepHz == 0;
}

// The rate the channeliser runs at: Fs itself, or the sub-band rate Fs/32 behind the bank
inline int64_t stage2_rate(int64_t rate_hz)
{
    return is_bank_rate(rate_hz) ? rate_hz / kBankDecimation : rate_hz;
}

// Band of channel offset f_c at a bank rate: k = floor((64 f_c + Fs/2) / Fs), -32..32 for |f_c| <= Fs/2 (band 32 is band -32); the
// residual offset f_c - k Fs/64 is an integer with |f_c - k Fs/64| <= Fs/128
inline int bank_band(int64_t rate_hz, int64_t f_hz)
{
    const int64_t num = kBankBands * f_hz + rate_hz / 2;
    return static_cast<int>(num >= 0 ? num / rate_hz : -((-num + rate_hz - 1) / rate_hz));
}

inline int64_t bank_residual(int64_t rate_hz, int64_t f_hz)
{
    return f_hz - static_cast<int64_t>(bank_band(rate_hz, f_hz)) * (rate_hz / kBankBands);
}

// Default analysis-bank prototype, L1 = 64 K1 taps at Fs: a Kaiser-windowed sinc (beta 8) with its cut-off half way between the
// pass edge Fs/128 + 4 kHz (a channel's 4 kHz pass band at the largest residual offset) and the stop edge 3 Fs/128 - 8 kHz (what
// the decimation by 32 folds onto a channel's 8 kHz stop edge), scaled to unit DC gain.  Symmetric about (L1-1)/2.
inline std::vector<double> design_bank_taps(int64_t rate_hz, int K1)
{
    const double fs = static_cast<double>(rate_hz);
    return kaiser_sinc(kBankBands * K1, 0.5 * ((fs / 128.0 + kPassHz) + (3.0 * fs / 128.0 - kStopHz)) / fs, kBankKaiserBeta);
}

// ---- per-channel levels and the stepped AGC (msk144_set_wideband_gains, msk144_set_wideband_agc, msk144_wideband_levels) ----

#ifdef __HIP__
#define MSK144WB_HD __host__ __device__
#else
#define MSK144WB_HD
#endif

// msk144_wideband_agc, field for field.  The defaults are design parameters, not measurements: a window of 8 .. 32 LSB rms per
// component (Gaussian noise at 32 LSB rms clips below 100 ppm), 0.1 % clipped components, 4 quiet pushes (about 0.9 s) before a
// step up, +-20 steps of 6 dB.
struct AgcParams
{
    int32_t lo_sq = 64, hi_sq = 1024;
    int32_t clip_ppm = 1000;
    int32_t hold = 4;
    int32_t min_exp = -20, max_exp = 20;
};

// One channel's statistics of a push live in one 64-bit word, so that one atomic per channel, half-wave and tile carries both:
// sum_sq (< 2^28 per push) in the low half, clipped components (<= 10368) in the high half.
MSK144WB_HD inline uint64_t pack_level(uint32_t sum_sq, uint32_t clipped) { return static_cast<uint64_t>(sum_sq) | (static_cast<uint64_t>(clipped) << 32); }
MSK144WB_HD inline int64_t level_sum_sq(uint64_t w) { return static_cast<int64_t>(w & 0xffffffffull); }
MSK144WB_HD inline int64_t level_clipped(uint64_t w) { return static_cast<int64_t>(w >> 32); }

// The step rule, once: after a push of n complex outputs with S = sum of I^2 + Q^2 over the stored int8 values and k clipped
// components, channel state (e, quiet) moves one 6 dB step down at once (too many clipped, or above the window), one step up after
// `hold` pushes in a row below the window.  Only integers decide (64-bit products), so the trajectory is a pure function of the
// reported statistics; hi_sq > 4 lo_sq (a step multiplies the power by 4) rules out a limit cycle on a stationary channel.
MSK144WB_HD inline void agc_step(const AgcParams& p, int64_t n, int64_t S, int64_t k, int32_t& e, int32_t& quiet)
{
    if(k * 1000000 > static_cast<int64_t>(p.clip_ppm) * 2 * n || S > static_cast<int64_t>(p.hi_sq) * 2 * n)
    {
        e = e - 1 > p.min_exp ? e - 1 : p.min_exp;
        quiet = 0;
    }
    else if(S < static_cast<int64_t>(p.lo_sq) * 2 * n)
    {
        if(++quiet >= p.hold)
        {
            e = e + 1 < p.max_exp ? e + 1 : p.max_exp;
            quiet = 0;
        }
    }
    else quiet = 0;
}

// the scale a channel with base gain g is quantised with at exponent e: a 6 dB ladder is exact in f32
MSK144WB_HD inline float agc_scale(float g, int32_t e) { return ldexpf(128.0f * g, e); }

// The rules of msk144_set_wideband_agc that need no handle.  Empty string = valid.
inline std::string check_agc(const AgcParams& p)
{
    if(p.lo_sq < 0 || static_cast<int64_t>(p.hi_sq) <= 4 * static_cast<int64_t>(p.lo_sq))
        return "AGC window needs 0 <= lo_sq and hi_sq > 4 x lo_sq (one 6 dB step multiplies the power by 4)";
    if(p.clip_ppm < 0) return "AGC clip_ppm must not be negative";
    if(p.hold < 1) return "AGC hold must be at least 1 push";
    if(p.min_exp > p.max_exp) return "AGC needs min_exp <= max_exp";
    if(p.min_exp < -126 || p.max_exp > 126) return "AGC exponents must lie within -126..126";
    return std::string();
}

// a per-channel gain the quantiser takes at every exponent up to max_exp: 0 < g, and 128 g 2^max_exp finite in f32 (an infinite
// scale would turn an exact 0 into NaN)
inline bool gain_ok(float g, int32_t max_exp) { return g > 0.0f && std::isfinite(g) && std::isfinite(agc_scale(g, max_exp)); }

// ---- impulse-noise blanker on the input stream (msk144_set_wideband_blanker, msk144_wideband_blanker_stats) ----

constexpr int kBlankerMinThresholdQ4 = 16;  // 1 x mean power
constexpr int kBlankerMaxThresholdQ4 = 65535;
constexpr int kBlankerMaxGuard = 4096;      // pre, post: samples; a push has at least 5184, so a guard owes to the next push at most

// msk144_wideband_blanker, field for field.  The defaults are design parameters, not measurements: 16 x the push's mean power
// (complex Gaussian noise exceeds it with probability e^-16 per sample), 2 samples blanked ahead of a hit and 8 behind it.
struct BlankerParams
{
    int32_t threshold_q4 = 256;
    int32_t pre = 2, post = 8;
};

// The threshold of a push, once: N samples whose powers cI^2 + cQ^2 (integer component units of the input format) sum to S give
// T = (floor(S / N) x threshold_q4) >> 4, and a sample is a hit iff its power exceeds T.  S <= 2^56 and floor(S / N) <= 2^31, so
// unsigned 64 bits hold every step.
MSK144WB_HD inline uint64_t blanker_threshold(uint64_t S, uint64_t N, uint32_t threshold_q4) { return ((S / N) * threshold_q4) >> 4; }

// The rules of msk144_set_wideband_blanker that need no handle.  Empty string = valid.
inline std::string check_blanker(const BlankerParams& p)
{
    if(p.threshold_q4 < kBlankerMinThresholdQ4 || p.threshold_q4 > kBlankerMaxThresholdQ4) return "blanker threshold_q4 must lie within 16..65535 (1 .. 4095.94 x mean power)";
    if(p.pre < 0 || p.pre > kBlankerMaxGuard || p.post < 0 || p.post > kBlankerMaxGuard) return "blanker guards pre and post must lie within 0..4096 samples";
    return std::string();
}

// ---- power spectrum of the input stream (msk144_set_wideband_spectrum, msk144_wideband_spectrum) ----

constexpr int kSpectrumMinBins = 256;   // B, a power of two
constexpr int kSpectrumMaxBins = 8192;
constexpr int kSpectrumDefaultBins = 1024;

// the default window, periodic Hann: w[i] = 0.5 - 0.5 cos(2 pi i / B)
inline std::vector<double> spectrum_window(int B)
{
    std::vector<double> w(static_cast<size_t>(B));
    for(int i = 0; i < B; i++) w[static_cast<size_t>(i)] = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / B);
    return w;
}

// The rules of msk144_set_wideband_spectrum: B a power of two within 256..8192 and no longer than a later push of hop_samples
// input samples, every window value finite (window NULL: the default).  Empty string = valid.
inline std::string check_spectrum(int B, const double* window, int64_t hop_samples)
{
    if(B < kSpectrumMinBins || B > kSpectrumMaxBins || (B & (B - 1)) != 0) return "spectrum bins must be a power of two within 256..8192";
    if(B > hop_samples) return "spectrum bins exceed the " + std::to_string(hop_samples) + " input samples of a push at this rate";
    for(int i = 0; window && i < B; i++)
        if(!std::isfinite(window[i])) return "spectrum window value " + std::to_string(i) + " is not finite";
    return std::string();
}

// ---- per-channel ping detection (msk144_set_wideband_pings, msk144_wideband_pings) ----

constexpr int kPingBlock = 96;        // B: samples per block, 8 ms; a 72 ms frame is 9 blocks
constexpr int kPingMaxBlocks = 54;    // nb of a first push (5184 / 96); a later push has 27
constexpr int kHopBlocks = 27;        // a hop is 27 blocks
constexpr int kPingEnergyBits = 22;   // E <= 96 x 2 x 128^2 = 3145728 < 2^22
constexpr int kPingMaxMemory = 16;
constexpr int kPingMinRatioQ4 = 16;   // 1 x the reference
constexpr int kPingMaxRatioQ4 = 65535;
constexpr int kPingMaxMinRef = 1 << kPingEnergyBits;
constexpr int kPingDefaultMinBlocks = 2;  // the event rule's, a parameter of the program and the model
constexpr int kPingMaxMinBlocks = 64;

// msk144_wideband_pings_params, field for field.  The defaults are design parameters, not measurements: 2.0 x the reference, the
// quiet levels of 8 earlier pushes (about 1.7 s), and a floor of 1 LSB^2 per sample under the reference.
struct PingParams
{
    int32_t ratio_q4 = 32;
    int32_t memory = 8;
    int32_t min_ref = 96;
};

// msk144_wideband_ping, field for field: what the kernel writes
struct PingRecord
{
    uint64_t up_mask;
    int32_t blocks, history, quiet, reference, peak, peak_block;
};
static_assert(sizeof(PingRecord) == 32, "msk144_wideband_ping is 32 bytes");

// A channel's memory on the device: the quiet levels of its last pushes (a ring of 16, the next one goes to q[pos]), how many of
// them belong to the running history (at most 16), and the scale the last push was quantised with.
struct PingHistory
{
    int32_t q[kPingMaxMemory];
    int32_t count, pos;
    float scale;
    int32_t reserved;
};

// the rank, counted from 0 in ascending order, of the quiet level among the nb block energies of a push: a lower quartile
MSK144WB_HD inline int ping_rank(int nb) { return nb / 4; }

// The history rule, once.  `restart`: a first push, or the first one after msk144_set_wideband_pings; a scale other than the last
// push's restarts the history as well.  Returns the minimum of q and the quiet levels of the h earlier pushes that count.
MSK144WB_HD inline int32_t ping_history_min(const PingHistory& s, bool restart, float scale, int32_t memory, int32_t q, int32_t& h)
{
    const int32_t n = restart || s.scale != scale ? 0 : s.count;
    h = n < memory ? n : memory;
    int32_t m = q;
    for(int32_t i = 1; i <= h; i++)
    {
        const int32_t v = s.q[(s.pos - i) & (kPingMaxMemory - 1)];
        m = v < m ? v : m;
    }
    return m;
}

// ... and the push's own quiet level joins the history behind it
MSK144WB_HD inline void ping_history_put(PingHistory& s, bool restart, float scale, int32_t q)
{
    if(restart || s.scale != scale) s.count = s.pos = 0;
    s.q[s.pos] = q;
    s.pos = (s.pos + 1) & (kPingMaxMemory - 1);
    s.count = s.count < kPingMaxMemory ? s.count + 1 : kPingMaxMemory;
    s.scale = scale;
}

// R = max(min(q, history), min_ref), and the up rule: E x 16 > R x ratio_q4, strictly, in 64 bits
MSK144WB_HD inline int32_t ping_reference(int32_t history_min, int32_t min_ref) { return history_min > min_ref ? history_min : min_ref; }
MSK144WB_HD inline bool ping_up(int32_t E, int32_t R, int32_t ratio_q4) { return static_cast<int64_t>(E) * 16 > static_cast<int64_t>(R) * ratio_q4; }

// The rules of msk144_set_wideband_pings that need no handle.  Empty string = valid.
inline std::string check_pings(const PingParams& p)
{
    if(p.ratio_q4 < kPingMinRatioQ4 || p.ratio_q4 > kPingMaxRatioQ4) return "ping ratio_q4 must lie within 16..65535 (1 .. 4095.94 x the reference)";
    if(p.memory < 0 || p.memory > kPingMaxMemory) return "ping memory must lie within 0..16 pushes";
    if(p.min_ref < 1 || p.min_ref > kPingMaxMinRef) return "ping min_ref must lie within 1..4194304";
    return std::string();
}

// One push of one channel on the host, from its nb block energies: the record the kernel writes (the radix select there and the
// sort here pick the same value).  What libmsk144host.so holds the Python model to.
inline PingRecord ping_record(const PingParams& p, PingHistory& s, bool restart, float scale, const int32_t* E, int nb)
{
    std::vector<int32_t> sorted(E, E + nb);
    std::sort(sorted.begin(), sorted.end());
    PingRecord r{};
    r.blocks = nb;
    r.quiet = sorted[static_cast<size_t>(ping_rank(nb))];
    r.reference = ping_reference(ping_history_min(s, restart, scale, p.memory, r.quiet, r.history), p.min_ref);
    ping_history_put(s, restart, scale, r.quiet);
    r.peak = E[0];
    for(int b = 0; b < nb; b++)
    {
        if(ping_up(E[b], r.reference, p.ratio_q4)) r.up_mask |= 1ull << b;
        if(E[b] > r.peak) r.peak = E[b], r.peak_block = b;
    }
    return r;
}

// ---- the 64-tap complex int8 FIR on a channel's stored samples, behind the ping band and the notch (the kernels': csrc/fir64.h) ----

constexpr int kFirTaps = 64, kFirTail = kFirTaps - 1;   // the tail: the stored samples a channel keeps between pushes

// 64 complex int8 taps (br, bi) and a shift: msk144_wideband_ping_band_params and msk144_wideband_notch_params, field for field
struct FirParams
{
    int8_t taps[kFirTaps][2];
    int32_t shift;
};

// (re, im) += gain x B(f), B(f) = sum b[k] e^{-j 2 pi f k / 12000} of the integer taps, term by term in ascending k
inline void fir_response_add(const FirParams& p, double f_hz, double gain, double& re, double& im)
{
    for(int k = 0; k < kFirTaps; k++)
    {
        const double a = -2.0 * M_PI * f_hz * k / kOutRate, c = std::cos(a), s = std::sin(a);
        re += gain * (p.taps[k][0] * c - p.taps[k][1] * s);
        im += gain * (p.taps[k][0] * s + p.taps[k][1] * c);
    }
}

// h[N]: a Hamming-windowed sinc low-pass with cutoff halfwidth_hz, centred on k = mid, unscaled
inline void hamming_sinc(int N, double mid, int halfwidth_hz, double* h)
{
    for(int k = 0; k < N; k++)
    {
        const double arg = 2.0 * halfwidth_hz * (k - mid) / kOutRate;
        const double sinc = std::fabs(arg) < 1e-12 ? 1.0 : std::sin(M_PI * arg) / (M_PI * arg);
        h[k] = sinc * (0.54 - 0.46 * std::cos(2.0 * M_PI * k / (N - 1)));
    }
}

// The filter on the host, for one channel and one push: x[n][2] the n stored int8 samples of the push, tail[63][2] the channel's 63
// stored samples before them, oldest first.  Leaves the joined stream in s[63 + n][2], so that x[m - k] is s[63 + m - k], returns
// z[n][2], z[m] = sum_k b[k] x[m - k] in int32 (|Re z|, |Im z| <= 2^21), and moves the tail on to the last 63 samples of x.
inline std::vector<int32_t> fir_push(const FirParams& p, const int8_t* x, int n, int8_t* tail, std::vector<int8_t>& s)
{
    s.assign(tail, tail + 2 * kFirTail);
    s.insert(s.end(), x, x + 2 * n);
    std::vector<int32_t> z(static_cast<size_t>(2 * n), 0);
    for(int m = 0; m < n; m++)
        for(int k = 0; k < kFirTaps; k++)
        {
            const int32_t xr = s[static_cast<size_t>(2 * (kFirTail + m - k))], xi = s[static_cast<size_t>(2 * (kFirTail + m - k) + 1)];
            z[static_cast<size_t>(2 * m)] += p.taps[k][0] * xr - p.taps[k][1] * xi;
            z[static_cast<size_t>(2 * m + 1)] += p.taps[k][0] * xi + p.taps[k][1] * xr;
        }
    std::copy(s.end() - 2 * kFirTail, s.end(), tail);
    return z;
}

// ---- the ping band: an in-band filter ahead of the block energies (msk144_set_wideband_ping_band) ----

constexpr int kPingBandTaps = kFirTaps, kPingBandTail = kFirTail;
constexpr int kPingBandMaxShift = 40;
constexpr int32_t kPingBandMaxEnergy = (1 << kPingEnergyBits) - 1;
constexpr int kPingBandMinHalfwidthHz = 500;
constexpr int kPingBandMaxHalfwidthHz = 3000;
constexpr int kPingBandDefaultHalfwidthHz = 1500;
// The detector's default ratio with the default band on, in sixteenths: the smallest multiple of 0.25 with no noise block up in
// the CPU simulation that include/msk144hip.h tabulates
constexpr int kPingBandDefaultRatioQ4 = 52;

using PingBandParams = FirParams;
static_assert(sizeof(PingBandParams) == 132, "msk144_wideband_ping_band_params is 132 bytes");

// The rules of msk144_set_wideband_ping_band that need no handle: any int8 taps.  Empty string = valid.
inline std::string check_ping_band(const PingBandParams& p)
{
    if(p.shift < 0 || p.shift > kPingBandMaxShift) return "ping band shift must lie within 0..40";
    return std::string();
}

// The rules of the default design.  Empty string = valid.
inline std::string check_ping_band_design(int centre_hz, int halfwidth_hz)
{
    if(halfwidth_hz < kPingBandMinHalfwidthHz || halfwidth_hz > kPingBandMaxHalfwidthHz) return "ping band half-width must lie within 500..3000 Hz";
    if(std::abs(static_cast<long long>(centre_hz)) + halfwidth_hz > kOutRate / 2) return "ping band must lie within +-6000 Hz: |centre| + half-width <= 6000";
    return std::string();
}

// |B(f)|^2 of the integer taps
inline double ping_band_response(const PingBandParams& p, double f_hz)
{
    double re = 0.0, im = 0.0;
    fir_response_add(p, f_hz, 1.0, re, im);
    return re * re + im * im;
}

// The default design, in double: a Hamming-windowed sinc low-pass with cutoff halfwidth_hz centred on k = 31.5, turned to centre_hz,
// scaled so that the largest |component| is 127 and rounded; shift = rint(log2 |B(centre)|^2) of the rounded taps, so that a signal
// inside the band comes out at about the level it went in with.  The caller has checked the arguments.
inline PingBandParams ping_band_design(int centre_hz, int halfwidth_hz)
{
    constexpr double mid = 0.5 * (kPingBandTaps - 1);
    double h[kPingBandTaps], re[kPingBandTaps], im[kPingBandTaps], top = 0.0;
    hamming_sinc(kPingBandTaps, mid, halfwidth_hz, h);
    for(int k = 0; k < kPingBandTaps; k++)
    {
        const double a = 2.0 * M_PI * centre_hz * (k - mid) / kOutRate;
        re[k] = h[k] * std::cos(a);
        im[k] = h[k] * std::sin(a);
        top = std::max(top, std::max(std::fabs(re[k]), std::fabs(im[k])));
    }
    PingBandParams p{};
    for(int k = 0; k < kPingBandTaps; k++)
    {
        p.taps[k][0] = static_cast<int8_t>(std::rint(re[k] * 127.0 / top));
        p.taps[k][1] = static_cast<int8_t>(std::rint(im[k] * 127.0 / top));
    }
    p.shift = static_cast<int32_t>(std::rint(std::log2(ping_band_response(p, centre_hz))));
    return p;
}

// The filter and its energies on the host, for one channel and one push: x[n][2] the n stored int8 samples of the push (n a multiple
// of 96), tail[63][2] the channel's 63 stored samples before them, oldest first (all zero where the ping kernel restarts); writes
// Ef[n / 96] and moves the tail on to the last 63 samples of x.  With fir_push's z, Ef[b] = min((sum over the block of Re z^2 +
// Im z^2) >> shift, 2^22 - 1) in 64 bits.  What libmsk144host.so holds the Python model and the kernel (pingband.hip) to.
inline void ping_band_energies(const PingBandParams& p, const int8_t* x, int n, int8_t* tail, int32_t* Ef)
{
    std::vector<int8_t> s;
    const std::vector<int32_t> z = fir_push(p, x, n, tail, s);
    for(int b = 0; b < n / kPingBlock; b++)
    {
        uint64_t sum = 0;
        for(size_t i = static_cast<size_t>(2 * b * kPingBlock); i < static_cast<size_t>(2 * (b + 1) * kPingBlock); i++) sum += static_cast<uint64_t>(static_cast<int64_t>(z[i]) * z[i]);
        sum >>= p.shift;
        Ef[b] = sum > static_cast<uint64_t>(kPingBandMaxEnergy) ? kPingBandMaxEnergy : static_cast<int32_t>(sum);
    }
}

// An event: a maximal run of consecutive up blocks of one channel in g = (blocks of all earlier pushes) + b
struct PingEvent
{
    int32_t channel;
    int64_t start, blocks;  // in blocks of 8 ms
    int32_t peak;           // the largest E of the run (at its lowest g on a tie) ...
    int32_t reference;      // ... and the R of the push that block lay in
};

// The event rule, once.  A run that reaches a push's last block stays open into the next push; a history restart does not close
// it; close() (the end of the stream) does.  An event is reported when it closes, if it has at least min_blocks blocks: by push,
// then by channel, then by start.  Host only: the program's log and, through libmsk144host.so, the yardstick of the Python model.
class PingTracker
{
public:
    PingTracker(int channels, int min_blocks) : min_blocks_(min_blocks), open_(static_cast<size_t>(channels)), count_(static_cast<size_t>(channels), 0), up_(static_cast<size_t>(channels), 0) {}

    // records[channels] of one push and its block energies [channels][kPingMaxBlocks]
    void push(const PingRecord* records, const int32_t* energies, std::vector<PingEvent>& out)
    {
        int nb = 0;
        for(size_t c = 0; c < open_.size(); c++)
        {
            const PingRecord& r = records[c];
            const int32_t* E = energies + c * kPingMaxBlocks;
            Run& o = open_[c];
            nb = r.blocks;
            for(int b = 0; b < r.blocks; b++)
            {
                if((r.up_mask >> b) & 1)
                {
                    if(!o.blocks) o = Run{base_ + b, 0, E[b], r.reference};
                    else if(E[b] > o.peak) o.peak = E[b], o.reference = r.reference;
                    o.blocks++;
                    up_[c]++;
                }
                else finish(static_cast<int32_t>(c), out);
            }
            total_ += r.blocks;
        }
        base_ += nb;
    }

    void close(std::vector<PingEvent>& out)
    {
        for(size_t c = 0; c < open_.size(); c++) finish(static_cast<int32_t>(c), out);
    }

    int64_t events() const { return events_; }
    int64_t up_blocks() const { return std::accumulate(up_.begin(), up_.end(), static_cast<int64_t>(0)); }
    int64_t total_blocks() const { return total_; }
    const std::vector<int64_t>& channel_events() const { return count_; }  // reported events per channel
    const std::vector<int64_t>& channel_up_blocks() const { return up_; }

private:
    struct Run
    {
        int64_t start = 0, blocks = 0;
        int32_t peak = 0, reference = 0;
    };

    void finish(int32_t c, std::vector<PingEvent>& out)
    {
        Run& o = open_[static_cast<size_t>(c)];
        if(o.blocks >= min_blocks_)
        {
            out.push_back(PingEvent{c, o.start, o.blocks, o.peak, o.reference});
            count_[static_cast<size_t>(c)]++;
            events_++;
        }
        o.blocks = 0;
    }

    int64_t min_blocks_;
    int64_t base_ = 0, total_ = 0, events_ = 0;
    std::vector<Run> open_;
    std::vector<int64_t> count_, up_;
};

// One line of the event log (--wideband-pings=FILE).  start and dur are block counts x 8 ms, exact in three decimals.
inline std::string ping_event_line(const PingEvent& e, int32_t offset_hz)
{
    char buf[256];
    const long long s = static_cast<long long>(e.start) * 8, d = static_cast<long long>(e.blocks) * 8;
    snprintf(buf, sizeof(buf), "ping ch=%d offset=%d start=%lld.%03lld dur=%lld.%03lld blocks=%lld peak=%d ref=%d peak_db=%.1f", e.channel, offset_hz, s / 1000, s % 1000,
             d / 1000, d % 1000, static_cast<long long>(e.blocks), e.peak, e.reference, 10.0 * std::log10(static_cast<double>(e.peak) / static_cast<double>(e.reference)));
    return buf;
}

// ---- per-channel waterfall (msk144_set_wideband_waterfall, msk144_wideband_waterfall, msk144_wideband_waterfall_sums) ----

constexpr int kWaterfallBins = kPingBlock;   // one 96-point transform per block of the ping detector: 125 Hz per bin
constexpr int kWaterfallRows = kPingMaxBlocks;
constexpr double kWaterfallFloor = 1e-10;    // -100 dB under a tone of 1 LSB on a bin centre
constexpr double kWaterfallCarrierDb = 10.0; // the summary's carrier rule; a design parameter, not a measurement
constexpr int kWaterfallMaxListed = 16;      // channels of --wideband-waterfall=FILE:c0,c1,...
constexpr int kWaterfallHandful = 4;         // up to this many channels are read one by one, more in one copy of all

// the default window, periodic Hann: w[i] = 0.5 - 0.5 cos(2 pi i / 96)
inline std::vector<double> waterfall_window()
{
    std::vector<double> w(static_cast<size_t>(kWaterfallBins));
    for(int i = 0; i < kWaterfallBins; i++) w[static_cast<size_t>(i)] = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / kWaterfallBins);
    return w;
}

// The rule of msk144_set_wideband_waterfall that needs no handle: every window value finite (NULL: the default).  Empty string = valid.
inline std::string check_waterfall(const double* window)
{
    for(int i = 0; window && i < kWaterfallBins; i++)
        if(!std::isfinite(window[i])) return "waterfall window value " + std::to_string(i) + " is not finite";
    return std::string();
}

// 0 dB of the program's output: (sum w)^2 of the window the device holds, rounded to f32 (NULL: the default)
inline double waterfall_full(const double* window)
{
    const std::vector<double> hann = window ? std::vector<double>() : waterfall_window();
    const double* w = window ? window : hann.data();
    double sum = 0.0;
    for(int i = 0; i < kWaterfallBins; i++) sum += static_cast<double>(static_cast<float>(w[i]));
    return sum * sum;
}

// 10 log10(max(P / (sum w)^2, floor)): 0 dB is a tone of 1 LSB on a bin centre, the floor -100 dB
inline double waterfall_db(double power, double full)
{
    const double r = power / full;
    return r > kWaterfallFloor ? 10.0 * std::log10(r) : 10.0 * std::log10(kWaterfallFloor);
}

// (j - 48) x 125 Hz: slot j of a row from the channel's offset
inline int32_t waterfall_hz(int j) { return (j - kWaterfallBins / 2) * (12000 / kWaterfallBins); }

// One line of the waterfall log (--wideband-waterfall=FILE): row `row`[96] of global block g, t = 0.008 g exact in three decimals,
// two decimals per bin and no "-0.00"
inline std::string waterfall_line(int32_t channel, int32_t offset_hz, int64_t g, const float* row, double full)
{
    char buf[128];
    const long long ms = static_cast<long long>(g) * 8;
    snprintf(buf, sizeof(buf), "wf ch=%d offset=%d block=%lld t=%lld.%03lld db=", channel, offset_hz, static_cast<long long>(g), ms / 1000, ms % 1000);
    std::string line = buf;
    for(int j = 0; j < kWaterfallBins; j++)
    {
        snprintf(buf, sizeof(buf), "%.2f", waterfall_db(static_cast<double>(row[j]), full));
        if(j) line += ',';
        line += std::strcmp(buf, "-0.00") ? buf : "0.00";
    }
    return line;
}

// The frequency of a ping event, once: one double accumulator [96] per channel.  Blocks are taken in stream order; a block that is
// up adds its row, a block that is not up clears the accumulator, so that when PingTracker closes an event the accumulator holds
// exactly that event's rows.  push and close append one frequency - (j* - 48) x 125 Hz, j* the lowest j at the maximum - per event
// PingTracker reports from the same records (runs of at least min_blocks blocks), in its order.  Host only.
class PingSpectra
{
public:
    PingSpectra(int channels, int min_blocks) : min_blocks_(min_blocks), acc_(static_cast<size_t>(channels) * kWaterfallBins, 0.0), blocks_(static_cast<size_t>(channels), 0) {}

    // records[channels] of one push and its rows [channels][54][96]; only the rows of up blocks are read
    void push(const PingRecord* records, const float* rows, std::vector<int32_t>& out)
    {
        for(size_t c = 0; c < blocks_.size(); c++)
        {
            const PingRecord& r = records[c];
            double* a = &acc_[c * kWaterfallBins];
            for(int b = 0; b < r.blocks; b++)
            {
                if((r.up_mask >> b) & 1)
                {
                    const float* row = rows + (c * kWaterfallRows + static_cast<size_t>(b)) * kWaterfallBins;
                    for(int j = 0; j < kWaterfallBins; j++) a[j] += static_cast<double>(row[j]);
                    blocks_[c]++;
                }
                else finish(c, out);
            }
        }
    }

    void close(std::vector<int32_t>& out)
    {
        for(size_t c = 0; c < blocks_.size(); c++) finish(c, out);
    }

private:
    void finish(size_t c, std::vector<int32_t>& out)
    {
        double* a = &acc_[c * kWaterfallBins];
        if(blocks_[c] >= min_blocks_) out.push_back(waterfall_hz(static_cast<int>(std::max_element(a, a + kWaterfallBins) - a)));
        if(blocks_[c]) std::fill(a, a + kWaterfallBins, 0.0);
        blocks_[c] = 0;
    }

    int64_t min_blocks_;
    std::vector<double> acc_;
    std::vector<int64_t> blocks_;
};

// The summary's carrier rule on a channel's run-summed spectrum [96]: the excess in dB of its highest bin (the lowest j at the
// maximum, in j_top) over its median bin (rank 48 in ascending order); 0 when the median bin is not positive
inline double waterfall_excess_db(const double* sum, int& j_top)
{
    std::vector<double> sorted(sum, sum + kWaterfallBins);
    std::nth_element(sorted.begin(), sorted.begin() + kWaterfallBins / 2, sorted.end());
    j_top = static_cast<int>(std::max_element(sum, sum + kWaterfallBins) - sum);
    const double median = sorted[kWaterfallBins / 2];
    return median > 0.0 ? 10.0 * std::log10(sum[j_top] / median) : 0.0;
}

// ---- the hop rule and the plan of a push, which the capture and the gate share ----

// Both read the ping detector's up_mask hop by hop and keep, per channel, `since`: the hops since its last active one.
constexpr int kSinceQuiet = 17;   // `since` saturates here: no activity that any `post` or `hold` still reaches

// The 27 up bits of hop i of a push.  `first`: the push carries hops 0 and 1 (up_mask bits 0..26 and 27..53), i = 0 and 1 in that
// order; else the newest hop alone (bits 0..26), i = 1.  up_mask is 0 when the detector was off.
MSK144WB_HD inline uint64_t hop_up_bits(uint64_t up_mask, bool first, int i) { return (up_mask >> (first ? kHopBlocks * i : 0)) & ((1ull << kHopBlocks) - 1); }

// `since` behind one more hop
MSK144WB_HD inline int32_t since_next(int32_t since, bool active) { return active ? 0 : since < kSinceQuiet ? since + 1 : kSinceQuiet; }

// What the plan of a push leaves in front of its entries (the capture's units, the gate's channels), which come in ascending
// channel order: the entries stored, all entries the push had, and the newest hop of the push
struct PlanHeader
{
    int32_t count, total;
    int64_t hop;
};
static_assert(sizeof(PlanHeader) == 16, "the plan header is 16 bytes");

// ---- per-ping capture of a channel's hops (msk144_set_wideband_capture, msk144_wideband_capture) ----

constexpr int kCaptureUnitBytes = 5184;                   // one hop of one channel: 2592 int8 I/Q pairs, what --read-mode=2 reads
constexpr int kCaptureMaxPost = 16;
constexpr int kCaptureMaxUnits = 16384;
constexpr int kCaptureMaxListed = kWaterfallMaxListed;
constexpr int kCaptureDefaultMaxUnits = 512;              // the program's and the Python view's: min(2 x channels, 512)
static_assert(kCaptureUnitBytes % 16 == 0 && kHopBlocks * kPingBlock * 2 == kCaptureUnitBytes && 2 * kHopBlocks == kPingMaxBlocks, "a unit is a hop");

enum CaptureFlags
{
    kCaptureActive = 1,   // a(k): an up block among the hop's 27
    kCaptureListed = 2,   // L
    kCapturePre = 4,      // emitted as P(k), one push late
    kCaptureTail = 8      // not active, but active within `post` hops before
};

// msk144_wideband_capture_params without the list.  The defaults are design parameters, not measurements.
struct CaptureParams
{
    int32_t pre = 1, post = 1, max_units = kCaptureDefaultMaxUnits;
};

// msk144_wideband_capture_unit, field for field: what the plan kernel writes
struct CaptureUnit
{
    int32_t channel, flags;
    int64_t hop;
};
static_assert(sizeof(CaptureUnit) == 16, "msk144_wideband_capture_unit is 16 bytes");

// a channel's memory: hops since the last active one (kSinceQuiet: none that counts), and whether its newest hop was emitted
struct CaptureState
{
    int32_t since, emitted;
};

// The capture rule, once, for one channel and one push.  `first` and up_mask: as hop_up_bits takes them; a hop is active iff one of
// its blocks is up.  `clear`: a first push, or the first push after msk144_set_wideband_capture: earlier activity counts as none
// and the previous hop as not emitted.  Returns the channel's units of this push, 0 .. 2 in ascending hop order: half[i] is the
// half of the channel's ring window the unit lies in (0: the hop before the newest, 1: the newest), flags[i] its CaptureFlags.
//   W(k) = listed, or a(j) for some k - post <= j <= k   -> hop k is emitted in its own push
//   P(k) = pre and not W(k) and a(k + 1)                 -> hop k is emitted in the next push (for k = 0 that is the same push)
MSK144WB_HD inline int capture_step(CaptureState& s, bool first, bool clear, uint64_t up_mask, bool listed, int32_t pre, int32_t post, int32_t flags[2], int32_t half[2])
{
    int32_t since = clear ? kSinceQuiet : s.since;
    bool emitted = clear ? false : s.emitted != 0;
    int n = 0;
    for(int i = first ? 0 : 1; i < 2; i++)
    {
        const bool a = hop_up_bits(up_mask, first, i) != 0;
        since = since_next(since, a);
        const bool w = listed || since <= post;
        // the hop before this one: in the ring since the push before, or hop 0 of this first push
        if(i == 1 && pre && a && !emitted)
        {
            flags[n] = kCapturePre;
            half[n++] = 0;
        }
        if(w)
        {
            flags[n] = (a ? kCaptureActive : 0) | (listed ? kCaptureListed : 0) | (!a && since <= post ? kCaptureTail : 0);
            half[n++] = i;
        }
        emitted = w;
    }
    s.since = since;
    s.emitted = emitted ? 1 : 0;
    return n;
}

// The rules of msk144_set_wideband_capture.  Empty string = valid.
inline std::string check_capture(const CaptureParams& p, const int32_t* listed, int num_listed, int channels)
{
    if(p.pre != 0 && p.pre != 1) return "capture pre must be 0 or 1 (the ring holds one hop of pre-roll)";
    if(p.post < 0 || p.post > kCaptureMaxPost) return "capture post must lie within 0..16 hops";
    if(p.max_units < 1 || p.max_units > kCaptureMaxUnits) return "capture max_units must lie within 1..16384";
    if(num_listed < 0 || num_listed > kCaptureMaxListed) return "capture lists at most 16 channels";
    for(int i = 0; i < num_listed; i++)
    {
        if(listed[i] < 0 || listed[i] >= channels) return "capture channel " + std::to_string(listed[i]) + " is out of range";
        for(int j = 0; j < i; j++)
            if(listed[j] == listed[i]) return "capture channel " + std::to_string(listed[i]) + " is listed twice";
    }
    return std::string();
}

// The rule over all channels of a stream on the host: what the plan kernel computes, and through libmsk144host.so the yardstick of
// wideband.Capture.  Units come by channel, then by hop; the first max_units of a push are stored, the rest only counted - the
// state moves the same either way.
class Capture
{
public:
    Capture(int channels, const CaptureParams& p, const int32_t* listed, int num_listed) : p_(p), state_(static_cast<size_t>(channels)), listed_(static_cast<size_t>(channels), 0)
    {
        for(int i = 0; i < num_listed; i++) listed_[static_cast<size_t>(listed[i])] = 1;
    }

    // as msk144_set_wideband_capture in mid-stream: the state cleared, the hop count kept
    void restart() { clear_ = true; }
    // the newest hop of the last push, for a rule that joins a stream in mid-stream
    void set_hop(int64_t hop) { hop_ = hop; }
    int64_t hop() const { return hop_; }

    // records[channels] of one push, or nullptr: the detector was off.  Appends the stored units and returns the total.
    int32_t push(const PingRecord* records, bool first, std::vector<CaptureUnit>& out)
    {
        hop_ = first ? 1 : hop_ + 1;
        int32_t total = 0;
        for(size_t c = 0; c < state_.size(); c++)
        {
            int32_t flags[2], half[2];
            const int n = capture_step(state_[c], first, first || clear_, records ? records[c].up_mask : 0, listed_[c] != 0, p_.pre, p_.post, flags, half);
            for(int i = 0; i < n; i++, total++)
                if(total < p_.max_units) out.push_back(CaptureUnit{static_cast<int32_t>(c), flags[i], hop_ - 1 + half[i]});
        }
        clear_ = false;
        return total;
    }

private:
    CaptureParams p_;
    std::vector<CaptureState> state_;
    std::vector<uint8_t> listed_;
    bool clear_ = true;
    int64_t hop_ = 0;
};

// ---- each captured hop as 12 kHz audio (msk144_set_wideband_audio, msk144_wideband_capture_audio; the kernels': csrc/audio.hip) ----

constexpr int kAudioPhasors = 96;                          // w[n mod 96]: a hop is 27 x 96 samples, so there is no phase state
constexpr int kAudioHopSamples = kCaptureUnitBytes / 2;    // 2592 int16 per unit
constexpr int kAudioMinShift = 1, kAudioMaxShift = 40;
constexpr int kAudioToneStepHz = kOutRate / kAudioPhasors; // 125: tone - centre is a multiple of it
constexpr int kAudioPhasorScale = 16384;
constexpr int kAudioLevelBits = 6;                         // shift = log2 |B| + 14 - 8: amplitude A comes out near 256 A
// the defaults are design parameters, not measurements
constexpr int kAudioDefaultHalfwidthHz = 1250;
constexpr int kAudioDefaultToneHz = 1500;
static_assert(kAudioHopSamples % kAudioPhasors == 0 && kOutRate % kAudioPhasors == 0, "whole turns of the table per hop");

// msk144_wideband_audio_params, field for field
struct AudioParams
{
    int8_t taps[kFirTaps][2];
    int16_t phasor[kAudioPhasors][2];
    int32_t shift;
};
static_assert(sizeof(AudioParams) == 516, "msk144_wideband_audio_params is 516 bytes");

// One output sample, for device and host: y = clamp((Re z pr - Im z pi + 2^(shift - 1)) >> shift) in int64 (|a| <= 2^37); adds 1 to
// `clamped` when the clamp changed the value
MSK144WB_HD inline int32_t audio_out(int32_t zr, int32_t zi, int32_t pr, int32_t pi, int32_t shift, int32_t& clamped)
{
    const long long a = static_cast<long long>(zr) * pr - static_cast<long long>(zi) * pi;
    const long long v = (a + (1ll << (shift - 1))) >> shift;
    const long long y = v < -32768 ? -32768 : v > 32767 ? 32767 : v;
    clamped += y != v ? 1 : 0;
    return static_cast<int32_t>(y);
}

// The rules of msk144_set_wideband_audio that need no handle: any int8 taps and int16 phasors.  Empty string = valid.
inline std::string check_audio(const AudioParams& p)
{
    if(p.shift < kAudioMinShift || p.shift > kAudioMaxShift) return "audio shift must lie within 1..40";
    return std::string();
}

// The rules of the default design.  Empty string = valid.
inline std::string check_audio_design(int centre_hz, int halfwidth_hz, int tone_hz)
{
    if(halfwidth_hz < kPingBandMinHalfwidthHz || halfwidth_hz > kPingBandMaxHalfwidthHz) return "audio half-width must lie within 500..3000 Hz";
    if(std::abs(static_cast<long long>(centre_hz)) + halfwidth_hz > kOutRate / 2) return "audio band must lie within +-6000 Hz: |centre| + half-width <= 6000";
    if(tone_hz < halfwidth_hz || tone_hz > kOutRate / 2 - halfwidth_hz) return "audio tone must lie within half-width .. 6000 - half-width Hz";
    if((static_cast<long long>(tone_hz) - centre_hz) % kAudioToneStepHz != 0) return "audio tone - centre must be a multiple of 125 Hz (the phasor table has 96 entries)";
    return std::string();
}

// The default design: the ping band's taps for (centre_hz, halfwidth_hz), w[m] = 16384 e^{j 2 pi (tone - centre) m / 12000} rounded
// with rint - the angle reduced in integers first, (tone - centre) m mod 12000 - and shift = rint(log2 |B(centre)| + 6), so that a
// tone of amplitude A inside the band comes out at tone + (f - centre) Hz with amplitude near 256 A.  The caller has checked the
// arguments.  The band's skirt reaches the stop band about 310 Hz outside the half-width; with halfwidth > tone - 310 part of it
// folds over 0 Hz.
inline AudioParams audio_design(int centre_hz, int halfwidth_hz, int tone_hz)
{
    const PingBandParams b = ping_band_design(centre_hz, halfwidth_hz);
    AudioParams p{};
    std::memcpy(p.taps, b.taps, sizeof(p.taps));
    for(int m = 0; m < kAudioPhasors; m++)
    {
        const long long turn = ((static_cast<long long>(tone_hz) - centre_hz) * m % kOutRate + kOutRate) % kOutRate;
        const double t = 2.0 * M_PI * static_cast<double>(turn) / kOutRate;
        p.phasor[m][0] = static_cast<int16_t>(std::rint(kAudioPhasorScale * std::cos(t)));
        p.phasor[m][1] = static_cast<int16_t>(std::rint(kAudioPhasorScale * std::sin(t)));
    }
    p.shift = static_cast<int32_t>(std::rint(0.5 * std::log2(ping_band_response(b, centre_hz)) + kAudioLevelBits));
    return p;
}

// The audio on the host, for one channel and one push: x[n][2] the n stored int8 samples of the push (n a multiple of 2592, the
// first of them the first sample of a hop), tail[63][2] the channel's 63 stored samples before them, oldest first (all zero where
// the library restarts: a first push, the first push after msk144_set_wideband_audio); writes y[n] and clamped[n / 2592] and moves
// the tail on to the last 63 samples of x.  What libmsk144host.so holds the Python model and the kernel (audio.hip) to.
inline void audio_push(const AudioParams& p, const int8_t* x, int n, int8_t* tail, int16_t* y, int32_t* clamped)
{
    FirParams f{};
    std::memcpy(f.taps, p.taps, sizeof(f.taps));
    std::vector<int8_t> s;
    const std::vector<int32_t> z = fir_push(f, x, n, tail, s);
    for(int k = 0; k < n / kAudioHopSamples; k++) clamped[k] = 0;
    for(int m = 0; m < n; m++)
        y[m] = static_cast<int16_t>(audio_out(z[static_cast<size_t>(2 * m)], z[static_cast<size_t>(2 * m + 1)], p.phasor[m % kAudioPhasors][0], p.phasor[m % kAudioPhasors][1], p.shift,
                                              clamped[m / kAudioHopSamples]));
}

// The 44-byte RIFF/WAVE header of `samples` int16 samples of one channel at 12000 Hz: PCM format 1, block align 2, byte rate 24000
constexpr int kWavHeaderBytes = 44;
inline void wav_header(uint8_t* out, uint32_t samples)
{
    const uint32_t data = 2 * samples;
    auto le = [&](int at, uint32_t v, int bytes) {
        for(int i = 0; i < bytes; i++) out[at + i] = static_cast<uint8_t>(v >> (8 * i));
    };
    std::memcpy(out, "RIFF", 4);
    le(4, data + kWavHeaderBytes - 8, 4);
    std::memcpy(out + 8, "WAVEfmt ", 8);
    le(16, 16, 4);
    le(20, 1, 2);
    le(22, 1, 2);
    le(24, kOutRate, 4);
    le(28, 2 * kOutRate, 4);
    le(32, 2, 2);
    le(34, 16, 2);
    std::memcpy(out + 36, "data", 4);
    le(40, data, 4);
}

// The file rule of --wideband-capture=DIR, once.  A channel's unit continues the channel's open segment iff its hop is the segment's
// last hop + 1; otherwise the open segment ends and DIR/ch<c>_hop<k0>.cs8 begins.  Every write is open-append-close.  A segment
// that ends - when the channel's next unit does not continue it, or at close() - appends one line to DIR/capture.log.  The last
// segments of every channel are remembered, so that a ping line can name the file and the sample its event starts at.  A segment's
// first write truncates a file of that name, while the log is only ever appended to: whoever writes a second stream into the same
// DIR starts capture.log afresh first, as the program does, or its old lines name files whose content is no longer theirs.  Host only.
// With audio rows (--wideband-audio) every segment has DIR/ch<c>_hop<k0>.wav beside it: wav_header, then the segment's audio rows as
// little-endian int16; the header's two sizes are written when the segment ends, and its log line gains " wav=<name>".
class CaptureSegments
{
public:
    CaptureSegments(const std::string& dir, const std::vector<int32_t>& offsets) : dir_(dir), offsets_(offsets), chan_(offsets.size()) {}

    static std::string segment_name(int32_t channel, int64_t hop, const char* ext = ".cs8")
    {
        return "ch" + std::to_string(channel) + "_hop" + std::to_string(hop) + ext;
    }
    static std::string wav_name(int32_t channel, int64_t hop) { return segment_name(channel, hop, ".wav"); }

    // `count` units of one push and their rows data[count][5184], and with the audio on their audio[count][2592] and
    // clamped[count] (else null); false when a file could not be written
    bool push(const CaptureUnit* units, const int8_t* data, int count, const int16_t* audio = nullptr, const int32_t* clamped = nullptr)
    {
        wav_ = wav_ || audio;
        for(int u = 0; u < count; u++)
        {
            const CaptureUnit& x = units[u];
            Chan& ch = chan_[static_cast<size_t>(x.channel)];
            if(ch.hops && x.hop != ch.k0 + ch.hops && !finish(x.channel)) return false;
            if(!ch.hops)
            {
                ch.k0 = x.hop;
                segments_++;
            }
            FILE* f = fopen((dir_ + "/" + segment_name(x.channel, ch.k0)).c_str(), ch.hops ? "ab" : "wb");
            if(!f) return false;
            const bool ok = fwrite(data + static_cast<size_t>(u) * kCaptureUnitBytes, 1, kCaptureUnitBytes, f) == kCaptureUnitBytes;
            if(fclose(f) != 0 || !ok) return false;
            if(audio && !push_wav(x.channel, ch, audio + static_cast<size_t>(u) * kAudioHopSamples)) return false;
            if(audio) wav_clamped_ += clamped[u];
            ch.hops++;
            hops_++;
        }
        return true;
    }

    // the end of the stream: every open segment ends, in channel order
    bool close()
    {
        for(size_t c = 0; c < chan_.size(); c++)
            if(chan_[c].hops && !finish(static_cast<int32_t>(c))) return false;
        return true;
    }

    // What a ping line gains for an event of `channel` that starts at global block g: " file=<name> at=<sample offset of that block
    // in the file>", or " file=-" when the hop the block lies in is in none of the channel's remembered segments (it was dropped).
    std::string locate(int32_t channel, int64_t g) const
    {
        const Chan& ch = chan_[static_cast<size_t>(channel)];
        const int64_t k = g / kHopBlocks;
        int64_t k0 = -1;
        if(ch.hops && k >= ch.k0 && k < ch.k0 + ch.hops) k0 = ch.k0;
        for(int i = 0; k0 < 0 && i < kRemembered; i++)
            if(ch.past_hops[i] && k >= ch.past_k0[i] && k < ch.past_k0[i] + ch.past_hops[i]) k0 = ch.past_k0[i];
        if(k0 < 0) return " file=-";
        return " file=" + segment_name(channel, k0) + " at=" + std::to_string((k - k0) * (kCaptureUnitBytes / 2) + (g % kHopBlocks) * kPingBlock);
    }

    int64_t segments() const { return segments_; }
    int64_t hops() const { return hops_; }
    int64_t bytes() const { return hops_ * kCaptureUnitBytes; }
    // the audio beside them: one WAV file per segment, a hop's samples per unit, and the samples of them that the clamp changed
    int64_t wav_files() const { return wav_ ? segments_ : 0; }
    int64_t wav_samples() const { return wav_ ? hops_ * kAudioHopSamples : 0; }
    int64_t wav_clamped() const { return wav_clamped_; }

    // one line of DIR/capture.log; t = 0.216 k0 exact in three decimals
    static std::string log_line(int32_t channel, int32_t offset_hz, int64_t k0, int64_t hops, bool wav = false)
    {
        char buf[256];
        const long long ms = static_cast<long long>(k0) * 216;
        snprintf(buf, sizeof(buf), "capture ch=%d offset=%d hop=%lld t=%lld.%03lld hops=%lld file=%s", channel, offset_hz, static_cast<long long>(k0), ms / 1000, ms % 1000,
                 static_cast<long long>(hops), segment_name(channel, k0).c_str());
        return wav ? std::string(buf) + " wav=" + wav_name(channel, k0) : std::string(buf);
    }

private:
    static constexpr int kRemembered = 4;
    struct Chan
    {
        int64_t k0 = 0, hops = 0;  // the open segment; hops = 0: none
        int64_t past_k0[kRemembered] = {0, 0, 0, 0}, past_hops[kRemembered] = {0, 0, 0, 0};
        int next = 0;
    };

    // the segment's WAV file: begun with a header of no samples, or appended to
    bool push_wav(int32_t c, const Chan& ch, const int16_t* row)
    {
        FILE* f = fopen((dir_ + "/" + wav_name(c, ch.k0)).c_str(), ch.hops ? "ab" : "wb");
        if(!f) return false;
        uint8_t head[kWavHeaderBytes], bytes[2 * kAudioHopSamples];
        wav_header(head, 0);
        for(int i = 0; i < kAudioHopSamples; i++)
        {
            bytes[2 * i] = static_cast<uint8_t>(static_cast<uint16_t>(row[i]) & 0xffu);
            bytes[2 * i + 1] = static_cast<uint8_t>(static_cast<uint16_t>(row[i]) >> 8);
        }
        const bool ok = (ch.hops || fwrite(head, 1, sizeof(head), f) == sizeof(head)) && fwrite(bytes, 1, sizeof(bytes), f) == sizeof(bytes);
        return fclose(f) == 0 && ok;
    }

    // the two sizes of a finished segment's WAV header
    bool finish_wav(int32_t c, const Chan& ch)
    {
        FILE* f = fopen((dir_ + "/" + wav_name(c, ch.k0)).c_str(), "r+b");
        if(!f) return false;
        uint8_t head[kWavHeaderBytes];
        wav_header(head, static_cast<uint32_t>(ch.hops * kAudioHopSamples));
        const bool ok = fwrite(head, 1, sizeof(head), f) == sizeof(head);
        return fclose(f) == 0 && ok;
    }

    bool finish(int32_t c)
    {
        Chan& ch = chan_[static_cast<size_t>(c)];
        if(wav_ && !finish_wav(c, ch)) return false;
        FILE* f = fopen((dir_ + "/capture.log").c_str(), "a");
        if(!f) return false;
        const bool ok = fprintf(f, "%s\n", log_line(c, offsets_[static_cast<size_t>(c)], ch.k0, ch.hops, wav_).c_str()) > 0;
        if(fclose(f) != 0 || !ok) return false;
        ch.past_k0[ch.next] = ch.k0;
        ch.past_hops[ch.next] = ch.hops;
        ch.next = (ch.next + 1) % kRemembered;
        ch.hops = 0;
        return true;
    }

    std::string dir_;
    std::vector<int32_t> offsets_;
    std::vector<Chan> chan_;
    int64_t segments_ = 0, hops_ = 0, wav_clamped_ = 0;
    bool wav_ = false;  // the pushes carry audio rows
};

// ---- the gate: only the channels with activity are decoded (msk144_set_wideband_gate, msk144_wideband_gate) ----

constexpr int kGateMaxHold = 16;
static_assert(kCaptureMaxPost < kSinceQuiet && kGateMaxHold < kSinceQuiet, "a saturated `since` lies beyond every post and hold");

// msk144_wideband_gate_params, field for field.  The defaults are design parameters, not measurements.
struct GateParams
{
    int32_t hold = 1, min_up = 1, max_channels = 0;   // max_channels 0: every channel
};

// The gate rule, once, for one channel and one push.  `since`: hops since the channel's last active one, saturating at kSinceQuiet.
// `first` and up_mask: as hop_up_bits takes them; a hop is active iff at least min_up of its 27 blocks are up.  `clear`: a first
// push, or the first push after msk144_set_wideband_gate: earlier activity counts as none.  Returns whether the channel's window
// of this push is decoded: always, or since <= hold after the walk.
//   The window of push k covers hops k - 1 and k.  With hold >= 1 every window that contains an active hop is decoded: an active
//   hop k gives since = 0 in push k and since <= 1 in push k + 1.  No window is decoded because of activity more than `hold` hops
//   old.  hold = 0 decodes only the windows whose newest hop is active.
MSK144WB_HD inline bool gate_step(int32_t& since, bool first, bool clear, uint64_t up_mask, bool always, int32_t hold, int32_t min_up)
{
    int32_t s = clear ? kSinceQuiet : since;
    for(int i = first ? 0 : 1; i < 2; i++)
    {
        int32_t up = 0;
        for(uint64_t b = hop_up_bits(up_mask, first, i); b; b &= b - 1) up++;
        s = since_next(s, up >= min_up);
    }
    since = s;
    return always || s <= hold;
}

// max_channels as the rule uses it: 0 stands for every channel
inline int32_t gate_max_channels(const GateParams& p, int channels) { return p.max_channels ? p.max_channels : channels; }

// The rules of msk144_set_wideband_gate.  Empty string = valid.
inline std::string check_gate(const GateParams& p, int channels)
{
    if(p.hold < 0 || p.hold > kGateMaxHold) return "gate hold must lie within 0..16 hops";
    if(p.min_up < 1 || p.min_up > kHopBlocks) return "gate min_up must lie within 1..27 blocks";
    if(p.max_channels < 0 || p.max_channels > channels) return "gate max_channels must lie within 1.." + std::to_string(channels) + ", or be 0 for all";
    return std::string();
}

// The rule over all channels of a stream on the host: what the plan kernel computes, and through libmsk144host.so the yardstick of
// wideband.Gate.  Channels come in ascending order; the first max_channels that qualify are listed, the rest only counted - the
// state moves the same either way.
class Gate
{
public:
    Gate(int channels, const GateParams& p, const uint8_t* always) : p_(p), since_(static_cast<size_t>(channels), kSinceQuiet), always_(static_cast<size_t>(channels), 0)
    {
        for(int c = 0; always && c < channels; c++) always_[static_cast<size_t>(c)] = always[c] != 0;
    }

    // as msk144_set_wideband_gate in mid-stream: the state cleared
    void restart() { clear_ = true; }

    // records[channels] of one push, or nullptr: the detector was off.  Appends the listed channels and returns the total.
    int32_t push(const PingRecord* records, bool first, std::vector<int32_t>& out)
    {
        const int32_t cap = gate_max_channels(p_, static_cast<int>(since_.size()));
        int32_t total = 0;
        for(size_t c = 0; c < since_.size(); c++)
            if(gate_step(since_[c], first, first || clear_, records ? records[c].up_mask : 0, always_[c] != 0, p_.hold, p_.min_up) && total++ < cap)
                out.push_back(static_cast<int32_t>(c));
        clear_ = false;
        return total;
    }

private:
    GateParams p_;
    std::vector<int32_t> since_;
    std::vector<uint8_t> always_;
    bool clear_ = true;
};

// ---- the notch: steady carriers taken out of a channel's stored samples (msk144_set_wideband_notch, msk144_wideband_notch_stats) ----

constexpr int kNotchTaps = kFirTaps, kNotchTail = kFirTail;   // a tail of raw (pre-notch) samples
constexpr int kNotchDelay = 31;              // the output is the input delayed by this many samples, minus the estimate
constexpr int kNotchMaxShift = 15;
constexpr int kNotchMaxFreqs = 2;            // carriers of one channel's default design
constexpr int kNotchMinHalfwidthHz = 50;
constexpr int kNotchMaxHalfwidthHz = 500;
constexpr int kNotchDefaultHalfwidthHz = 100;
constexpr int kNotchMinSpacingHz = 1000;     // closer carriers over-subtract: the two pass bands of the estimate add

using NotchParams = FirParams;
static_assert(sizeof(NotchParams) == 132, "msk144_wideband_notch_params is 132 bytes");

// The rule of msk144_set_wideband_notch that needs no handle: any int8 taps.  Empty string = valid.
inline std::string check_notch(int32_t shift)
{
    if(shift < 0 || shift > kNotchMaxShift) return "notch shift must lie within 0..15";
    return std::string();
}

// The rules of the default design.  Empty string = valid.
inline std::string check_notch_design(const int32_t* freqs_hz, int n, int halfwidth_hz)
{
    if(n < 1 || n > kNotchMaxFreqs || !freqs_hz) return "a notch takes 1 or 2 frequencies";
    if(halfwidth_hz < kNotchMinHalfwidthHz || halfwidth_hz > kNotchMaxHalfwidthHz) return "notch half-width must lie within 50..500 Hz";
    for(int i = 0; i < n; i++)
        if(std::abs(static_cast<long long>(freqs_hz[i])) + halfwidth_hz > kOutRate / 2) return "notch must lie within +-6000 Hz: |frequency| + half-width <= 6000";
    if(n == 2 && std::abs(static_cast<long long>(freqs_hz[0]) - freqs_hz[1]) < kNotchMinSpacingHz) return "two notches of a channel must lie at least 1000 Hz apart";
    return std::string();
}

// |H(f)|^2 of the whole stage, H(f) = e^{-j 2 pi f 31 / 12000} - B(f) / 2^shift: what a component at f_hz keeps of its power (without
// the rounding of the output)
inline double notch_response(const NotchParams& p, double f_hz)
{
    const double d = -2.0 * M_PI * f_hz * kNotchDelay / kOutRate;
    double re = std::cos(d), im = std::sin(d);
    fir_response_add(p, f_hz, -std::ldexp(1.0, -p.shift), re, im);
    return re * re + im * im;
}

// The default design, in double: a 63-tap Hamming-windowed sinc low-pass with cutoff halfwidth_hz centred on k = 31 and scaled to unit
// DC gain, turned to each frequency by e^{+j 2 pi f (k - 31) / 12000} and summed: the estimate of the carriers, which the stage takes
// from the input delayed by 31 samples.  shift = min(15, floor(log2(127 / largest |component|))), taps rint(value x 2^shift), tap 63 = 0.
// The caller has checked the arguments.
inline NotchParams notch_design(const int32_t* freqs_hz, int n, int halfwidth_hz)
{
    constexpr int N = kNotchTaps - 1;
    double h[N], re[N] = {}, im[N] = {}, sum = 0.0, top = 0.0;
    hamming_sinc(N, kNotchDelay, halfwidth_hz, h);
    for(int k = 0; k < N; k++) sum += h[k];
    for(int k = 0; k < N; k++)
    {
        for(int i = 0; i < n; i++)
        {
            const double a = 2.0 * M_PI * freqs_hz[i] * (k - kNotchDelay) / kOutRate;
            re[k] += h[k] / sum * std::cos(a);
            im[k] += h[k] / sum * std::sin(a);
        }
        top = std::max(top, std::max(std::fabs(re[k]), std::fabs(im[k])));
    }
    NotchParams p{};
    p.shift = std::min(kNotchMaxShift, static_cast<int>(std::floor(std::log2(127.0 / top))));
    for(int k = 0; k < N; k++)
    {
        p.taps[k][0] = static_cast<int8_t>(std::rint(std::ldexp(re[k], p.shift)));
        p.taps[k][1] = static_cast<int8_t>(std::rint(std::ldexp(im[k], p.shift)));
    }
    return p;
}

MSK144WB_HD inline int32_t notch_sat8(int32_t v) { return v < -128 ? -128 : v > 127 ? 127 : v; }

// One component of the stage: x the component of x[n - 31], z that of z[n].  The shift right is arithmetic.
MSK144WB_HD inline int32_t notch_out(int32_t x, int32_t z, int32_t shift) { return (x * (1 << shift) - z + (shift ? 1 << (shift - 1) : 0)) >> shift; }

// The stage on the host, for one channel and one push: x[n][2] the n stored int8 samples of the push, tail[63][2] the channel's 63 raw
// (pre-notch) stored samples before them, oldest first (all zero where the channel's filter starts); writes y[n][2] (y may be x),
// adds the components that sat8 clamped to *clipped and moves the tail on to the last 63 samples of x.  With fir_push's z,
// y[m] = sat8(((x[m - 31] << shift) - z[m] + r) >> shift).  What libmsk144host.so holds the Python model and the kernel (notch.hip) to.
inline void notch_filter(const NotchParams& p, const int8_t* x, int n, int8_t* tail, int8_t* y, int32_t* clipped)
{
    std::vector<int8_t> s;
    const std::vector<int32_t> z = fir_push(p, x, n, tail, s);
    for(size_t i = 0; i < z.size(); i++)
    {
        const int32_t v = notch_out(s[2 * (kNotchTail - kNotchDelay) + i], z[i], p.shift), sat = notch_sat8(v);
        *clipped += sat != v;
        y[i] = static_cast<int8_t>(sat);
    }
}

// The host rule of --wideband-notch=auto: which carriers get a notch, from every push's msk144_wideband_waterfall_sums.  Host only,
// with a Python twin (wideband.NotchPlanner).  db, period and persist are design parameters, not measurements.
struct NotchPlan
{
    double db = kWaterfallCarrierDb;  // a bin is hot when it lies at least this far over the period's median bin
    int32_t period = 23;              // pushes whose sums are added, about 5 s
    int32_t persist = 2;              // consecutive periods the same bin, +-1, must be hot in
};
constexpr int kNotchPlanGuardBins = 3;     // bins either side of a channel's notches that the search leaves out
constexpr int kNotchPlanMaxPeriod = 100000;
constexpr int kNotchPlanMaxPersist = 1000;

inline std::string check_notch_plan(const NotchPlan& p)
{
    if(!(p.db >= 1.0 && p.db <= 100.0)) return "notch auto DB must lie within 1..100 dB";
    if(p.period < 1 || p.period > kNotchPlanMaxPeriod) return "notch auto PERIOD must lie within 1..100000 pushes";
    if(p.persist < 1 || p.persist > kNotchPlanMaxPersist) return "notch auto PERSIST must lie within 1..1000 periods";
    return std::string();
}

// a notch the planner added: at hz from the channel's offset, for a bin excess_db over the period's median bin
struct NotchAdded
{
    int32_t channel, hz;
    double excess_db;
};

// Per channel the planner adds the sums of `period` pushes.  At the end of a period it takes the highest bin j (the lowest at the
// maximum) that is not within 3 bins of one of the channel's notches; the bin is hot when it lies at least db over the period's
// median bin (rank 48 of all 96 in ascending order, which must be positive).  The same bin, +-1 from the period before, hot in
// `persist` consecutive periods adds a notch at rint(125 (j - 48 + d)) Hz if the channel has fewer than 2 and check_notch_design
// takes the new list (the spacing rule); d is the vertex of the parabola through 10 log10 of bins j - 1, j, j + 1, clamped to +-0.5,
// and 0 at j = 0 or 95, where a neighbour is not positive or where the three do not form a peak.  Notches are only ever added
// during a run: the notch is ahead of the waterfall, so a released notch could not be told from a carrier that left.
class NotchPlanner
{
public:
    NotchPlanner(int channels, const NotchPlan& plan, int halfwidth_hz)
        : plan_(plan), halfwidth_(halfwidth_hz), acc_(static_cast<size_t>(channels) * kWaterfallBins, 0.0), chan_(static_cast<size_t>(channels))
    {
    }

    // sums[channels][96] of one push; appends what this push added, by channel
    void push(const double* sums, std::vector<NotchAdded>& out)
    {
        for(size_t k = 0; k < acc_.size(); k++) acc_[k] += sums[k];
        if(++pushes_ < plan_.period) return;
        pushes_ = 0;
        for(size_t c = 0; c < chan_.size(); c++) end_period(static_cast<int32_t>(c), &acc_[c * kWaterfallBins], out);
        std::fill(acc_.begin(), acc_.end(), 0.0);
    }

    const std::vector<int32_t>& notches(int channel) const { return chan_[static_cast<size_t>(channel)].hz; }

    static double vertex(const double* a, int j)
    {
        if(j <= 0 || j >= kWaterfallBins - 1 || !(a[j - 1] > 0.0) || !(a[j + 1] > 0.0) || !(a[j] > 0.0)) return 0.0;
        const double lm = 10.0 * std::log10(a[j - 1]), l0 = 10.0 * std::log10(a[j]), lp = 10.0 * std::log10(a[j + 1]);
        const double den = lm - 2.0 * l0 + lp;
        if(!(den < 0.0)) return 0.0;
        const double d = 0.5 * (lm - lp) / den;
        return d < -0.5 ? -0.5 : d > 0.5 ? 0.5 : d;
    }

private:
    struct Chan
    {
        std::vector<int32_t> hz;  // the channel's notches
        int32_t bin = -1, run = 0;  // the hot bin of the last period and the periods in a row it has been hot
    };

    void end_period(int32_t c, const double* a, std::vector<NotchAdded>& out)
    {
        Chan& s = chan_[static_cast<size_t>(c)];
        int j = -1;
        for(int i = 0; i < kWaterfallBins; i++)
        {
            bool guarded = false;
            for(int32_t f : s.hz) guarded = guarded || std::abs(i - (static_cast<int>(std::lrint(f / 125.0)) + kWaterfallBins / 2)) <= kNotchPlanGuardBins;
            if(!guarded && (j < 0 || a[i] > a[j])) j = i;
        }
        std::vector<double> sorted(a, a + kWaterfallBins);
        std::nth_element(sorted.begin(), sorted.begin() + kWaterfallBins / 2, sorted.end());
        const double median = sorted[kWaterfallBins / 2];
        const double excess = j >= 0 && median > 0.0 && a[j] > 0.0 ? 10.0 * std::log10(a[j] / median) : 0.0;
        if(!(j >= 0 && median > 0.0 && excess >= plan_.db))
        {
            s.bin = -1, s.run = 0;
            return;
        }
        s.run = s.bin >= 0 && std::abs(j - s.bin) <= 1 ? s.run + 1 : 1;
        s.bin = j;
        if(s.run < plan_.persist || s.hz.size() >= static_cast<size_t>(kNotchMaxFreqs)) return;
        std::vector<int32_t> next = s.hz;
        next.push_back(static_cast<int32_t>(std::lrint(125.0 * (j - kWaterfallBins / 2 + vertex(a, j)))));
        if(!check_notch_design(next.data(), static_cast<int>(next.size()), halfwidth_).empty()) return;
        s.hz = next;
        s.bin = -1, s.run = 0;
        out.push_back(NotchAdded{c, next.back(), excess});
    }

    NotchPlan plan_;
    int halfwidth_;
    int32_t pushes_ = 0;
    std::vector<double> acc_;
    std::vector<Chan> chan_;
};

// The stderr line of a notch the planner added at hop k
inline std::string notch_added_line(const NotchAdded& n, int32_t offset_hz, long long hop)
{
    char buf[192];
    snprintf(buf, sizeof(buf), "msk144hipdecoder: wideband notch: ch=%d offset=%d notch=%d excess=%.1f at hop %lld", n.channel, offset_hz, n.hz, n.excess_db, hop);
    return buf;
}

// Every rule of the contract (include/msk144hip.h) except the ones that need a handle.  Empty string = valid.
inline std::string check_config(int64_t rate_hz, int format, int K, float gain, const int32_t* offsets, int count)
{
    if(rate_hz <= 0 || rate_hz % kRateStepHz != 0) return "wideband rate must be a positive multiple of 125 Hz; a multiple of 12000 Hz decimates by an integer";
    if((rate_hz < kMinRateHz || rate_hz > kMaxRateHz) && !is_bank_rate(rate_hz))
        return "wideband rate must be D x 12000 Hz with 2 <= D <= 512 (D = P/Q may be a fraction: 24000..6144000 Hz), or a multiple of 8000 Hz "
               "above 6144000 up to 61440000 Hz (two-stage bank)";
    if(format != kCu8 && format != kCs8 && format != kCs16) return "wideband format must be cu8, cs8 or cs16";
    if(K < 1 || K > kMaxTapsPerPhase) return "taps per phase must be 1..64";
    if(!(gain > 0.0f) || !std::isfinite(gain) || gain > kMaxGain) return "wideband gain must be a positive finite number no larger than 1e36";
    if(count < 1 || !offsets) return "at least one channel offset is needed";
    const int64_t lim = rate_hz / 2 - kGuardHz;
    for(int i = 0; i < count; i++)
        if(std::llabs(static_cast<long long>(offsets[i])) > lim)
            return "channel offset " + std::to_string(offsets[i]) + " Hz is outside +-(rate/2 - 6000) = +-" + std::to_string(lim) + " Hz";
    return std::string();
}

}  // namespace msk144wb
