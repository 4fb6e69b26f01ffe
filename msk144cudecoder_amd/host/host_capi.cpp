// C entry points of the GPU-independent host logic, for the CPU test-suite (libmsk144host.so).
#include "stream_gate_cli.h"
#include "stream_pings_cli.h"
#include "wideband_cli.h"
#include "window_decoder.h"

#include "../csrc/input_rate.h"
#include "../csrc/msk144_tables.h"
#include "../csrc/stream_gate.h"
#include "../csrc/stream_pings.h"
#include "../csrc/wideband.h"

#include <cstring>

using namespace msk144host;

extern "C" {

// The default wideband prototype filter for any rate Fs = 12000 P/Q (csrc/wideband.h design_taps_rate): L = K*P taps summing to Q
// into out; returns L, or -1 for a rate the contract refuses (not a multiple of 125 Hz, outside 24000..6144000 Hz) or K outside
// 1..64.  The same taps msk144hipdecoder hands to msk144_set_wideband.
int msk144host_wideband_taps_rate(int64_t rate_hz, int K, double* out)
{
    if(rate_hz <= 0 || rate_hz % msk144wb::kRateStepHz != 0 || rate_hz < msk144wb::kMinRateHz || rate_hz > msk144wb::kMaxRateHz || K < 1 || K > msk144wb::kMaxTapsPerPhase)
        return -1;
    const std::vector<double> h = msk144wb::design_taps_rate(rate_hz, K);
    if(out) std::memcpy(out, h.data(), sizeof(double) * h.size());
    return static_cast<int>(h.size());
}

// The same by integer decimation, Fs = D x 12000 (include/msk144hip.h names it): L = K*D taps, or -1 for D outside 2..512
int msk144host_wideband_taps(int D, int K, double* out) { return msk144host_wideband_taps_rate(static_cast<int64_t>(D) * msk144wb::kOutRate, K, out); }

// The default analysis-bank prototype above 6.144 Msps (csrc/wideband.h design_bank_taps): L1 = 64 K1 taps summing to 1 into out;
// returns L1, or -1 for a rate the bank does not take (a multiple of 8000 Hz above 6144000 up to 61440000) or K1 outside 1..16.
int msk144host_wideband_bank_taps(int64_t rate_hz, int K1, double* out)
{
    if(!msk144wb::is_bank_rate(rate_hz) || K1 < 1 || K1 > msk144wb::kMaxBankTapsPerBand) return -1;
    const std::vector<double> h = msk144wb::design_bank_taps(rate_hz, K1);
    if(out) std::memcpy(out, h.data(), sizeof(double) * h.size());
    return static_cast<int>(h.size());
}

// The band of channel offset f_hz at a bank rate (csrc/wideband.h bank_band), -32..32
int msk144host_wideband_band(int64_t rate_hz, int64_t f_hz) { return msk144wb::bank_band(rate_hz, f_hz); }

// The contract's configuration rules (csrc/wideband.h check_config), the ones msk144_set_wideband and msk144hipdecoder apply:
// returns 0 when valid, else -1 with the refusal text in why (NUL-terminated, at most why_len bytes).
int msk144host_wideband_check(int64_t rate_hz, int format, int K, float gain, const int32_t* offsets, int count, char* why, int why_len)
{
    const std::string s = msk144wb::check_config(rate_hz, format, K, gain, offsets, count);
    if(why && why_len > 0)
    {
        std::strncpy(why, s.c_str(), static_cast<size_t>(why_len) - 1);
        why[why_len - 1] = 0;
    }
    return s.empty() ? 0 : -1;
}

// The AGC step rule (csrc/wideband.h agc_step, the function the device runs): p = {lo_sq, hi_sq, clip_ppm, hold, min_exp, max_exp};
// (*e, *quiet) move by one push of n outputs with sum_sq S and k clipped components.  Returns 0, or -1 for parameters that
// msk144_set_wideband_agc refuses (the text in why when given).
int msk144host_wideband_agc_step(const int32_t* p, int64_t n, int64_t S, int64_t k, int32_t* e, int32_t* quiet, char* why, int why_len)
{
    const msk144wb::AgcParams ap{p[0], p[1], p[2], p[3], p[4], p[5]};
    const std::string s = msk144wb::check_agc(ap);
    if(why && why_len > 0)
    {
        std::strncpy(why, s.c_str(), static_cast<size_t>(why_len) - 1);
        why[why_len - 1] = 0;
    }
    if(!s.empty()) return -1;
    msk144wb::agc_step(ap, n, S, k, *e, *quiet);
    return 0;
}

// whether msk144_set_wideband_gains takes gain g with the AGC's top exponent max_exp (0: AGC off), and the f32 scale at exponent e
int msk144host_wideband_gain_ok(float g, int32_t max_exp) { return msk144wb::gain_ok(g, max_exp) ? 1 : 0; }
float msk144host_wideband_agc_scale(float g, int32_t e) { return msk144wb::agc_scale(g, e); }

// The blanker's threshold rule (csrc/wideband.h blanker_threshold, the function the device runs): T of a push of N samples whose
// powers sum to S, or -1 for N < 1, S < 0 or a threshold_q4 that msk144_set_wideband_blanker refuses.
int64_t msk144host_wideband_blanker_threshold(int64_t S, int64_t N, int32_t threshold_q4)
{
    if(N < 1 || S < 0 || threshold_q4 < msk144wb::kBlankerMinThresholdQ4 || threshold_q4 > msk144wb::kBlankerMaxThresholdQ4) return -1;
    return static_cast<int64_t>(msk144wb::blanker_threshold(static_cast<uint64_t>(S), static_cast<uint64_t>(N), static_cast<uint32_t>(threshold_q4)));
}

// The default spectrum window of msk144_set_wideband_spectrum (csrc/wideband.h spectrum_window), periodic Hann: B values into out;
// returns B, or -1 for a B that is not a power of two within 256..8192.
int msk144host_wideband_spectrum_window(int B, double* out)
{
    if(B < msk144wb::kSpectrumMinBins || B > msk144wb::kSpectrumMaxBins || (B & (B - 1)) != 0) return -1;
    const std::vector<double> w = msk144wb::spectrum_window(B);
    if(out) std::memcpy(out, w.data(), sizeof(double) * w.size());
    return B;
}

// ---- ping detection (csrc/wideband.h: the rule the device runs, and the event tracker the program runs) ----

namespace
{
int copy_why(const std::string& s, char* why, int why_len)
{
    if(why && why_len > 0)
    {
        std::strncpy(why, s.c_str(), static_cast<size_t>(why_len) - 1);
        why[why_len - 1] = 0;
    }
    return s.empty() ? 0 : -1;
}

struct PingModel
{
    msk144wb::PingParams p;
    std::vector<msk144wb::PingHistory> state;
};
}  // namespace

// p = {ratio_q4, memory, min_ref}: 0 when msk144_set_wideband_pings takes them, else -1 with the refusal text in why
int msk144host_wideband_ping_check(const int32_t* p, char* why, int why_len) { return copy_why(msk144wb::check_pings(msk144wb::PingParams{p[0], p[1], p[2]}), why, why_len); }
int msk144host_wideband_ping_rank(int nb) { return msk144wb::ping_rank(nb); }
int msk144host_wideband_ping_up(int32_t E, int32_t R, int32_t ratio_q4) { return msk144wb::ping_up(E, R, ratio_q4) ? 1 : 0; }

// the detector of `channels` channels with their histories (NULL for parameters the library refuses) ...
void* msk144host_wideband_ping_new(int channels, const int32_t* p)
{
    const msk144wb::PingParams pp{p[0], p[1], p[2]};
    if(channels < 1 || !msk144wb::check_pings(pp).empty()) return nullptr;
    return new PingModel{pp, std::vector<msk144wb::PingHistory>(static_cast<size_t>(channels))};
}
void msk144host_wideband_ping_free(void* m) { delete static_cast<PingModel*>(m); }
// ... and one push of it: energies[channels][54] with nb blocks each, scales[channels], restart as the library passes it (a first
// push, or the first push after `set`); out[channels] msk144_wideband_ping records
void msk144host_wideband_ping_push(void* m, int restart, const float* scales, const int32_t* energies, int nb, msk144wb::PingRecord* out)
{
    PingModel& pm = *static_cast<PingModel*>(m);
    for(size_t c = 0; c < pm.state.size(); c++) out[c] = msk144wb::ping_record(pm.p, pm.state[c], restart != 0, scales[c], energies + c * msk144wb::kPingMaxBlocks, nb);
}

// the event tracker: push and close write at most cap events {channel, start, blocks, peak, reference} and return their number
void* msk144host_wideband_ping_tracker_new(int channels, int min_blocks)
{
    if(channels < 1 || min_blocks < 1 || min_blocks > msk144wb::kPingMaxMinBlocks) return nullptr;
    return new msk144wb::PingTracker(channels, min_blocks);
}
void msk144host_wideband_ping_tracker_free(void* t) { delete static_cast<msk144wb::PingTracker*>(t); }
int msk144host_wideband_ping_tracker_push(void* t, const msk144wb::PingRecord* records, const int32_t* energies, msk144wb::PingEvent* out, int cap)
{
    std::vector<msk144wb::PingEvent> ev;
    static_cast<msk144wb::PingTracker*>(t)->push(records, energies, ev);
    for(int i = 0; i < static_cast<int>(ev.size()) && i < cap; i++) out[i] = ev[static_cast<size_t>(i)];
    return static_cast<int>(ev.size());
}
int msk144host_wideband_ping_tracker_close(void* t, msk144wb::PingEvent* out, int cap)
{
    std::vector<msk144wb::PingEvent> ev;
    static_cast<msk144wb::PingTracker*>(t)->close(ev);
    for(int i = 0; i < static_cast<int>(ev.size()) && i < cap; i++) out[i] = ev[static_cast<size_t>(i)];
    return static_cast<int>(ev.size());
}
// {events, up blocks, total blocks} of the tracker so far
void msk144host_wideband_ping_tracker_counts(void* t, int64_t* out3)
{
    const msk144wb::PingTracker& tr = *static_cast<msk144wb::PingTracker*>(t);
    out3[0] = tr.events(), out3[1] = tr.up_blocks(), out3[2] = tr.total_blocks();
}
// the event's line of the log (--wideband-pings=FILE), NUL-terminated in out
void msk144host_wideband_ping_line(const msk144wb::PingEvent* e, int32_t offset_hz, char* out, int cap)
{
    std::strncpy(out, msk144wb::ping_event_line(*e, offset_hz).c_str(), static_cast<size_t>(cap) - 1);
    out[cap - 1] = 0;
}
// "FILE[:RATIO[:MIN_BLOCKS[:MEMORY]]]" as the program parses it: 0 and out4 = {ratio_q4, min_blocks, memory, length of FILE}, else -1
int msk144host_wideband_pings_parse(const char* arg, int32_t* out4)
{
    WidebandOptions w;
    if(!parse_wideband_pings(arg, w)) return -1;
    out4[0] = w.ping_params.ratio_q4, out4[1] = w.ping_min_blocks, out4[2] = w.ping_params.memory, out4[3] = static_cast<int32_t>(w.pings_file.size());
    return 0;
}

// ---- the ping band (csrc/wideband.h: the default design, the check, the filter and its energies) ----

// The default design of msk144_set_wideband_ping_band: taps[64][2] int8 and the shift; -1 with the refusal text for a band the design
// does not take.  The taps the program and msk144cudecoder_amd.wideband.ping_band_taps hand to the library.
int msk144host_wideband_ping_band_design(int32_t centre_hz, int32_t halfwidth_hz, int8_t* taps, int32_t* shift, char* why, int why_len)
{
    const std::string s = msk144wb::check_ping_band_design(centre_hz, halfwidth_hz);
    if(!s.empty()) return copy_why(s, why, why_len);
    const msk144wb::PingBandParams p = msk144wb::ping_band_design(centre_hz, halfwidth_hz);
    std::memcpy(taps, p.taps, sizeof(p.taps));
    *shift = p.shift;
    return copy_why(s, why, why_len);
}
// 0 when msk144_set_wideband_ping_band takes the shift (any int8 taps are valid), else -1 with the refusal text
int msk144host_wideband_ping_band_check(int32_t shift, char* why, int why_len)
{
    msk144wb::PingBandParams p{};
    p.shift = shift;
    return copy_why(msk144wb::check_ping_band(p), why, why_len);
}
// One push of `channels` channels: x[channels][n][2] stored int8 samples (n a multiple of 96), tails[channels][63][2] in and out,
// Ef[channels][n / 96].  -1 for a shift or an n out of range.
int msk144host_wideband_ping_band_energies(const int8_t* taps, int32_t shift, int channels, const int8_t* x, int n, int8_t* tails, int32_t* Ef)
{
    msk144wb::PingBandParams p{};
    std::memcpy(p.taps, taps, sizeof(p.taps));
    p.shift = shift;
    if(!msk144wb::check_ping_band(p).empty() || channels < 1 || n < 0 || n % msk144wb::kPingBlock != 0) return -1;
    for(int c = 0; c < channels; c++)
        msk144wb::ping_band_energies(p, x + static_cast<size_t>(c) * 2 * n, n, tails + static_cast<size_t>(c) * 2 * msk144wb::kPingBandTail, Ef + static_cast<size_t>(c) * (n / msk144wb::kPingBlock));
    return 0;
}
// "[HALFWIDTH[:CENTRE]]" as the program parses the value of --wideband-pings-band (centre_default: --center-frequency): 0 and
// out2 = {halfwidth, centre}, else -1
int msk144host_wideband_ping_band_parse(const char* arg, int32_t centre_default, int32_t* out2)
{
    WidebandOptions w;
    if(!parse_wideband_ping_band(arg, centre_default, w)) return -1;
    out2[0] = w.ping_band_halfwidth, out2[1] = w.ping_band_centre;
    return 0;
}

// ---- the audio (csrc/wideband.h: the default design, the check, the filter and its mix to int16) ----

// The default design of msk144_set_wideband_audio: taps[64][2] int8, phasor[96][2] int16 and the shift; -1 with the refusal text for
// arguments the design does not take.  What the program and msk144cudecoder_amd.wideband.audio_design hand to the library.
int msk144host_wideband_audio_design(int32_t centre_hz, int32_t halfwidth_hz, int32_t tone_hz, int8_t* taps, int16_t* phasor, int32_t* shift, char* why, int why_len)
{
    const std::string s = msk144wb::check_audio_design(centre_hz, halfwidth_hz, tone_hz);
    if(!s.empty()) return copy_why(s, why, why_len);
    const msk144wb::AudioParams p = msk144wb::audio_design(centre_hz, halfwidth_hz, tone_hz);
    std::memcpy(taps, p.taps, sizeof(p.taps));
    std::memcpy(phasor, p.phasor, sizeof(p.phasor));
    *shift = p.shift;
    return copy_why(s, why, why_len);
}
// 0 when msk144_set_wideband_audio takes the shift (any int8 taps and int16 phasors are valid), else -1 with the refusal text
int msk144host_wideband_audio_check(int32_t shift, char* why, int why_len)
{
    msk144wb::AudioParams p{};
    p.shift = shift;
    return copy_why(msk144wb::check_audio(p), why, why_len);
}
// One push of `channels` channels: x[channels][n][2] stored int8 samples (n a multiple of 2592), tails[channels][63][2] in and out,
// y[channels][n] and clamped[channels][n / 2592].  -1 for a shift or an n out of range.
int msk144host_wideband_audio_push(const int8_t* taps, const int16_t* phasor, int32_t shift, int channels, const int8_t* x, int n, int8_t* tails, int16_t* y, int32_t* clamped)
{
    msk144wb::AudioParams p{};
    std::memcpy(p.taps, taps, sizeof(p.taps));
    std::memcpy(p.phasor, phasor, sizeof(p.phasor));
    p.shift = shift;
    if(!msk144wb::check_audio(p).empty() || channels < 1 || n < 0 || n % msk144wb::kAudioHopSamples != 0) return -1;
    for(int c = 0; c < channels; c++)
        msk144wb::audio_push(p, x + static_cast<size_t>(c) * 2 * n, n, tails + static_cast<size_t>(c) * 2 * msk144wb::kFirTail, y + static_cast<size_t>(c) * n,
                             clamped + static_cast<size_t>(c) * (n / msk144wb::kAudioHopSamples));
    return 0;
}
// the 44-byte header of a WAV file of `samples` samples, as --wideband-audio writes it
void msk144host_wideband_wav_header(uint32_t samples, uint8_t* out44)
{
    msk144wb::wav_header(out44, samples);
}
// "[HALFWIDTH[:CENTRE[:TONE]]]" as the program parses the value of --wideband-audio (centre_default: --center-frequency): 0 and
// out3 = {halfwidth, centre, tone}, else -1 with the design's refusal text, or an empty one for a value that does not parse
int msk144host_wideband_audio_parse(const char* arg, int32_t centre_default, int32_t* out3, char* why, int why_len)
{
    WidebandOptions w;
    std::string text;
    if(!parse_wideband_audio(arg, centre_default, w, text))
    {
        copy_why(text, why, why_len);
        return -1;
    }
    out3[0] = w.audio_halfwidth, out3[1] = w.audio_centre, out3[2] = w.audio_tone;
    return 0;
}

// ---- the notch (csrc/wideband.h: the default design, the checks, the response, the filter) ----

// The default design of a channel's notch: taps[64][2] int8 and the shift for n frequencies; -1 with the refusal text for what the
// design does not take.  The taps msk144cudecoder_amd.wideband.notch_taps hands to the library.
int msk144host_wideband_notch_design(const int32_t* freqs_hz, int32_t n, int32_t halfwidth_hz, int8_t* taps, int32_t* shift, char* why, int why_len)
{
    const std::string s = msk144wb::check_notch_design(freqs_hz, n, halfwidth_hz);
    if(!s.empty()) return copy_why(s, why, why_len);
    const msk144wb::NotchParams p = msk144wb::notch_design(freqs_hz, n, halfwidth_hz);
    std::memcpy(taps, p.taps, sizeof(p.taps));
    *shift = p.shift;
    return copy_why(s, why, why_len);
}
// 0 when msk144_set_wideband_notch takes the shift (any int8 taps are valid), else -1 with the refusal text
int msk144host_wideband_notch_check(int32_t shift, char* why, int why_len) { return copy_why(msk144wb::check_notch(shift), why, why_len); }
// |H(f)|^2 of the stage with these taps and shift (csrc/wideband.h notch_response)
double msk144host_wideband_notch_response(const int8_t* taps, int32_t shift, double f_hz)
{
    msk144wb::NotchParams p{};
    std::memcpy(p.taps, taps, sizeof(p.taps));
    p.shift = shift;
    return msk144wb::notch_response(p, f_hz);
}
// One push of `channels` channels, each with its own entry: taps[channels][64][2], shifts[channels], x[channels][n][2] stored int8
// samples, tails[channels][63][2] raw samples in and out, y[channels][n][2], clipped[channels] (set, not added to).  -1 for a shift
// or an n out of range.
int msk144host_wideband_notch_filter(const int8_t* taps, const int32_t* shifts, int channels, const int8_t* x, int n, int8_t* tails, int8_t* y, int32_t* clipped)
{
    if(channels < 1 || n < 0) return -1;
    for(int c = 0; c < channels; c++)
        if(!msk144wb::check_notch(shifts[c]).empty()) return -1;
    for(int c = 0; c < channels; c++)
    {
        msk144wb::NotchParams p{};
        std::memcpy(p.taps, taps + static_cast<size_t>(c) * sizeof(p.taps), sizeof(p.taps));
        p.shift = shifts[c];
        clipped[c] = 0;
        msk144wb::notch_filter(p, x + static_cast<size_t>(c) * 2 * n, n, tails + static_cast<size_t>(c) * 2 * msk144wb::kNotchTail, y + static_cast<size_t>(c) * 2 * n, &clipped[c]);
    }
    return 0;
}

// "SPEC[/HALFWIDTH]" as the program parses the value of --wideband-notch: -1 when it refuses it; else the number of table entries
// (0 with auto) and out = {auto, halfwidth, period, persist, then per entry: channel, n, f0, f1}, *db the rule's DB; cap counts int32
int msk144host_wideband_notch_parse(const char* arg, int32_t* out, int cap, double* db)
{
    WidebandOptions w;
    if(!parse_wideband_notch(arg, w) || static_cast<size_t>(cap) < 4 + 4 * w.notch_table.size()) return -1;
    out[0] = w.notch_auto ? 1 : 0, out[1] = w.notch_halfwidth, out[2] = w.notch_plan.period, out[3] = w.notch_plan.persist;
    *db = w.notch_plan.db;
    for(size_t i = 0; i < w.notch_table.size(); i++)
    {
        const std::vector<int32_t>& f = w.notch_table[i].second;
        int32_t* e = out + 4 + 4 * i;
        e[0] = w.notch_table[i].first, e[1] = static_cast<int32_t>(f.size()), e[2] = f[0], e[3] = f.size() > 1 ? f[1] : 0;
    }
    return static_cast<int>(w.notch_table.size());
}
// The planner of --wideband-notch=auto (csrc/wideband.h NotchPlanner); nullptr for a plan check_notch_plan refuses
void* msk144host_wideband_notch_planner_new(int channels, double db, int32_t period, int32_t persist, int32_t halfwidth_hz)
{
    msk144wb::NotchPlan plan;
    plan.db = db, plan.period = period, plan.persist = persist;
    if(channels < 1 || !msk144wb::check_notch_plan(plan).empty()) return nullptr;
    return new msk144wb::NotchPlanner(channels, plan, halfwidth_hz);
}
void msk144host_wideband_notch_planner_free(void* p) { delete static_cast<msk144wb::NotchPlanner*>(p); }
// sums[channels][96] of one push; what it added into out_channel, out_hz, out_excess (at most cap; the count is returned)
int msk144host_wideband_notch_planner_push(void* p, const double* sums, int32_t* out_channel, int32_t* out_hz, double* out_excess, int cap)
{
    std::vector<msk144wb::NotchAdded> added;
    static_cast<msk144wb::NotchPlanner*>(p)->push(sums, added);
    for(size_t i = 0; i < added.size() && i < static_cast<size_t>(cap); i++) out_channel[i] = added[i].channel, out_hz[i] = added[i].hz, out_excess[i] = added[i].excess_db;
    return static_cast<int>(added.size());
}
// the stderr line of an added notch
void msk144host_wideband_notch_line(int32_t channel, int32_t hz, double excess_db, int32_t offset_hz, int64_t hop, char* out, int cap)
{
    std::strncpy(out, msk144wb::notch_added_line(msk144wb::NotchAdded{channel, hz, excess_db}, offset_hz, hop).c_str(), static_cast<size_t>(cap) - 1);
    out[cap - 1] = 0;
}

// ---- the per-channel waterfall (csrc/wideband.h: the window, the check, the dB scale, the line, the frequency rule of a ping event) ----

// the default window of msk144_set_wideband_waterfall (periodic Hann) in out[96]; returns 96
int msk144host_wideband_waterfall_window(double* out)
{
    const std::vector<double> w = msk144wb::waterfall_window();
    std::copy(w.begin(), w.end(), out);
    return msk144wb::kWaterfallBins;
}
// 0 when msk144_set_wideband_waterfall takes the window [96] (NULL: the default), else -1 with the refusal text in why
int msk144host_wideband_waterfall_check(const double* window, char* why, int why_len) { return copy_why(msk144wb::check_waterfall(window), why, why_len); }
// (sum w)^2 over the f32 window (NULL: the default), and the dB of a power against it
double msk144host_wideband_waterfall_full(const double* window) { return msk144wb::waterfall_full(window); }
double msk144host_wideband_waterfall_db(double power, double full) { return msk144wb::waterfall_db(power, full); }
// the row's line of the log (--wideband-waterfall=FILE), NUL-terminated in out
void msk144host_wideband_waterfall_line(int32_t channel, int32_t offset_hz, int64_t block, const float* row, double full, char* out, int cap)
{
    std::strncpy(out, msk144wb::waterfall_line(channel, offset_hz, block, row, full).c_str(), static_cast<size_t>(cap) - 1);
    out[cap - 1] = 0;
}
// "FILE[:CHANNELS]" as the program parses it: 0 and out = {1 for `pings` else 0, listed channels, length of FILE, the channels ...}
// (19 values), else -1
int msk144host_wideband_waterfall_parse(const char* arg, int32_t* out)
{
    WidebandOptions w;
    if(!parse_wideband_waterfall(arg, w)) return -1;
    out[0] = w.waterfall_by_pings ? 1 : 0, out[1] = static_cast<int32_t>(w.waterfall_channels.size()), out[2] = static_cast<int32_t>(w.waterfall_file.size());
    for(size_t i = 0; i < w.waterfall_channels.size(); i++) out[3 + i] = w.waterfall_channels[i];
    return 0;
}
// the frequency rule: push and close write at most cap frequencies in Hz, one per reported event, and return their number
void* msk144host_wideband_ping_spectra_new(int channels, int min_blocks)
{
    if(channels < 1 || min_blocks < 1 || min_blocks > msk144wb::kPingMaxMinBlocks) return nullptr;
    return new msk144wb::PingSpectra(channels, min_blocks);
}
void msk144host_wideband_ping_spectra_free(void* s) { delete static_cast<msk144wb::PingSpectra*>(s); }
// records[channels], rows[channels][54][96]
int msk144host_wideband_ping_spectra_push(void* s, const msk144wb::PingRecord* records, const float* rows, int32_t* out, int cap)
{
    std::vector<int32_t> f;
    static_cast<msk144wb::PingSpectra*>(s)->push(records, rows, f);
    for(int i = 0; i < static_cast<int>(f.size()) && i < cap; i++) out[i] = f[static_cast<size_t>(i)];
    return static_cast<int>(f.size());
}
int msk144host_wideband_ping_spectra_close(void* s, int32_t* out, int cap)
{
    std::vector<int32_t> f;
    static_cast<msk144wb::PingSpectra*>(s)->close(f);
    for(int i = 0; i < static_cast<int>(f.size()) && i < cap; i++) out[i] = f[static_cast<size_t>(i)];
    return static_cast<int>(f.size());
}

// "DIR[:CHANNELS[:POST[:PRE]]]" as the program parses it: out[0] = by pings, out[1] = post, out[2] = pre, out[3] = the length of
// DIR, out[4] = listed channels, then the channels (5 + 16 = 21 values at most); -1: refused
int msk144host_wideband_capture_parse(const char* arg, int32_t* out)
{
    WidebandOptions w;
    if(!parse_wideband_capture(arg, w)) return -1;
    out[0] = w.capture_by_pings ? 1 : 0, out[1] = w.capture_params.post, out[2] = w.capture_params.pre, out[3] = static_cast<int32_t>(w.capture_dir.size());
    out[4] = static_cast<int32_t>(w.capture_channels.size());
    for(size_t i = 0; i < w.capture_channels.size(); i++) out[5 + i] = w.capture_channels[i];
    return 0;
}
int msk144host_wideband_capture_default_max_units(int channels) { return capture_default_max_units(static_cast<size_t>(channels)); }
// the capture rule: nullptr for parameters msk144_set_wideband_capture refuses
void* msk144host_wideband_capture_new(int channels, int pre, int post, int max_units, const int32_t* listed, int num_listed)
{
    const msk144wb::CaptureParams p{pre, post, max_units};
    if(channels < 1 || !msk144wb::check_capture(p, listed, num_listed, channels).empty()) return nullptr;
    return new msk144wb::Capture(channels, p, listed, num_listed);
}
void msk144host_wideband_capture_free(void* s) { delete static_cast<msk144wb::Capture*>(s); }
void msk144host_wideband_capture_restart(void* s) { static_cast<msk144wb::Capture*>(s)->restart(); }
void msk144host_wideband_capture_set_hop(void* s, int64_t hop) { static_cast<msk144wb::Capture*>(s)->set_hop(hop); }
// records[channels] or NULL (the detector off): writes at most cap units, *count = the stored ones, and returns the total
int msk144host_wideband_capture_push(void* s, const msk144wb::PingRecord* records, int first, msk144wb::CaptureUnit* out, int cap, int32_t* count)
{
    std::vector<msk144wb::CaptureUnit> u;
    const int32_t total = static_cast<msk144wb::Capture*>(s)->push(records, first != 0, u);
    for(int i = 0; i < static_cast<int>(u.size()) && i < cap; i++) out[i] = u[static_cast<size_t>(i)];
    *count = static_cast<int32_t>(u.size());
    return total;
}
// the file rule: offsets[channels]
void* msk144host_wideband_capture_segments_new(const char* dir, const int32_t* offsets, int channels)
{
    return new msk144wb::CaptureSegments(dir, std::vector<int32_t>(offsets, offsets + channels));
}
void msk144host_wideband_capture_segments_free(void* s) { delete static_cast<msk144wb::CaptureSegments*>(s); }
int msk144host_wideband_capture_segments_push(void* s, const msk144wb::CaptureUnit* units, const int8_t* data, int count)
{
    return static_cast<msk144wb::CaptureSegments*>(s)->push(units, data, count) ? 0 : -1;
}
int msk144host_wideband_capture_segments_close(void* s) { return static_cast<msk144wb::CaptureSegments*>(s)->close() ? 0 : -1; }
// out: at least 96 bytes
void msk144host_wideband_capture_segments_locate(void* s, int channel, int64_t block, char* out)
{
    const std::string f = static_cast<msk144wb::CaptureSegments*>(s)->locate(channel, block);
    std::strncpy(out, f.c_str(), 95);
    out[95] = 0;
}

// "[HOLD[:MIN_UP[:MAX[:ALWAYS]]]]" as the program parses it (NULL: the bare option): out[0] = hold, out[1] = min_up, out[2] = max
// channels, out[3] = always channels, then the first cap - 4 of them; -1: refused
int msk144host_wideband_gate_parse(const char* arg, int32_t* out, int cap)
{
    WidebandOptions w;
    if(!parse_wideband_gate(arg, w)) return -1;
    out[0] = w.gate_params.hold, out[1] = w.gate_params.min_up, out[2] = w.gate_params.max_channels, out[3] = static_cast<int32_t>(w.gate_always.size());
    for(size_t i = 0; i < w.gate_always.size() && 4 + i < static_cast<size_t>(cap); i++) out[4 + i] = w.gate_always[i];
    return 0;
}
// the gate rule: nullptr for parameters msk144_set_wideband_gate refuses; always[channels] or NULL
void* msk144host_wideband_gate_new(int channels, int hold, int min_up, int max_channels, const uint8_t* always)
{
    const msk144wb::GateParams p{hold, min_up, max_channels};
    if(channels < 1 || !msk144wb::check_gate(p, channels).empty()) return nullptr;
    return new msk144wb::Gate(channels, p, always);
}
void msk144host_wideband_gate_free(void* s) { delete static_cast<msk144wb::Gate*>(s); }
void msk144host_wideband_gate_restart(void* s) { static_cast<msk144wb::Gate*>(s)->restart(); }
// records[channels] or NULL (the detector off): writes at most cap channels, *count = the listed ones, and returns the total
int msk144host_wideband_gate_push(void* s, const msk144wb::PingRecord* records, int first, int32_t* out, int cap, int32_t* count)
{
    std::vector<int32_t> list;
    const int32_t total = static_cast<msk144wb::Gate*>(s)->push(records, first != 0, list);
    for(int i = 0; i < static_cast<int>(list.size()) && i < cap; i++) out[i] = list[static_cast<size_t>(i)];
    *count = static_cast<int32_t>(list.size());
    return total;
}
// out: at least 128 bytes; the text msk144_set_wideband_gate refuses the parameters with, empty when it takes them
void msk144host_wideband_gate_check(int channels, int hold, int min_up, int max_channels, char* out)
{
    const std::string why = msk144wb::check_gate(msk144wb::GateParams{hold, min_up, max_channels}, channels);
    std::strncpy(out, why.c_str(), 127);
    out[127] = 0;
}

void* msk144host_table_new(){ return new CallHashTable(); }
void msk144host_table_free(void* t) { delete static_cast<CallHashTable*>(t); }
void msk144host_table_clear(void* t) { static_cast<CallHashTable*>(t)->clear(); }
unsigned msk144host_hash(const char* call, int bits) { return CallHashTable::hash(call, bits); }

int msk144host_message_gate(const unsigned char* bits77) { return message_gate(bits77) ? 1 : 0; }

// out: at least 64 bytes
int msk144host_decode_message(void* table, const unsigned char* bits77, char* out)
{
    std::string text;
    const bool ok = decode_message(bits77, *static_cast<CallHashTable*>(table), text);
    std::strncpy(out, text.c_str(), 63);
    out[63] = 0;
    return ok ? 1 : 0;
}

void* msk144host_snr_new() { return new SnrTracker(); }
void msk144host_snr_free(void* s) { delete static_cast<SnrTracker*>(s); }
int msk144host_snr_update(void* s, const float* seg8)
{
    static_cast<SnrTracker*>(s)->update(seg8);
    return static_cast<SnrTracker*>(s)->snr_int();
}
float msk144host_snr_db(void* s) { return static_cast<SnrTracker*>(s)->snr_db(); }

// Post-process one window.  accepted: n records of {f0, num_avg, nbadsync, pattern_idx, bits[77]} in
// item order.  Lines are written as a '\n'-joined string of format_line() outputs with the date field
// blanked (tests mask it anyway).  Returns the number of lines.
struct msk144host_accepted
{
    float f0;
    int num_avg;
    int nbadsync;
    int pattern_idx;
    unsigned char bits[77];
};

int msk144host_postprocess(void* table, const msk144host_accepted* acc, int n, int snr, int quirk, char* out, int out_cap)
{
    std::vector<AcceptedCandidate> v(n);
    for(int i = 0; i < n; i++)
    {
        v[i].f0 = acc[i].f0;
        v[i].num_avg = acc[i].num_avg;
        v[i].nbadsync = acc[i].nbadsync;
        v[i].pattern_idx = acc[i].pattern_idx;
        std::memcpy(v[i].bits, acc[i].bits, 77);
    }
    ResultFilter filter;
    std::vector<FilteredResult> lines = postprocess_window(v, snr, quirk != 0, *static_cast<CallHashTable*>(table), filter);
    std::string joined;
    for(size_t i = 0; i < lines.size(); i++)
    {
        if(i) joined += "\n";
        joined += lines[i].format_line();
    }
    std::strncpy(out, joined.c_str(), out_cap - 1);
    out[out_cap - 1] = 0;
    return static_cast<int>(lines.size());
}

// ---- ResultFilter alone (tests/test_ref_host.py drives it side by side with the reference's compiled class) ----
void* msk144host_filter_new() { return new ResultFilter(); }
void msk144host_filter_free(void* f) { delete static_cast<ResultFilter*>(f); }
void msk144host_filter_begin(void* f) { static_cast<ResultFilter*>(f)->begin_window(); }
void msk144host_filter_put(void* f, int snr, float f0, int num_avg, int nbadsync, int pattern_idx, const char* text)
{
    static_cast<ResultFilter*>(f)->put(snr, f0, num_avg, nbadsync, pattern_idx, text);
}
// writes the window's lines as records {snr, f0, num_avg, nbadsync, pattern_idx, text[64]}; returns their number
struct msk144host_filtered
{
    int snr;
    float f0;
    int num_avg;
    int nbadsync;
    int pattern_idx;
    char text[64];
};
int msk144host_filter_end(void* f, msk144host_filtered* out, int cap)
{
    const std::vector<FilteredResult> r = static_cast<ResultFilter*>(f)->end_window();
    for(int i = 0; i < static_cast<int>(r.size()) && i < cap; i++)
    {
        out[i].snr = r[i].snr;
        out[i].f0 = r[i].f0;
        out[i].num_avg = r[i].num_avg;
        out[i].nbadsync = r[i].nbadsync;
        out[i].pattern_idx = r[i].pattern_idx;
        std::strncpy(out[i].text, r[i].text.c_str(), sizeof(out[i].text) - 1);
        out[i].text[sizeof(out[i].text) - 1] = 0;
    }
    return static_cast<int>(r.size());
}

// ---- the search-context tables libmsk144hip.so hands to its kernels (csrc/msk144_tables.h), for CPU-side pinning ----
void msk144host_sync_template(float* re42, float* im42, float* pp12) { msk144::sync_template(re42, im42, pp12); }
int msk144host_frequency_grid(float center, float width, float step, float* out, int cap)
{
    const std::vector<float> f = msk144::frequency_grid(center, width, step);
    for(int i = 0; i < static_cast<int>(f.size()) && i < cap; i++) out[i] = f[i];
    return static_cast<int>(f.size());
}
int msk144host_fft_band_mask(float* out, int cap)
{
    const std::vector<float> w = msk144::fft_band_mask();
    for(int i = 0; i < static_cast<int>(w.size()) && i < cap; i++) out[i] = w[i];
    return static_cast<int>(w.size());
}

// ---- the input-rate contract (csrc/input_rate.h), the functions msk144_set_input_rate and msk144hipdecoder apply ----
// The default integer taps for Fs = 12000 P/Q, h[k] = rint(2^14 d[k]) with d the channel filter's design, for shift 14: L = K*P taps
// into out; returns L, or -1 for a rate or K the contract refuses.
int msk144host_input_rate_taps(int64_t rate_hz, int K, int16_t* out)
{
    if(!msk144ir::check_rate(rate_hz).empty() || K < 1 || K > msk144ir::kMaxTapsPerPhase) return -1;
    const std::vector<int16_t> h = msk144ir::default_taps(rate_hz, K);
    if(out) std::memcpy(out, h.data(), sizeof(int16_t) * h.size());
    return static_cast<int>(h.size());
}

// check_config: returns 0 when valid, else -1 with the refusal text in why
int msk144host_input_rate_check(int64_t rate_hz, int shift, int num_taps, const int16_t* taps, char* why, int why_len)
{
    const std::string s = msk144ir::check_config(rate_hz, shift, num_taps, taps);
    if(why && why_len > 0)
    {
        std::strncpy(why, s.c_str(), static_cast<size_t>(why_len) - 1);
        why[why_len - 1] = 0;
    }
    return s.empty() ? 0 : -1;
}

// The resampler in the integers of the contract (msk144ir::Resampler), for a configuration msk144host_input_rate_check accepts (NULL
// otherwise).  push: x holds 2 x 2592 P/Q samples for a first hop, else 2592 P/Q; y gets 5184 or 2592; returns the clamped outputs,
// or -1 for a later hop before a first one.
void* msk144host_input_rate_new(int channels, int64_t rate_hz, const int16_t* taps, int num_taps, int shift)
{
    if(channels < 1 || !msk144ir::check_config(rate_hz, shift, num_taps, taps).empty()) return nullptr;
    return new msk144ir::Resampler(channels, rate_hz, taps, num_taps, shift);
}
int msk144host_input_rate_push(void* r, int stream, const int16_t* x, int first, int16_t* y)
{
    msk144ir::Resampler* p = static_cast<msk144ir::Resampler*>(r);
    if(!p || stream < 0 || stream >= static_cast<int>(p->started.size())) return -1;
    return p->push(stream, x, first != 0, y);
}
void msk144host_input_rate_free(void* r) { delete static_cast<msk144ir::Resampler*>(r); }

// ---- per-stream levels and pings (csrc/stream_pings.h: what msk144_set_stream_pings checks and the kernel computes) ----
// p = {ratio_q4, memory, min_ref, shift}: 0 when msk144_set_stream_pings takes them, else -1 with the refusal text in why
int msk144host_stream_pings_check(const int32_t* p, char* why, int why_len) { return copy_why(msk144sp::check_params(msk144sp::Params{p[0], p[1], p[2], p[3]}), why, why_len); }
// the defaults of msk144_stream_pings_params, in the same order
void msk144host_stream_pings_defaults(int32_t* out4)
{
    const msk144sp::Params p;
    out4[0] = p.ratio_q4, out4[1] = p.memory, out4[2] = p.min_ref, out4[3] = p.shift;
}
// the detector of `streams` streams with their histories and seen-bits (NULL for parameters the library refuses) ...
void* msk144host_stream_pings_new(int streams, const int32_t* p)
{
    const msk144sp::Params pp{p[0], p[1], p[2], p[3]};
    if(streams < 1 || !msk144sp::check_params(pp).empty()) return nullptr;
    return new msk144sp::Model(streams, pp);
}
void msk144host_stream_pings_free(void* m) { delete static_cast<msk144sp::Model*>(m); }
// ... and one listed position of a push: x holds 5184 samples when first, else 2592; record, level and energies[54] come back.
// -1 for a stream the model does not have
int msk144host_stream_pings_push(void* m, int stream, int first, const int16_t* x, msk144wb::PingRecord* record, msk144sp::Level* level, int32_t* energies)
{
    msk144sp::Model* pm = static_cast<msk144sp::Model*>(m);
    if(!pm || stream < 0 || stream >= pm->streams()) return -1;
    *record = pm->push(stream, first != 0, x, *level, energies);
    return 0;
}
// the event's line of the log (--stream-pings=FILE), NUL-terminated in out
void msk144host_stream_ping_line(const msk144wb::PingEvent* e, char* out, int cap)
{
    std::strncpy(out, msk144sp::event_line(*e).c_str(), static_cast<size_t>(cap) - 1);
    out[cap - 1] = 0;
}
// "FILE[:RATIO[:MIN_BLOCKS[:MEMORY[:SHIFT]]]]" as the program parses it: 0 and out5 = {ratio_q4, min_blocks, memory, shift, length of FILE}, else -1
int msk144host_stream_pings_parse(const char* arg, int32_t* out5)
{
    std::string file;
    msk144sp::Params p;
    int min_blocks = 0;
    if(!parse_stream_pings(arg, file, p, min_blocks)) return -1;
    out5[0] = p.ratio_q4, out5[1] = min_blocks, out5[2] = p.memory, out5[3] = p.shift, out5[4] = static_cast<int32_t>(file.size());
    return 0;
}

// ---- the stream gate (csrc/stream_gate.h: what msk144_set_stream_gate checks and the plan kernel computes) ----
// p = {hold, min_up, max_streams, ratio_q4}: 0 when msk144_set_stream_gate takes them on a handle of `streams` streams, else -1 with
// the refusal text in why
int msk144host_stream_gate_check(int streams, const int32_t* p, char* why, int why_len)
{
    return copy_why(msk144sg::check_params(msk144sg::Params{p[0], p[1], p[2], p[3]}, streams), why, why_len);
}
// the gate of `streams` streams with their `since` and seen-bits; always[streams] or NULL (NULL back for parameters the library refuses) ...
void* msk144host_stream_gate_new(int streams, const int32_t* p, const uint8_t* always)
{
    const msk144sg::Params pp{p[0], p[1], p[2], p[3]};
    if(streams < 1 || !msk144sg::check_params(pp, streams).empty()) return nullptr;
    return new msk144sg::Model(streams, pp, always);
}
void msk144host_stream_gate_free(void* m) { delete static_cast<msk144sg::Model*>(m); }
// ... and one push of n listed positions: ids[n] ascending, is_first[n], the detector's records[n] and energies[n][54], or both NULL
// (the detector is off).  list[n] gets the listed positions; returns the total, or -1 for ids the model does not take.  since_out
// (or NULL): since[streams] behind the push
int msk144host_stream_gate_push(void* m, int n, const int32_t* ids, const uint8_t* is_first, const msk144wb::PingRecord* records, const int32_t* energies, int32_t* list,
                                int32_t* count, int32_t* since_out)
{
    msk144sg::Model* pm = static_cast<msk144sg::Model*>(m);
    if(!pm || n < 0 || n > pm->streams() || (records == nullptr) != (energies == nullptr)) return -1;
    for(int j = 0; j < n; j++)
        if(ids[j] < 0 || ids[j] >= pm->streams() || (j > 0 && ids[j] <= ids[j - 1])) return -1;
    std::vector<int32_t> out;
    const int32_t total = pm->push(n, ids, is_first, records, energies, out);
    std::copy(out.begin(), out.end(), list);
    *count = static_cast<int32_t>(out.size());
    for(int s = 0; since_out && s < pm->streams(); s++) since_out[s] = pm->since(s);
    return total;
}
// "[HOLD[:MIN_UP[:MAX[:RATIO[:ALWAYS]]]]]" as the program parses it: the number of ALWAYS streams (into always, at most cap of
// them) and out4 = {hold, min_up, max_streams, ratio_q4}, else -1
int msk144host_stream_gate_parse(const char* arg, int32_t* out4, int32_t* always, int cap)
{
    msk144sg::Params p;
    std::vector<int32_t> a;
    if(!parse_stream_gate(arg, p, a)) return -1;
    out4[0] = p.hold, out4[1] = p.min_up, out4[2] = p.max_streams, out4[3] = p.ratio_q4;
    for(size_t i = 0; i < a.size() && i < static_cast<size_t>(cap); i++) always[i] = a[i];
    return static_cast<int>(a.size());
}

}  // extern "C"
