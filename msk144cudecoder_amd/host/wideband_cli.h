// msk144hipdecoder --wideband-rate: option parsing and the library entries of the wideband channeliser.  Header-only: the entries
// are resolved with dlsym when the option is given, so a program built against a library without them still links and runs in
// every other mode.
#pragma once

#include "../../include/msk144hip.h"
#include "../csrc/wideband.h"

#include <dlfcn.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace msk144host
{

struct WidebandOptions
{
    long long rate_hz = 0;  // 0: not in wideband mode
    int format = msk144wb::kCu8;
    int taps_per_phase = msk144wb::kDefaultTapsPerPhase;
    float gain = msk144wb::kDefaultGain;
    bool agc = false;     // --wideband-gain=auto[:G0]: the stepped AGC with the default parameters, base gain `gain`
    bool levels = false;  // --wideband-levels: the per-channel table in the summary
    bool blanker = false; // --wideband-blanker[=RATIO[:PRE[:POST]]]: the impulse-noise blanker on the input stream
    msk144wb::BlankerParams blanker_params;
    bool spectrum = false; // --wideband-spectrum=FILE[:BINS[:HOPS]]: the input spectrum, one line per HOPS pushes appended to FILE
    std::string spectrum_file;
    int spectrum_bins = msk144wb::kSpectrumDefaultBins;
    int spectrum_hops = 5;
    bool pings = false;    // --wideband-pings=FILE[:RATIO[:MIN_BLOCKS[:MEMORY]]]: the ping detector, one line per closed event appended to FILE
    std::string pings_file;
    msk144wb::PingParams ping_params;
    int ping_min_blocks = msk144wb::kPingDefaultMinBlocks;
    bool ping_ratio_given = false;  // --wideband-pings carried a RATIO
    bool ping_band = false;         // --wideband-pings-band[=HALFWIDTH[:CENTRE]]: the in-band filter ahead of the detector's energies
    std::string ping_band_arg;      // its value, parsed once --center-frequency is known (parse_wideband_ping_band)
    int ping_band_halfwidth = msk144wb::kPingBandDefaultHalfwidthHz;
    int ping_band_centre = 0;
    bool waterfall = false;       // --wideband-waterfall=FILE[:CHANNELS]: the per-channel waterfall, one line per selected row appended to FILE
    std::string waterfall_file;
    bool waterfall_by_pings = true;            // CHANNELS is `pings` (the default; needs --wideband-pings): every up block of every channel
    std::vector<int32_t> waterfall_channels;   // ... or a list of up to 16 channel indices: every block of these
    bool capture = false;         // --wideband-capture=DIR[:CHANNELS[:POST[:PRE]]]: every kept hop of a channel appended to a segment file under DIR
    std::string capture_dir;
    bool capture_by_pings = true;              // CHANNELS is `pings` (the default; needs --wideband-pings): what the rule keeps around activity
    std::vector<int32_t> capture_channels;     // ... or a list of up to 16 channel indices, kept whether active or not
    msk144wb::CaptureParams capture_params;    // max_units is set once the channels are known: min(2 x channels, 512)
    bool audio = false;           // --wideband-audio[=HALFWIDTH[:CENTRE[:TONE]]]: a 12 kHz int16 WAV file beside every capture segment
    std::string audio_arg;                     // its value, parsed once --center-frequency is known (parse_wideband_audio)
    int audio_halfwidth = msk144wb::kAudioDefaultHalfwidthHz;
    int audio_centre = 0;
    int audio_tone = msk144wb::kAudioDefaultToneHz;
    bool notch = false;           // --wideband-notch=SPEC[/HALFWIDTH]: steady carriers taken out of single channels
    bool notch_auto = false;                   // SPEC is auto[:DB[:PERIOD[:PERSIST]]]: the host rule msk144wb::NotchPlanner on the waterfall sums
    msk144wb::NotchPlan notch_plan;
    int notch_halfwidth = msk144wb::kNotchDefaultHalfwidthHz;
    std::vector<std::pair<int32_t, std::vector<int32_t>>> notch_table;  // ... or ch:Hz[+Hz],...: (channel, its frequencies from the channel's offset)
    bool gate = false;            // --wideband-gate[=HOLD[:MIN_UP[:MAX[:ALWAYS]]]]: only the channels with activity are decoded
    msk144wb::GateParams gate_params;          // max_channels 0: every channel
    std::vector<int32_t> gate_always;          // channel indices decoded on every push
    std::vector<int32_t> offsets;
    bool any_option = false;  // some wideband option was given (they all need --wideband-rate)
    int offset_sources = 0;   // --channel-offsets and --channel-grid given (exactly one is needed)
    std::string parse_error;  // first malformed value
};

// One entry of the library that the program takes at run time: its name, and the function-pointer member that receives it
struct ApiEntry
{
    const char* name;
    void* pointer;
};

// Resolves every entry with dlsym; false with "the loaded libmsk144hip has no <feature> (<first missing symbol>)<needs>"
inline bool resolve_entries(const ApiEntry* entries, size_t count, const char* feature, const char* needs, std::string& err)
{
    const char* missing = nullptr;
    for(size_t i = 0; i < count; i++)
    {
        void* p = dlsym(RTLD_DEFAULT, entries[i].name);
        std::memcpy(entries[i].pointer, &p, sizeof(p));  // POSIX: a function pointer and void* have one representation
        if(!p && !missing) missing = entries[i].name;
    }
    if(missing) err = std::string("the loaded libmsk144hip has no ") + feature + " (" + missing + ")" + needs;
    return !missing;
}

// The library entries of wideband mode.  The four of the channeliser are always resolved, those of an option only when it is given.
struct WidebandApi
{
    int (*set)(msk144_handle*, const msk144_wideband_params*) = nullptr;
    int (*slot)(msk144_handle*, int32_t, void**, size_t*) = nullptr;
    int (*push)(msk144_handle*, int32_t, int32_t) = nullptr;
    int (*clip)(msk144_handle*, int64_t*) = nullptr;
    // --wideband-gain=auto, --wideband-levels
    int (*levels)(msk144_handle*, msk144_wideband_level*) = nullptr;
    int (*set_gains)(msk144_handle*, const float*) = nullptr;
    int (*set_agc)(msk144_handle*, const msk144_wideband_agc*) = nullptr;
    // --wideband-blanker
    int (*set_blanker)(msk144_handle*, const msk144_wideband_blanker*) = nullptr;
    int (*blanker_stats)(msk144_handle*, msk144_wideband_blanker_counts*) = nullptr;
    // --wideband-spectrum
    int (*set_spectrum)(msk144_handle*, const msk144_wideband_spectrum_params*) = nullptr;
    int (*spectrum)(msk144_handle*, double*, int64_t*) = nullptr;
    // --wideband-pings
    int (*set_pings)(msk144_handle*, const msk144_wideband_pings_params*) = nullptr;
    int (*pings)(msk144_handle*, msk144_wideband_ping*) = nullptr;
    int (*ping_blocks)(msk144_handle*, int32_t, int32_t*, int32_t*) = nullptr;
    // --wideband-pings-band
    int (*set_ping_band)(msk144_handle*, const msk144_wideband_ping_band_params*) = nullptr;
    // --wideband-waterfall
    int (*set_waterfall)(msk144_handle*, const msk144_wideband_waterfall_params*) = nullptr;
    int (*waterfall)(msk144_handle*, int32_t, float*, int32_t*) = nullptr;
    int (*waterfall_sums)(msk144_handle*, double*) = nullptr;
    // --wideband-notch
    int (*set_notch)(msk144_handle*, const int32_t*, int32_t, const msk144_wideband_notch_params*) = nullptr;
    int (*notch_stats)(msk144_handle*, msk144_wideband_notch_count*) = nullptr;
    // --wideband-capture
    int (*set_capture)(msk144_handle*, const msk144_wideband_capture_params*) = nullptr;
    int (*capture)(msk144_handle*, msk144_wideband_capture_unit*, int8_t*, int32_t*, int32_t*) = nullptr;
    // --wideband-audio
    int (*set_audio)(msk144_handle*, const msk144_wideband_audio_params*) = nullptr;
    int (*capture_audio)(msk144_handle*, int16_t*, int32_t*, int32_t*) = nullptr;
    // --wideband-gate
    int (*set_gate)(msk144_handle*, const msk144_wideband_gate_params*, const uint8_t*) = nullptr;
    int (*gate)(msk144_handle*, int32_t*, int32_t*, int32_t*) = nullptr;

    // Resolves the channeliser's entries and those of every option of `w`, group after group; false with the first group that lacks
    // one: "the loaded libmsk144hip has no <feature> (<first missing symbol>)[: <who> need(s) it]".
    bool resolve(const WidebandOptions& w, std::string& err)
    {
        struct Group
        {
            bool wanted;
            const char *feature, *needs;
            std::vector<ApiEntry> entries;
        };
        const Group groups[] = {
            {true, "wideband channeliser", "", {{"msk144_set_wideband", &set}, {"msk144_wideband_slot", &slot}, {"msk144_push_wideband", &push}, {"msk144_wideband_clip_count", &clip}}},
            {w.agc || w.levels, "per-channel levels or AGC", ": --wideband-gain=auto and --wideband-levels need them",
             {{"msk144_wideband_levels", &levels}, {"msk144_set_wideband_gains", &set_gains}, {"msk144_set_wideband_agc", &set_agc}}},
            {w.blanker, "impulse-noise blanker", ": --wideband-blanker needs it", {{"msk144_set_wideband_blanker", &set_blanker}, {"msk144_wideband_blanker_stats", &blanker_stats}}},
            {w.spectrum, "input spectrum", ": --wideband-spectrum needs it", {{"msk144_set_wideband_spectrum", &set_spectrum}, {"msk144_wideband_spectrum", &spectrum}}},
            {w.pings, "ping detector", ": --wideband-pings needs it", {{"msk144_set_wideband_pings", &set_pings}, {"msk144_wideband_pings", &pings}, {"msk144_wideband_ping_blocks", &ping_blocks}}},
            {w.ping_band, "ping band", ": --wideband-pings-band needs it", {{"msk144_set_wideband_ping_band", &set_ping_band}}},
            {w.waterfall, "waterfall", ": --wideband-waterfall needs it",
             {{"msk144_set_wideband_waterfall", &set_waterfall}, {"msk144_wideband_waterfall", &waterfall}, {"msk144_wideband_waterfall_sums", &waterfall_sums}}},
            {w.notch, "notch", ": --wideband-notch needs it", {{"msk144_set_wideband_notch", &set_notch}, {"msk144_wideband_notch_stats", &notch_stats}}},
            {w.notch && w.notch_auto, "waterfall", ": --wideband-notch=auto needs it", {{"msk144_set_wideband_waterfall", &set_waterfall}, {"msk144_wideband_waterfall_sums", &waterfall_sums}}},
            {w.capture, "capture", ": --wideband-capture needs it", {{"msk144_set_wideband_capture", &set_capture}, {"msk144_wideband_capture", &capture}}},
            {w.audio, "audio", ": --wideband-audio needs it", {{"msk144_set_wideband_audio", &set_audio}, {"msk144_wideband_capture_audio", &capture_audio}}},
            {w.gate, "gate", ": --wideband-gate needs it", {{"msk144_set_wideband_gate", &set_gate}, {"msk144_wideband_gate", &gate}}},
        };
        for(const Group& g : groups)
            if(g.wanted && !resolve_entries(g.entries.data(), g.entries.size(), g.feature, g.needs, err)) return false;
        return true;
    }
};

// ---- the shared parse helpers ----

inline bool parse_int(const std::string& s, long long& v)
{
    if(s.empty()) return false;
    char* end = nullptr;
    errno = 0;
    v = std::strtoll(s.c_str(), &end, 10);
    return errno == 0 && end && *end == 0;
}

// an integer within lo..hi into `out`
template <class T>
inline bool parse_int_in(const std::string& s, long long lo, long long hi, T& out)
{
    long long v = 0;
    if(!parse_int(s, v) || v < lo || v > hi) return false;
    out = static_cast<T>(v);
    return true;
}

// the fields of "a<sep>b<sep>...", empty ones kept: at least one
inline std::vector<std::string> split_fields(const std::string& s, char sep)
{
    std::vector<std::string> f;
    size_t a = 0;
    while(true)
    {
        const size_t b = s.find(sep, a);
        f.push_back(s.substr(a, b == std::string::npos ? b : b - a));
        if(b == std::string::npos) return f;
        a = b + 1;
    }
}

// "c0,c1,...": up to `max` different non-negative channel indices
inline bool parse_channel_list(const std::string& list, int max, std::vector<int32_t>& out)
{
    for(const std::string& item : split_fields(list, ','))
    {
        int32_t c = 0;
        if(!parse_int_in(item, 0, INT32_MAX, c) || std::find(out.begin(), out.end(), c) != out.end()) return false;
        out.push_back(c);
        if(out.size() > static_cast<size_t>(max)) return false;
    }
    return true;
}

// RATIO, a decimal ratio within 0..1e6, kept as rint(16 x RATIO) (whether the library takes it is the option's own check)
inline bool parse_ratio_q4(const std::string& s, int32_t& q4)
{
    char* end = nullptr;
    const double r = std::strtod(s.c_str(), &end);
    if(s.empty() || !end || *end != 0 || !(r >= 0.0 && r <= 1e6)) return false;
    q4 = static_cast<int32_t>(std::lrint(16.0 * r));
    return true;
}

// ---- the options ----

// "G" or "auto[:G0]"
inline bool parse_wideband_gain(const std::string& s, WidebandOptions& w)
{
    std::string g = s;
    w.agc = false;
    if(s.compare(0, 4, "auto") == 0)
    {
        w.agc = true;
        w.gain = msk144wb::kDefaultGain;
        if(s.size() == 4) return true;
        if(s[4] != ':') return false;
        g = s.substr(5);
    }
    char* end = nullptr;
    w.gain = std::strtof(g.c_str(), &end);
    return !g.empty() && end && *end == 0;
}

// "RATIO[:PRE[:POST]]": RATIO a decimal power ratio to the push's mean power; PRE, POST in samples.  NULL (the bare option): the
// defaults.
inline bool parse_wideband_blanker(const char* arg, WidebandOptions& w)
{
    w.blanker = true;
    w.blanker_params = msk144wb::BlankerParams();
    if(!arg) return true;
    const std::vector<std::string> f = split_fields(arg, ':');
    if(f.size() > 3 || !parse_ratio_q4(f[0], w.blanker_params.threshold_q4)) return false;
    if(f.size() > 1 && !parse_int_in(f[1], INT32_MIN, INT32_MAX, w.blanker_params.pre)) return false;
    if(f.size() > 2 && !parse_int_in(f[2], INT32_MIN, INT32_MAX, w.blanker_params.post)) return false;
    return msk144wb::check_blanker(w.blanker_params).empty();
}

// "FILE[:BINS[:HOPS]]": BINS a power of two within 256..8192 (whether a push is long enough needs the rate: check_wideband_options),
// HOPS >= 1 pushes per line
inline bool parse_wideband_spectrum(const std::string& s, WidebandOptions& w)
{
    w.spectrum = true;
    const std::vector<std::string> f = split_fields(s, ':');
    w.spectrum_file = f[0];
    if(f[0].empty() || f.size() > 3) return false;
    if(f.size() > 1 && (!parse_int_in(f[1], msk144wb::kSpectrumMinBins, msk144wb::kSpectrumMaxBins, w.spectrum_bins) || (w.spectrum_bins & (w.spectrum_bins - 1)) != 0)) return false;
    return f.size() < 3 || parse_int_in(f[2], 1, 1000000, w.spectrum_hops);
}

// "FILE[:RATIO[:MIN_BLOCKS[:MEMORY]]]": RATIO a decimal ratio to the reference, within 16..65535 as q4; MIN_BLOCKS 1..64 blocks of
// 8 ms an event must have; MEMORY 0..16 earlier pushes
inline bool parse_wideband_pings(const std::string& s, WidebandOptions& w)
{
    w.pings = true;
    w.ping_params = msk144wb::PingParams();
    w.ping_min_blocks = msk144wb::kPingDefaultMinBlocks;
    const std::vector<std::string> f = split_fields(s, ':');
    w.pings_file = f[0];
    w.ping_ratio_given = f.size() > 1;
    if(f[0].empty() || f.size() > 4) return false;
    if(f.size() > 1 && !parse_ratio_q4(f[1], w.ping_params.ratio_q4)) return false;
    if(f.size() > 2 && !parse_int_in(f[2], 1, msk144wb::kPingMaxMinBlocks, w.ping_min_blocks)) return false;
    if(f.size() > 3 && !parse_int_in(f[3], INT32_MIN, INT32_MAX, w.ping_params.memory)) return false;
    return msk144wb::check_pings(w.ping_params).empty();
}

// "[HALFWIDTH[:CENTRE]]", behind every other option: HALFWIDTH 500..3000 Hz (1500), CENTRE an integer (centre_default, the value of
// --center-frequency) with |CENTRE| + HALFWIDTH <= 6000.  Without a RATIO in --wideband-pings the detector's ratio becomes the
// band's default.  (Whether there is a detector needs the other options: check_wideband_options.)
inline bool parse_wideband_ping_band(const std::string& s, int centre_default, WidebandOptions& w)
{
    w.ping_band = true;
    w.ping_band_halfwidth = msk144wb::kPingBandDefaultHalfwidthHz;
    w.ping_band_centre = centre_default;
    if(!w.ping_ratio_given) w.ping_params.ratio_q4 = msk144wb::kPingBandDefaultRatioQ4;
    if(!s.empty())
    {
        const std::vector<std::string> f = split_fields(s, ':');
        if(f.size() > 2 || !parse_int_in(f[0], INT32_MIN, INT32_MAX, w.ping_band_halfwidth)) return false;
        if(f.size() > 1 && !parse_int_in(f[1], INT32_MIN, INT32_MAX, w.ping_band_centre)) return false;
    }
    return msk144wb::check_ping_band_design(w.ping_band_centre, w.ping_band_halfwidth).empty();
}

// "FILE[:CHANNELS]": CHANNELS `pings`, or up to 16 different channel indices c0,c1,... (whether they exist and whether `pings` has a
// detector to follow needs the other options: check_wideband_options)
inline bool parse_wideband_waterfall(const std::string& s, WidebandOptions& w)
{
    w.waterfall = true;
    w.waterfall_channels.clear();
    const std::vector<std::string> f = split_fields(s, ':');
    w.waterfall_file = f[0];
    w.waterfall_by_pings = f.size() == 1 || (f.size() == 2 && f[1] == "pings");
    if(f[0].empty() || f.size() > 2) return false;
    return w.waterfall_by_pings || parse_channel_list(f[1], msk144wb::kWaterfallMaxListed, w.waterfall_channels);
}

// "DIR[:CHANNELS[:POST[:PRE]]]": CHANNELS `pings`, or up to 16 different channel indices c0,c1,...; POST 0..16 hops, PRE 0 or 1
// (whether the channels exist and whether `pings` has a detector to follow needs the other options: check_wideband_options)
inline bool parse_wideband_capture(const std::string& s, WidebandOptions& w)
{
    w.capture = true;
    w.capture_channels.clear();
    w.capture_params = msk144wb::CaptureParams();
    const std::vector<std::string> f = split_fields(s, ':');
    w.capture_dir = f[0];
    w.capture_by_pings = f.size() == 1 || f[1] == "pings";
    if(f[0].empty() || f.size() > 4) return false;
    if(!w.capture_by_pings && !parse_channel_list(f[1], msk144wb::kCaptureMaxListed, w.capture_channels)) return false;
    if(f.size() > 2 && !parse_int_in(f[2], 0, msk144wb::kCaptureMaxPost, w.capture_params.post)) return false;
    return f.size() < 4 || parse_int_in(f[3], 0, 1, w.capture_params.pre);
}

// "[HALFWIDTH[:CENTRE[:TONE]]]", behind every other option: HALFWIDTH 500..3000 Hz (1250), CENTRE an integer (centre_default, the
// value of --center-frequency), TONE the audio frequency CENTRE comes out at (1500); what msk144wb::check_audio_design takes, whose
// refusal text goes to `why` (empty for a value that does not parse).  (Whether there is a capture needs the other options:
// check_wideband_options.)
inline bool parse_wideband_audio(const std::string& s, int centre_default, WidebandOptions& w, std::string& why)
{
    w.audio = true;
    w.audio_halfwidth = msk144wb::kAudioDefaultHalfwidthHz;
    w.audio_centre = centre_default;
    w.audio_tone = msk144wb::kAudioDefaultToneHz;
    why.clear();
    if(!s.empty())
    {
        const std::vector<std::string> f = split_fields(s, ':');
        if(f.size() > 3 || !parse_int_in(f[0], INT32_MIN, INT32_MAX, w.audio_halfwidth)) return false;
        if(f.size() > 1 && !parse_int_in(f[1], INT32_MIN, INT32_MAX, w.audio_centre)) return false;
        if(f.size() > 2 && !parse_int_in(f[2], INT32_MIN, INT32_MAX, w.audio_tone)) return false;
    }
    why = msk144wb::check_audio_design(w.audio_centre, w.audio_halfwidth, w.audio_tone);
    return why.empty();
}

// "SPEC[/HALFWIDTH]": HALFWIDTH 50..500 Hz (100); SPEC "auto[:DB[:PERIOD[:PERSIST]]]" - DB a decimal within 1..100, PERIOD 1..100000
// pushes, PERSIST 1..1000 periods - or "ch:Hz[+Hz],ch:Hz,...": different channels, each with one or two integer frequencies that
// msk144wb::check_notch_design takes (whether the channels exist needs the other options: check_wideband_options)
inline bool parse_wideband_notch(const std::string& s, WidebandOptions& w)
{
    w.notch = true;
    w.notch_auto = false;
    w.notch_plan = msk144wb::NotchPlan();
    w.notch_halfwidth = msk144wb::kNotchDefaultHalfwidthHz;
    w.notch_table.clear();
    const std::vector<std::string> parts = split_fields(s, '/');
    if(parts.size() > 2 || parts[0].empty()) return false;
    if(parts.size() > 1 && !parse_int_in(parts[1], msk144wb::kNotchMinHalfwidthHz, msk144wb::kNotchMaxHalfwidthHz, w.notch_halfwidth)) return false;
    if(parts[0].compare(0, 4, "auto") == 0)
    {
        const std::vector<std::string> f = split_fields(parts[0], ':');
        w.notch_auto = true;
        if(f[0] != "auto" || f.size() > 4) return false;
        if(f.size() > 1)
        {
            char* end = nullptr;
            w.notch_plan.db = std::strtod(f[1].c_str(), &end);
            if(f[1].empty() || !end || *end != 0) return false;
        }
        if(f.size() > 2 && !parse_int_in(f[2], 1, msk144wb::kNotchPlanMaxPeriod, w.notch_plan.period)) return false;
        if(f.size() > 3 && !parse_int_in(f[3], 1, msk144wb::kNotchPlanMaxPersist, w.notch_plan.persist)) return false;
        return msk144wb::check_notch_plan(w.notch_plan).empty();
    }
    for(const std::string& item : split_fields(parts[0], ','))
    {
        const size_t colon = item.find(':');
        int32_t c = 0;
        if(colon == std::string::npos || !parse_int_in(item.substr(0, colon), 0, INT32_MAX, c)) return false;
        for(const auto& e : w.notch_table)
            if(e.first == c) return false;
        std::string list = item.substr(colon + 1);
        if(!list.empty() && list[0] == '+') list.erase(0, 1);  // "+300" is 300
        std::vector<int32_t> freqs;
        for(const std::string& hz : split_fields(list, '+'))
        {
            int32_t f = 0;
            if(!parse_int_in(hz, INT32_MIN, INT32_MAX, f)) return false;
            freqs.push_back(f);
        }
        if(!msk144wb::check_notch_design(freqs.data(), static_cast<int>(freqs.size()), w.notch_halfwidth).empty()) return false;
        w.notch_table.emplace_back(c, freqs);
    }
    return true;
}

// "[HOLD[:MIN_UP[:MAX[:ALWAYS]]]]": HOLD 0..16 hops, MIN_UP 1..27 blocks, MAX channels decoded per push (0: all), ALWAYS different
// channel indices c0,c1,... decoded on every push; an empty field keeps its default.  NULL (the bare option): the defaults.
// (Whether MAX and the channels fit, and whether there is a detector to follow, needs the other options: check_wideband_options.)
inline bool parse_wideband_gate(const char* arg, WidebandOptions& w)
{
    w.gate = true;
    w.gate_params = msk144wb::GateParams();
    w.gate_always.clear();
    if(!arg) return true;
    const std::vector<std::string> f = split_fields(arg, ':');
    if(f.size() > 4) return false;
    if(!f[0].empty() && !parse_int_in(f[0], 0, msk144wb::kGateMaxHold, w.gate_params.hold)) return false;
    if(f.size() > 1 && !f[1].empty() && !parse_int_in(f[1], 1, msk144wb::kHopBlocks, w.gate_params.min_up)) return false;
    if(f.size() > 2 && !f[2].empty() && !parse_int_in(f[2], 0, INT32_MAX, w.gate_params.max_channels)) return false;
    return f.size() < 4 || f[3].empty() || parse_channel_list(f[3], INT32_MAX - 1, w.gate_always);
}

inline bool parse_wideband_format(const std::string& s, int& fmt)
{
    if(s == "cu8") fmt = msk144wb::kCu8;
    else if(s == "cs8") fmt = msk144wb::kCs8;
    else if(s == "cs16") fmt = msk144wb::kCs16;
    else return false;
    return true;
}

// "f1,f2,..." in integer Hz
inline bool parse_offset_list(const std::string& list, std::vector<int32_t>& out)
{
    for(const std::string& item : split_fields(list, ','))
    {
        int32_t f = 0;
        if(!parse_int_in(item, INT32_MIN, INT32_MAX, f)) return false;
        out.push_back(f);
    }
    return true;
}

// "first:step:count" -> first, first+step, ... (count >= 1)
inline bool parse_offset_grid(const std::string& spec, std::vector<int32_t>& out)
{
    const std::vector<std::string> f = split_fields(spec, ':');
    long long first = 0, step = 0, count = 0;
    if(f.size() != 3 || !parse_int(f[0], first) || !parse_int(f[1], step) || !parse_int_in(f[2], 1, 1000000, count)) return false;
    for(long long i = 0; i < count; i++)
    {
        const long long hz = first + i * step;
        if(hz < INT32_MIN || hz > INT32_MAX) return false;
        out.push_back(static_cast<int32_t>(hz));
    }
    return true;
}

// One option of the command line by its name: false when `name` is no wideband option, else it is taken into `w` - a malformed value
// as the first parse error, which check_wideband_options reports.  --wideband-pings-band and --wideband-audio keep their values for
// parse_wideband_ping_band and parse_wideband_audio, behind the whole line.
inline bool take_wideband_option(const std::string& name, const char* arg, WidebandOptions& w)
{
    const std::string value = arg ? arg : "";
    long long v = 0;
    bool good = true;
    if(name == "wideband-rate") good = parse_int(value, v) && (w.rate_hz = v) > 0;
    else if(name == "wideband-format") good = parse_wideband_format(value, w.format);
    else if(name == "channel-offsets") good = parse_offset_list(value, w.offsets), w.offset_sources++;
    else if(name == "channel-grid") good = parse_offset_grid(value, w.offsets), w.offset_sources++;
    else if(name == "wideband-gain") good = parse_wideband_gain(value, w);
    else if(name == "taps-per-phase") good = parse_int_in(value, 1, msk144wb::kMaxTapsPerPhase, w.taps_per_phase);
    else if(name == "wideband-levels") w.levels = true;
    else if(name == "wideband-blanker") good = parse_wideband_blanker(arg, w);
    else if(name == "wideband-spectrum") good = parse_wideband_spectrum(value, w);
    else if(name == "wideband-pings") good = parse_wideband_pings(value, w);
    else if(name == "wideband-waterfall") good = parse_wideband_waterfall(value, w);
    else if(name == "wideband-capture") good = parse_wideband_capture(value, w);
    else if(name == "wideband-pings-band") w.ping_band = true, w.ping_band_arg = value;
    else if(name == "wideband-audio") w.audio = true, w.audio_arg = value;
    else if(name == "wideband-notch") good = parse_wideband_notch(value, w);
    else if(name == "wideband-gate") good = parse_wideband_gate(arg, w);
    else return false;
    w.any_option = true;
    if(!good && w.parse_error.empty()) w.parse_error = "bad value for --" + name + ": '" + value + "'";
    return true;
}

// every rule the program checks before it touches the library; empty = valid
inline std::string check_wideband_options(const WidebandOptions& w)
{
    if(!w.parse_error.empty()) return w.parse_error;
    if(w.rate_hz <= 0)
    {
        const std::pair<bool, const char*> own_line[] = {{w.blanker, "--wideband-blanker"},      {w.spectrum, "--wideband-spectrum"},   {w.pings, "--wideband-pings"},
                                                         {w.ping_band, "--wideband-pings-band"}, {w.waterfall, "--wideband-waterfall"}, {w.capture, "--wideband-capture"},
                                                         {w.notch, "--wideband-notch"},          {w.gate, "--wideband-gate"},
                                                         {w.audio, "--wideband-audio"}};
        for(const auto& o : own_line)
            if(o.first) return std::string(o.second) + " needs --wideband-rate=HZ";
        return w.levels ? "--wideband-format, --channel-offsets, --channel-grid, --wideband-gain, --wideband-levels and --taps-per-phase need --wideband-rate=HZ"
                        : "--wideband-format, --channel-offsets, --channel-grid, --wideband-gain and --taps-per-phase need --wideband-rate=HZ";
    }
    if(w.offset_sources != 1) return "--wideband-rate needs exactly one of --channel-offsets=f1,f2,... or --channel-grid=first:step:count";
    const std::string why = msk144wb::check_config(w.rate_hz, w.format, w.taps_per_phase, w.gain, w.offsets.data(), static_cast<int>(w.offsets.size()));
    if(!why.empty()) return why;
    if(w.agc && !msk144wb::gain_ok(w.gain, msk144wb::AgcParams().max_exp)) return "--wideband-gain=auto:G0 needs 128 x G0 x 2^20 finite (the top of the AGC's ladder)";
    if(w.spectrum)
    {
        const std::string bad = msk144wb::check_spectrum(w.spectrum_bins, nullptr, 2592 * w.rate_hz / msk144wb::kOutRate);
        if(!bad.empty()) return "--wideband-spectrum: " + bad;
    }
    if(w.ping_band && !w.pings) return "--wideband-pings-band needs --wideband-pings=FILE";
    if(w.waterfall && w.waterfall_by_pings && !w.pings) return "--wideband-waterfall=FILE needs a channel list (FILE:c0,c1,...) without --wideband-pings";
    for(size_t i = 0; w.waterfall && i < w.waterfall_channels.size(); i++)
        if(static_cast<size_t>(w.waterfall_channels[i]) >= w.offsets.size())
            return "--wideband-waterfall: channel " + std::to_string(w.waterfall_channels[i]) + " is not one of the " + std::to_string(w.offsets.size()) + " channels";
    if(w.capture && w.capture_by_pings && !w.pings) return "--wideband-capture=DIR needs a channel list (DIR:c0,c1,...) without --wideband-pings";
    for(size_t i = 0; w.capture && i < w.capture_channels.size(); i++)
        if(static_cast<size_t>(w.capture_channels[i]) >= w.offsets.size())
            return "--wideband-capture: channel " + std::to_string(w.capture_channels[i]) + " is not one of the " + std::to_string(w.offsets.size()) + " channels";
    if(w.audio && !w.capture) return "--wideband-audio needs --wideband-capture=DIR";
    for(const auto& e : w.notch_table)
        if(static_cast<size_t>(e.first) >= w.offsets.size())
            return "--wideband-notch: channel " + std::to_string(e.first) + " is not one of the " + std::to_string(w.offsets.size()) + " channels";
    if(w.gate)
    {
        if(!w.pings && w.gate_always.empty()) return "--wideband-gate needs --wideband-pings=FILE, or a list of channels that are always decoded (HOLD:MIN_UP:MAX:c0,c1,...)";
        const std::string bad = msk144wb::check_gate(w.gate_params, static_cast<int>(w.offsets.size()));
        if(!bad.empty()) return "--wideband-gate: " + bad;
        for(int32_t c : w.gate_always)
            if(static_cast<size_t>(c) >= w.offsets.size())
                return "--wideband-gate: channel " + std::to_string(c) + " is not one of the " + std::to_string(w.offsets.size()) + " channels";
    }
    return "";
}

// the program's max_units: min(2 x channels, 512)
inline int32_t capture_default_max_units(size_t channels)
{
    return static_cast<int32_t>(std::min<size_t>(2 * channels, static_cast<size_t>(msk144wb::kCaptureDefaultMaxUnits)));
}

}  // namespace msk144host
