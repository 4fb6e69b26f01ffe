// msk144hipdecoder --wideband-rate: option parsing and the library entries of the wideband channeliser.  Header-only: the entries
// are resolved with dlsym when the option is given, so a program built against a library without them still links and runs in
// every other mode.
#pragma once

#include "../../include/msk144hip.h"
#include "../csrc/wideband.h"

#include <dlfcn.h>

#include <cerrno>
#include <cstdlib>
#include <string>
#include <vector>

namespace msk144host
{

struct WidebandApi
{
    int (*set)(msk144_handle*, const msk144_wideband_params*) = nullptr;
    int (*slot)(msk144_handle*, int32_t, void**, size_t*) = nullptr;
    int (*push)(msk144_handle*, int32_t, int32_t) = nullptr;
    int (*clip)(msk144_handle*, int64_t*) = nullptr;
    // --wideband-gain=auto, --wideband-levels: resolved only when one of them is given (load_levels)
    int (*levels)(msk144_handle*, msk144_wideband_level*) = nullptr;
    int (*set_gains)(msk144_handle*, const float*) = nullptr;
    int (*set_agc)(msk144_handle*, const msk144_wideband_agc*) = nullptr;

    bool load_levels(std::string& err)
    {
        levels = reinterpret_cast<decltype(levels)>(dlsym(RTLD_DEFAULT, "msk144_wideband_levels"));
        set_gains = reinterpret_cast<decltype(set_gains)>(dlsym(RTLD_DEFAULT, "msk144_set_wideband_gains"));
        set_agc = reinterpret_cast<decltype(set_agc)>(dlsym(RTLD_DEFAULT, "msk144_set_wideband_agc"));
        if(levels && set_gains && set_agc) return true;
        err = "the loaded libmsk144hip has no per-channel levels or AGC (msk144_wideband_levels): --wideband-gain=auto and --wideband-levels need them";
        return false;
    }

    // --wideband-blanker: resolved only when it is given (load_blanker)
    int (*set_blanker)(msk144_handle*, const msk144_wideband_blanker*) = nullptr;
    int (*blanker_stats)(msk144_handle*, msk144_wideband_blanker_counts*) = nullptr;

    bool load_blanker(std::string& err)
    {
        set_blanker = reinterpret_cast<decltype(set_blanker)>(dlsym(RTLD_DEFAULT, "msk144_set_wideband_blanker"));
        blanker_stats = reinterpret_cast<decltype(blanker_stats)>(dlsym(RTLD_DEFAULT, "msk144_wideband_blanker_stats"));
        if(set_blanker && blanker_stats) return true;
        err = std::string("the loaded libmsk144hip has no impulse-noise blanker (") + (set_blanker ? "msk144_wideband_blanker_stats" : "msk144_set_wideband_blanker") +
              "): --wideband-blanker needs it";
        return false;
    }

    // --wideband-spectrum: resolved only when it is given (load_spectrum)
    int (*set_spectrum)(msk144_handle*, const msk144_wideband_spectrum_params*) = nullptr;
    int (*spectrum)(msk144_handle*, double*, int64_t*) = nullptr;

    bool load_spectrum(std::string& err)
    {
        set_spectrum = reinterpret_cast<decltype(set_spectrum)>(dlsym(RTLD_DEFAULT, "msk144_set_wideband_spectrum"));
        spectrum = reinterpret_cast<decltype(spectrum)>(dlsym(RTLD_DEFAULT, "msk144_wideband_spectrum"));
        if(set_spectrum && spectrum) return true;
        err = std::string("the loaded libmsk144hip has no input spectrum (") + (set_spectrum ? "msk144_wideband_spectrum" : "msk144_set_wideband_spectrum") +
              "): --wideband-spectrum needs it";
        return false;
    }

    // --wideband-pings: resolved only when it is given (load_pings)
    int (*set_pings)(msk144_handle*, const msk144_wideband_pings_params*) = nullptr;
    int (*pings)(msk144_handle*, msk144_wideband_ping*) = nullptr;
    int (*ping_blocks)(msk144_handle*, int32_t, int32_t*, int32_t*) = nullptr;

    bool load_pings(std::string& err)
    {
        set_pings = reinterpret_cast<decltype(set_pings)>(dlsym(RTLD_DEFAULT, "msk144_set_wideband_pings"));
        pings = reinterpret_cast<decltype(pings)>(dlsym(RTLD_DEFAULT, "msk144_wideband_pings"));
        ping_blocks = reinterpret_cast<decltype(ping_blocks)>(dlsym(RTLD_DEFAULT, "msk144_wideband_ping_blocks"));
        if(set_pings && pings && ping_blocks) return true;
        err = std::string("the loaded libmsk144hip has no ping detector (") + (!set_pings ? "msk144_set_wideband_pings" : !pings ? "msk144_wideband_pings" : "msk144_wideband_ping_blocks") +
              "): --wideband-pings needs it";
        return false;
    }

    // --wideband-pings-band: resolved only when it is given (load_ping_band)
    int (*set_ping_band)(msk144_handle*, const msk144_wideband_ping_band_params*) = nullptr;

    bool load_ping_band(std::string& err)
    {
        set_ping_band = reinterpret_cast<decltype(set_ping_band)>(dlsym(RTLD_DEFAULT, "msk144_set_wideband_ping_band"));
        if(set_ping_band) return true;
        err = "the loaded libmsk144hip has no ping band (msk144_set_wideband_ping_band): --wideband-pings-band needs it";
        return false;
    }

    // --wideband-waterfall: resolved only when it is given (load_waterfall)
    int (*set_waterfall)(msk144_handle*, const msk144_wideband_waterfall_params*) = nullptr;
    int (*waterfall)(msk144_handle*, int32_t, float*, int32_t*) = nullptr;
    int (*waterfall_sums)(msk144_handle*, double*) = nullptr;

    bool load_waterfall(std::string& err)
    {
        set_waterfall = reinterpret_cast<decltype(set_waterfall)>(dlsym(RTLD_DEFAULT, "msk144_set_wideband_waterfall"));
        waterfall = reinterpret_cast<decltype(waterfall)>(dlsym(RTLD_DEFAULT, "msk144_wideband_waterfall"));
        waterfall_sums = reinterpret_cast<decltype(waterfall_sums)>(dlsym(RTLD_DEFAULT, "msk144_wideband_waterfall_sums"));
        if(set_waterfall && waterfall && waterfall_sums) return true;
        err = std::string("the loaded libmsk144hip has no waterfall (") +
              (!set_waterfall ? "msk144_set_wideband_waterfall" : !waterfall ? "msk144_wideband_waterfall" : "msk144_wideband_waterfall_sums") + "): --wideband-waterfall needs it";
        return false;
    }

    // --wideband-capture: resolved only when it is given (load_capture)
    int (*set_capture)(msk144_handle*, const msk144_wideband_capture_params*) = nullptr;
    int (*capture)(msk144_handle*, msk144_wideband_capture_unit*, int8_t*, int32_t*, int32_t*) = nullptr;

    bool load_capture(std::string& err)
    {
        set_capture = reinterpret_cast<decltype(set_capture)>(dlsym(RTLD_DEFAULT, "msk144_set_wideband_capture"));
        capture = reinterpret_cast<decltype(capture)>(dlsym(RTLD_DEFAULT, "msk144_wideband_capture"));
        if(set_capture && capture) return true;
        err = std::string("the loaded libmsk144hip has no capture (") + (!set_capture ? "msk144_set_wideband_capture" : "msk144_wideband_capture") + "): --wideband-capture needs it";
        return false;
    }

    bool load(std::string& err)
    {
        set = reinterpret_cast<decltype(set)>(dlsym(RTLD_DEFAULT, "msk144_set_wideband"));
        slot = reinterpret_cast<decltype(slot)>(dlsym(RTLD_DEFAULT, "msk144_wideband_slot"));
        push = reinterpret_cast<decltype(push)>(dlsym(RTLD_DEFAULT, "msk144_push_wideband"));
        clip = reinterpret_cast<decltype(clip)>(dlsym(RTLD_DEFAULT, "msk144_wideband_clip_count"));
        if(set && slot && push && clip) return true;
        err = "the loaded libmsk144hip has no wideband channeliser (msk144_set_wideband)";
        return false;
    }
};

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
    std::vector<int32_t> offsets;
    bool any_option = false;  // some wideband option was given (they all need --wideband-rate)
    int offset_sources = 0;   // --channel-offsets and --channel-grid given (exactly one is needed)
    std::string parse_error;  // first malformed value
};

inline bool parse_int(const std::string& s, long long& v)
{
    if(s.empty()) return false;
    char* end = nullptr;
    errno = 0;
    v = std::strtoll(s.c_str(), &end, 10);
    return errno == 0 && end && *end == 0;
}

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

// "RATIO[:PRE[:POST]]": RATIO a decimal power ratio to the push's mean power, kept as rint(16 x RATIO); PRE, POST in samples.
// NULL (the bare option): the defaults.
inline bool parse_wideband_blanker(const char* arg, WidebandOptions& w)
{
    w.blanker = true;
    w.blanker_params = msk144wb::BlankerParams();
    if(!arg) return true;
    const std::string s = arg;
    const size_t a = s.find(':');
    const size_t b = a == std::string::npos ? a : s.find(':', a + 1);
    const std::string ratio = s.substr(0, a);
    char* end = nullptr;
    const double r = std::strtod(ratio.c_str(), &end);
    if(ratio.empty() || !end || *end != 0 || !(r >= 0.0 && r <= 1e6)) return false;
    w.blanker_params.threshold_q4 = static_cast<int32_t>(std::lrint(16.0 * r));
    long long v = 0;
    if(a != std::string::npos)
    {
        if(!parse_int(s.substr(a + 1, b == std::string::npos ? b : b - a - 1), v) || v < INT32_MIN || v > INT32_MAX) return false;
        w.blanker_params.pre = static_cast<int32_t>(v);
    }
    if(b != std::string::npos)
    {
        if(!parse_int(s.substr(b + 1), v) || v < INT32_MIN || v > INT32_MAX) return false;
        w.blanker_params.post = static_cast<int32_t>(v);
    }
    return msk144wb::check_blanker(w.blanker_params).empty();
}

// "FILE[:BINS[:HOPS]]": BINS a power of two within 256..8192 (whether a push is long enough needs the rate: check_wideband_options),
// HOPS >= 1 pushes per line
inline bool parse_wideband_spectrum(const std::string& s, WidebandOptions& w)
{
    w.spectrum = true;
    const size_t a = s.find(':');
    const size_t b = a == std::string::npos ? a : s.find(':', a + 1);
    w.spectrum_file = s.substr(0, a);
    if(w.spectrum_file.empty() || (b != std::string::npos && s.find(':', b + 1) != std::string::npos)) return false;
    long long v = 0;
    if(a != std::string::npos)
    {
        if(!parse_int(s.substr(a + 1, b == std::string::npos ? b : b - a - 1), v) || v < msk144wb::kSpectrumMinBins || v > msk144wb::kSpectrumMaxBins || (v & (v - 1)) != 0) return false;
        w.spectrum_bins = static_cast<int>(v);
    }
    if(b != std::string::npos)
    {
        if(!parse_int(s.substr(b + 1), v) || v < 1 || v > 1000000) return false;
        w.spectrum_hops = static_cast<int>(v);
    }
    return true;
}

// "FILE[:RATIO[:MIN_BLOCKS[:MEMORY]]]": RATIO a decimal ratio to the reference, kept as rint(16 x RATIO) within 16..65535;
// MIN_BLOCKS 1..64 blocks of 8 ms an event must have; MEMORY 0..16 earlier pushes
inline bool parse_wideband_pings(const std::string& s, WidebandOptions& w)
{
    w.pings = true;
    w.ping_params = msk144wb::PingParams();
    w.ping_min_blocks = msk144wb::kPingDefaultMinBlocks;
    w.ping_ratio_given = false;
    std::vector<std::string> f;
    size_t a = 0;
    while(true)
    {
        const size_t b = s.find(':', a);
        f.push_back(s.substr(a, b == std::string::npos ? b : b - a));
        if(b == std::string::npos) break;
        a = b + 1;
    }
    w.pings_file = f[0];
    if(f[0].empty() || f.size() > 4) return false;
    long long v = 0;
    if(f.size() > 1)
    {
        char* end = nullptr;
        const double r = std::strtod(f[1].c_str(), &end);
        if(f[1].empty() || !end || *end != 0 || !(r >= 0.0 && r <= 1e6)) return false;
        w.ping_params.ratio_q4 = static_cast<int32_t>(std::lrint(16.0 * r));
        w.ping_ratio_given = true;
    }
    if(f.size() > 2)
    {
        if(!parse_int(f[2], v) || v < 1 || v > msk144wb::kPingMaxMinBlocks) return false;
        w.ping_min_blocks = static_cast<int>(v);
    }
    if(f.size() > 3)
    {
        if(!parse_int(f[3], v) || v < INT32_MIN || v > INT32_MAX) return false;
        w.ping_params.memory = static_cast<int32_t>(v);
    }
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
    long long v = 0;
    if(!s.empty())
    {
        const size_t a = s.find(':');
        if(!parse_int(s.substr(0, a), v) || v < INT32_MIN || v > INT32_MAX) return false;
        w.ping_band_halfwidth = static_cast<int>(v);
        if(a != std::string::npos)
        {
            if(!parse_int(s.substr(a + 1), v) || v < INT32_MIN || v > INT32_MAX) return false;
            w.ping_band_centre = static_cast<int>(v);
        }
    }
    return msk144wb::check_ping_band_design(w.ping_band_centre, w.ping_band_halfwidth).empty();
}

// "FILE[:CHANNELS]": CHANNELS `pings`, or up to 16 different channel indices c0,c1,... (whether they exist and whether `pings` has a
// detector to follow needs the other options: check_wideband_options)
inline bool parse_wideband_waterfall(const std::string& s, WidebandOptions& w)
{
    w.waterfall = true;
    w.waterfall_by_pings = true;
    w.waterfall_channels.clear();
    const size_t a = s.find(':');
    w.waterfall_file = s.substr(0, a);
    if(w.waterfall_file.empty()) return false;
    if(a == std::string::npos) return true;
    const std::string list = s.substr(a + 1);
    if(list == "pings") return true;
    w.waterfall_by_pings = false;
    size_t p = 0;
    while(true)
    {
        const size_t q = list.find(',', p);
        long long v = 0;
        if(!parse_int(list.substr(p, q == std::string::npos ? q : q - p), v) || v < 0 || v > INT32_MAX) return false;
        if(std::find(w.waterfall_channels.begin(), w.waterfall_channels.end(), static_cast<int32_t>(v)) != w.waterfall_channels.end()) return false;
        w.waterfall_channels.push_back(static_cast<int32_t>(v));
        if(w.waterfall_channels.size() > static_cast<size_t>(msk144wb::kWaterfallMaxListed)) return false;
        if(q == std::string::npos) break;
        p = q + 1;
    }
    return true;
}

// "DIR[:CHANNELS[:POST[:PRE]]]": CHANNELS `pings`, or up to 16 different channel indices c0,c1,...; POST 0..16 hops, PRE 0 or 1
// (whether the channels exist and whether `pings` has a detector to follow needs the other options: check_wideband_options)
inline bool parse_wideband_capture(const std::string& s, WidebandOptions& w)
{
    w.capture = true;
    w.capture_by_pings = true;
    w.capture_channels.clear();
    w.capture_params = msk144wb::CaptureParams();
    std::vector<std::string> f;
    size_t a = 0;
    while(true)
    {
        const size_t b = s.find(':', a);
        f.push_back(s.substr(a, b == std::string::npos ? b : b - a));
        if(b == std::string::npos) break;
        a = b + 1;
    }
    w.capture_dir = f[0];
    if(f[0].empty() || f.size() > 4) return false;
    long long v = 0;
    if(f.size() > 1 && f[1] != "pings")
    {
        w.capture_by_pings = false;
        size_t p = 0;
        while(true)
        {
            const size_t q = f[1].find(',', p);
            if(!parse_int(f[1].substr(p, q == std::string::npos ? q : q - p), v) || v < 0 || v > INT32_MAX) return false;
            if(std::find(w.capture_channels.begin(), w.capture_channels.end(), static_cast<int32_t>(v)) != w.capture_channels.end()) return false;
            w.capture_channels.push_back(static_cast<int32_t>(v));
            if(w.capture_channels.size() > static_cast<size_t>(msk144wb::kCaptureMaxListed)) return false;
            if(q == std::string::npos) break;
            p = q + 1;
        }
    }
    if(f.size() > 2)
    {
        if(!parse_int(f[2], v) || v < 0 || v > msk144wb::kCaptureMaxPost) return false;
        w.capture_params.post = static_cast<int32_t>(v);
    }
    if(f.size() > 3)
    {
        if(!parse_int(f[3], v) || v < 0 || v > 1) return false;
        w.capture_params.pre = static_cast<int32_t>(v);
    }
    return true;
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
    size_t a = 0;
    while(a <= list.size())
    {
        const size_t b = list.find(',', a);
        long long v = 0;
        if(!parse_int(list.substr(a, b == std::string::npos ? std::string::npos : b - a), v) || v < INT32_MIN || v > INT32_MAX) return false;
        out.push_back(static_cast<int32_t>(v));
        if(b == std::string::npos) break;
        a = b + 1;
    }
    return !out.empty();
}

// "first:step:count" -> first, first+step, ... (count >= 1)
inline bool parse_offset_grid(const std::string& spec, std::vector<int32_t>& out)
{
    const size_t a = spec.find(':');
    const size_t b = a == std::string::npos ? a : spec.find(':', a + 1);
    long long first = 0, step = 0, count = 0;
    if(b == std::string::npos || !parse_int(spec.substr(0, a), first) || !parse_int(spec.substr(a + 1, b - a - 1), step) || !parse_int(spec.substr(b + 1), count))
        return false;
    if(count < 1 || count > 1000000) return false;
    for(long long i = 0; i < count; i++)
    {
        const long long f = first + i * step;
        if(f < INT32_MIN || f > INT32_MAX) return false;
        out.push_back(static_cast<int32_t>(f));
    }
    return true;
}

// every rule the program checks before it touches the library; empty = valid
inline std::string check_wideband_options(const WidebandOptions& w)
{
    if(!w.parse_error.empty()) return w.parse_error;
    if(w.rate_hz <= 0 && w.blanker) return "--wideband-blanker needs --wideband-rate=HZ";
    if(w.rate_hz <= 0 && w.spectrum) return "--wideband-spectrum needs --wideband-rate=HZ";
    if(w.rate_hz <= 0 && w.pings) return "--wideband-pings needs --wideband-rate=HZ";
    if(w.rate_hz <= 0 && w.ping_band) return "--wideband-pings-band needs --wideband-rate=HZ";
    if(w.rate_hz <= 0 && w.waterfall) return "--wideband-waterfall needs --wideband-rate=HZ";
    if(w.rate_hz <= 0 && w.capture) return "--wideband-capture needs --wideband-rate=HZ";
    if(w.rate_hz <= 0)
        return w.levels ? "--wideband-format, --channel-offsets, --channel-grid, --wideband-gain, --wideband-levels and --taps-per-phase need --wideband-rate=HZ"
                        : "--wideband-format, --channel-offsets, --channel-grid, --wideband-gain and --taps-per-phase need --wideband-rate=HZ";
    if(w.offset_sources != 1) return "--wideband-rate needs exactly one of --channel-offsets=f1,f2,... or --channel-grid=first:step:count";
    const std::string why = msk144wb::check_config(w.rate_hz, w.format, w.taps_per_phase, w.gain, w.offsets.data(), static_cast<int>(w.offsets.size()));
    if(why.empty() && w.agc && !msk144wb::gain_ok(w.gain, msk144wb::AgcParams().max_exp))
        return "--wideband-gain=auto:G0 needs 128 x G0 x 2^20 finite (the top of the AGC's ladder)";
    if(why.empty() && w.spectrum)
    {
        const std::string bad = msk144wb::check_spectrum(w.spectrum_bins, nullptr, 2592 * w.rate_hz / msk144wb::kOutRate);
        if(!bad.empty()) return "--wideband-spectrum: " + bad;
    }
    if(why.empty() && w.ping_band && !w.pings) return "--wideband-pings-band needs --wideband-pings=FILE";
    if(why.empty() && w.waterfall && w.waterfall_by_pings && !w.pings) return "--wideband-waterfall=FILE needs a channel list (FILE:c0,c1,...) without --wideband-pings";
    for(size_t i = 0; why.empty() && w.waterfall && i < w.waterfall_channels.size(); i++)
        if(static_cast<size_t>(w.waterfall_channels[i]) >= w.offsets.size())
            return "--wideband-waterfall: channel " + std::to_string(w.waterfall_channels[i]) + " is not one of the " + std::to_string(w.offsets.size()) + " channels";
    if(why.empty() && w.capture && w.capture_by_pings && !w.pings) return "--wideband-capture=DIR needs a channel list (DIR:c0,c1,...) without --wideband-pings";
    for(size_t i = 0; why.empty() && w.capture && i < w.capture_channels.size(); i++)
        if(static_cast<size_t>(w.capture_channels[i]) >= w.offsets.size())
            return "--wideband-capture: channel " + std::to_string(w.capture_channels[i]) + " is not one of the " + std::to_string(w.offsets.size()) + " channels";
    return why;
}

// the program's max_units: min(2 x channels, 512)
inline int32_t capture_default_max_units(size_t channels)
{
    return static_cast<int32_t>(std::min<size_t>(2 * channels, static_cast<size_t>(msk144wb::kCaptureDefaultMaxUnits)));
}

}  // namespace msk144host
