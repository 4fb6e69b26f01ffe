// msk144hipdecoder --input-rate: the option, the library entries of the resampler in front of the hop ring and the end-of-run line.
// Header-only: the entries are resolved with dlsym when the option is given, so a program built against a library without them still
// links and runs in every other mode.
#pragma once

#include "../../include/msk144hip.h"
#include "../csrc/input_rate.h"
#include "wideband_cli.h"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace msk144host
{

struct InputRateApi
{
    int (*set)(msk144_handle*, const msk144_input_rate_params*) = nullptr;
    int (*slot)(msk144_handle*, int32_t, void**, void**, int32_t**, uint8_t**, int32_t*) = nullptr;
    int (*push)(msk144_handle*, int32_t, int32_t) = nullptr;
    int (*slot_clamped)(msk144_handle*, int32_t, const int32_t**, int32_t*) = nullptr;

    bool resolve(std::string& err)
    {
        const ApiEntry entries[] = {{"msk144_set_input_rate", &set}, {"msk144_rate_hop_slot", &slot}, {"msk144_push_rate_hops", &push}, {"msk144_input_rate_slot_clamped", &slot_clamped}};
        return resolve_entries(entries, 4, "input-rate resampler", ": --input-rate needs a library built from these sources", err);
    }
};

// --input-rate=HZ | wav, with --taps-per-phase=K
struct InputRate
{
    bool given = false;     // the option stood on the line
    bool from_wav = false;  // --input-rate=wav: the rate comes from the stream's header
    bool on = false;        // the streams are resampled (a rate other than 12000)
    int64_t rate_hz = 0;
    int taps_per_phase = msk144ir::kDefaultTapsPerPhase;
    InputRateApi api;
    msk144ir::Shape shape;
    std::vector<int16_t> taps;
    std::atomic<long long> clamped{0};  // output samples clamped, every loop's

    // '' or the refusal
    std::string parse(const std::string& value)
    {
        given = true;
        if(value == "wav")
        {
            from_wav = true;
            return "";
        }
        char* end = nullptr;
        const long long v = strtoll(value.c_str(), &end, 10);
        if(value.empty() || *end) return "bad value for --input-rate: '" + value + "' (a rate in Hz, or wav)";
        return set_rate(v);
    }

    // 12000 is the program without the option; any other rate must be one the library takes
    std::string set_rate(int64_t hz)
    {
        rate_hz = hz;
        on = hz != msk144wb::kOutRate;
        if(!on) return "";
        const std::string why = msk144ir::check_rate(hz);
        return why.empty() ? "" : "--input-rate: " + why;
    }

    // after the options are read: the entries and the default taps
    bool prepare(std::string& err)
    {
        if(!on) return true;
        if(!api.resolve(err)) return false;
        taps = msk144ir::default_taps(rate_hz, taps_per_phase);
        shape = msk144ir::shape(rate_hz, static_cast<int>(taps.size()));
        return true;
    }

    bool configure(msk144_handle* h, std::string& err) const
    {
        msk144_input_rate_params p{};
        p.rate_hz = rate_hz;
        p.shift = msk144ir::kDefaultShift;
        p.num_taps = static_cast<int32_t>(taps.size());
        p.taps = taps.data();
        if(api.set(h, &p) == MSK144_OK) return true;
        err = msk144_last_error(h);
        return false;
    }

    size_t row_bytes() const { return static_cast<size_t>(shape.row) * sizeof(int16_t); }

    std::string summary() const
    {
        return "msk144hipdecoder: input rate " + std::to_string(rate_hz) + " Hz = 12000 x " + std::to_string(shape.P) + "/" + std::to_string(shape.Q) + ", " + std::to_string(taps.size()) +
               " taps (" + std::to_string(taps_per_phase) + " per phase), shift " + std::to_string(msk144ir::kDefaultShift) + ", " + std::to_string(clamped.load()) + " samples clamped";
    }
};

// The rate of a canonical 44-byte WAV header: RIFF/WAVE, a 16-byte fmt chunk with PCM tag 1, one channel, 16 bits, then data.
// '' and the rate, or why the header is refused.
inline std::string wav_header_rate(const unsigned char* h, int64_t& rate_hz)
{
    auto u16 = [&](int i) { return static_cast<unsigned>(h[i]) | (static_cast<unsigned>(h[i + 1]) << 8); };
    auto u32 = [&](int i) { return static_cast<uint32_t>(u16(i)) | (static_cast<uint32_t>(u16(i + 2)) << 16); };
    if(std::memcmp(h, "RIFF", 4) != 0 || std::memcmp(h + 8, "WAVEfmt ", 8) != 0 || u32(16) != 16 || std::memcmp(h + 36, "data", 4) != 0)
        return "--input-rate=wav: the stream does not start with a canonical 44-byte WAV header";
    if(u16(20) != 1) return "--input-rate=wav: the header's format tag is " + std::to_string(u16(20)) + ", not PCM (1)";
    if(u16(22) != 1) return "--input-rate=wav: the header has " + std::to_string(u16(22)) + " channels, not one";
    if(u16(34) != 16) return "--input-rate=wav: the header has " + std::to_string(u16(34)) + " bits per sample, not 16";
    rate_hz = u32(24);
    return "";
}

}  // namespace msk144host
