// msk144hipdecoder --stream-gate: the option, the library entries of the stream gate (include/msk144hip.h "Stream gate") and the
// end-of-run line.  Header-only: the entries are resolved with dlsym when the option is given, so a program built against a library
// without them still links and runs in every other mode.  The rule is the library's (csrc/stream_gate.h); nothing here touches the
// GPU or waits for it.
#pragma once

#include "../../include/msk144hip.h"
#include "../csrc/stream_gate.h"
#include "../csrc/stream_pings.h"
#include "wideband_cli.h"

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace msk144host
{

struct StreamGateApi
{
    int (*set)(msk144_handle*, const msk144_stream_gate_params*, const uint8_t*) = nullptr;
    int (*slot)(msk144_handle*, int32_t, const int32_t**, int32_t*, int32_t*) = nullptr;
    int (*set_pings)(msk144_handle*, const msk144_stream_pings_params*) = nullptr;  // the detector, where no other option switches it on

    bool resolve(std::string& err)
    {
        const ApiEntry entries[] = {{"msk144_set_stream_gate", &set}, {"msk144_stream_gate_slot", &slot}, {"msk144_set_stream_pings", &set_pings}};
        return resolve_entries(entries, 3, "stream gate", ": --stream-gate needs a library built from these sources", err);
    }
};

// "[HOLD[:MIN_UP[:MAX[:RATIO[:ALWAYS]]]]]": an empty field keeps its default; RATIO empty or 0 is the detector's own mask.  MAX and
// ALWAYS are held against the number of streams by StreamGate::check
inline bool parse_stream_gate(const std::string& s, msk144sg::Params& p, std::vector<int32_t>& always)
{
    p = msk144sg::Params();
    always.clear();
    const std::vector<std::string> f = split_fields(s, ':');
    if(f.size() > 5) return false;
    if(!f[0].empty() && !parse_int_in(f[0], 0, msk144wb::kGateMaxHold, p.hold)) return false;
    if(f.size() > 1 && !f[1].empty() && !parse_int_in(f[1], 1, msk144wb::kHopBlocks, p.min_up)) return false;
    if(f.size() > 2 && !f[2].empty() && !parse_int_in(f[2], 0, INT32_MAX, p.max_streams)) return false;
    if(f.size() > 3 && !f[3].empty() && (!parse_ratio_q4(f[3], p.ratio_q4) || (p.ratio_q4 != 0 && (p.ratio_q4 < 16 || p.ratio_q4 > 65535)))) return false;
    return f.size() < 5 || f[4].empty() || parse_channel_list(f[4], INT32_MAX - 1, always);
}

// The option of a run.  One object serves every device loop: a loop's collect() reports the slot's list under the mutex.
struct StreamGate
{
    bool on = false;
    msk144sg::Params params;
    std::vector<int32_t> always;  // program stream numbers
    StreamGateApi api;

    // '' or the refusal
    std::string parse(const char* value)
    {
        on = true;
        const std::string v = value ? value : "";
        return parse_stream_gate(v, params, always) ? "" : "bad value for --stream-gate: '" + v + "' ([HOLD[:MIN_UP[:MAX[:RATIO[:ALWAYS]]]]])";
    }

    // what needs the number of streams of the run; '' or the refusal
    std::string check(int streams) const
    {
        if(params.max_streams > streams) return "--stream-gate: MAX must lie within 1.." + std::to_string(streams) + ", or be 0 for all";
        for(int32_t s : always)
            if(s >= streams) return "--stream-gate: stream " + std::to_string(s) + " is not one of the " + std::to_string(streams) + " streams";
        return "";
    }

    // a decoder's share: streams base .. base + count - 1 of the program.  MAX is per decoder, held to its stream count.
    // detector_on: --stream-pings or --stream-levels has switched the detector on; else it is switched on here with its defaults
    bool configure(msk144_handle* h, int base, int count, bool detector_on, std::string& err) const
    {
        const msk144sp::Params d;
        const msk144_stream_pings_params dp{d.ratio_q4, d.memory, d.min_ref, d.shift};
        if(!detector_on && api.set_pings(h, &dp) != MSK144_OK)
        {
            err = msk144_last_error(h);
            return false;
        }
        std::vector<uint8_t> flags(static_cast<size_t>(count), 0);
        for(int32_t s : always)
            if(s >= base && s < base + count) flags[static_cast<size_t>(s - base)] = 1;
        const msk144_stream_gate_params p{params.hold, params.min_up, params.max_streams > count ? count : params.max_streams, params.ratio_q4};
        if(api.set(h, &p, flags.data()) == MSK144_OK) return true;
        err = msk144_last_error(h);
        return false;
    }

    // behind msk144_fetch_wait of the slot's hop of n positions (msk144_stream_gate_slot: no wait of its own): the listed positions
    bool take(msk144_handle* h, int slot, int n, const int32_t*& positions, int32_t& count, std::string& err)
    {
        int32_t total = 0;
        if(api.slot(h, slot, &positions, &count, &total) != MSK144_OK)
        {
            err = msk144_last_error(h);
            return false;
        }
        if(count < 0 || count > n || total < count)
        {
            err = "stream gate: the slot lists " + std::to_string(count) + " of " + std::to_string(total) + " positions, the hop had " + std::to_string(n);
            return false;
        }
        std::lock_guard<std::mutex> lock(mutex_);
        decoded_ += count;
        pushed_ += n;
        dropped_ += total - count;
        if(count > busiest_) busiest_ = count;
        return true;
    }

    // the end-of-run line, for stderr
    std::string summary() const
    {
        char buf[320], ratio[48];
        if(params.ratio_q4) snprintf(ratio, sizeof(ratio), "ratio %g", params.ratio_q4 / 16.0);
        else snprintf(ratio, sizeof(ratio), "ratio the detector's");
        snprintf(buf, sizeof(buf), "msk144hipdecoder: stream gate: %lld of %lld stream windows decoded, %lld dropped over max, busiest hop %d (hold %d, min up %d, max %d, %s, %zu always)",
                 decoded_, pushed_, dropped_, busiest_, params.hold, params.min_up, params.max_streams, ratio, always.size());
        return buf;
    }

private:
    std::mutex mutex_;
    long long decoded_ = 0, pushed_ = 0, dropped_ = 0;
    int busiest_ = 0;
};

}  // namespace msk144host
