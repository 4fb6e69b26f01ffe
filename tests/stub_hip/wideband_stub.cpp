// Wideband entries for the stand-in library (compiled together with msk144hip_stub.cpp), for every rate: a slot holds 5184 Fs/12000
// input samples (5184 P/Q with Fs = 12000 P/Q), and the channel taps the program passes are reported with the rate, so that a test can
// check they are the design for that rate - above 6.144 Msps the one for Fs/32 (K x P2 taps summing to Q2).  No bank and no
// channeliser: the push hands every channel a hop through the stub's own hop ring, marked like the --inputs streams of
// tests/test_host_loop.py - half-window k of channel c starts with the int16 pair (0x7777, 100 c + k) - so that the records show
// which push reached which channel.
#include "../../include/msk144hip.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <vector>

namespace
{

struct Wide
{
    int channels = 0;
    long long rate = 0;
    int format = 0;
    int pushes = 0;
    std::vector<unsigned char> slot[MSK144_SLOTS];
};
std::map<const msk144_handle*, Wide> g_wide;

}  // namespace

extern "C" {

int msk144_set_wideband(msk144_handle* h, const msk144_wideband_params* p)
{
    if(!h || !p || p->num_offsets < 1) return MSK144_EINVAL;
    Wide& w = g_wide[h];
    w.channels = p->num_offsets;
    w.rate = p->rate_hz;
    w.format = p->format;
    w.pushes = 0;
    const long long g = std::gcd(static_cast<long long>(p->rate_hz), 12000LL);
    const size_t P = static_cast<size_t>(p->rate_hz / g), Q = static_cast<size_t>(12000 / g);
    const size_t bytes = static_cast<size_t>(MSK144_WINDOW_SAMPLES) / Q * P * (p->format == MSK144_WB_CS16 ? 4 : 2);
    for(auto& s : w.slot) s.assign(bytes, 0);
    double sum = 0.0;
    for(int k = 0; k < p->num_taps; k++) sum += p->taps[k];
    fprintf(stderr, "stub: msk144_set_wideband(rate %lld, format %d, K %d, gain %g, %d taps summing to %.6f, %d offsets, first %d, last %d)\n", static_cast<long long>(p->rate_hz),
            p->format, p->taps_per_phase, static_cast<double>(p->gain), p->num_taps, sum, p->num_offsets, p->offsets_hz[0], p->offsets_hz[p->num_offsets - 1]);
    return MSK144_OK;
}

int msk144_set_wideband_ex(msk144_handle* h, const msk144_wideband_params* p, const double*, int32_t)
{
    return msk144_set_wideband(h, p);
}

int msk144_dump_wideband_band(msk144_handle*, int32_t, float*) { return MSK144_ESTATE; }

int msk144_wideband_slot(msk144_handle* h, int32_t s, void** buf, size_t* bytes)
{
    auto it = g_wide.find(h);
    if(it == g_wide.end() || s < 0 || s >= MSK144_SLOTS) return MSK144_ESTATE;
    *buf = it->second.slot[s].data();
    *bytes = it->second.slot[s].size();
    return MSK144_OK;
}

int msk144_push_wideband(msk144_handle* h, int32_t s, int32_t first)
{
    auto it = g_wide.find(h);
    if(it == g_wide.end()) return MSK144_ESTATE;
    Wide& w = it->second;
    if(!first && w.pushes == 0) return MSK144_ESTATE;
    if(first) w.pushes = 0;
    void *hops = nullptr, *heads = nullptr;
    int32_t* streams = nullptr;
    uint8_t* is_first = nullptr;
    int rc = msk144_hop_slot(h, s, &hops, &heads, &streams, &is_first);
    if(rc != MSK144_OK) return rc;
    const size_t half = MSK144_HOP_SAMPLES;
    for(int c = 0; c < w.channels; c++)
    {
        int16_t* hp = static_cast<int16_t*>(hops) + half * c;
        int16_t* fp = static_cast<int16_t*>(heads) + half * c;
        memset(hp, 0, half * sizeof(int16_t));
        hp[0] = 0x7777;
        hp[1] = static_cast<int16_t>(100 * c + w.pushes + (first ? 1 : 0));
        if(first)
        {
            memset(fp, 0, half * sizeof(int16_t));
            fp[0] = 0x7777;
            fp[1] = static_cast<int16_t>(100 * c);
        }
        streams[c] = c;
        is_first[c] = first ? 1 : 0;
    }
    w.pushes += first ? 2 : 1;
    return msk144_push_hops(h, s, w.channels);
}

int msk144_dump_wideband_hop(msk144_handle*, int32_t, int8_t*) { return MSK144_ESTATE; }

int msk144_wideband_clip_count(msk144_handle* h, int64_t* clipped)
{
    if(!g_wide.count(h) || !clipped) return MSK144_ESTATE;
    *clipped = 7;
    return MSK144_OK;
}

}  // extern "C"
