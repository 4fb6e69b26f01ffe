// The notch entries for the stand-in library (compiled together with msk144hip_stub.cpp and wideband_stub.cpp): what msk144hipdecoder
// resolves for --wideband-notch.  Every call is reported on stderr: a `set` with its channels, each with its shift and its 128 tap
// bytes in hexadecimal, (br, bi) of b[0] first; a stats read with its index.  The stats are fixed: a channel of the table has clamped
// 10 c + 1 components in every push, any other none.  The stand-in's hops do not depend on the table.
#include "../../include/msk144hip.h"

#include <cstdio>
#include <map>
#include <vector>

namespace
{

struct Notch
{
    std::vector<int32_t> channels;
    int reads = 0;
};
std::map<const msk144_handle*, Notch> g_notch;

}  // namespace

extern "C" {

int msk144_set_wideband_notch(msk144_handle* h, const int32_t* channels, int32_t count, const msk144_wideband_notch_params* params)
{
    if(!h) return MSK144_EINVAL;
    Notch& g = g_notch[h];
    g.channels.clear();
    if(!channels || count <= 0)
    {
        fprintf(stderr, "stub: msk144_set_wideband_notch(off)\n");
        return MSK144_OK;
    }
    if(!params) return MSK144_EINVAL;
    fprintf(stderr, "stub: msk144_set_wideband_notch(%d channels:", count);
    for(int i = 0; i < count; i++)
    {
        g.channels.push_back(channels[i]);
        fprintf(stderr, " ch=%d shift %d taps ", channels[i], params[i].shift);
        for(int k = 0; k < 64; k++)
            fprintf(stderr, "%02x%02x", static_cast<unsigned>(static_cast<uint8_t>(params[i].taps[k][0])), static_cast<unsigned>(static_cast<uint8_t>(params[i].taps[k][1])));
    }
    fprintf(stderr, ")\n");
    return MSK144_OK;
}

int msk144_wideband_notch_stats(msk144_handle* h, msk144_wideband_notch_count* out)
{
    if(!h || !out) return MSK144_EINVAL;
    Notch& g = g_notch[h];
    int32_t n = 0;
    if(g.channels.empty() || msk144_llr_block_channels(h, &n) != MSK144_OK || n < 1) return MSK144_ESTATE;  // the stand-in reports the handle's channels
    fprintf(stderr, "stub: msk144_wideband_notch_stats read %d\n", g.reads++);
    for(int c = 0; c < n; c++) out[c] = msk144_wideband_notch_count{0, 0};
    for(int32_t c : g.channels)
        if(c >= 0 && c < n) out[c] = msk144_wideband_notch_count{1, 10 * c + 1};
    return MSK144_OK;
}

}  // extern "C"
