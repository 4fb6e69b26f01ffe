// The ping-detector entries for the stand-in library (compiled together with msk144hip_stub.cpp and wideband_stub.cpp): what
// msk144hipdecoder resolves for --wideband-pings.  Every call is reported on stderr.  Read i (0 the first: 54 blocks, then 27) gives
// channel c the reference 1000 (c + 1) + i and these up blocks:
//   channel 0   blocks 25 and 26 of every read but the first: a run that is open at the end of every push, closed by block 0 of the
//               next one, the last by the end of the stream;
//   channel 1   blocks 50..53 of read 0 and 0..2 of read 1: one run of 7 across the boundary;
//   channel 3   block 5 of read 2: a run of one block;
// with E = 10 x reference + b for an up block b and reference / 2 for any other.  tests/test_wideband_pings_cli.py holds the same rule.
#include "../../include/msk144hip.h"

#include <cstdio>
#include <map>
#include <vector>

namespace
{

struct Pings
{
    bool on = false;
    int channels = 0;
    int reads = 0;
    int blocks = 0;
    std::vector<int32_t> energies;  // [channels][54] of the last read
};
std::map<const msk144_handle*, Pings> g_pings;

bool up(int i, int c, int b)
{
    if(c == 0) return i >= 1 && (b == 25 || b == 26);
    if(c == 1) return (i == 0 && b >= 50) || (i == 1 && b <= 2);
    return c == 3 && i == 2 && b == 5;
}

}  // namespace

extern "C" {

int msk144_set_wideband_pings(msk144_handle* h, const msk144_wideband_pings_params* p)
{
    if(!h) return MSK144_EINVAL;
    if(!p) fprintf(stderr, "stub: msk144_set_wideband_pings(off)\n");
    else fprintf(stderr, "stub: msk144_set_wideband_pings(ratio_q4 %d, memory %d, min_ref %d)\n", p->ratio_q4, p->memory, p->min_ref);
    g_pings[h].on = p != nullptr;
    return MSK144_OK;
}

int msk144_wideband_pings(msk144_handle* h, msk144_wideband_ping* out)
{
    if(!h || !out) return MSK144_EINVAL;
    Pings& g = g_pings[h];
    if(!g.on) return MSK144_ESTATE;
    if(!g.channels)
    {
        int32_t n = 0;
        if(msk144_llr_block_channels(h, &n) != MSK144_OK || n < 1) return MSK144_ESTATE;  // the stand-in reports the handle's channels
        g.channels = n;
    }
    const int i = g.reads++;
    fprintf(stderr, "stub: msk144_wideband_pings read %d\n", i);
    g.blocks = i == 0 ? MSK144_PING_MAX_BLOCKS : MSK144_PING_MAX_BLOCKS / 2;
    g.energies.assign(static_cast<size_t>(g.channels) * MSK144_PING_MAX_BLOCKS, 0);
    for(int c = 0; c < g.channels; c++)
    {
        msk144_wideband_ping& r = out[c];
        r = msk144_wideband_ping{};
        r.blocks = g.blocks;
        r.history = i < 8 ? i : 8;
        r.reference = 1000 * (c + 1) + i;
        r.quiet = r.reference;
        for(int b = 0; b < g.blocks; b++)
        {
            const int32_t e = up(i, c, b) ? 10 * r.reference + b : r.reference / 2;
            g.energies[static_cast<size_t>(c) * MSK144_PING_MAX_BLOCKS + b] = e;
            if(up(i, c, b)) r.up_mask |= 1ull << b;
            if(e > r.peak) r.peak = e, r.peak_block = b;
        }
    }
    return MSK144_OK;
}

int msk144_wideband_ping_blocks(msk144_handle* h, int32_t channel, int32_t* energies, int32_t* n)
{
    if(!h || !energies || !n) return MSK144_EINVAL;
    Pings& g = g_pings[h];
    if(!g.on || !g.reads) return MSK144_ESTATE;
    if(channel < -1 || channel >= g.channels) return MSK144_EINVAL;
    fprintf(stderr, "stub: msk144_wideband_ping_blocks(channel %d) after read %d\n", channel, g.reads - 1);
    const size_t row = MSK144_PING_MAX_BLOCKS;
    const size_t first = channel < 0 ? 0 : row * static_cast<size_t>(channel), count = channel < 0 ? g.energies.size() : row;
    for(size_t k = 0; k < count; k++) energies[k] = g.energies[first + k];
    *n = g.blocks;
    return MSK144_OK;
}

}  // extern "C"
