// The capture entries for the stand-in library (compiled together with msk144hip_stub.cpp, wideband_stub.cpp and
// wideband_pings_stub.cpp): what msk144hipdecoder resolves for --wideband-capture.  Every call is reported on stderr.  Read i (0 the
// first: hops 0 and 1, then hop i + 1) gives these units, which follow the up blocks of wideband_pings_stub.cpp with one hop of
// pre-roll and one of tail, (channel, hop, flags):
//   read 0   (1, 0, pre) (1, 1, active)
//   read 1   (0, 1, pre) (0, 2, active) (1, 2, active)
//   read 2   (0, 3, active) (1, 3, tail) (3, 2, pre), and (3, 3, active) dropped: total = count + 1
//   read 3   (0, 4, active) (3, 4, tail)
// and every hop of every listed channel with flags = listed, all in channel then hop order.  Byte j of the row of (c, k) is
// (31 c + 7 k + j) mod 251 - 125.  tests/test_wideband_capture_cli.py holds the same rule.
#include "../../include/msk144hip.h"

#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

namespace
{

struct Capture
{
    bool on = false;
    int reads = 0;
    msk144_wideband_capture_params p{};
};
std::map<const msk144_handle*, Capture> g_capture;

struct Planned
{
    int read, channel, hop, flags;
};
const Planned kPlan[] = {{0, 1, 0, 4}, {0, 1, 1, 1}, {1, 0, 1, 4}, {1, 0, 2, 1}, {1, 1, 2, 1}, {2, 0, 3, 1}, {2, 1, 3, 8}, {2, 3, 2, 4}, {3, 0, 4, 1}, {3, 3, 4, 8}};

}  // namespace

extern "C" {

int msk144_set_wideband_capture(msk144_handle* h, const msk144_wideband_capture_params* p)
{
    if(!h) return MSK144_EINVAL;
    if(!p) fprintf(stderr, "stub: msk144_set_wideband_capture(off)\n");
    else
    {
        fprintf(stderr, "stub: msk144_set_wideband_capture(pre %d, post %d, max_units %d, listed", p->pre, p->post, p->max_units);
        for(int i = 0; i < p->num_listed; i++) fprintf(stderr, " %d", p->listed[i]);
        fprintf(stderr, ")\n");
    }
    Capture& g = g_capture[h];
    g.on = p != nullptr;
    if(p) g.p = *p;
    return MSK144_OK;
}

int msk144_wideband_capture(msk144_handle* h, msk144_wideband_capture_unit* units, int8_t* data, int32_t* count, int32_t* total)
{
    if(!h || !units || !data || !count || !total) return MSK144_EINVAL;
    Capture& g = g_capture[h];
    if(!g.on) return MSK144_ESTATE;
    const int i = g.reads++;
    std::vector<msk144_wideband_capture_unit> u;
    for(const Planned& x : kPlan)
        if(x.read == i) u.push_back(msk144_wideband_capture_unit{x.channel, x.flags, x.hop});
    for(int k = i == 0 ? 0 : i + 1; k <= i + 1; k++)
        for(int l = 0; l < g.p.num_listed; l++) u.push_back(msk144_wideband_capture_unit{g.p.listed[l], 2, k});
    std::sort(u.begin(), u.end(), [](const msk144_wideband_capture_unit& a, const msk144_wideband_capture_unit& b) { return a.channel != b.channel ? a.channel < b.channel : a.hop < b.hop; });
    *count = static_cast<int32_t>(std::min<size_t>(u.size(), static_cast<size_t>(g.p.max_units)));
    *total = static_cast<int32_t>(u.size()) + (i == 2 ? 1 : 0);
    fprintf(stderr, "stub: msk144_wideband_capture read %d: %d of %d units\n", i, *count, *total);
    for(int n = 0; n < *count; n++)
    {
        units[n] = u[static_cast<size_t>(n)];
        for(int j = 0; j < MSK144_CAPTURE_UNIT_BYTES; j++)
            data[static_cast<size_t>(n) * MSK144_CAPTURE_UNIT_BYTES + j] = static_cast<int8_t>((31 * units[n].channel + 7 * static_cast<int>(units[n].hop) + j) % 251 - 125);
    }
    return MSK144_OK;
}

}  // extern "C"
