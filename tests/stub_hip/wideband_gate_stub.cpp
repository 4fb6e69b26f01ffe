// The stand-in library with the gate (compiled ALONE: it takes msk144hip_stub.cpp and wideband_stub.cpp in as they are, under other
// names for the two entries it has to stand in front of), for msk144hipdecoder --wideband-gate.
//
//   msk144_set_wideband_gate   reported on stderr with its parameters and the always channels.
//   msk144_push_wideband       the base push of every channel (every channel's ring moves on, as the library's hop ring does); with the
//                              gate on the slot's windows are then packed to the listed channels and the hop covers those alone, so a
//                              record's channel is a position in the list.  The stand-in has no detector; its list of push k (k = 0,
//                              1, ... from the first push) is fixed: no channel at push 1, otherwise the channels with (c + k) % 3 == 0,
//                              and always the always channels; of those the first max_channels.
//   msk144_wideband_gate       the list of the last push; every call is reported with its index.
//   msk144_fetch_wait          the base one, with segment powers that differ by channel and by push - channel c of push k has seven
//                              segments of 1 + k + c and one of four times that - BY CHANNEL, for all channels, gate or no gate: so the
//                              snr= of a line tells whether every channel's tracker saw every push.
#include "../../include/msk144hip.h"

#define msk144_push_wideband msk144stub_push_wideband_all
#define msk144_fetch_wait msk144stub_fetch_wait_base
#include "msk144hip_stub.cpp"
#include "wideband_stub.cpp"
#undef msk144_push_wideband
#undef msk144_fetch_wait

namespace
{

struct GateStub
{
    bool on = false;
    msk144_wideband_gate_params p{};
    std::vector<uint8_t> always;
    std::vector<int32_t> list;
    int32_t total = 0;
    int push = -1, reads = 0;        // the index of the last push
    int slot_push[MSK144_SLOTS] = {0, 0};
};
std::map<const msk144_handle*, GateStub> g_gate;

}  // namespace

extern "C" {

int msk144_set_wideband_gate(msk144_handle* h, const msk144_wideband_gate_params* p, const uint8_t* always)
{
    if(!h || !g_wide.count(h)) return MSK144_EINVAL;
    GateStub& g = g_gate[h];
    g.on = p != nullptr;
    if(!p)
    {
        fprintf(stderr, "stub: msk144_set_wideband_gate(off)\n");
        return MSK144_OK;
    }
    g.p = *p;
    g.always.assign(static_cast<size_t>(h->p.channels), 0);
    fprintf(stderr, "stub: msk144_set_wideband_gate(hold %d, min_up %d, max_channels %d, always", p->hold, p->min_up, p->max_channels);
    for(int c = 0; always && c < h->p.channels; c++)
        if((g.always[static_cast<size_t>(c)] = always[c] != 0)) fprintf(stderr, " %d", c);
    fprintf(stderr, ")\n");
    return MSK144_OK;
}

int msk144_push_wideband(msk144_handle* h, int32_t s, int32_t first)
{
    const int rc = msk144stub_push_wideband_all(h, s, first);
    if(rc != MSK144_OK) return rc;
    GateStub& g = g_gate[h];
    g.push = first ? 0 : g.push + 1;
    g.slot_push[s] = g.push;
    if(!g.on) return MSK144_OK;
    const int C = h->p.channels, cap = g.p.max_channels ? g.p.max_channels : C;
    g.list.clear();
    g.total = 0;
    for(int c = 0; c < C; c++)
        if(g.always[static_cast<size_t>(c)] || (g.push != 1 && (c + g.push) % 3 == 0))
            if(g.total++ < cap) g.list.push_back(c);
    // the windows of the listed channels, packed: position j <= list[j], so ascending order overwrites nothing still needed
    for(size_t j = 0; j < g.list.size(); j++)
        std::memmove(h->in[s].data() + j * MSK144_WINDOW_SAMPLES, h->in[s].data() + static_cast<size_t>(g.list[j]) * MSK144_WINDOW_SAMPLES, MSK144_WINDOW_SAMPLES * sizeof(int16_t));
    h->active[s] = static_cast<int>(g.list.size());
    return MSK144_OK;
}

int msk144_wideband_gate(msk144_handle* h, int32_t* channels_out, int32_t* count, int32_t* total)
{
    if(!h || !channels_out || !count || !total) return MSK144_EINVAL;
    GateStub& g = g_gate[h];
    if(!g.on || g.push < 0) return MSK144_ESTATE;
    fprintf(stderr, "stub: msk144_wideband_gate read %d\n", g.reads++);
    for(size_t j = 0; j < g.list.size(); j++) channels_out[j] = g.list[j];
    *count = static_cast<int32_t>(g.list.size());
    *total = g.total;
    return MSK144_OK;
}

int msk144_fetch_wait(msk144_handle* h, int32_t s, const msk144_result** rec, int32_t* n, const float** seg)
{
    const int rc = msk144stub_fetch_wait_base(h, s, rec, n, seg);
    if(rc != MSK144_OK && rc != MSK144_EOVERFLOW) return rc;
    if(g_wide.count(h))
        for(int c = 0; c < h->p.channels; c++)
            for(int i = 0; i < 8; i++) h->seg[s][static_cast<size_t>(c) * 8 + i] = static_cast<float>(1 + g_gate[h].slot_push[s] + c) * (i == 0 ? 4.0f : 1.0f);
    return rc;
}

}  // extern "C"
