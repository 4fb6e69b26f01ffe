// Stream-ping entries for the stand-in library (compiled together with msk144hip_stub.cpp).  No kernel: the records of a slot are
// worked out on the CPU, with the host rule of csrc/stream_pings.h (msk144sp::Model), when the program asks for them - behind
// msk144_fetch_wait, while the slot's pinned hop inputs still hold what was pushed.  The stand-in's handle is opaque here, so the n of
// the slot's push is read off its stream list: the ascending prefix, which this file ends by writing -1 over the list once it has
// been read (the program fills the list anew before every push and asks once per hop).  `set` is reported on stderr.
#include "../../include/msk144hip.h"
#include "../../msk144cudecoder_amd/csrc/stream_pings.h"

#include <cstdio>
#include <map>
#include <memory>
#include <vector>

namespace
{

struct State
{
    int channels = 0;
    std::unique_ptr<msk144sp::Model> model;
    std::vector<msk144wb::PingRecord> records[MSK144_SLOTS];
    std::vector<msk144sp::Level> levels[MSK144_SLOTS];
    std::vector<int32_t> energies[MSK144_SLOTS];
};
std::map<const msk144_handle*, State> g_state;

}  // namespace

extern "C" {

int msk144_set_stream_pings(msk144_handle* h, const msk144_stream_pings_params* p)
{
    if(!h) return MSK144_EINVAL;
    if(!p)
    {
        g_state.erase(h);
        return MSK144_OK;
    }
    const msk144sp::Params pp{p->ratio_q4, p->memory, p->min_ref, p->shift};
    int32_t nch = 0;
    if(!msk144sp::check_params(pp).empty() || msk144_llr_block_channels(h, &nch) != MSK144_OK) return MSK144_EINVAL;  // the stub reports the handle's channels there
    State& s = g_state[h];
    s = State{};
    s.channels = nch;
    s.model.reset(new msk144sp::Model(nch, pp));
    fprintf(stderr, "stub: msk144_set_stream_pings(ratio_q4 %d, memory %d, min_ref %d, shift %d, %d streams)\n", p->ratio_q4, p->memory, p->min_ref, p->shift, nch);
    return MSK144_OK;
}

int msk144_stream_pings_slot(msk144_handle* h, int32_t slot, const msk144_wideband_ping** records, const msk144_stream_level** levels, const int32_t** energies, int32_t* n)
{
    auto it = g_state.find(h);
    if(it == g_state.end() || slot < 0 || slot >= MSK144_SLOTS || !records || !levels || !energies || !n) return MSK144_ESTATE;
    State& s = it->second;
    void *hops = nullptr, *first_halves = nullptr;
    int32_t* streams = nullptr;
    uint8_t* is_first = nullptr;
    if(msk144_hop_slot(h, slot, &hops, &first_halves, &streams, &is_first) != MSK144_OK) return MSK144_ESTATE;
    int count = 0;
    while(count < s.channels && streams[count] >= 0 && streams[count] < s.channels && (count == 0 || streams[count] > streams[count - 1])) count++;
    if(count == 0) return MSK144_ESTATE;
    s.records[slot].resize(static_cast<size_t>(count));
    s.levels[slot].resize(static_cast<size_t>(count));
    s.energies[slot].assign(static_cast<size_t>(count) * msk144sp::kMaxBlocks, 0);
    std::vector<int16_t> x(MSK144_WINDOW_SAMPLES);
    for(int j = 0; j < count; j++)
    {
        const int16_t* hp = static_cast<const int16_t*>(hops) + static_cast<size_t>(MSK144_HOP_SAMPLES) * j;
        const int16_t* fp = static_cast<const int16_t*>(first_halves) + static_cast<size_t>(MSK144_HOP_SAMPLES) * j;
        const bool first = is_first[j] != 0;
        if(first) std::copy(fp, fp + MSK144_HOP_SAMPLES, x.begin());
        std::copy(hp, hp + MSK144_HOP_SAMPLES, x.begin() + (first ? MSK144_HOP_SAMPLES : 0));
        s.records[slot][static_cast<size_t>(j)] = s.model->push(streams[j], first, x.data(), s.levels[slot][static_cast<size_t>(j)], s.energies[slot].data() + static_cast<size_t>(j) * msk144sp::kMaxBlocks);
    }
    for(int j = 0; j < s.channels; j++) streams[j] = -1;
    static_assert(sizeof(msk144_wideband_ping) == sizeof(msk144wb::PingRecord) && sizeof(msk144_stream_level) == sizeof(msk144sp::Level), "the library's records");
    *records = reinterpret_cast<const msk144_wideband_ping*>(s.records[slot].data());
    *levels = reinterpret_cast<const msk144_stream_level*>(s.levels[slot].data());
    *energies = s.energies[slot].data();
    *n = count;
    return MSK144_OK;
}

int msk144_stream_pings(msk144_handle*, msk144_wideband_ping*, msk144_stream_level*, int32_t*) { return MSK144_ESTATE; }
int msk144_stream_ping_blocks(msk144_handle*, int32_t, int32_t*, int32_t*) { return MSK144_ESTATE; }

}  // extern "C"
