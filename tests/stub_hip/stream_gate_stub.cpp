// The stand-in library with the stream gate (compiled ALONE: it takes msk144hip_stub.cpp, input_rate_stub.cpp and
// stream_pings_stub.cpp in as they are, under other names for the entries it has to stand in front of), for msk144hipdecoder
// --stream-gate.  No kernel: the list of a push is worked out on the CPU with the host rules of csrc/stream_pings.h and
// csrc/stream_gate.h (msk144sp::Model, msk144sg::Model) on the slot's pinned hop inputs.
//
//   msk144_set_stream_pings    the base one; the parameters are kept, and a detector of the gate's own is made from them (the base
//                              one works its records out when the program asks for them, which with --stream-gate alone it never does).
//   msk144_set_stream_gate     reported on stderr with its parameters and the always streams.
//   msk144_push_hops           the base push of the n listed streams (their rings move on); with the gate on the slot's windows are
//                              then packed to the listed positions and the hop covers those alone, so a record's channel is an index
//                              in the list.  msk144_push_rate_hops of input_rate_stub.cpp ends in this entry.
//   msk144_stream_gate_slot    the list of the slot's last push; every call is reported with the slot and the counts.
//   msk144_fetch_wait          the base one, with segment powers that differ by stream and by hop - hop k of stream s has seven
//                              segments of 1 + k + s and one of four times that - BY POSITION, for all n positions, gate or no gate:
//                              so the snr= of a line tells whether every stream's tracker saw every hop.
#include "../../include/msk144hip.h"
#include "../../msk144cudecoder_amd/csrc/stream_gate.h"

#include <mutex>

#define msk144_push_hops msk144stub_push_hops_all
#define msk144_fetch_wait msk144stub_fetch_wait_base
#include "msk144hip_stub.cpp"
#undef msk144_push_hops
#undef msk144_fetch_wait
#include "input_rate_stub.cpp"
#define msk144_set_stream_pings msk144stub_set_stream_pings_base
#include "stream_pings_stub.cpp"
#undef msk144_set_stream_pings

namespace
{

struct StreamGateStub
{
    bool on = false;
    msk144_stream_gate_params p{};
    std::unique_ptr<msk144sg::Model> gate;
    std::unique_ptr<msk144sp::Model> pings;   // null: the detector is off
    std::vector<int> hops;                    // [channels] hops each stream has had
    std::vector<int32_t> list[MSK144_SLOTS];
    int32_t total[MSK144_SLOTS] = {0, 0};
    bool pushed[MSK144_SLOTS] = {false, false};
    std::vector<float> seg[MSK144_SLOTS];
};
std::map<const msk144_handle*, StreamGateStub> g_sgate;
std::mutex g_sgate_lock;

// The handle's entry, made at the first call.  Every device loop has a push thread and a collect thread, and without the gate a
// handle's entry is first asked for from those: the map is only ever touched under the lock (its references stay valid).  What an
// entry holds is the handle's own - `hops` the push thread's, list, total and seg per slot, handed over as the slot's results are
StreamGateStub& sgate_of(const msk144_handle* h)
{
    std::lock_guard<std::mutex> lock(g_sgate_lock);
    return g_sgate[h];
}

}  // namespace

extern "C" {

int msk144_set_stream_pings(msk144_handle* h, const msk144_stream_pings_params* p)
{
    const int rc = msk144stub_set_stream_pings_base(h, p);
    if(rc != MSK144_OK) return rc;
    StreamGateStub& g = sgate_of(h);
    g.pings.reset(p ? new msk144sp::Model(h->p.channels, msk144sp::Params{p->ratio_q4, p->memory, p->min_ref, p->shift}) : nullptr);
    return MSK144_OK;
}

int msk144_set_stream_gate(msk144_handle* h, const msk144_stream_gate_params* p, const uint8_t* always)
{
    if(!h) return MSK144_EINVAL;
    StreamGateStub& g = sgate_of(h);
    if(!p)
    {
        g.on = false;
        fprintf(stderr, "stub: msk144_set_stream_gate(off)\n");
        return MSK144_OK;
    }
    const msk144sg::Params pp{p->hold, p->min_up, p->max_streams, p->ratio_q4};
    if(h->p.read_mode != 1 || !msk144sg::check_params(pp, h->p.channels).empty())
    {
        h->error = "stub: msk144_set_stream_gate refused";
        return MSK144_EINVAL;
    }
    g.on = true;
    g.p = *p;
    g.gate.reset(new msk144sg::Model(h->p.channels, pp, always));
    for(bool& b : g.pushed) b = false;
    fprintf(stderr, "stub: msk144_set_stream_gate(hold %d, min_up %d, max_streams %d, ratio_q4 %d, %d streams, always", p->hold, p->min_up, p->max_streams, p->ratio_q4, h->p.channels);
    for(int c = 0; always && c < h->p.channels; c++)
        if(always[c]) fprintf(stderr, " %d", c);
    fprintf(stderr, ")\n");
    return MSK144_OK;
}

int msk144_push_hops(msk144_handle* h, int32_t s, int32_t n)
{
    const int rc = msk144stub_push_hops_all(h, s, n);
    if(rc != MSK144_OK) return rc;
    StreamGateStub& g = sgate_of(h);
    if(g.hops.empty()) g.hops.assign(static_cast<size_t>(h->p.channels), 0);
    g.seg[s].assign(static_cast<size_t>(h->p.channels) * 8, 1.0f);
    for(int j = 0; j < n; j++)
    {
        const int c = h->streams[s][j];
        const int k = h->is_first[s][j] ? (g.hops[static_cast<size_t>(c)] = 0) : ++g.hops[static_cast<size_t>(c)];
        for(int i = 0; i < 8; i++) g.seg[s][static_cast<size_t>(j) * 8 + i] = static_cast<float>(1 + k + c) * (i == 0 ? 4.0f : 1.0f);
    }
    if(!g.on) return MSK144_OK;
    // the detector's records of the push, then the gate's list
    std::vector<msk144wb::PingRecord> records(static_cast<size_t>(n));
    std::vector<int32_t> energies(static_cast<size_t>(n) * msk144sp::kMaxBlocks, 0);
    std::vector<int16_t> x(MSK144_WINDOW_SAMPLES);
    for(int j = 0; g.pings && j < n; j++)
    {
        const int16_t* hp = h->hops[s].data() + static_cast<size_t>(MSK144_HOP_SAMPLES) * j;
        const int16_t* fp = h->first_halves[s].data() + static_cast<size_t>(MSK144_HOP_SAMPLES) * j;
        const bool first = h->is_first[s][j] != 0;
        if(first) std::copy(fp, fp + MSK144_HOP_SAMPLES, x.begin());
        std::copy(hp, hp + MSK144_HOP_SAMPLES, x.begin() + (first ? MSK144_HOP_SAMPLES : 0));
        msk144sp::Level level;
        records[static_cast<size_t>(j)] = g.pings->push(h->streams[s][j], first, x.data(), level, energies.data() + static_cast<size_t>(j) * msk144sp::kMaxBlocks);
    }
    g.list[s].clear();
    g.total[s] = g.gate->push(n, h->streams[s].data(), h->is_first[s].data(), g.pings ? records.data() : nullptr, g.pings ? energies.data() : nullptr, g.list[s]);
    g.pushed[s] = true;
    // the windows of the listed positions, packed: index i <= list[i], so ascending order overwrites nothing still needed
    for(size_t i = 0; i < g.list[s].size(); i++)
        std::memmove(h->in[s].data() + i * MSK144_WINDOW_SAMPLES, h->in[s].data() + static_cast<size_t>(g.list[s][i]) * MSK144_WINDOW_SAMPLES, MSK144_WINDOW_SAMPLES * sizeof(int16_t));
    h->active[s] = static_cast<int>(g.list[s].size());
    return MSK144_OK;
}

int msk144_stream_gate_slot(msk144_handle* h, int32_t s, const int32_t** positions, int32_t* count, int32_t* total)
{
    if(!h || s < 0 || s >= MSK144_SLOTS || !positions || !count || !total) return MSK144_EINVAL;
    StreamGateStub& g = sgate_of(h);
    if(!g.on || !g.pushed[s])
    {
        h->error = "stub: msk144_stream_gate_slot before a gated push on the slot";
        return MSK144_ESTATE;
    }
    fprintf(stderr, "stub: msk144_stream_gate_slot(slot %d) %d of %d\n", s, static_cast<int>(g.list[s].size()), g.total[s]);
    *positions = g.list[s].data();
    *count = static_cast<int32_t>(g.list[s].size());
    *total = g.total[s];
    return MSK144_OK;
}

int msk144_stream_gate(msk144_handle*, int32_t*, int32_t*, int32_t*) { return MSK144_ESTATE; }

int msk144_fetch_wait(msk144_handle* h, int32_t s, const msk144_result** rec, int32_t* n, const float** seg)
{
    const int rc = msk144stub_fetch_wait_base(h, s, rec, n, seg);
    if(rc != MSK144_OK && rc != MSK144_EOVERFLOW) return rc;
    const StreamGateStub& g = sgate_of(h);
    if(g.seg[s].size() == h->seg[s].size()) h->seg[s] = g.seg[s];
    return rc;
}

}  // extern "C"
