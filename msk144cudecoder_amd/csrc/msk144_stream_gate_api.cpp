// The stream-gate entries of the C ABI (include/msk144hip.h, "Stream gate"): msk144_set_stream_gate, the two read entries, and
// sg_plan / sg_gather, the steps the push (push_stream_hops, msk144_api.cpp) runs while the gate is on - the plan behind sp_push,
// the gather behind run_frontend.  The decode of a gated hop is msk144_api.cpp's, which takes header, event and store from h->gate_of.
#include "api_handle.h"

#include <cstring>

using namespace msk144;

namespace
{

constexpr size_t kHeaderWords = sizeof(msk144wb::PlanHeader) / sizeof(int32_t);   // the pinned block: 16 bytes are four int32, the list behind them

// the header a plan left in a slot's pinned block, as a read entry takes it: a count within 0..channels
int sg_header(msk144_handle* h, const char* who, int slot, msk144wb::PlanHeader& head)
{
    head = *h->sg.header[slot];
    return head.count < 0 || head.count > h->st.channels || head.total < head.count ? fail(h, MSK144_EHIP, std::string(who) + ": the device left a header out of range") : MSK144_OK;
}

}  // namespace

void sg_release(msk144_handle* h)
{
    for(hipEvent_t& e : h->sg.planned)
    {
        if(e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

int sg_plan(msk144_handle* h, int32_t slot, int32_t n)
{
    StreamGate& g = h->sg;
    const StreamPings& sp = h->sp;
    const int32_t* streams = h->slots[slot].streams;
    g.since.stage(slot, streams, n);
    // the detector's results of this push, where sp_push has just left them (the layout is StreamPings', api_handle.h); off: no
    // record, every mask 0
    const auto* records = sp.on ? reinterpret_cast<const msk144wb::PingRecord*>(sp.d_out) : nullptr;
    const auto* energies = sp.on ? reinterpret_cast<const int32_t*>(sp.d_out + StreamPings::energies_at(n)) : nullptr;
    const bool own = records && g.params.ratio_q4 != 0;
    const int32_t most = msk144sg::cap(g.params, h->st.channels);
    ev_begin(h);
    hipError_t e = hipMemcpyAsync(g.since.d_restart, g.since.restart[slot], static_cast<size_t>(n), hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess)
    {
        if(own) launch_stream_gate_mask(records, energies, n, g.params.ratio_q4, g.d_masks, h->stream);
        launch_stream_gate_plan(h->d_streams, h->d_isfirst, g.since.d_restart, records, own ? g.d_masks : nullptr, g.d_always, g.d_since, n, g.params, most, g.pushes, g.d_header, g.d_list,
                                h->stream);
        e = hipGetLastError();
    }
    // header and list in one copy to the slot's pinned block: the device keeps them adjacent, as the block does; a push lists at
    // most min(n, max_streams) positions
    if(e == hipSuccess)
        e = hipMemcpyAsync(g.header[slot], g.d_header, sizeof(msk144wb::PlanHeader) + sizeof(int32_t) * static_cast<size_t>(std::min(n, most)), hipMemcpyDeviceToHost, h->stream);
    if(e == hipSuccess) e = hipEventRecord(g.planned[slot], h->stream);
    ev_end(h, MSK144_T_FRONTEND);
    if(e != hipSuccess) return fail(h, MSK144_EHIP, std::string("stream gate: ") + hipGetErrorString(e));
    g.since.commit(streams, n);
    g.pushes++;
    g.slot_pushed[slot] = true;
    g.last_slot = slot;
    g.pushed = true;
    return MSK144_OK;
}

int sg_gather(msk144_handle* h, int32_t n)
{
    StreamGate& g = h->sg;
    h->gated = true;
    h->gate_of = {g.header[g.last_slot], g.planned[g.last_slot], g.d_analytic};
    ev_begin(h);
    launch_gate_gather(h->st.analytic, g.d_header, g.d_list, n, g.d_analytic, h->stream);
    ev_end(h, MSK144_T_FRONTEND);
    HIP_TRY(h, hipGetLastError());
    return MSK144_OK;
}

extern "C" {

int msk144_set_stream_gate(msk144_handle* h, const msk144_stream_gate_params* p, const uint8_t* always)
{
    if(!h) return fail(h, MSK144_EINVAL, "null argument");
    if(const int rc = streams_only(h, "msk144_set_stream_gate", "the stream gate reads the pings of int16 audio"); rc != MSK144_OK) return rc;
    StreamGate& g = h->sg;
    msk144sg::Params gp;
    if(p)
    {
        gp = msk144sg::Params{p->hold, p->min_up, p->max_streams, p->ratio_q4};
        if(const std::string why = msk144sg::check_params(gp, h->st.channels); !why.empty()) return fail(h, MSK144_EINVAL, "msk144_set_stream_gate: " + why);
    }
    // nothing of an earlier push still runs when the next one finds the gate changed
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t nch = static_cast<size_t>(h->st.channels);
    const int rows = msk144sg::cap(gp, h->st.channels);
    if(p)
    {
        // everything the gate needs, before anything of its state is touched: a `set` that cannot allocate leaves the gate as it was
        int rc;
        if(!g.d_always && (rc = dev_alloc(h, h->mem, &g.d_always, nch)) != MSK144_OK) return rc;
        if(!g.d_since && (rc = dev_alloc(h, h->mem, &g.d_since, nch)) != MSK144_OK) return rc;
        if(!g.since.d_restart && (rc = dev_alloc(h, h->mem, &g.since.d_restart, nch)) != MSK144_OK) return rc;
        if(!g.d_masks && (rc = dev_alloc(h, h->mem, &g.d_masks, nch)) != MSK144_OK) return rc;
        if(!g.d_header)
        {
            // header and list adjacent on the device too, so that one copy takes both
            int32_t* block = nullptr;
            if((rc = dev_alloc(h, h->mem, &block, kHeaderWords + nch)) != MSK144_OK) return rc;
            g.d_header = reinterpret_cast<msk144wb::PlanHeader*>(block);
            g.d_list = block + kHeaderWords;
        }
        for(int s = 0; s < MSK144_SLOTS; s++)
        {
            if(!g.since.restart[s] && (rc = host_alloc(h, h->mem, &g.since.restart[s], nch)) != MSK144_OK) return rc;
            if(!g.header[s])
            {
                int32_t* block = nullptr;
                if((rc = host_alloc(h, h->mem, &block, kHeaderWords + nch)) != MSK144_OK) return rc;
                g.header[s] = reinterpret_cast<msk144wb::PlanHeader*>(block);
            }
            if(!g.planned[s]) HIP_TRY(h, hipEventCreateWithFlags(&g.planned[s], hipEventBlockingSync | hipEventDisableTiming));
        }
        if(rows > g.rows)
        {
            // the larger store first, the smaller one freed only once it is there
            float2* store = nullptr;
            if((rc = dev_alloc(h, h->mem, &store, static_cast<size_t>(rows) * kWindowSamples)) != MSK144_OK) return rc;
            if(g.d_analytic) dev_free(h->mem, &g.d_analytic);
            g.d_analytic = store;
            g.rows = rows;
        }
    }
    // an accepted `set` ends the last push's list, and a window pushed through the gate can no longer be decoded
    g.on = g.pushed = false;
    for(bool& b : g.slot_pushed) b = false;
    if(h->gated) h->have_window = false;
    h->gated = false;
    if(!p) return MSK144_OK;

    std::vector<uint8_t> flags(nch, 0);
    for(size_t s = 0; always && s < nch; s++) flags[s] = always[s] != 0;
    HIP_TRY(h, hipMemcpy(g.d_always, flags.data(), nch, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemset(g.d_since, 0, nch * sizeof(int32_t)));
    g.since.reset(nch);
    g.pushes = 0;
    g.params = gp;
    g.on = true;
    return MSK144_OK;
}

int msk144_stream_gate(msk144_handle* h, int32_t* positions_out, int32_t* count, int32_t* total)
{
    if(!h || !positions_out || !count || !total) return fail(h, MSK144_EINVAL, "null argument");
    const StreamGate& g = h->sg;
    if(!g.on) return fail(h, MSK144_ESTATE, "msk144_stream_gate: the stream gate is off (msk144_set_stream_gate)");
    if(!g.pushed) return fail(h, MSK144_ESTATE, "msk144_stream_gate before a msk144_push_hops or msk144_push_rate_hops since msk144_set_stream_gate");
    // it waits for the gate's event alone: the list is ready long before the push's front end is
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipEventSynchronize(g.planned[g.last_slot]));
    msk144wb::PlanHeader head;
    if(const int rc = sg_header(h, "msk144_stream_gate", g.last_slot, head); rc != MSK144_OK) return rc;
    std::memcpy(positions_out, g.header[g.last_slot] + 1, sizeof(int32_t) * static_cast<size_t>(head.count));
    *count = head.count;
    *total = head.total;
    return MSK144_OK;
}

int msk144_stream_gate_slot(msk144_handle* h, int32_t slot, const int32_t** positions, int32_t* count, int32_t* total)
{
    if(!h || !positions || !count || !total || slot < 0 || slot >= MSK144_SLOTS) return fail(h, MSK144_EINVAL, "bad argument");
    const StreamGate& g = h->sg;
    if(!g.on) return fail(h, MSK144_ESTATE, "msk144_stream_gate_slot: the stream gate is off (msk144_set_stream_gate)");
    if(!g.slot_pushed[slot]) return fail(h, MSK144_ESTATE, "msk144_stream_gate_slot before a push on this slot since msk144_set_stream_gate");
    msk144wb::PlanHeader head;
    if(const int rc = sg_header(h, "msk144_stream_gate_slot", slot, head); rc != MSK144_OK) return rc;
    *positions = reinterpret_cast<const int32_t*>(g.header[slot] + 1);
    *count = head.count;
    *total = head.total;
    return MSK144_OK;
}

}  // extern "C"
