// The stream-ping entries of the C ABI (include/msk144hip.h, "Stream levels and pings"): msk144_set_stream_pings, the three read
// entries, and sp_push, the step the push (push_stream_hops, msk144_api.cpp) runs while the option is on.
#include "api_handle.h"

#include <cstring>

using namespace msk144;

namespace
{

// the read entries that wait: on, and a push has been made since the `set`
int sp_read_ready(msk144_handle* h, const char* entry)
{
    if(!h) return fail(h, MSK144_EINVAL, "null argument");
    if(!h->sp.on) return fail(h, MSK144_ESTATE, std::string(entry) + ": stream pings are off (msk144_set_stream_pings)");
    if(!h->sp.pushed) return fail(h, MSK144_ESTATE, std::string(entry) + " before a msk144_push_hops or msk144_push_rate_hops since msk144_set_stream_pings");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MSK144_OK;
}

}  // namespace

int sp_push(msk144_handle* h, int32_t slot, int32_t n)
{
    StreamPings& sp = h->sp;
    const int32_t* streams = h->slots[slot].streams;
    sp.since.stage(slot, streams, n);
    ev_begin(h);
    hipError_t e = hipMemcpyAsync(sp.since.d_restart, sp.since.restart[slot], static_cast<size_t>(n), hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess)
    {
        launch_stream_pings(h->d_first, h->d_hops, h->d_streams, h->d_isfirst, sp.since.d_restart, n, sp.params, sp.d_state, reinterpret_cast<msk144wb::PingRecord*>(sp.d_out),
                            reinterpret_cast<msk144sp::Level*>(sp.d_out + StreamPings::levels_at(n)), reinterpret_cast<int32_t*>(sp.d_out + StreamPings::energies_at(n)), h->stream);
        e = hipGetLastError();
    }
    // the slot's own copy: complete when the slot's fetch is, whatever the other slot pushes meanwhile
    if(e == hipSuccess) e = hipMemcpyAsync(sp.out[slot], sp.d_out, StreamPings::out_bytes(n), hipMemcpyDeviceToHost, h->stream);
    ev_end(h, MSK144_T_FRONTEND);
    if(e != hipSuccess) return fail(h, MSK144_EHIP, std::string("stream pings: ") + hipGetErrorString(e));
    sp.since.commit(streams, n);
    sp.slot_n[slot] = n;
    sp.last_slot = slot;
    sp.pushed = true;
    return MSK144_OK;
}

extern "C" {

int msk144_set_stream_pings(msk144_handle* h, const msk144_stream_pings_params* p)
{
    if(!h) return fail(h, MSK144_EINVAL, "null argument");
    if(const int rc = streams_only(h, "msk144_set_stream_pings", "stream pings take int16 audio"); rc != MSK144_OK) return rc;
    StreamPings& sp = h->sp;
    msk144sp::Params pp;
    if(p)
    {
        pp = msk144sp::Params{p->ratio_q4, p->memory, p->min_ref, p->shift};
        if(const std::string why = msk144sp::check_params(pp); !why.empty()) return fail(h, MSK144_EINVAL, "msk144_set_stream_pings: " + why);
    }
    // nothing of an earlier push still runs when the next one finds the option changed
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    sp.on = sp.pushed = false;
    for(int& n : sp.slot_n) n = 0;
    if(!p) return MSK144_OK;

    const size_t nch = static_cast<size_t>(h->st.channels);
    const size_t bytes = StreamPings::out_bytes(h->st.channels);
    int rc;
    if(!sp.d_state && (rc = dev_alloc(h, h->mem, &sp.d_state, nch)) != MSK144_OK) return rc;
    if(!sp.since.d_restart && (rc = dev_alloc(h, h->mem, &sp.since.d_restart, nch)) != MSK144_OK) return rc;
    if(!sp.d_out && (rc = dev_alloc(h, h->mem, &sp.d_out, bytes)) != MSK144_OK) return rc;
    for(int s = 0; s < MSK144_SLOTS; s++)
    {
        if(!sp.since.restart[s] && (rc = host_alloc(h, h->mem, &sp.since.restart[s], nch)) != MSK144_OK) return rc;
        if(!sp.out[s] && (rc = host_alloc(h, h->mem, &sp.out[s], bytes)) != MSK144_OK) return rc;
    }
    HIP_TRY(h, hipMemset(sp.d_state, 0, nch * sizeof(msk144wb::PingHistory)));
    sp.since.reset(nch);
    sp.params = pp;
    sp.on = true;
    return MSK144_OK;
}

int msk144_stream_pings(msk144_handle* h, msk144_wideband_ping* records, msk144_stream_level* levels, int32_t* n)
{
    if(const int rc = sp_read_ready(h, "msk144_stream_pings"); rc != MSK144_OK) return rc;
    if(!records || !levels || !n) return fail(h, MSK144_EINVAL, "null argument");
    const StreamPings& sp = h->sp;
    const int count = sp.slot_n[sp.last_slot];
    std::memcpy(records, sp.out[sp.last_slot], sizeof(msk144wb::PingRecord) * static_cast<size_t>(count));
    std::memcpy(levels, sp.out[sp.last_slot] + StreamPings::levels_at(count), sizeof(msk144sp::Level) * static_cast<size_t>(count));
    *n = count;
    return MSK144_OK;
}

int msk144_stream_ping_blocks(msk144_handle* h, int32_t j, int32_t* out, int32_t* nb)
{
    if(const int rc = sp_read_ready(h, "msk144_stream_ping_blocks"); rc != MSK144_OK) return rc;
    const StreamPings& sp = h->sp;
    const int count = sp.slot_n[sp.last_slot];
    if(!out || !nb || j < 0 || j >= count) return fail(h, MSK144_EINVAL, "bad argument: position must be below n of the last push");
    std::memcpy(out, sp.out[sp.last_slot] + StreamPings::energies_at(count) + sizeof(int32_t) * msk144sp::kMaxBlocks * static_cast<size_t>(j), sizeof(int32_t) * msk144sp::kMaxBlocks);
    *nb = reinterpret_cast<const msk144wb::PingRecord*>(sp.out[sp.last_slot])[j].blocks;
    return MSK144_OK;
}

int msk144_stream_pings_slot(msk144_handle* h, int32_t slot, const msk144_wideband_ping** records, const msk144_stream_level** levels, const int32_t** energies, int32_t* n)
{
    if(!h || !records || !levels || !energies || !n || slot < 0 || slot >= MSK144_SLOTS) return fail(h, MSK144_EINVAL, "bad argument");
    const StreamPings& sp = h->sp;
    if(!sp.on) return fail(h, MSK144_ESTATE, "msk144_stream_pings_slot: stream pings are off (msk144_set_stream_pings)");
    const int count = sp.slot_n[slot];
    if(count == 0) return fail(h, MSK144_ESTATE, "msk144_stream_pings_slot before a push on this slot since msk144_set_stream_pings");
    *records = reinterpret_cast<const msk144_wideband_ping*>(sp.out[slot]);
    *levels = reinterpret_cast<const msk144_stream_level*>(sp.out[slot] + StreamPings::levels_at(count));
    *energies = reinterpret_cast<const int32_t*>(sp.out[slot] + StreamPings::energies_at(count));
    *n = count;
    return MSK144_OK;
}

}  // extern "C"
