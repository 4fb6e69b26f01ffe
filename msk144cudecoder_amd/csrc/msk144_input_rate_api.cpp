// The input-rate entries of the C ABI (include/msk144hip.h, "Audio input at 24 to 192 kHz"): msk144_set_input_rate,
// msk144_rate_hop_slot, the read entries, and ir_resample, the step the push (push_stream_hops, msk144_api.cpp) runs for
// msk144_push_rate_hops between the staging copies and everything else - pings, gate, hop ring, front end.
#include "api_handle.h"

#include <cstring>

using namespace msk144;

namespace
{

void ir_release(msk144_handle* h)
{
    InputRate& ir = h->ir;
    for(int s = 0; s < MSK144_SLOTS; s++)
    {
        if(ir.hops[s]) host_free(h->mem, &ir.hops[s]);
        if(ir.first_halves[s]) host_free(h->mem, &ir.first_halves[s]);
        if(ir.slot_clamped[s]) host_free(h->mem, &ir.slot_clamped[s]);
    }
    if(ir.d_in_hops) dev_free(h->mem, &ir.d_in_hops);
    if(ir.d_in_first) dev_free(h->mem, &ir.d_in_first);
    if(ir.d_hist) dev_free(h->mem, &ir.d_hist);
    if(ir.d_taps) dev_free(h->mem, &ir.d_taps);
    if(ir.d_clamped) dev_free(h->mem, &ir.d_clamped);
    ir = InputRate{};
}

// the read entries: a msk144_push_rate_hops has been made since the `set`
int ir_read_ready(msk144_handle* h, const char* entry)
{
    if(!h) return fail(h, MSK144_EINVAL, "null argument");
    if(!h->ir.on) return fail(h, MSK144_EINVAL, std::string(entry) + ": the handle has no input rate (msk144_set_input_rate)");
    if(!h->ir.pushed) return fail(h, MSK144_ESTATE, std::string(entry) + " before msk144_push_rate_hops");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MSK144_OK;
}

}  // namespace

int ir_resample(msk144_handle* h, int32_t slot, int32_t n, bool any_first)
{
    InputRate& ir = h->ir;
    const msk144_handle::Slot& sl = h->slots[slot];
    ev_begin(h);
    hipError_t e = hipMemsetAsync(ir.d_clamped, 0, sizeof(int32_t) * n, h->stream);
    if(e == hipSuccess)
    {
        ResampleArgs a{};
        a.in_first = ir.d_in_first;
        a.in_hops = ir.d_in_hops;
        a.streams = h->d_streams;
        a.is_first = h->d_isfirst;
        a.taps = ir.d_taps;
        a.hist = ir.d_hist;
        a.out_first = reinterpret_cast<int16_t*>(h->d_first);
        a.out_hops = reinterpret_cast<int16_t*>(h->d_hops);
        a.clamped = ir.d_clamped;
        a.P = ir.shape.P;
        a.Q = ir.shape.Q;
        a.H = ir.shape.H;
        a.hist_stride = ir.hist_stride;
        a.row = ir.shape.row;
        a.dwords = ir.shape.dwords;
        a.shift = ir.shift;
        launch_resample(a, n, any_first, h->stream);
        e = hipGetLastError();
        // the slot's own copy of the counts: complete when the slot's fetch is, whatever the other slot pushes meanwhile
        if(e == hipSuccess) e = hipMemcpyAsync(ir.slot_clamped[slot], ir.d_clamped, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream);
    }
    ev_end(h, MSK144_T_FRONTEND);
    if(e != hipSuccess) return fail(h, MSK144_EHIP, std::string("msk144_push_rate_hops: ") + hipGetErrorString(e));
    ir.last_n = n;
    ir.last_first.assign(sl.is_first, sl.is_first + n);
    for(int32_t j = 0; j < n; j++) ir.started[static_cast<size_t>(sl.streams[j])] = 1;
    ir.pushed = true;
    ir.slot_n[slot] = n;
    return MSK144_OK;
}

extern "C" {

int msk144_set_input_rate(msk144_handle* h, const msk144_input_rate_params* p)
{
    if(!h) return fail(h, MSK144_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->params.device));
    if(!p)
    {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        ir_release(h);
        return MSK144_OK;
    }
    if(const int rc = streams_only(h, "msk144_set_input_rate", "the resampler takes int16 audio"); rc != MSK144_OK) return rc;
    const std::string why = msk144ir::check_config(p->rate_hz, p->shift, p->num_taps, p->taps);
    if(!why.empty()) return fail(h, MSK144_EINVAL, "msk144_set_input_rate: " + why);

    HIP_TRY(h, hipStreamSynchronize(h->stream));
    ir_release(h);
    InputRate& ir = h->ir;
    ir.rate_hz = p->rate_hz;
    ir.shape = msk144ir::shape(p->rate_hz, p->num_taps);
    ir.shift = p->shift;
    ir.hist_stride = std::max(ir.shape.H, 1);
    const size_t nch = static_cast<size_t>(h->st.channels);
    const std::vector<uint32_t> packed = msk144ir::pack_taps(ir.shape, p->taps);
    int rc;
    if((rc = dev_alloc(h, h->mem, &ir.d_taps, packed.size())) != MSK144_OK || (rc = dev_alloc(h, h->mem, &ir.d_hist, nch * ir.hist_stride)) != MSK144_OK ||
       (rc = dev_alloc(h, h->mem, &ir.d_clamped, nch)) != MSK144_OK || (rc = dev_alloc(h, h->mem, &ir.d_in_hops, nch * ir.shape.row)) != MSK144_OK ||
       (rc = dev_alloc(h, h->mem, &ir.d_in_first, nch * ir.shape.row)) != MSK144_OK ||
       (rc = host_alloc(h, h->mem, &ir.slot_clamped[0], nch)) != MSK144_OK || (rc = host_alloc(h, h->mem, &ir.slot_clamped[1], nch)) != MSK144_OK)
    {
        ir_release(h);
        return rc;
    }
    hipError_t e = hipMemcpy(ir.d_taps, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if(e == hipSuccess) e = hipMemset(ir.d_hist, 0, nch * ir.hist_stride * sizeof(int16_t));
    if(e == hipSuccess) e = hipMemset(ir.d_clamped, 0, nch * sizeof(int32_t));
    if(e != hipSuccess)
    {
        ir_release(h);
        return fail(h, MSK144_EHIP, std::string("msk144_set_input_rate: ") + hipGetErrorString(e));
    }
    ir.started.assign(nch, 0);
    ir.on = true;
    return MSK144_OK;
}

int msk144_rate_hop_slot(msk144_handle* h, int32_t slot, void** hops, void** first_halves, int32_t** streams, uint8_t** is_first, int32_t* row_samples)
{
    if(!h || !hops || !first_halves || !streams || !is_first || !row_samples || slot < 0 || slot >= MSK144_SLOTS) return fail(h, MSK144_EINVAL, "bad argument");
    if(!h->ir.on) return fail(h, MSK144_ESTATE, "msk144_rate_hop_slot before msk144_set_input_rate");
    HIP_TRY(h, hipSetDevice(h->params.device));
    int rc = ensure_ring(h);
    if(rc != MSK144_OK) return rc;
    InputRate& ir = h->ir;
    const size_t count = static_cast<size_t>(h->st.channels) * ir.shape.row;
    for(int s = 0; s < MSK144_SLOTS; s++)
    {
        if(!ir.hops[s] && (rc = host_alloc(h, h->mem, &ir.hops[s], count)) != MSK144_OK) return rc;
        if(!ir.first_halves[s] && (rc = host_alloc(h, h->mem, &ir.first_halves[s], count)) != MSK144_OK) return rc;
    }
    *hops = ir.hops[slot];
    *first_halves = ir.first_halves[slot];
    *streams = h->slots[slot].streams;
    *is_first = h->slots[slot].is_first;
    *row_samples = ir.shape.row;
    return MSK144_OK;
}

int msk144_push_rate_hops(msk144_handle* h, int32_t slot, int32_t n)
{
    return push_stream_hops(h, slot, n, "msk144_push_rate_hops", true);
}

int msk144_dump_rate_hop(msk144_handle* h, int32_t j, int16_t* out, int32_t* n)
{
    int rc = ir_read_ready(h, "msk144_dump_rate_hop");
    if(rc != MSK144_OK) return rc;
    if(!out || !n || j < 0 || j >= h->ir.last_n) return fail(h, MSK144_EINVAL, "bad argument: position must be below n of the last push");
    const size_t half = MSK144_HOP_SAMPLES * sizeof(int16_t);
    const bool first = h->ir.last_first[static_cast<size_t>(j)] != 0;
    if(first) HIP_TRY(h, hipMemcpy(out, h->d_first + half * j, half, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(out + (first ? MSK144_HOP_SAMPLES : 0), h->d_hops + half * j, half, hipMemcpyDeviceToHost));
    *n = first ? MSK144_WINDOW_SAMPLES : MSK144_HOP_SAMPLES;
    return MSK144_OK;
}

int msk144_input_rate_clamped(msk144_handle* h, int32_t* clamped)
{
    int rc = ir_read_ready(h, "msk144_input_rate_clamped");
    if(rc != MSK144_OK) return rc;
    if(!clamped) return fail(h, MSK144_EINVAL, "null argument");
    HIP_TRY(h, hipMemcpy(clamped, h->ir.d_clamped, sizeof(int32_t) * h->ir.last_n, hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_input_rate_slot_clamped(msk144_handle* h, int32_t slot, const int32_t** clamped, int32_t* n)
{
    if(!h || !clamped || !n || slot < 0 || slot >= MSK144_SLOTS) return fail(h, MSK144_EINVAL, "bad argument");
    if(!h->ir.on) return fail(h, MSK144_EINVAL, "msk144_input_rate_slot_clamped: the handle has no input rate (msk144_set_input_rate)");
    if(h->ir.slot_n[slot] == 0) return fail(h, MSK144_ESTATE, "msk144_input_rate_slot_clamped before msk144_push_rate_hops on this slot");
    *clamped = h->ir.slot_clamped[slot];
    *n = h->ir.slot_n[slot];
    return MSK144_OK;
}

}  // extern "C"
