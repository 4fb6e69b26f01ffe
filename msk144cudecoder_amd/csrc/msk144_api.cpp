// C ABI of libmsk144hip.so (include/msk144hip.h): handle lifetime, buffers, launch order.
// Host-side restatement of the reference's setup code; compiled with -ffp-contract=off so that the
// frequency grid, the sync template and the FFT mask are computed with the reference's float ops.
#include "../../include/msk144hip.h"

#include "msk144_kernels.h"
#include "msk144_tables.h"
#include "wideband.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace msk144;

static_assert(sizeof(msk144_candidate) == kReferenceResultItemBytes, "msk144_candidate must mirror the reference ResultItem");
static_assert(sizeof(msk144_result) == 52, "msk144_result layout");

// Device and pinned host buffers that are freed together (dev_alloc, host_alloc register them)
struct Buffers
{
    std::vector<void*> device, pinned;

    void release()
    {
        for(void* p : device) (void)hipFree(p);
        for(void* p : pinned) (void)hipHostFree(p);
        device.clear();
        pinned.clear();
    }
};

struct msk144_handle
{
    msk144_params params{};
    DeviceStore st{};
    SyncTemplate tpl{};
    std::vector<float> freq_host;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    // every buffer of the handle except those of its wideband configuration
    Buffers mem;
    float* d_freq = nullptr;
    float2* d_cb42 = nullptr;
    uint8_t* d_input = nullptr;  // staging for host-submitted windows
    float2* d_twiddle = nullptr;
    float* d_fft_mask = nullptr;

    int llr_block = 1;  // channels per softbits->index->LDPC block
    bool retained = true;  // every LLR row of a decode stays readable (one block covers all channels and msk144_set_llr_retention was not switched off)
    bool rows_valid = true;  // the LLR store holds every row of the last softbits run (false after a decode without retention, until the next retained one)
    int active = 1;     // channels the current hop covers (msk144_submit_slot_n: the first n of the slot); <= st.channels
    bool have_window = false;
    bool decoded = false;
    bool profiling = false;
    // HIP-event pairs recorded around each stage; a pool so that many steps can be in flight
    // before the times are harvested at the next synchronisation point
    struct Span
    {
        int stage;
        int call;  // spans of one decode/submit call are summed into one sample
        hipEvent_t e0, e1;
    };
    int call_id = 0;
    int last_call[MSK144_T_COUNT];
    std::vector<Span> spans_pending;
    std::vector<hipEvent_t> ev_free;
    hipEvent_t ev_open = nullptr;
    double t_sum[MSK144_T_COUNT]{};
    int t_cnt[MSK144_T_COUNT]{};

    // Pinned staging slots (msk144_input_slot .. msk144_fetch_wait), allocated on first use.  Slot 0's device record list is
    // st.results of the plain calls; slot 1 has its own, so the list of one slot survives the decode of the other.
    struct Slot
    {
        uint8_t* in = nullptr;              // pinned windows, input_bytes()
        msk144_result* d_records = nullptr; // device record list this slot's decode writes
        msk144_result* out = nullptr;       // pinned records, max_results
        int32_t* out_count = nullptr;       // pinned
        float* out_seg = nullptr;           // pinned [channels][8]
        int32_t copied = 0;                 // records covered by the asynchronous copy
        hipEvent_t done = nullptr;
        bool pending = false;
        // hop-ring inputs (msk144_hop_slot), pinned, allocated on first use
        uint8_t* hops = nullptr;          // [channels][half window]
        uint8_t* first_halves = nullptr;  // [channels][half window]
        int32_t* streams = nullptr;    // [channels]
        uint8_t* is_first = nullptr;   // [channels]
    };
    Slot slots[MSK144_SLOTS];
    bool slots_ready = false;
    int cur_slot = 0;                        // the slot whose record list the next decode writes
    std::atomic<int32_t> last_total{0};      // record count of the last fetched hop: sizes the next asynchronous copy
    hipStream_t copy_stream = nullptr;       // remainder copies of msk144_fetch_wait (may run on a second thread)
    // device side of the hop ring: every stream's current window, and the staging of one batch of hops
    uint8_t* d_ring = nullptr;
    uint8_t* d_hops = nullptr;
    uint8_t* d_first = nullptr;
    int32_t* d_streams = nullptr;
    uint8_t* d_isfirst = nullptr;
    bool ring_ready = false;
    // msk144_clock_probe: its own stream, so that the probe wave runs beside the decode kernels
    hipStream_t probe_stream = nullptr;
    uint64_t* d_probe = nullptr;

    // wideband channeliser (msk144_set_wideband); its buffers have their own owner, as a new configuration replaces them
    struct Wideband
    {
        Buffers mem;
        bool configured = false;
        bool started = false;     // a first push has been made since the configuration
        bool last_first = false;  // the last push was a first push (5184 samples per channel)
        int P = 0, Q = 0;         // Fs = 12000 P/Q in lowest terms; Q = 1: decimation by D = P
        int K = 0, L = 0, format = 0;
        int hist = 0;             // history samples kept between pushes: ceil(L/Q) - 1 (L - 1 for Q = 1)
        float gain = 0.0f;
        long long m_next = 0;     // output sample index of the next push
        size_t slot_bytes = 0;    // pinned bytes per slot: 5184*P/Q samples
        uint8_t* pinned[MSK144_SLOTS] = {};
        uint8_t* d_raw = nullptr; // history samples + the samples of one push, raw format
        float2* d_G = nullptr;    // one block per branch (WidebandBranch); Q = 1: the one block [ceil(channels/32)][D][K][32]
        WidebandBranch* d_branches = nullptr;  // [Q]
        int32_t* d_fmod = nullptr;
        float2* d_rot = nullptr;  // [12000]
        unsigned long long* d_clip = nullptr;
        // per-channel levels, gains and the stepped AGC (msk144_wideband_levels, msk144_set_wideband_gains, msk144_set_wideband_agc)
        std::vector<float> gains;              // base gain of every channel (params.gain until msk144_set_wideband_gains)
        std::vector<float> push_gains;         // the base gains the last push was quantised with, and whether the AGC ran behind it
        bool push_agc = false;
        std::vector<int32_t> slot_channel;     // the channel of every slot (-1: padding)
        bool agc = false;
        msk144wb::AgcParams agc_params;
        unsigned long long* d_levels = nullptr;  // [channels] msk144wb::pack_level of the last push
        float* d_scale = nullptr;              // [slots] what the next push is quantised with: 128 x gain x 2^exponent
        float* d_base_scale = nullptr;         // [slots] the same at exponent 0
        float* d_gains = nullptr;              // [channels]
        int32_t* d_exp = nullptr;              // [channels] AGC exponent of the next push
        int32_t* d_quiet = nullptr;            // [channels] pushes in a row below the window
        int32_t* d_used_exp = nullptr;         // [channels] AGC exponent of the last push
        // impulse-noise blanker (msk144_set_wideband_blanker): what is set applies from the next first push; a running stream keeps
        // what it started with.  A blanked stream lives on the device as cs16 in d_blanked (history + one push, as d_raw), made from
        // the raw push in d_stage
        bool blanker_set = false, blanker_on = false;
        msk144wb::BlankerParams blanker_next, blanker;
        uint8_t* d_stage = nullptr;
        uint8_t* d_blanked = nullptr;
        BlankerCounters* d_blanker = nullptr;
        long long blanker_pushes = 0;   // of the running stream: its parity picks the carry word
        long long blanker_samples = 0;  // input samples since the first push
        // power spectrum of the input stream (msk144_set_wideband_spectrum): applies from the next push; `set` allocates - tables and
        // result for the largest B once, the partial sums for the largest B set so far (spectrum_rows_bins).  spectrum_pushed: the last
        // push left a spectrum of spectrum_last_bins bins
        int spectrum_bins = 0;          // B of the next push; 0: off
        int spectrum_last_bins = 0;
        int spectrum_rows_bins = 0;
        bool spectrum_pushed = false;
        float* d_spec_window = nullptr;     // [B]
        float2* d_spec_tw = nullptr;        // [B] e^{-j2pi m/B}
        double* d_spec_partials = nullptr;  // [kSpectrumMaxGroups][spectrum_rows_bins]
        double* d_spec_out = nullptr;       // [B] ascending frequency
        // ping detection (msk144_set_wideband_pings): applies from the next push; `set` allocates.  ping_restart: the next push is
        // the first since `set`; ping_pushed: the last push left records
        bool pings = false, ping_restart = false, ping_pushed = false;
        msk144wb::PingParams ping_params;
        msk144wb::PingHistory* d_ping_state = nullptr;   // [channels]
        msk144wb::PingRecord* d_ping_records = nullptr;  // [channels]
        int32_t* d_ping_energies = nullptr;              // [channels][54]
        // the ping band (msk144_set_wideband_ping_band): applies from the next push made with the detector on; `set` allocates
        bool ping_band = false;
        int32_t ping_band_shift = 0;
        int8_t* d_ping_band_taps = nullptr;    // [64][2]
        uint8_t* d_ping_band_tails = nullptr;  // [channels][128]: two zero bytes, then the 63 stored samples before the next push
        // per-channel waterfall (msk144_set_wideband_waterfall): applies from the next push; `set` allocates.  waterfall_pushed: the
        // last push left rows and sums
        bool waterfall = false, waterfall_pushed = false;
        float2* d_wf_dft = nullptr;   // [3][96][32] the windowed DFT matrix in the kernel's order
        float* d_wf_rows = nullptr;   // [channels][54][96]
        double* d_wf_sums = nullptr;  // [channels][96]
        // per-ping capture (msk144_set_wideband_capture): applies from the next push; `set` allocates - the descriptors and rows for
        // the largest max_units set so far (capture_rows; a larger one frees them and allocates anew).  capture_restart: the next
        // push is the first since `set`; capture_pushed: the last push left a header and no `set` has come since
        bool capture = false, capture_restart = false, capture_pushed = false;
        msk144wb::CaptureParams capture_params;
        int capture_rows = 0;
        uint8_t* d_cap_listed = nullptr;                  // [channels]
        msk144wb::CaptureState* d_cap_state = nullptr;    // [channels]
        msk144wb::CaptureHeader* d_cap_header = nullptr;  // [1]
        msk144wb::CaptureUnit* d_cap_units = nullptr;     // [capture_rows]
        uint8_t* d_cap_data = nullptr;                    // [capture_rows][5184]
        // Fs = 12000 Pin/Qin, the input rate (= P/Q without the bank); raw history samples kept between pushes
        int Pin = 0, Qin = 0, raw_hist = 0;
        // two-stage bank (rates above 6.144 Msps): P/Q, K, L, hist above are those of the channeliser at Fs/32
        bool bank = false;
        int K1 = 0;
        int slots = 0;                 // channel slots: each band's channels padded to whole waves of 32
        std::vector<int> band_index;   // occupied band k mod 64 of sub-band stream j
        long long stride = 0;          // float2 per sub-band stream: hist + 5184 P/Q frames
        long long n_next = 0;          // bank frame index of the next push
        int last_frames = 0;           // frames of the last push
        float* d_h1 = nullptr;
        int32_t* d_bands = nullptr;
        float2* d_tw = nullptr;        // [64]
        float2* d_sub = nullptr;       // [bands][stride]
        int32_t* d_wave_band = nullptr;
        int32_t* d_slot_channel = nullptr;
    } wb;

    std::string error;
};

namespace
{

thread_local std::string g_create_error;

// Channels per softbits -> index -> LDPC block when the caller leaves msk144_params.llr_block_channels at 0 (include/msk144hip.h): the
// bottom of a flat valley on the 1024-channel bench step (profiles/r06_sweep_ldpc_grid_and_block.txt, r06_sweep_block.txt)
constexpr int kDefaultLlrBlockChannels = 128;

int fail(msk144_handle* h, int code, const std::string& msg)
{
    if(h) h->error = msg;
    else g_create_error = msg;
    return code;
}

#define HIP_TRY(h, expr)                                                                                   \
    do                                                                                                     \
    {                                                                                                      \
        hipError_t e_ = (expr);                                                                            \
        if(e_ != hipSuccess) return fail(h, MSK144_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while(0)

// count elements of device (hipMalloc) or pinned host (hipHostMalloc) memory, registered with the owner that frees them
template<typename T>
int alloc(msk144_handle* h, Buffers& owner, bool pinned, T** p, size_t count)
{
    void* q = nullptr;
    const size_t bytes = count * sizeof(T);
    hipError_t e = pinned ? hipHostMalloc(&q, bytes ? bytes : 1, hipHostMallocDefault) : hipMalloc(&q, bytes ? bytes : 1);
    if(e != hipSuccess)
    {
        char buf[160];
        snprintf(buf, sizeof(buf), "%s(%zu bytes): %s", pinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
        return fail(h, MSK144_ENOMEM, buf);
    }
    (pinned ? owner.pinned : owner.device).push_back(q);
    *p = static_cast<T*>(q);
    return MSK144_OK;
}

template<typename T>
int dev_alloc(msk144_handle* h, Buffers& owner, T** p, size_t count)
{
    return alloc(h, owner, false, p, count);
}

// frees one buffer that dev_alloc registered with `owner` ahead of the rest; *p = nullptr
template<typename T>
void dev_free(Buffers& owner, T** p)
{
    const auto it = std::find(owner.device.begin(), owner.device.end(), static_cast<void*>(*p));
    if(it != owner.device.end())
    {
        (void)hipFree(*it);
        owner.device.erase(it);
    }
    *p = nullptr;
}

template<typename T>
int host_alloc(msk144_handle* h, Buffers& owner, T** p, size_t count)
{
    return alloc(h, owner, true, p, count);
}

size_t window_bytes(const msk144_handle* h)
{
    return (h->params.read_mode == 2) ? 2 * kWindowSamples : kWindowSamples * sizeof(int16_t);
}

size_t input_bytes(const msk144_handle* h)
{
    return window_bytes(h) * h->params.channels;
}

// the store as the kernels of the current hop see it: the first `active` channels
DeviceStore active_store(const msk144_handle* h)
{
    DeviceStore st = h->st;
    st.channels = h->active;
    st.nch = h->active;
    return st;
}

// the device record list of the current slot, which the last decode wrote; st.results for slot 0 and before any slot exists
msk144_result* current_records(const msk144_handle* h)
{
    return h->slots_ready ? h->slots[h->cur_slot].d_records : static_cast<msk144_result*>(h->st.results);
}

hipEvent_t ev_take(msk144_handle* h)
{
    if(!h->ev_free.empty())
    {
        hipEvent_t e = h->ev_free.back();
        h->ev_free.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if(hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void ev_begin(msk144_handle* h)
{
    if(!h->profiling) return;
    h->ev_open = ev_take(h);
    if(h->ev_open) (void)hipEventRecord(h->ev_open, h->stream);
}

void ev_end(msk144_handle* h, int stage)
{
    if(!h->profiling || !h->ev_open) return;
    hipEvent_t e1 = ev_take(h);
    if(!e1)
    {
        h->ev_free.push_back(h->ev_open);
        h->ev_open = nullptr;
        return;
    }
    (void)hipEventRecord(e1, h->stream);
    h->spans_pending.push_back({stage, h->call_id, h->ev_open, e1});
    h->ev_open = nullptr;
}

// fold finished event pairs into the running sums; requires the stream to be idle
void harvest_times(msk144_handle* h)
{
    for(const auto& sp : h->spans_pending)
    {
        float ms = 0.0f;
        if(hipEventElapsedTime(&ms, sp.e0, sp.e1) == hipSuccess)
        {
            h->t_sum[sp.stage] += ms;
            if(h->last_call[sp.stage] != sp.call)
            {
                h->last_call[sp.stage] = sp.call;
                h->t_cnt[sp.stage]++;
            }
        }
        h->ev_free.push_back(sp.e0);
        h->ev_free.push_back(sp.e1);
    }
    h->spans_pending.clear();
}

int ensure_slots(msk144_handle* h)
{
    if(h->slots_ready) return MSK144_OK;
    HIP_TRY(h, hipSetDevice(h->params.device));
    if(!h->copy_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    for(int s = 0; s < MSK144_SLOTS; s++)
    {
        msk144_handle::Slot& sl = h->slots[s];
        int rc = MSK144_OK;
        if(!sl.in && (rc = host_alloc(h, h->mem, &sl.in, input_bytes(h))) != MSK144_OK) return rc;
        if(!sl.out && (rc = host_alloc(h, h->mem, &sl.out, h->st.max_results)) != MSK144_OK) return rc;
        if(!sl.out_count && (rc = host_alloc(h, h->mem, &sl.out_count, 1)) != MSK144_OK) return rc;
        if(!sl.out_seg && (rc = host_alloc(h, h->mem, &sl.out_seg, 8 * static_cast<size_t>(h->st.channels))) != MSK144_OK) return rc;
        if(!sl.d_records)
        {
            if(s == 0) sl.d_records = static_cast<msk144_result*>(h->st.results);
            else if((rc = dev_alloc(h, h->mem, &sl.d_records, h->st.max_results)) != MSK144_OK) return rc;
        }
        // blocking-sync event: the waiting thread sleeps instead of spinning on a core the ingest thread needs
        if(!sl.done) HIP_TRY(h, hipEventCreateWithFlags(&sl.done, hipEventBlockingSync | hipEventDisableTiming));
    }
    h->slots_ready = true;
    return MSK144_OK;
}

int ensure_ring(msk144_handle* h)
{
    if(h->ring_ready) return MSK144_OK;
    int rc = ensure_slots(h);
    if(rc != MSK144_OK) return rc;
    // only what is still missing, so that a retry after a failed allocation allocates nothing twice
    const size_t nch = static_cast<size_t>(h->st.channels);
    const size_t half = window_bytes(h) / 2;
    if(!h->d_ring && (rc = dev_alloc(h, h->mem, &h->d_ring, nch * window_bytes(h))) != MSK144_OK) return rc;
    if(!h->d_hops && (rc = dev_alloc(h, h->mem, &h->d_hops, nch * half)) != MSK144_OK) return rc;
    if(!h->d_first && (rc = dev_alloc(h, h->mem, &h->d_first, nch * half)) != MSK144_OK) return rc;
    if(!h->d_streams && (rc = dev_alloc(h, h->mem, &h->d_streams, nch)) != MSK144_OK) return rc;
    if(!h->d_isfirst && (rc = dev_alloc(h, h->mem, &h->d_isfirst, nch)) != MSK144_OK) return rc;
    HIP_TRY(h, hipMemsetAsync(h->d_ring, 0, nch * window_bytes(h), h->stream));
    for(auto& sl : h->slots)
    {
        if(!sl.hops && (rc = host_alloc(h, h->mem, &sl.hops, nch * half)) != MSK144_OK) return rc;
        if(!sl.first_halves && (rc = host_alloc(h, h->mem, &sl.first_halves, nch * half)) != MSK144_OK) return rc;
        if(!sl.streams && (rc = host_alloc(h, h->mem, &sl.streams, nch)) != MSK144_OK) return rc;
        if(!sl.is_first && (rc = host_alloc(h, h->mem, &sl.is_first, nch)) != MSK144_OK) return rc;
        std::memset(sl.is_first, 0, nch);
    }
    h->ring_ready = true;
    return MSK144_OK;
}

int copy_windows_in(msk144_handle* h, const void* host_windows)
{
    ev_begin(h);
    hipError_t e = hipMemcpyAsync(h->d_input, host_windows, window_bytes(h) * h->active, hipMemcpyHostToDevice, h->stream);
    ev_end(h, MSK144_T_H2D);
    if(e != hipSuccess) return fail(h, MSK144_EHIP, std::string("hipMemcpyAsync(windows): ") + hipGetErrorString(e));
    return MSK144_OK;
}

// Long profiled runs (msk144hipdecoder --timing) never reach a synchronisation point: fold the spans whose end event has already
// completed, oldest first, so that the pending list stays short without waiting for anything.
void harvest_finished(msk144_handle* h)
{
    if(h->spans_pending.size() < 4096) return;
    size_t done = 0;
    while(done < h->spans_pending.size() && hipEventQuery(h->spans_pending[done].e1) == hipSuccess) done++;
    if(done == 0) return;
    std::vector<msk144_handle::Span> rest(h->spans_pending.begin() + static_cast<long>(done), h->spans_pending.end());
    h->spans_pending.resize(done);
    harvest_times(h);
    h->spans_pending = std::move(rest);
}

int run_frontend(msk144_handle* h, const void* d_in)
{
    ev_begin(h);
    const DeviceStore st = active_store(h);
    if(h->params.read_mode == 2) launch_frontend_iq(st, static_cast<const int8_t*>(d_in), h->stream);
    else launch_frontend_audio(st, static_cast<const int16_t*>(d_in), h->params.analytic_method, h->d_twiddle, h->d_fft_mask, h->stream);
    ev_end(h, MSK144_T_FRONTEND);
    HIP_TRY(h, hipGetLastError());
    h->have_window = true;
    h->decoded = false;
    return MSK144_OK;
}

// back to no wideband configuration: its buffers freed, every field reset
void wb_release(msk144_handle* h)
{
    h->wb.mem.release();
    h->wb = {};
}

// ---- msk144_set_wideband_ex, step by step ----

// Every rule a configuration must meet (csrc/wideband.h check_config and the ones that need the handle); h1 = the bank prototype
// above 6.144 Msps, the caller's or the default one
int wb_validate(msk144_handle* h, const msk144_wideband_params* wp, const double* bank_taps, int32_t bank_num_taps, std::vector<double>& h1)
{
    if(!h || !wp) return fail(h, MSK144_EINVAL, "null argument");
    if(h->params.read_mode != 2) return fail(h, MSK144_EINVAL, "wideband input needs an IQ handle (read_mode 2)");
    if(wp->num_offsets != h->params.channels) return fail(h, MSK144_EINVAL, "the number of channel offsets must equal the handle's channels");
    const std::string why = msk144wb::check_config(wp->rate_hz, wp->format, wp->taps_per_phase, wp->gain, wp->offsets_hz, wp->num_offsets);
    if(!why.empty()) return fail(h, MSK144_EINVAL, why);
    const bool bank = msk144wb::is_bank_rate(wp->rate_hz);
    if(!bank && (bank_taps || bank_num_taps)) return fail(h, MSK144_EINVAL, "bank taps are only taken above 6144000 Hz (two-stage bank)");
    if(bank && !bank_taps) h1 = msk144wb::design_bank_taps(wp->rate_hz, msk144wb::kDefaultBankTapsPerBand);
    else if(bank)
    {
        if(bank_num_taps < msk144wb::kBankBands || bank_num_taps > msk144wb::kBankBands * msk144wb::kMaxBankTapsPerBand || bank_num_taps % msk144wb::kBankBands)
            return fail(h, MSK144_EINVAL, "the bank filter needs 64 x K1 taps, 1 <= K1 <= 16");
        h1.assign(bank_taps, bank_taps + bank_num_taps);
        for(double v : h1)
            if(!std::isfinite(v)) return fail(h, MSK144_EINVAL, "bank taps must be finite");
    }
    const msk144wb::RateRatio rr = msk144wb::rate_ratio(msk144wb::stage2_rate(wp->rate_hz));
    const int L = wp->taps_per_phase * rr.P;
    if(!wp->taps || wp->num_taps != L)
        return fail(h, MSK144_EINVAL, rr.Q == 1 ? "the filter needs taps_per_phase x D taps" : "the filter needs taps_per_phase x P taps (rate = 12000 x P/Q)");
    for(int k = 0; k < L; k++)
        if(!std::isfinite(wp->taps[k])) return fail(h, MSK144_EINVAL, "filter taps must be finite");
    return MSK144_OK;
}

// Channel slots: without the bank slot c is channel c; with it, the channels of each occupied band (k mod 64, ascending) one after
// another, each band's group padded to whole waves, at the residual offset f_c - k Fs/64
struct WbSlots
{
    std::vector<int32_t> slot_channel;   // the channel of slot c; -1: padding
    std::vector<long long> slot_offset;  // its offset at the channeliser's rate
    std::vector<int32_t> wave_band;      // bank: the sub-band stream of each wave of 32 slots
    std::vector<int32_t> band_list;      // bank: the occupied band k mod 64 of stream j
};

WbSlots wb_slot_layout(const msk144_wideband_params* wp, bool bank)
{
    WbSlots sl;
    const int C = wp->num_offsets;
    if(!bank)
    {
        for(int c = 0; c < C; c++)
        {
            sl.slot_channel.push_back(c);
            sl.slot_offset.push_back(wp->offsets_hz[c]);
        }
        return sl;
    }
    std::vector<std::vector<int>> by_band(msk144wb::kBankBands);
    for(int c = 0; c < C; c++) by_band[static_cast<size_t>(msk144wb::bank_band(wp->rate_hz, wp->offsets_hz[c]) & (msk144wb::kBankBands - 1))].push_back(c);
    for(int b = 0; b < msk144wb::kBankBands; b++)
    {
        const auto& chs = by_band[static_cast<size_t>(b)];
        if(chs.empty()) continue;
        const int j = static_cast<int>(sl.band_list.size());
        sl.band_list.push_back(b);
        const size_t n = (chs.size() + 31) / 32 * 32;
        for(size_t i = 0; i < n; i++)
        {
            const int c = i < chs.size() ? chs[i] : -1;
            sl.slot_channel.push_back(c);
            sl.slot_offset.push_back(c < 0 ? 0 : msk144wb::bank_residual(wp->rate_hz, wp->offsets_hz[c]));
            if(i % 32 == 0) sl.wave_band.push_back(j);
        }
    }
    return sl;
}

// The channeliser's tables at Fs = 12000 P/Q (fs = Fs, the rate it runs at), slot by slot with f_c the slot's offset.  Branch mr
// (outputs mr + Q a) has r = mr P mod Q, n0 = floor(mr P/Q) and the K_r = ceil((L - r)/Q) taps
//     G_r[c][k] = h[r + kQ] e^{+j2pi (f_c (k - n0) mod Fs)/Fs}
// computed in double with the phases in integers, stored f32 at [c/32][p][q][c%32] with k = p + P q (phase-major, the order the kernel
// walks), the blocks one after another by mr.  Q = 1 is the one branch {0, 0, L}: G[c][k] = h[k] e^{+j2pi (f_c k mod Fs)/Fs}.
struct WbTables
{
    std::vector<float2> G;
    std::vector<WidebandBranch> branches;
    std::vector<int32_t> fmod;  // f_c mod 12000 in 0..11999
};

WbTables wb_tap_tables(const msk144_wideband_params* wp, const WbSlots& sl, long long fs, int P, int Q)
{
    const int L = wp->num_taps;
    const int S = static_cast<int>(sl.slot_channel.size());
    const int C32 = (S + 31) / 32;
    WbTables t;
    long long off = 0;
    for(int mr = 0; mr < Q; mr++)
    {
        const int r = static_cast<int>(static_cast<long long>(mr) * P % Q);
        const int Kr = (L - r + Q - 1) / Q;
        t.branches.push_back(WidebandBranch{off, static_cast<int>(static_cast<long long>(mr) * P / Q), Kr});
        off += static_cast<long long>(C32) * Kr * 32;
    }
    t.G.assign(static_cast<size_t>(off), make_float2(0.0f, 0.0f));  // C32 x L x 32: the branches share the L taps out
    t.fmod.assign(static_cast<size_t>(S), 0);
    for(int c = 0; c < S; c++)
    {
        if(sl.slot_channel[static_cast<size_t>(c)] < 0) continue;
        const long long f = sl.slot_offset[static_cast<size_t>(c)];
        t.fmod[static_cast<size_t>(c)] = static_cast<int32_t>(((f % msk144wb::kOutRate) + msk144wb::kOutRate) % msk144wb::kOutRate);
        const long long fpos = ((f % fs) + fs) % fs;
        for(int mr = 0; mr < Q; mr++)
        {
            const WidebandBranch& br = t.branches[static_cast<size_t>(mr)];
            const int r = static_cast<int>(static_cast<long long>(mr) * P % Q);
            const long long rot0 = (fpos * br.n0) % fs;
            size_t at = static_cast<size_t>(br.g_off) + static_cast<size_t>(c / 32) * br.taps * 32 + (c % 32);
            for(int p = 0; p < std::min(P, br.taps); p++)
                for(int k = p; k < br.taps; k += P, at += 32)
                {
                    const long long ph_i = ((fpos * k) % fs - rot0 + fs) % fs;
                    const double ph = 2.0 * M_PI * static_cast<double>(ph_i) / static_cast<double>(fs);
                    const double hk = wp->taps[r + static_cast<size_t>(k) * Q];
                    t.G[at] = make_float2(static_cast<float>(hk * std::cos(ph)), static_cast<float>(hk * std::sin(ph)));
                }
        }
    }
    return t;
}

// e^{sign j2pi t/n}, t < n: the output rotation (n = 12000, sign -1) and the bank's twiddles (n = 64, sign +1)
std::vector<float2> unit_circle(int n, double sign)
{
    std::vector<float2> v(static_cast<size_t>(n));
    for(int t = 0; t < n; t++)
    {
        const double ph = 2.0 * M_PI * t / n;
        v[static_cast<size_t>(t)] = make_float2(static_cast<float>(std::cos(ph)), static_cast<float>(sign * std::sin(ph)));
    }
    return v;
}

// a device table of the wideband configuration, allocated and filled
template<typename T>
int wb_table(msk144_handle* h, T** d, const std::vector<T>& v)
{
    const int rc = dev_alloc(h, h->wb.mem, d, v.size());
    if(rc != MSK144_OK) return rc;
    HIP_TRY(h, hipMemcpy(*d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return MSK144_OK;
}

// The base gains to the device: every slot's scale at exponent 0 (a padding slot's is never read; it gets 0), which is also what
// the next push is quantised with, and the AGC state back to exponent 0 with no quiet pushes counted.  What the last push was
// quantised with (push_gains, d_used_exp) stays, for msk144_wideband_levels.
int wb_upload_gains(msk144_handle* h)
{
    auto& w = h->wb;
    std::vector<float> scale(w.slot_channel.size(), 0.0f);
    for(size_t c = 0; c < scale.size(); c++)
        if(w.slot_channel[c] >= 0) scale[c] = msk144wb::agc_scale(w.gains[static_cast<size_t>(w.slot_channel[c])], 0);
    // on the handle's stream, so that the next push is ordered behind them; waited for, as the sources live on this stack
    const size_t C = w.gains.size();
    HIP_TRY(h, hipMemcpyAsync(w.d_base_scale, scale.data(), sizeof(float) * scale.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(w.d_scale, scale.data(), sizeof(float) * scale.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(w.d_gains, w.gains.data(), sizeof(float) * C, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(w.d_exp, 0, sizeof(int32_t) * C, h->stream));
    HIP_TRY(h, hipMemsetAsync(w.d_quiet, 0, sizeof(int32_t) * C, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MSK144_OK;
}

// the entries below change what the next push is quantised with: configured, and nothing of an earlier push still running
int wb_quiesce(msk144_handle* h, const char* who)
{
    if(!h) return fail(h, MSK144_EINVAL, "null argument");
    if(!h->wb.configured) return fail(h, MSK144_EINVAL, std::string(who) + " needs wideband mode (msk144_set_wideband)");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MSK144_OK;
}

// the read entries of the ping detector: wideband mode, and the last push made with the detector on; waits for that push
int wb_ping_ready(msk144_handle* h, const char* who)
{
    const auto& w = h->wb;
    if(!w.configured) return fail(h, MSK144_EINVAL, std::string(who) + " needs wideband mode (msk144_set_wideband)");
    if(!w.started || !w.ping_pushed) return fail(h, MSK144_ESTATE, w.started ? "the last wideband push was made without the ping detector" : "no wideband push has been made");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MSK144_OK;
}

// the read entries of the waterfall: wideband mode, and the last push made with the waterfall on; waits for that push
int wb_waterfall_ready(msk144_handle* h, const char* who)
{
    const auto& w = h->wb;
    if(!w.configured) return fail(h, MSK144_EINVAL, std::string(who) + " needs wideband mode (msk144_set_wideband)");
    if(!w.started || !w.waterfall_pushed) return fail(h, MSK144_ESTATE, w.started ? "the last wideband push was made without the waterfall" : "no wideband push has been made");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MSK144_OK;
}

// Every buffer of the configuration whose shape h->wb already holds; on failure the caller releases what was allocated
int wb_allocate(msk144_handle* h, const WbSlots& sl, const WbTables& t, const std::vector<double>& h1)
{
    auto& w = h->wb;
    const size_t sb = static_cast<size_t>(msk144wb::sample_bytes(w.format));
    w.slot_bytes = static_cast<size_t>(kWindowSamples) / w.Qin * w.Pin * sb;
    int rc = MSK144_OK;
    for(uint8_t*& p : w.pinned)
        if((rc = host_alloc(h, w.mem, &p, w.slot_bytes)) != MSK144_OK) return rc;
    if((rc = dev_alloc(h, w.mem, &w.d_raw, static_cast<size_t>(w.raw_hist) * sb + w.slot_bytes)) != MSK144_OK) return rc;
    if((rc = wb_table(h, &w.d_G, t.G)) != MSK144_OK || (rc = wb_table(h, &w.d_branches, t.branches)) != MSK144_OK ||
       (rc = wb_table(h, &w.d_fmod, t.fmod)) != MSK144_OK || (rc = wb_table(h, &w.d_rot, unit_circle(msk144wb::kOutRate, -1.0))) != MSK144_OK)
        return rc;
    if((rc = dev_alloc(h, w.mem, &w.d_clip, 1)) != MSK144_OK) return rc;
    HIP_TRY(h, hipMemset(w.d_clip, 0, sizeof(unsigned long long)));
    const size_t C = w.gains.size(), S = w.slot_channel.size();
    if((rc = dev_alloc(h, w.mem, &w.d_levels, C)) != MSK144_OK || (rc = dev_alloc(h, w.mem, &w.d_scale, S)) != MSK144_OK ||
       (rc = dev_alloc(h, w.mem, &w.d_base_scale, S)) != MSK144_OK || (rc = dev_alloc(h, w.mem, &w.d_gains, C)) != MSK144_OK ||
       (rc = dev_alloc(h, w.mem, &w.d_exp, C)) != MSK144_OK || (rc = dev_alloc(h, w.mem, &w.d_quiet, C)) != MSK144_OK ||
       (rc = dev_alloc(h, w.mem, &w.d_used_exp, C)) != MSK144_OK)
        return rc;
    HIP_TRY(h, hipMemset(w.d_levels, 0, sizeof(unsigned long long) * C));
    HIP_TRY(h, hipMemset(w.d_used_exp, 0, sizeof(int32_t) * C));
    if((rc = wb_upload_gains(h)) != MSK144_OK) return rc;
    if(!w.bank) return MSK144_OK;
    if((rc = wb_table(h, &w.d_h1, std::vector<float>(h1.begin(), h1.end()))) != MSK144_OK || (rc = wb_table(h, &w.d_bands, sl.band_list)) != MSK144_OK ||
       (rc = wb_table(h, &w.d_tw, unit_circle(msk144wb::kBankBands, 1.0))) != MSK144_OK || (rc = wb_table(h, &w.d_wave_band, sl.wave_band)) != MSK144_OK ||
       (rc = wb_table(h, &w.d_slot_channel, sl.slot_channel)) != MSK144_OK)
        return rc;
    return dev_alloc(h, w.mem, &w.d_sub, w.band_index.size() * static_cast<size_t>(w.stride));
}

// the slot argument of an entry that begins a hop: in range, and not still waiting for msk144_fetch_wait
int check_hop_slot(msk144_handle* h, int32_t slot)
{
    if(!h || slot < 0 || slot >= MSK144_SLOTS) return fail(h, MSK144_EINVAL, "bad argument");
    if(h->slots[slot].pending) return fail(h, MSK144_ESTATE, "slot submitted again before its results were fetched (msk144_fetch_wait)");
    return MSK144_OK;
}

// every entry that begins a hop: a new call (one stage-time sample), the slot whose record list the decode writes, its channels
int begin_hop(msk144_handle* h, int32_t slot, int32_t n)
{
    HIP_TRY(h, hipSetDevice(h->params.device));
    h->call_id++;
    h->cur_slot = slot;
    h->active = n;
    return MSK144_OK;
}

// msk144_submit_{audio,iq}[_device]: every channel, into slot 0's record list; windows in host memory are staged in d_input first
int submit_windows(msk144_handle* h, const void* windows, int read_mode, bool host)
{
    if(!h || !windows) return fail(h, MSK144_EINVAL, "null argument");
    if(h->params.read_mode != read_mode)
        return fail(h, MSK144_ESTATE, read_mode == 1 ? "handle was created for IQ input (read_mode 2)" : "handle was created for audio input (read_mode 1)");
    int rc = begin_hop(h, 0, h->st.channels);
    if(rc == MSK144_OK && host) rc = copy_windows_in(h, windows);
    return rc == MSK144_OK ? run_frontend(h, host ? h->d_input : windows) : rc;
}

}  // namespace

extern "C" {

void msk144_default_params(msk144_params* p)
{
    if(!p) return;
    std::memset(p, 0, sizeof(*p));
    p->center_hz = 1500.0f;  // main.cu:124 (audio); IQ callers set 0 (main.cu:125)
    p->width_hz = 200.0f;    // main.cu:130
    p->step_hz = 2.0f;       // main.cu:129
    p->scan_depth = 4;       // main.cu:131
    p->nbadsync_threshold = 1;  // main.cu:133
    p->read_mode = 1;
    p->analytic_method = 2;  // main.cu:132
    p->channels = 1;
    p->device = 0;
    p->max_results = 0;
    p->llr_block_channels = 0;
}

const char* msk144_last_error(const msk144_handle* h)
{
    return h ? h->error.c_str() : g_create_error.c_str();
}

int msk144_device_count(int32_t* n)
{
    if(!n) return fail(nullptr, MSK144_EINVAL, "null argument");
    int ndev = 0;
    if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    {
        *n = 0;
        return fail(nullptr, MSK144_EHIP, "no HIP device available (libmsk144hip has no CPU fallback)");
    }
    *n = ndev;
    return MSK144_OK;
}

int msk144_create(const msk144_params* params, msk144_handle** out)
{
    if(!params || !out) return fail(nullptr, MSK144_EINVAL, "null argument");
    *out = nullptr;
    if(!(params->step_hz > 0.0f)) return fail(nullptr, MSK144_EINVAL, "search step must be > 0");  // assert at msk_context.cuh:97
    if(!(params->width_hz >= 0.0f)) return fail(nullptr, MSK144_EINVAL, "search width must be >= 0");
    if(params->channels < 1) return fail(nullptr, MSK144_EINVAL, "channels must be >= 1");
    if(params->llr_block_channels < 0) return fail(nullptr, MSK144_EINVAL, "llr_block_channels must be >= 0");
    if(params->read_mode != 1 && params->read_mode != 2) return fail(nullptr, MSK144_EINVAL, "read_mode must be 1 (audio) or 2 (IQ)");
    if(params->read_mode == 1 && params->analytic_method != 1 && params->analytic_method != 2)
        return fail(nullptr, MSK144_EINVAL, "analytic_method must be 1 (FFT) or 2 (shift-filter-shift)");

    msk144_handle* h = new(std::nothrow) msk144_handle();
    if(!h) return fail(nullptr, MSK144_ENOMEM, "out of host memory");
    h->params = *params;
    h->params.scan_depth = clamp_scan_depth(params->scan_depth);
    h->llr_block = params->llr_block_channels > 0 ? params->llr_block_channels : (params->channels <= kDefaultLlrBlockChannels ? params->channels : kDefaultLlrBlockChannels);
    if(h->llr_block > params->channels) h->llr_block = params->channels;
    h->params.llr_block_channels = h->llr_block;
    for(int s = 0; s < MSK144_T_COUNT; s++) h->last_call[s] = -1;

    // every failure below has set h->error through fail(h, ...)
    auto bail = [&](int code) {
        g_create_error = h->error;
        msk144_destroy(h);
        return code;
    };

    int ndev = 0;
    if(hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return bail(fail(h, MSK144_EHIP, "no HIP device available (libmsk144hip has no CPU fallback)"));
    if(params->device < 0 || params->device >= ndev) return bail(fail(h, MSK144_EINVAL, "device ordinal out of range"));
    if(hipSetDevice(params->device) != hipSuccess) return bail(fail(h, MSK144_EHIP, "hipSetDevice failed"));

    h->freq_host = frequency_grid(params->center_hz, params->width_hz, params->step_hz);
    const int F = static_cast<int>(h->freq_host.size());

    DeviceStore& st = h->st;
    st.channels = params->channels;
    st.F = F;
    st.D = h->params.scan_depth;
    st.K = F * st.D * kSlotsPerPattern;
    st.nbadsync_threshold = params->nbadsync_threshold;
    st.ch0 = 0;
    st.nch = st.channels;
    h->retained = h->llr_block >= st.channels;
    st.gate_early = h->retained ? 0 : 1;
    st.handover = st.gate_early;  // msk144_set_copy_handover
    h->active = st.channels;
    const long long total = static_cast<long long>(st.channels) * st.K;
    long long maxr = params->max_results > 0 ? params->max_results : (1 << 20);
    if(maxr > total) maxr = total;
    st.max_results = static_cast<int32_t>(maxr);
    h->params.max_results = st.max_results;

    sync_template(h->tpl.re, h->tpl.im, h->tpl.pp);
    // the kernels skip the multiplications by pp[0] and pp[6] (softbits.hip, scan.hip): exact only for these values
    if(h->tpl.pp[0] != 0.0f || h->tpl.pp[kPulseSamples / 2] != 1.0f) return bail(fail(h, MSK144_EINVAL, "half-sine pulse table: pp[0] != 0 or pp[6] != 1"));
    if(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(h, MSK144_EHIP, "hipStreamCreate failed"));
    h->stream = h->own_stream;

    const size_t ck = static_cast<size_t>(total);
    const size_t nch = static_cast<size_t>(st.channels);
    Buffers& m = h->mem;
    msk144_result* results = nullptr;
    // a failed dev_alloc has set the message; its code is MSK144_ENOMEM
    bool ok = dev_alloc(h, m, &h->d_freq, F) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &h->d_cb42, kSyncTaps) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.analytic, nch * kWindowSamples) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.seg_power, nch * 8) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.pos, ck) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.xb, ck) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.nbadsync, ck) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.llr, static_cast<size_t>(h->llr_block) * st.K * kCodeBits) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.idx, ck) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.n_idx, nch) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.dec_flag, ck) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.dec_iter, ck) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.dec_nhard, ck) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.dec_msg, ck * 3) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.dec_count, nch) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.copy_count, nch) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &st.result_count, 1) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &results, st.max_results) == MSK144_OK;
    ok = ok && dev_alloc(h, m, &h->d_input, input_bytes(h)) == MSK144_OK;
    if(!ok) return bail(MSK144_ENOMEM);
    st.results = results;
    st.freq = h->d_freq;
    st.cb42 = h->d_cb42;

    ok = ok && hipMemcpy(h->d_freq, h->freq_host.data(), sizeof(float) * F, hipMemcpyHostToDevice) == hipSuccess;
    {
        float2 cb[kSyncTaps];
        for(int k = 0; k < kSyncTaps; k++) cb[k] = make_float2(h->tpl.re[k], h->tpl.im[k]);
        ok = ok && hipMemcpy(h->d_cb42, cb, sizeof(cb), hipMemcpyHostToDevice) == hipSuccess;
    }
    // initial state on the handle's own (non-blocking) stream, which does not synchronise with the null stream; create
    // returns only after these have completed
    hipStream_t s0 = h->own_stream;
    ok = ok && hipMemsetAsync(st.dec_flag, 0, ck, s0) == hipSuccess;
    ok = ok && hipMemsetAsync(st.n_idx, 0, sizeof(int32_t) * st.channels, s0) == hipSuccess;
    ok = ok && hipMemsetAsync(st.dec_count, 0, sizeof(int32_t) * st.channels, s0) == hipSuccess;
    ok = ok && hipMemsetAsync(st.copy_count, 0, sizeof(int32_t) * st.channels, s0) == hipSuccess;
    ok = ok && hipMemsetAsync(st.result_count, 0, sizeof(int32_t), s0) == hipSuccess;
    ok = ok && hipMemsetAsync(st.pos, 0, ck * sizeof(uint32_t), s0) == hipSuccess;
    ok = ok && hipMemsetAsync(st.nbadsync, 0, ck * sizeof(int32_t), s0) == hipSuccess;
    ok = ok && hipStreamSynchronize(s0) == hipSuccess;

    if(ok && params->read_mode == 1 && params->analytic_method == 1)
    {
        const std::vector<float> mask = fft_band_mask();
        std::vector<float2> tw(kFftSize / 2);
        for(int j = 0; j < kFftSize / 2; j++)
        {
            const double ang = -2.0 * M_PI * j / kFftSize;
            tw[j] = make_float2(static_cast<float>(cos(ang)), static_cast<float>(sin(ang)));
        }
        if(dev_alloc(h, m, &h->d_twiddle, tw.size()) != MSK144_OK || dev_alloc(h, m, &h->d_fft_mask, mask.size()) != MSK144_OK) return bail(MSK144_ENOMEM);
        ok = ok && hipMemcpy(h->d_twiddle, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(h->d_fft_mask, mask.data(), mask.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    }
    if(!ok) return bail(fail(h, MSK144_EHIP, std::string("device initialisation failed: ") + hipGetErrorString(hipGetLastError())));
    *out = h;
    return MSK144_OK;
}

void msk144_destroy(msk144_handle* h)
{
    if(!h) return;
    (void)hipSetDevice(h->params.device);
    if(h->probe_stream) (void)hipStreamSynchronize(h->probe_stream);
    if(h->stream) (void)hipStreamSynchronize(h->stream);
    h->wb.mem.release();
    h->mem.release();
    for(auto& sl : h->slots)
        if(sl.done) (void)hipEventDestroy(sl.done);
    if(h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if(h->probe_stream) (void)hipStreamDestroy(h->probe_stream);
    for(const auto& sp : h->spans_pending)
    {
        (void)hipEventDestroy(sp.e0);
        (void)hipEventDestroy(sp.e1);
    }
    for(hipEvent_t e : h->ev_free) (void)hipEventDestroy(e);
    if(h->ev_open) (void)hipEventDestroy(h->ev_open);
    if(h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

int msk144_geometry(const msk144_handle* h, int32_t* num_freqs, int32_t* scan_depth, int32_t* items_per_channel)
{
    if(!h) return MSK144_EINVAL;
    if(num_freqs) *num_freqs = h->st.F;
    if(scan_depth) *scan_depth = h->st.D;
    if(items_per_channel) *items_per_channel = h->st.K;
    return MSK144_OK;
}

int msk144_frequency(const msk144_handle* h, int32_t block_idx, float* hz)
{
    if(!h || !hz || block_idx < 0 || block_idx >= h->st.F) return MSK144_EINVAL;
    *hz = h->freq_host[block_idx];
    return MSK144_OK;
}

int msk144_set_stream(msk144_handle* h, void* hip_stream)
{
    if(!h) return MSK144_EINVAL;
    HIP_TRY(h, hipSetDevice(h->params.device));  // every entry that touches the device selects the handle's own first: a caller may hold handles on several
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    harvest_times(h);
    h->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
    return MSK144_OK;
}

int msk144_submit_audio(msk144_handle* h, const int16_t* windows)
{
    return submit_windows(h, windows, 1, true);
}

int msk144_submit_iq(msk144_handle* h, const int8_t* windows)
{
    return submit_windows(h, windows, 2, true);
}

int msk144_submit_audio_device(msk144_handle* h, const int16_t* d_windows)
{
    return submit_windows(h, d_windows, 1, false);
}

int msk144_submit_iq_device(msk144_handle* h, const int8_t* d_windows)
{
    return submit_windows(h, d_windows, 2, false);
}

int msk144_submit_analytic(msk144_handle* h, const float* windows)
{
    if(!h || !windows) return fail(h, MSK144_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipMemcpyAsync(h->st.analytic, windows, sizeof(float2) * kWindowSamples * h->st.channels, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->cur_slot = 0;
    h->active = h->st.channels;
    h->have_window = true;
    h->decoded = false;
    return MSK144_OK;
}

int msk144_decode_stages(msk144_handle* h, uint32_t stages)
{
    if(!h) return MSK144_EINVAL;
    if((stages & (MSK144_STAGE_SCAN | MSK144_STAGE_SOFTBITS)) && !h->have_window) return fail(h, MSK144_ESTATE, "decode before any window was submitted");
    const bool blocked = !h->retained;
    const uint32_t mid = MSK144_STAGE_SOFTBITS | MSK144_STAGE_INDEX | MSK144_STAGE_LDPC;
    if(blocked && (stages & mid) != 0 && (stages & mid) != mid)
        return fail(h, MSK144_ENOTRETAINED, "LLR rows are not retained (blocked staging, or msk144_set_llr_retention(h, 0)): softbits, index and LDPC run together per channel block; a partial stage run needs llr_block_channels = channels");
    HIP_TRY(h, hipSetDevice(h->params.device));
    h->call_id++;
    if(h->profiling) harvest_finished(h);
    const DeviceStore cur = active_store(h);
    if(stages & MSK144_STAGE_SCAN)
    {
        ev_begin(h);
        launch_scan(cur, h->tpl, h->stream);
        ev_end(h, MSK144_T_SCAN);
    }
    // softbits -> index -> LDPC, one channel block at a time (one block = everything unless llr_block_channels says otherwise)
    if(stages & MSK144_STAGE_SOFTBITS) h->rows_valid = h->retained;
    if(stages & mid)
    {
        DeviceStore blk = cur;
        for(int ch0 = 0; ch0 < cur.channels; ch0 += h->llr_block)
        {
            blk.ch0 = ch0;
            blk.nch = cur.channels - ch0 < h->llr_block ? cur.channels - ch0 : h->llr_block;
            if(stages & MSK144_STAGE_SOFTBITS)
            {
                ev_begin(h);
                launch_softbits(blk, h->tpl, h->stream);
                ev_end(h, MSK144_T_SOFTBITS);
            }
            if(stages & MSK144_STAGE_INDEX)
            {
                ev_begin(h);
                launch_index(blk, h->stream);
                ev_end(h, MSK144_T_INDEX);
            }
            if(stages & MSK144_STAGE_LDPC)
            {
                ev_begin(h);
                launch_ldpc(blk, h->stream);
                ev_end(h, MSK144_T_LDPC);
            }
        }
    }
    if(stages & MSK144_STAGE_COLLECT)
    {
        DeviceStore out = cur;
        out.results = current_records(h);
        ev_begin(h);
        launch_collect(out, h->stream);
        ev_end(h, MSK144_T_COLLECT);
    }
    HIP_TRY(h, hipGetLastError());
    h->decoded = true;
    return MSK144_OK;
}

int msk144_decode(msk144_handle* h)
{
    return msk144_decode_stages(h, MSK144_STAGE_ALL);
}

int msk144_synchronize(msk144_handle* h)
{
    if(!h) return MSK144_EINVAL;
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    harvest_times(h);
    return MSK144_OK;
}

int msk144_result_count(msk144_handle* h, int32_t* n)
{
    if(!h || !n) return fail(h, MSK144_EINVAL, "null argument");
    if(!h->decoded) return fail(h, MSK144_ESTATE, "no decode has been run");
    int rc = msk144_synchronize(h);
    if(rc != MSK144_OK) return rc;
    HIP_TRY(h, hipMemcpy(n, h->st.result_count, sizeof(int32_t), hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_results(msk144_handle* h, msk144_result* out, int32_t cap, int32_t* n)
{
    if(!h || !n || (cap > 0 && !out)) return fail(h, MSK144_EINVAL, "null argument");
    int32_t total = 0;
    int rc = msk144_result_count(h, &total);
    if(rc != MSK144_OK) return rc;
    *n = total;
    int32_t avail = total < h->st.max_results ? total : h->st.max_results;
    int32_t ncopy = avail < cap ? avail : cap;
    if(ncopy > 0) HIP_TRY(h, hipMemcpy(out, current_records(h), sizeof(msk144_result) * ncopy, hipMemcpyDeviceToHost));
    if(total > h->st.max_results) return fail(h, MSK144_EOVERFLOW, "more decodes than max_results; list truncated");
    return MSK144_OK;
}

int msk144_results_device(msk144_handle* h, const msk144_result** d_records, const int32_t** d_count)
{
    if(!h || !d_records || !d_count) return fail(h, MSK144_EINVAL, "null argument");
    *d_records = current_records(h);
    *d_count = h->st.result_count;
    return MSK144_OK;
}

int msk144_set_channel_base(msk144_handle* h, int32_t base)
{
    if(!h) return MSK144_EINVAL;
    if(base < 0) return fail(h, MSK144_EINVAL, "channel base must be >= 0");
    h->st.channel_base = base;  // kernel argument by value: takes effect at the next decode
    return MSK144_OK;
}

int msk144_set_llr_retention(msk144_handle* h, int32_t retain)
{
    if(!h) return MSK144_EINVAL;
    if(retain && h->llr_block < h->st.channels)
        return fail(h, MSK144_ENOTRETAINED, "this handle decodes in blocks of fewer channels than it holds: an LLR row never outlives its block; create it with llr_block_channels = channels");
    h->retained = retain != 0;
    h->st.gate_early = h->retained ? 0 : 1;
    h->st.handover = h->st.gate_early;
    return MSK144_OK;
}

int msk144_llr_block_channels(const msk144_handle* h, int32_t* channels_per_block)
{
    if(!h || !channels_per_block) return MSK144_EINVAL;
    *channels_per_block = h->llr_block;
    return MSK144_OK;
}

int msk144_set_copy_handover(msk144_handle* h, int32_t enable)
{
    if(!h) return MSK144_EINVAL;
    if(enable && h->retained)
        return fail(h, MSK144_ENOTRETAINED, "every LLR row of this handle is retained (llr_block_channels = channels): every slot is computed on its own; copies are handed over only when no row outlives its block (blocked staging, or msk144_set_llr_retention(h, 0))");
    h->st.handover = enable ? 1 : 0;  // kernel argument by value: takes effect at the next decode
    return MSK144_OK;
}

int msk144_copy_handover(const msk144_handle* h, int32_t* enabled)
{
    if(!h || !enabled) return MSK144_EINVAL;
    *enabled = h->st.handover;
    return MSK144_OK;
}

int msk144_copy_count(msk144_handle* h, int64_t* slots)
{
    if(!h || !slots) return fail(h, MSK144_EINVAL, "null argument");
    if(!h->decoded) return fail(h, MSK144_ESTATE, "no decode has been run");
    int rc = msk144_synchronize(h);
    if(rc != MSK144_OK) return rc;
    std::vector<int32_t> per_channel(static_cast<size_t>(h->active));
    HIP_TRY(h, hipMemcpy(per_channel.data(), h->st.copy_count, sizeof(int32_t) * per_channel.size(), hipMemcpyDeviceToHost));
    int64_t total = 0;
    for(int32_t c : per_channel) total += c;
    *slots = total;
    return MSK144_OK;
}

int msk144_segment_power(msk144_handle* h, float* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    if(!h->have_window) return fail(h, MSK144_ESTATE, "no window submitted");
    int rc = msk144_synchronize(h);
    if(rc != MSK144_OK) return rc;
    HIP_TRY(h, hipMemcpy(out, h->st.seg_power, sizeof(float) * 8 * h->st.channels, hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_input_slot(msk144_handle* h, int32_t slot, void** host_windows, size_t* bytes)
{
    if(!h || !host_windows || slot < 0 || slot >= MSK144_SLOTS) return fail(h, MSK144_EINVAL, "bad argument");
    int rc = ensure_slots(h);
    if(rc != MSK144_OK) return rc;
    *host_windows = h->slots[slot].in;
    if(bytes) *bytes = input_bytes(h);
    return MSK144_OK;
}

int msk144_submit_slot(msk144_handle* h, int32_t slot)
{
    return msk144_submit_slot_n(h, slot, h ? h->st.channels : 0);
}

int msk144_submit_slot_n(msk144_handle* h, int32_t slot, int32_t n_channels)
{
    int rc = check_hop_slot(h, slot);
    if(rc != MSK144_OK) return rc;
    if(n_channels < 1 || n_channels > h->st.channels) return fail(h, MSK144_EINVAL, "n_channels must be 1..channels");
    if((rc = ensure_slots(h)) != MSK144_OK || (rc = begin_hop(h, slot, n_channels)) != MSK144_OK) return rc;
    rc = copy_windows_in(h, h->slots[slot].in);
    return rc == MSK144_OK ? run_frontend(h, h->d_input) : rc;
}

int msk144_hop_slot(msk144_handle* h, int32_t slot, void** hops, void** first_halves, int32_t** streams, uint8_t** is_first)
{
    if(!h || !hops || !first_halves || !streams || !is_first || slot < 0 || slot >= MSK144_SLOTS) return fail(h, MSK144_EINVAL, "bad argument");
    HIP_TRY(h, hipSetDevice(h->params.device));
    int rc = ensure_ring(h);
    if(rc != MSK144_OK) return rc;
    msk144_handle::Slot& sl = h->slots[slot];
    *hops = sl.hops;
    *first_halves = sl.first_halves;
    *streams = sl.streams;
    *is_first = sl.is_first;
    return MSK144_OK;
}

int msk144_push_hops(msk144_handle* h, int32_t slot, int32_t n)
{
    int rc = check_hop_slot(h, slot);
    if(rc != MSK144_OK) return rc;
    if(!h->ring_ready) return fail(h, MSK144_ESTATE, "msk144_push_hops before msk144_hop_slot");
    if(n < 1 || n > h->st.channels) return fail(h, MSK144_EINVAL, "n must be 1..channels");
    msk144_handle::Slot& sl = h->slots[slot];
    bool any_first = false;
    for(int32_t j = 0; j < n; j++)
    {
        if(sl.streams[j] < 0 || sl.streams[j] >= h->st.channels || (j > 0 && sl.streams[j] <= sl.streams[j - 1]))
            return fail(h, MSK144_EINVAL, "streams must be ascending stream numbers below channels");
        any_first = any_first || sl.is_first[j] != 0;
    }
    if((rc = begin_hop(h, slot, n)) != MSK144_OK) return rc;
    const size_t half = window_bytes(h) / 2;
    ev_begin(h);
    hipError_t e = hipMemcpyAsync(h->d_hops, sl.hops, half * n, hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess && any_first) e = hipMemcpyAsync(h->d_first, sl.first_halves, half * n, hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess) e = hipMemcpyAsync(h->d_streams, sl.streams, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess) e = hipMemcpyAsync(h->d_isfirst, sl.is_first, n, hipMemcpyHostToDevice, h->stream);
    ev_end(h, MSK144_T_H2D);
    if(e != hipSuccess) return fail(h, MSK144_EHIP, std::string("msk144_push_hops: ") + hipGetErrorString(e));
    launch_hop_ring(h->d_ring, h->d_hops, h->d_first, h->d_streams, h->d_isfirst, h->d_input, n, h->stream);
    return run_frontend(h, h->d_input);
}

int msk144_fetch_async(msk144_handle* h, int32_t slot)
{
    if(!h || slot < 0 || slot >= MSK144_SLOTS) return fail(h, MSK144_EINVAL, "bad argument");
    if(!h->decoded) return fail(h, MSK144_ESTATE, "no decode has been run");
    int rc = ensure_slots(h);
    if(rc != MSK144_OK) return rc;
    if(slot != h->cur_slot) return fail(h, MSK144_ESTATE, "fetch of a slot other than the one just decoded");
    msk144_handle::Slot& sl = h->slots[slot];
    if(sl.pending) return fail(h, MSK144_ESTATE, "slot already has a fetch in flight");
    HIP_TRY(h, hipSetDevice(h->params.device));
    long long guess = 2ll * h->last_total.load(std::memory_order_relaxed) + 256;
    if(guess < 1024) guess = 1024;
    if(guess > h->st.max_results) guess = h->st.max_results;
    sl.copied = static_cast<int32_t>(guess);
    ev_begin(h);
    hipError_t e = hipMemcpyAsync(sl.out_count, h->st.result_count, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if(e == hipSuccess) e = hipMemcpyAsync(sl.out_seg, h->st.seg_power, sizeof(float) * 8 * h->active, hipMemcpyDeviceToHost, h->stream);
    if(e == hipSuccess) e = hipMemcpyAsync(sl.out, sl.d_records, sizeof(msk144_result) * static_cast<size_t>(sl.copied), hipMemcpyDeviceToHost, h->stream);
    ev_end(h, MSK144_T_D2H);
    if(e == hipSuccess) e = hipEventRecord(sl.done, h->stream);
    if(e != hipSuccess) return fail(h, MSK144_EHIP, std::string("msk144_fetch_async: ") + hipGetErrorString(e));
    sl.pending = true;
    return MSK144_OK;
}

// May run on a second thread (the other slot being submitted meanwhile): touches only this slot, last_total and copy_stream.
int msk144_fetch_wait(msk144_handle* h, int32_t slot, const msk144_result** records, int32_t* n, const float** seg_power)
{
    if(!h || !records || !n || slot < 0 || slot >= MSK144_SLOTS) return MSK144_EINVAL;
    msk144_handle::Slot& sl = h->slots[slot];
    if(!h->slots_ready || !sl.pending) return MSK144_ESTATE;
    if(hipSetDevice(h->params.device) != hipSuccess || hipEventSynchronize(sl.done) != hipSuccess) return MSK144_EHIP;
    const int32_t total = *sl.out_count;
    const int32_t avail = total < h->st.max_results ? total : h->st.max_results;
    if(avail > sl.copied)
    {
        // the estimate was short: the slot's own device list is still intact (the other slot decodes into its own)
        hipError_t e = hipMemcpyAsync(sl.out + sl.copied, sl.d_records + sl.copied, sizeof(msk144_result) * static_cast<size_t>(avail - sl.copied), hipMemcpyDeviceToHost,
                                      h->copy_stream);
        if(e == hipSuccess) e = hipStreamSynchronize(h->copy_stream);
        if(e != hipSuccess) return MSK144_EHIP;
    }
    h->last_total.store(total, std::memory_order_relaxed);
    sl.pending = false;
    *records = sl.out;
    *n = avail;
    if(seg_power) *seg_power = sl.out_seg;
    return total > h->st.max_results ? MSK144_EOVERFLOW : MSK144_OK;
}

int msk144_dump_analytic(msk144_handle* h, int32_t channel, float* out)
{
    if(!h || !out || channel < 0 || channel >= h->st.channels) return fail(h, MSK144_EINVAL, "bad argument");
    int rc = msk144_synchronize(h);
    if(rc != MSK144_OK) return rc;
    HIP_TRY(h, hipMemcpy(out, h->st.analytic + static_cast<size_t>(channel) * kWindowSamples, sizeof(float2) * kWindowSamples, hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_dump_candidates(msk144_handle* h, int32_t channel, msk144_candidate* out)
{
    if(!h || !out || channel < 0 || channel >= h->st.channels) return fail(h, MSK144_EINVAL, "bad argument");
    if(!h->retained) return fail(h, MSK144_ENOTRETAINED, "LLR rows are not retained (blocked staging, or msk144_set_llr_retention(h, 0)); create the handle with llr_block_channels = channels for candidate dumps");
    if(!h->rows_valid) return fail(h, MSK144_ENOTRETAINED, "the last decode ran without LLR retention: its rows are incomplete; decode again now that retention is on");
    int rc = msk144_synchronize(h);
    if(rc != MSK144_OK) return rc;
    const DeviceStore& st = h->st;
    const size_t K = st.K;
    const size_t off = static_cast<size_t>(channel) * K;
    std::vector<uint32_t> pos(K), msg(K * 3);
    std::vector<float> xb(K), llr(K * kCodeBits);
    std::vector<int32_t> nbad(K);
    std::vector<uint8_t> flag(K), iter(K), nhard(K);
    HIP_TRY(h, hipMemcpy(pos.data(), st.pos + off, K * 4, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(xb.data(), st.xb + off, K * 4, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(nbad.data(), st.nbadsync + off, K * 4, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(llr.data(), st.llr + off * kCodeBits, K * kCodeBits * 4, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(flag.data(), st.dec_flag + off, K, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(iter.data(), st.dec_iter + off, K, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(nhard.data(), st.dec_nhard + off, K, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(msg.data(), st.dec_msg + off * 3, K * 12, hipMemcpyDeviceToHost));
    const int per_freq = st.D * kSlotsPerPattern;
    std::memset(out, 0, sizeof(msk144_candidate) * K);
    for(size_t k = 0; k < K; k++)
    {
        msk144_candidate& c = out[k];
        const int b = static_cast<int>(k) / per_freq;
        const int p = (static_cast<int>(k) - b * per_freq) / kSlotsPerPattern;
        c.block_idx = b;
        c.pattern_idx = p;
        c.pos = pos[k];
        c.f0 = h->freq_host[b];
        c.nbadsync = nbad[k];
        c.xb = xb[k];
        c.num_avg = kPatternNumAvg[p];
        std::memcpy(c.softbits_wo_sync, &llr[k * kCodeBits], sizeof(float) * kCodeBits);
        if(flag[k])
        {
            c.is_message_present = 1;
            c.ldpc_num_iterations = iter[k];
            c.ldpc_num_hard_errors = nhard[k];
            for(int i = 0; i < kMessageBits; i++) c.message[i] = static_cast<char>((msg[k * 3 + i / 32] >> (31 - (i % 32))) & 1u);
        }
    }
    return MSK144_OK;
}

int msk144_dump_indexes(msk144_handle* h, int32_t channel, int32_t* out, int32_t* n)
{
    if(!h || !out || !n || channel < 0 || channel >= h->st.channels) return fail(h, MSK144_EINVAL, "bad argument");
    int rc = msk144_synchronize(h);
    if(rc != MSK144_OK) return rc;
    HIP_TRY(h, hipMemcpy(n, h->st.n_idx + channel, sizeof(int32_t), hipMemcpyDeviceToHost));
    if(*n > 0) HIP_TRY(h, hipMemcpy(out, h->st.idx + static_cast<size_t>(channel) * h->st.K, sizeof(int32_t) * (*n), hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_load_candidates(msk144_handle* h, int32_t channel, const msk144_candidate* items)
{
    if(!h || !items || channel < 0 || channel >= h->st.channels) return fail(h, MSK144_EINVAL, "bad argument");
    if(!h->retained) return fail(h, MSK144_ENOTRETAINED, "a handle that does not retain its LLR rows cannot take loaded candidates; create the handle with llr_block_channels = channels");
    int rc = msk144_synchronize(h);
    if(rc != MSK144_OK) return rc;
    const DeviceStore& st = h->st;
    const size_t K = st.K;
    const size_t off = static_cast<size_t>(channel) * K;
    std::vector<uint32_t> pos(K);
    std::vector<float> xb(K), llr(K * kCodeBits);
    std::vector<int32_t> nbad(K);
    for(size_t k = 0; k < K; k++)
    {
        pos[k] = items[k].pos;
        xb[k] = items[k].xb;
        nbad[k] = items[k].nbadsync;
        std::memcpy(&llr[k * kCodeBits], items[k].softbits_wo_sync, sizeof(float) * kCodeBits);
    }
    HIP_TRY(h, hipMemcpy(st.pos + off, pos.data(), K * 4, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(st.xb + off, xb.data(), K * 4, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(st.nbadsync + off, nbad.data(), K * 4, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(st.llr + off * kCodeBits, llr.data(), K * kCodeBits * 4, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemsetAsync(st.dec_flag + off, 0, K, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MSK144_OK;
}

int msk144_clock_probe(msk144_handle* h, int32_t spin_us, float* shader_mhz)
{
    if(!h || !shader_mhz) return fail(h, MSK144_EINVAL, "null argument");
    if(spin_us < 1 || spin_us > 100000) return fail(h, MSK144_EINVAL, "spin_us must be 1..100000");
    HIP_TRY(h, hipSetDevice(h->params.device));
    if(!h->probe_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->probe_stream, hipStreamNonBlocking));
    if(!h->d_probe)
    {
        int rc = dev_alloc(h, h->mem, &h->d_probe, 2);
        if(rc != MSK144_OK) return rc;
    }
    launch_clock_probe(h->d_probe, static_cast<uint32_t>(spin_us) * 100u, h->probe_stream);
    HIP_TRY(h, hipGetLastError());
    uint64_t v[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(v, h->d_probe, sizeof(v), hipMemcpyDeviceToHost, h->probe_stream));
    HIP_TRY(h, hipStreamSynchronize(h->probe_stream));
    if(v[1] == 0) return fail(h, MSK144_EHIP, "clock probe: the 100 MHz counter did not advance");
    *shader_mhz = static_cast<float>(static_cast<double>(v[0]) / static_cast<double>(v[1]) * 100.0);
    return MSK144_OK;
}

int msk144_set_profiling(msk144_handle* h, int32_t enable)
{
    if(!h) return MSK144_EINVAL;
    int rc = msk144_synchronize(h);
    if(rc != MSK144_OK) return rc;
    h->profiling = enable != 0;
    return MSK144_OK;
}

int msk144_stage_times(msk144_handle* h, float* avg_ms, int32_t* samples, int32_t reset)
{
    if(!h || !avg_ms) return fail(h, MSK144_EINVAL, "null argument");
    int rc = msk144_synchronize(h);
    if(rc != MSK144_OK) return rc;
    for(int s = 0; s < MSK144_T_COUNT; s++) avg_ms[s] = h->t_cnt[s] ? static_cast<float>(h->t_sum[s] / h->t_cnt[s]) : 0.0f;
    if(samples)
        for(int s = 0; s < MSK144_T_COUNT; s++) samples[s] = h->t_cnt[s];
    if(reset)
    {
        for(int s = 0; s < MSK144_T_COUNT; s++)
        {
            h->t_sum[s] = 0.0;
            h->t_cnt[s] = 0;
        }
    }
    return MSK144_OK;
}

// ---- wideband channeliser ----

int msk144_set_wideband(msk144_handle* h, const msk144_wideband_params* wp)
{
    return msk144_set_wideband_ex(h, wp, nullptr, 0);
}

int msk144_set_wideband_ex(msk144_handle* h, const msk144_wideband_params* wp, const double* bank_taps, int32_t bank_num_taps)
{
    std::vector<double> h1;
    int rc = wb_validate(h, wp, bank_taps, bank_num_taps, h1);
    if(rc != MSK144_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if((rc = ensure_ring(h)) != MSK144_OK) return rc;
    wb_release(h);

    const bool bank = msk144wb::is_bank_rate(wp->rate_hz);
    const int64_t rate2 = msk144wb::stage2_rate(wp->rate_hz);  // the channeliser's input rate
    const msk144wb::RateRatio rr = msk144wb::rate_ratio(rate2), rin = msk144wb::rate_ratio(wp->rate_hz);
    const WbSlots sl = wb_slot_layout(wp, bank);
    const WbTables t = wb_tap_tables(wp, sl, rate2, rr.P, rr.Q);

    auto& w = h->wb;
    w.P = rr.P;
    w.Q = rr.Q;
    w.K = wp->taps_per_phase;
    w.L = wp->num_taps;
    w.hist = (w.L + w.Q - 1) / w.Q - 1;
    w.Pin = rin.P;
    w.Qin = rin.Q;
    w.bank = bank;
    w.raw_hist = bank ? static_cast<int>(h1.size()) - 1 : w.hist;
    w.K1 = static_cast<int>(h1.size()) / msk144wb::kBankBands;
    w.band_index.assign(sl.band_list.begin(), sl.band_list.end());
    w.stride = bank ? w.hist + static_cast<long long>(kWindowSamples) / w.Q * w.P : 0;
    w.slots = static_cast<int>(sl.slot_channel.size());
    w.format = wp->format;
    w.gain = wp->gain;
    w.gains.assign(static_cast<size_t>(wp->num_offsets), wp->gain);
    w.slot_channel = sl.slot_channel;
    if((rc = wb_allocate(h, sl, t, h1)) != MSK144_OK)
    {
        wb_release(h);
        return rc;
    }
    w.configured = true;
    return MSK144_OK;
}

int msk144_wideband_slot(msk144_handle* h, int32_t slot, void** buf, size_t* bytes)
{
    if(!h || !buf || !bytes || slot < 0 || slot >= MSK144_SLOTS) return fail(h, MSK144_EINVAL, "bad argument");
    if(!h->wb.configured) return fail(h, MSK144_ESTATE, "msk144_wideband_slot before msk144_set_wideband");
    *buf = h->wb.pinned[slot];
    *bytes = h->wb.slot_bytes;
    return MSK144_OK;
}

int msk144_push_wideband(msk144_handle* h, int32_t slot, int32_t first)
{
    int rc = check_hop_slot(h, slot);
    if(rc != MSK144_OK) return rc;
    auto& w = h->wb;
    if(!w.configured) return fail(h, MSK144_ESTATE, "msk144_push_wideband before msk144_set_wideband");
    if(!first && !w.started) return fail(h, MSK144_ESTATE, "a later wideband push before the first one");
    const int C = h->params.channels;
    if((rc = begin_hop(h, slot, C)) != MSK144_OK) return rc;
    msk144_handle::Slot& sl = h->slots[slot];
    const int M = first ? kWindowSamples : kHopSamples;
    if(first)
    {
        w.blanker_on = w.blanker_set;
        w.blanker = w.blanker_next;
        w.blanker_pushes = 0;
        w.blanker_samples = 0;
    }
    // a blanked stream is cs16 on the device, whatever the input format
    const int dev_format = w.blanker_on ? static_cast<int>(msk144wb::kCs16) : w.format;
    const size_t sb = static_cast<size_t>(msk144wb::sample_bytes(dev_format));
    const size_t hist_bytes = static_cast<size_t>(w.raw_hist) * sb;
    const int new_samples = M / w.Qin * w.Pin;
    const size_t new_bytes = static_cast<size_t>(new_samples) * sb;
    const int frames = M / w.Q * w.P;         // bank: frames of 32 input samples = the channeliser's input samples
    if(first)
    {
        w.m_next = 0;
        w.n_next = 0;
    }
    for(int j = 0; j < C; j++)
    {
        sl.streams[j] = j;
        sl.is_first[j] = first ? 1 : 0;
    }
    uint8_t* raw = w.blanker_on ? w.d_blanked : w.d_raw;
    ev_begin(h);
    hipError_t e = hipSuccess;
    // the filter history: the last raw_hist samples of the previous push (a push has >= 2592*P/Q samples, raw_hist < ceil(64*P/Q)
    // without the bank and 1024 with it, so the ranges do not overlap)
    if(!first) e = hipMemcpyAsync(raw, raw + static_cast<size_t>(w.last_first ? kWindowSamples : kHopSamples) / w.Qin * w.Pin * sb, hist_bytes, hipMemcpyDeviceToDevice, h->stream);
    // the bank's sub-band streams: the channeliser's history, the last hist frames of the previous push, likewise apart
    if(e == hipSuccess && !first && w.bank && w.hist > 0)
        e = hipMemcpy2DAsync(w.d_sub, w.stride * sizeof(float2), w.d_sub + w.last_frames, w.stride * sizeof(float2), w.hist * sizeof(float2), w.band_index.size(),
                             hipMemcpyDeviceToDevice, h->stream);
    if(w.blanker_on)
    {
        // the raw push to the staging buffer; the counters of a push start at 0, those of a stream (totals, carry) with its first push
        if(e == hipSuccess) e = hipMemcpyAsync(w.d_stage, w.pinned[slot], static_cast<size_t>(new_samples) * msk144wb::sample_bytes(w.format), hipMemcpyHostToDevice, h->stream);
        if(e == hipSuccess) e = hipMemsetAsync(w.d_blanker, 0, first ? sizeof(BlankerCounters) : offsetof(BlankerCounters, carry), h->stream);
    }
    else if(e == hipSuccess) e = hipMemcpyAsync(raw + hist_bytes, w.pinned[slot], new_bytes, hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess) e = hipMemcpyAsync(h->d_streams, sl.streams, sizeof(int32_t) * C, hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess) e = hipMemcpyAsync(h->d_isfirst, sl.is_first, C, hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess) e = hipMemsetAsync(w.d_clip, 0, sizeof(unsigned long long), h->stream);
    if(e == hipSuccess) e = hipMemsetAsync(w.d_levels, 0, sizeof(unsigned long long) * C, h->stream);
    if(w.agc && first)
    {
        // a stream restart: exponent 0 and no quiet pushes counted, so that the same stream pushed twice gives the same bytes
        if(e == hipSuccess) e = hipMemcpyAsync(w.d_scale, w.d_base_scale, sizeof(float) * w.slots, hipMemcpyDeviceToDevice, h->stream);
        if(e == hipSuccess) e = hipMemsetAsync(w.d_exp, 0, sizeof(int32_t) * C, h->stream);
        if(e == hipSuccess) e = hipMemsetAsync(w.d_quiet, 0, sizeof(int32_t) * C, h->stream);
    }
    ev_end(h, MSK144_T_H2D);
    if(e != hipSuccess) return fail(h, MSK144_EHIP, std::string("msk144_push_wideband: ") + hipGetErrorString(e));
    ev_begin(h);
    if(w.blanker_on)
    {
        launch_blanker(w.d_stage, w.format, reinterpret_cast<short2*>(raw + hist_bytes), new_samples, w.blanker, static_cast<int>(w.blanker_pushes & 1), w.d_blanker, h->stream);
        w.blanker_pushes++;
        w.blanker_samples += new_samples;
    }
    if(w.spectrum_bins) launch_spectrum(raw + hist_bytes, dev_format, new_samples, w.spectrum_bins, w.d_spec_window, w.d_spec_tw, w.d_spec_partials, w.d_spec_out, h->stream);
    w.spectrum_pushed = w.spectrum_bins != 0;
    w.spectrum_last_bins = w.spectrum_bins;
    const void* in = raw;
    int format = dev_format;
    WidebandBands bands;
    if(w.bank)
    {
        launch_bank(raw, dev_format, w.d_h1, w.d_bands, w.d_tw, w.d_sub, static_cast<int>(w.band_index.size()), w.K1, frames, w.stride, w.hist, first ? 1 : 0,
                    w.n_next, h->stream);
        in = w.d_sub;
        format = kSubbandFormat;
        bands = WidebandBands{w.d_wave_band, w.d_slot_channel, w.stride};
    }
    launch_channelise(in, format, w.d_G, w.d_branches, w.d_fmod, w.d_rot, reinterpret_cast<int8_t*>(h->d_first), reinterpret_cast<int8_t*>(h->d_hops), w.d_clip, w.slots,
                      w.P, w.Q, w.hist, M, first ? 1 : 0, w.m_next, w.d_scale, w.d_levels, h->stream, bands);
    if(w.agc)
        launch_agc_step(w.d_levels, w.bank ? w.d_slot_channel : nullptr, w.d_gains, w.d_exp, w.d_quiet, w.d_used_exp, w.d_scale, w.slots, M, w.agc_params, h->stream);
    if(w.pings)
    {
        if(w.ping_band)
            launch_pingband(reinterpret_cast<int8_t*>(h->d_first), reinterpret_cast<int8_t*>(h->d_hops), first ? 1 : 0, C, w.d_ping_band_taps, w.ping_band_shift,
                            first || w.ping_restart ? 1 : 0, w.d_ping_band_tails, w.d_ping_energies, h->stream);
        launch_pings(reinterpret_cast<int8_t*>(h->d_first), reinterpret_cast<int8_t*>(h->d_hops), first ? 1 : 0, C, w.d_gains, w.agc ? w.d_used_exp : nullptr, w.ping_params,
                     first || w.ping_restart ? 1 : 0, w.d_ping_state, w.d_ping_records, w.d_ping_energies, w.ping_band, h->stream);
        w.ping_restart = false;
    }
    w.ping_pushed = w.pings;
    if(w.waterfall)
        launch_waterfall(reinterpret_cast<int8_t*>(h->d_first), reinterpret_cast<int8_t*>(h->d_hops), first ? 1 : 0, C, w.d_wf_dft, w.d_wf_rows, w.d_wf_sums, h->stream);
    w.waterfall_pushed = w.waterfall;
    ev_end(h, MSK144_T_FRONTEND);
    HIP_TRY(h, hipGetLastError());
    w.push_gains = w.gains;
    w.push_agc = w.agc;
    w.m_next += M;
    w.n_next += frames;
    w.last_frames = frames;
    w.started = true;
    w.last_first = first != 0;
    launch_hop_ring(h->d_ring, h->d_hops, h->d_first, h->d_streams, h->d_isfirst, h->d_input, C, h->stream);
    if(w.capture)
    {
        // behind the ring kernel: the ring now holds the push's newest hop, number m_next / 2592 - 1, and the one before it
        ev_begin(h);
        launch_capture(h->d_ring, w.pings ? w.d_ping_records : nullptr, w.d_cap_listed, w.d_cap_state, C, first ? 1 : 0, first || w.capture_restart ? 1 : 0, w.capture_params,
                       w.m_next / kHopSamples - 1, w.d_cap_header, w.d_cap_units, w.d_cap_data, h->stream);
        ev_end(h, MSK144_T_FRONTEND);
        w.capture_restart = false;
        HIP_TRY(h, hipGetLastError());
    }
    w.capture_pushed = w.capture;
    return run_frontend(h, h->d_input);
}

int msk144_dump_wideband_hop(msk144_handle* h, int32_t channel, int8_t* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    if(channel < 0 || channel >= h->params.channels) return fail(h, MSK144_EINVAL, "channel out of range");
    if(!h->wb.started) return fail(h, MSK144_ESTATE, "no wideband push has been made");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t half = 2 * static_cast<size_t>(kHopSamples);
    const uint8_t* first = h->d_first + half * channel;
    const uint8_t* hop = h->d_hops + half * channel;
    if(h->wb.last_first)
    {
        HIP_TRY(h, hipMemcpy(out, first, half, hipMemcpyDeviceToHost));
        out += half;
    }
    HIP_TRY(h, hipMemcpy(out, hop, half, hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_dump_wideband_band(msk144_handle* h, int32_t band, float* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(!w.started) return fail(h, MSK144_ESTATE, "no wideband push has been made");
    if(!w.bank) return fail(h, MSK144_ESTATE, "the wideband configuration has no bank (rate <= 6144000 Hz)");
    if(band < -msk144wb::kBankBands / 2 || band > msk144wb::kBankBands / 2) return fail(h, MSK144_EINVAL, "band out of range (-32..32)");
    size_t j = 0;
    while(j < w.band_index.size() && w.band_index[j] != (band & (msk144wb::kBankBands - 1))) j++;
    if(j == w.band_index.size()) return fail(h, MSK144_EINVAL, "no channel lies in band " + std::to_string(band));
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out, w.d_sub + static_cast<long long>(j) * w.stride + w.hist, sizeof(float2) * w.last_frames, hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_wideband_clip_count(msk144_handle* h, int64_t* clipped)
{
    if(!h || !clipped) return fail(h, MSK144_EINVAL, "null argument");
    if(!h->wb.configured) return fail(h, MSK144_ESTATE, "no wideband configuration");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    unsigned long long v = 0;
    HIP_TRY(h, hipMemcpy(&v, h->wb.d_clip, sizeof(v), hipMemcpyDeviceToHost));
    *clipped = static_cast<int64_t>(v);
    return MSK144_OK;
}

int msk144_set_wideband_gains(msk144_handle* h, const float* gains)
{
    int rc = wb_quiesce(h, "msk144_set_wideband_gains");
    if(rc != MSK144_OK) return rc;
    auto& w = h->wb;
    const int32_t top = w.agc ? w.agc_params.max_exp : 0;
    if(gains)
        for(size_t c = 0; c < w.gains.size(); c++)
            if(!msk144wb::gain_ok(gains[c], top))
                return fail(h, MSK144_EINVAL, "gain of channel " + std::to_string(c) + " must be positive with 128 x gain x 2^max_exp finite in f32");
    if(!gains && !msk144wb::gain_ok(w.gain, top))
        return fail(h, MSK144_EINVAL, "the configured gain cannot be restored while the AGC is on: 128 x gain x 2^max_exp is not finite in f32");
    if(gains) w.gains.assign(gains, gains + w.gains.size());
    else w.gains.assign(w.gains.size(), w.gain);
    return wb_upload_gains(h);
}

int msk144_set_wideband_agc(msk144_handle* h, const msk144_wideband_agc* p)
{
    int rc = wb_quiesce(h, "msk144_set_wideband_agc");
    if(rc != MSK144_OK) return rc;
    auto& w = h->wb;
    if(p)
    {
        const msk144wb::AgcParams ap{p->lo_sq, p->hi_sq, p->clip_ppm, p->hold, p->min_exp, p->max_exp};
        const std::string why = msk144wb::check_agc(ap);
        if(!why.empty()) return fail(h, MSK144_EINVAL, why);
        for(size_t c = 0; c < w.gains.size(); c++)
            if(!msk144wb::gain_ok(w.gains[c], ap.max_exp))
                return fail(h, MSK144_EINVAL, "128 x gain x 2^max_exp of channel " + std::to_string(c) + " is not finite in f32");
        w.agc_params = ap;
    }
    w.agc = p != nullptr;
    return wb_upload_gains(h);  // exponent 0, nothing counted: the AGC starts, or the base gains hold again
}

int msk144_set_wideband_blanker(msk144_handle* h, const msk144_wideband_blanker* p)
{
    int rc = wb_quiesce(h, "msk144_set_wideband_blanker");
    if(rc != MSK144_OK) return rc;
    auto& w = h->wb;
    if(!p)
    {
        w.blanker_set = false;
        return MSK144_OK;
    }
    const msk144wb::BlankerParams bp{p->threshold_q4, p->pre, p->post};
    const std::string why = msk144wb::check_blanker(bp);
    if(!why.empty()) return fail(h, MSK144_EINVAL, why);
    // the buffers of a blanked stream, once per configuration and never in a push: the raw staging, and history + one push as cs16
    const size_t cs16 = static_cast<size_t>(msk144wb::sample_bytes(msk144wb::kCs16));
    if(!w.d_stage && (rc = dev_alloc(h, w.mem, &w.d_stage, w.slot_bytes)) != MSK144_OK) return rc;
    if(!w.d_blanked && (rc = dev_alloc(h, w.mem, &w.d_blanked, (static_cast<size_t>(w.raw_hist) + static_cast<size_t>(kWindowSamples) / w.Qin * w.Pin) * cs16)) != MSK144_OK) return rc;
    if(!w.d_blanker && (rc = dev_alloc(h, w.mem, &w.d_blanker, 1)) != MSK144_OK) return rc;
    w.blanker_next = bp;
    w.blanker_set = true;
    return MSK144_OK;
}

int msk144_wideband_blanker_stats(msk144_handle* h, msk144_wideband_blanker_counts* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    auto& w = h->wb;
    if(!w.configured) return fail(h, MSK144_EINVAL, "msk144_wideband_blanker_stats needs wideband mode (msk144_set_wideband)");
    if(!w.started || !w.blanker_on) return fail(h, MSK144_ESTATE, w.started ? "the running wideband stream has no blanker" : "no wideband push has been made");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    BlankerCounters c;
    HIP_TRY(h, hipMemcpy(&c, w.d_blanker, sizeof(c), hipMemcpyDeviceToHost));
    out->samples = (w.last_first ? kWindowSamples : kHopSamples) / w.Qin * w.Pin;
    out->sum_power = static_cast<int64_t>(c.sum_power);
    out->threshold = static_cast<int64_t>(msk144wb::blanker_threshold(c.sum_power, static_cast<uint64_t>(out->samples), static_cast<uint32_t>(w.blanker.threshold_q4)));
    out->hits = static_cast<int64_t>(c.hits);
    out->blanked = static_cast<int64_t>(c.blanked);
    out->carry_out = static_cast<int64_t>(c.carry[(w.blanker_pushes - 1) & 1]);
    out->total_samples = w.blanker_samples;
    out->total_hits = static_cast<int64_t>(c.total_hits);
    out->total_blanked = static_cast<int64_t>(c.total_blanked);
    return MSK144_OK;
}

int msk144_dump_wideband_blanked(msk144_handle* h, int16_t* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(!w.started || !w.blanker_on) return fail(h, MSK144_ESTATE, w.started ? "the running wideband stream has no blanker" : "no wideband push has been made");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t cs16 = static_cast<size_t>(msk144wb::sample_bytes(msk144wb::kCs16));
    const size_t n = static_cast<size_t>(w.last_first ? kWindowSamples : kHopSamples) / w.Qin * w.Pin;
    HIP_TRY(h, hipMemcpy(out, w.d_blanked + static_cast<size_t>(w.raw_hist) * cs16, n * cs16, hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_set_wideband_spectrum(msk144_handle* h, const msk144_wideband_spectrum_params* p)
{
    int rc = wb_quiesce(h, "msk144_set_wideband_spectrum");
    if(rc != MSK144_OK) return rc;
    auto& w = h->wb;
    if(!p)
    {
        w.spectrum_bins = 0;
        return MSK144_OK;
    }
    const int B = p->bins;
    const std::string why = msk144wb::check_spectrum(B, p->window, static_cast<int64_t>(kHopSamples) / w.Qin * w.Pin);
    if(!why.empty()) return fail(h, MSK144_EINVAL, why);
    // never in a push
    constexpr size_t kMax = msk144wb::kSpectrumMaxBins;
    if(!w.d_spec_window && (rc = dev_alloc(h, w.mem, &w.d_spec_window, kMax)) != MSK144_OK) return rc;
    if(!w.d_spec_tw && (rc = dev_alloc(h, w.mem, &w.d_spec_tw, kMax)) != MSK144_OK) return rc;
    if(B > w.spectrum_rows_bins)
    {
        // a larger B than any before: new rows (the old ones stay with the configuration's owner until it is released)
        if((rc = dev_alloc(h, w.mem, &w.d_spec_partials, static_cast<size_t>(B) * kSpectrumMaxGroups)) != MSK144_OK) return rc;
        w.spectrum_rows_bins = B;
    }
    if(!w.d_spec_out && (rc = dev_alloc(h, w.mem, &w.d_spec_out, kMax)) != MSK144_OK) return rc;
    // window and twiddles: formed in double, stored f32
    const std::vector<double> hann = p->window ? std::vector<double>() : msk144wb::spectrum_window(B);
    const double* win = p->window ? p->window : hann.data();
    const std::vector<float> wf(win, win + B);
    const std::vector<float2> tw = unit_circle(B, -1.0);
    HIP_TRY(h, hipMemcpy(w.d_spec_window, wf.data(), sizeof(float) * wf.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(w.d_spec_tw, tw.data(), sizeof(float2) * tw.size(), hipMemcpyHostToDevice));
    w.spectrum_bins = B;
    return MSK144_OK;
}

int msk144_wideband_spectrum(msk144_handle* h, double* power, int64_t* segments)
{
    if(!h || !power || !segments) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(!w.configured) return fail(h, MSK144_EINVAL, "msk144_wideband_spectrum needs wideband mode (msk144_set_wideband)");
    if(!w.started || !w.spectrum_pushed) return fail(h, MSK144_ESTATE, w.started ? "the last wideband push was made without a spectrum" : "no wideband push has been made");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(power, w.d_spec_out, sizeof(double) * static_cast<size_t>(w.spectrum_last_bins), hipMemcpyDeviceToHost));
    *segments = static_cast<int64_t>(w.last_first ? kWindowSamples : kHopSamples) / w.Qin * w.Pin / w.spectrum_last_bins;
    return MSK144_OK;
}

int msk144_set_wideband_pings(msk144_handle* h, const msk144_wideband_pings_params* p)
{
    int rc = wb_quiesce(h, "msk144_set_wideband_pings");
    if(rc != MSK144_OK) return rc;
    auto& w = h->wb;
    if(!p)
    {
        w.pings = false;
        return MSK144_OK;
    }
    const msk144wb::PingParams pp{p->ratio_q4, p->memory, p->min_ref};
    const std::string why = msk144wb::check_pings(pp);
    if(!why.empty()) return fail(h, MSK144_EINVAL, why);
    // never in a push
    const size_t C = w.gains.size();
    if(!w.d_ping_state && (rc = dev_alloc(h, w.mem, &w.d_ping_state, C)) != MSK144_OK) return rc;
    if(!w.d_ping_records && (rc = dev_alloc(h, w.mem, &w.d_ping_records, C)) != MSK144_OK) return rc;
    if(!w.d_ping_energies && (rc = dev_alloc(h, w.mem, &w.d_ping_energies, C * msk144wb::kPingMaxBlocks)) != MSK144_OK) return rc;
    HIP_TRY(h, hipMemset(w.d_ping_state, 0, sizeof(msk144wb::PingHistory) * C));
    w.ping_params = pp;
    w.pings = true;
    w.ping_restart = true;
    return MSK144_OK;
}

int msk144_set_wideband_ping_band(msk144_handle* h, const msk144_wideband_ping_band_params* p)
{
    int rc = wb_quiesce(h, "msk144_set_wideband_ping_band");
    if(rc != MSK144_OK) return rc;
    auto& w = h->wb;
    static_assert(sizeof(msk144_wideband_ping_band_params) == sizeof(msk144wb::PingBandParams) && offsetof(msk144_wideband_ping_band_params, shift) == offsetof(msk144wb::PingBandParams, shift),
                  "msk144wb::PingBandParams is msk144_wideband_ping_band_params");
    if(p)
    {
        msk144wb::PingBandParams bp;
        std::memcpy(&bp, p, sizeof(bp));
        const std::string why = msk144wb::check_ping_band(bp);
        if(!why.empty()) return fail(h, MSK144_EINVAL, why);
        // never in a push; the energies are the detector's, whichever `set` comes first
        const size_t C = w.gains.size();
        if(!w.d_ping_band_taps && (rc = dev_alloc(h, w.mem, &w.d_ping_band_taps, sizeof(bp.taps))) != MSK144_OK) return rc;
        if(!w.d_ping_band_tails && (rc = dev_alloc(h, w.mem, &w.d_ping_band_tails, C * 2 * msk144wb::kPingBandTaps)) != MSK144_OK) return rc;
        if(!w.d_ping_energies && (rc = dev_alloc(h, w.mem, &w.d_ping_energies, C * msk144wb::kPingMaxBlocks)) != MSK144_OK) return rc;
        HIP_TRY(h, hipMemcpy(w.d_ping_band_taps, bp.taps, sizeof(bp.taps), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemset(w.d_ping_band_tails, 0, C * 2 * msk144wb::kPingBandTaps));
        w.ping_band_shift = bp.shift;
    }
    w.ping_band = p != nullptr;
    // E and Ef do not share a history: the next push with the detector on restarts it, and finds the tail all zero
    w.ping_restart = true;
    return MSK144_OK;
}

int msk144_wideband_pings(msk144_handle* h, msk144_wideband_ping* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    const int rc = wb_ping_ready(h, "msk144_wideband_pings");
    if(rc != MSK144_OK) return rc;
    static_assert(sizeof(msk144_wideband_ping) == sizeof(msk144wb::PingRecord) && offsetof(msk144_wideband_ping, peak_block) == offsetof(msk144wb::PingRecord, peak_block),
                  "the kernel writes msk144_wideband_ping");
    HIP_TRY(h, hipMemcpy(out, h->wb.d_ping_records, sizeof(msk144_wideband_ping) * h->wb.gains.size(), hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_wideband_ping_blocks(msk144_handle* h, int32_t channel, int32_t* energies, int32_t* n)
{
    if(!h || !energies || !n) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(w.configured && (channel < -1 || channel >= h->params.channels)) return fail(h, MSK144_EINVAL, "channel out of range");
    const int rc = wb_ping_ready(h, "msk144_wideband_ping_blocks");
    if(rc != MSK144_OK) return rc;
    const size_t row = msk144wb::kPingMaxBlocks;
    if(channel < 0) HIP_TRY(h, hipMemcpy(energies, w.d_ping_energies, sizeof(int32_t) * row * w.gains.size(), hipMemcpyDeviceToHost));
    else HIP_TRY(h, hipMemcpy(energies, w.d_ping_energies + row * static_cast<size_t>(channel), sizeof(int32_t) * row, hipMemcpyDeviceToHost));
    *n = (w.last_first ? kWindowSamples : kHopSamples) / msk144wb::kPingBlock;
    return MSK144_OK;
}

int msk144_set_wideband_waterfall(msk144_handle* h, const msk144_wideband_waterfall_params* p)
{
    int rc = wb_quiesce(h, "msk144_set_wideband_waterfall");
    if(rc != MSK144_OK) return rc;
    auto& w = h->wb;
    if(!p)
    {
        w.waterfall = false;
        return MSK144_OK;
    }
    const std::string why = msk144wb::check_waterfall(p->window);
    if(!why.empty()) return fail(h, MSK144_EINVAL, why);
    // never in a push
    constexpr int B = msk144wb::kWaterfallBins;
    const size_t C = w.gains.size();
    if(!w.d_wf_dft && (rc = dev_alloc(h, w.mem, &w.d_wf_dft, kWaterfallDftSize)) != MSK144_OK) return rc;
    if(!w.d_wf_rows && (rc = dev_alloc(h, w.mem, &w.d_wf_rows, C * msk144wb::kWaterfallRows * B)) != MSK144_OK) return rc;
    if(!w.d_wf_sums && (rc = dev_alloc(h, w.mem, &w.d_wf_sums, C * B)) != MSK144_OK) return rc;
    // the matrix: the window rounded to f32, times the twiddle in double, stored f32; slot j = 32 t + c is bin (j - 48) mod 96
    const std::vector<double> hann = p->window ? std::vector<double>() : msk144wb::waterfall_window();
    const double* win = p->window ? p->window : hann.data();
    std::vector<float2> dft(kWaterfallDftSize);
    for(int j = 0; j < B; j++)
        for(int i = 0; i < B; i++)
        {
            const double wi = static_cast<double>(static_cast<float>(win[i]));
            const double a = -2.0 * M_PI * static_cast<double>((i * ((j + B / 2) % B)) % B) / B;
            dft[(static_cast<size_t>(j / 32) * B + static_cast<size_t>(i)) * 32 + static_cast<size_t>(j % 32)] =
                make_float2(static_cast<float>(wi * std::cos(a)), static_cast<float>(wi * std::sin(a)));
        }
    HIP_TRY(h, hipMemcpy(w.d_wf_dft, dft.data(), sizeof(float2) * dft.size(), hipMemcpyHostToDevice));
    w.waterfall = true;
    return MSK144_OK;
}

int msk144_wideband_waterfall(msk144_handle* h, int32_t channel, float* rows, int32_t* n)
{
    if(!h || !rows || !n) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(w.configured && (channel < -1 || channel >= h->params.channels)) return fail(h, MSK144_EINVAL, "channel out of range");
    const int rc = wb_waterfall_ready(h, "msk144_wideband_waterfall");
    if(rc != MSK144_OK) return rc;
    constexpr size_t B = msk144wb::kWaterfallBins, R = msk144wb::kWaterfallRows;
    const size_t nb = static_cast<size_t>(w.last_first ? kWindowSamples : kHopSamples) / B;
    const size_t count = channel < 0 ? w.gains.size() : 1;
    // the device holds the rows of the push's blocks; what lies past them (an earlier first push's) is not part of this push
    if(nb == R) HIP_TRY(h, hipMemcpy(rows, w.d_wf_rows + (channel < 0 ? 0 : R * B * static_cast<size_t>(channel)), sizeof(float) * R * B * count, hipMemcpyDeviceToHost));
    else
    {
        HIP_TRY(h, hipMemcpy2D(rows, sizeof(float) * R * B, w.d_wf_rows + (channel < 0 ? 0 : R * B * static_cast<size_t>(channel)), sizeof(float) * R * B, sizeof(float) * nb * B, count,
                               hipMemcpyDeviceToHost));
        for(size_t c = 0; c < count; c++) std::fill(rows + (c * R + nb) * B, rows + (c + 1) * R * B, 0.0f);
    }
    *n = static_cast<int32_t>(nb);
    return MSK144_OK;
}

int msk144_wideband_waterfall_sums(msk144_handle* h, double* sums)
{
    if(!h || !sums) return fail(h, MSK144_EINVAL, "null argument");
    const int rc = wb_waterfall_ready(h, "msk144_wideband_waterfall_sums");
    if(rc != MSK144_OK) return rc;
    HIP_TRY(h, hipMemcpy(sums, h->wb.d_wf_sums, sizeof(double) * msk144wb::kWaterfallBins * h->wb.gains.size(), hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_set_wideband_capture(msk144_handle* h, const msk144_wideband_capture_params* p)
{
    int rc = wb_quiesce(h, "msk144_set_wideband_capture");
    if(rc != MSK144_OK) return rc;
    auto& w = h->wb;
    if(!p)
    {
        w.capture = w.capture_pushed = false;
        return MSK144_OK;
    }
    static_assert(sizeof(p->listed) / sizeof(p->listed[0]) == msk144wb::kCaptureMaxListed, "the list holds 16 channels");
    const msk144wb::CaptureParams cp{p->pre, p->post, p->max_units};
    const size_t C = w.gains.size();
    const std::string why = msk144wb::check_capture(cp, p->listed, p->num_listed, static_cast<int>(C));
    if(!why.empty()) return fail(h, MSK144_EINVAL, why);
    // An accepted `set` ends the last push's units: the read entry answers MSK144_ESTATE until the next push made with capture on.
    // So it never meets a count above the caller's max_units, nor rows that no push has written.
    w.capture = w.capture_pushed = false;
    // never in a push
    if(!w.d_cap_listed && (rc = dev_alloc(h, w.mem, &w.d_cap_listed, C)) != MSK144_OK) return rc;
    if(!w.d_cap_state && (rc = dev_alloc(h, w.mem, &w.d_cap_state, C)) != MSK144_OK) return rc;
    if(!w.d_cap_header && (rc = dev_alloc(h, w.mem, &w.d_cap_header, 1)) != MSK144_OK) return rc;
    if(cp.max_units > w.capture_rows)
    {
        // more units than any set before: the old rows, which nothing reads any more, are freed and larger ones take their place
        // (wb_quiesce has waited for the kernels that wrote them).  If that fails capture stays off, with no rows.
        w.capture_rows = 0;
        dev_free(w.mem, &w.d_cap_units);
        dev_free(w.mem, &w.d_cap_data);
        if((rc = dev_alloc(h, w.mem, &w.d_cap_units, static_cast<size_t>(cp.max_units))) != MSK144_OK) return rc;
        if((rc = dev_alloc(h, w.mem, &w.d_cap_data, static_cast<size_t>(cp.max_units) * msk144wb::kCaptureUnitBytes)) != MSK144_OK) return rc;
        w.capture_rows = cp.max_units;
    }
    std::vector<uint8_t> listed(C, 0);
    for(int i = 0; i < p->num_listed; i++) listed[static_cast<size_t>(p->listed[i])] = 1;
    HIP_TRY(h, hipMemcpy(w.d_cap_listed, listed.data(), C, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemset(w.d_cap_state, 0, sizeof(msk144wb::CaptureState) * C));
    w.capture_params = cp;
    w.capture = true;
    w.capture_restart = true;
    return MSK144_OK;
}

int msk144_wideband_capture(msk144_handle* h, msk144_wideband_capture_unit* units, int8_t* data, int32_t* count, int32_t* total)
{
    if(!h || !units || !data || !count || !total) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(!w.configured) return fail(h, MSK144_EINVAL, "msk144_wideband_capture needs wideband mode (msk144_set_wideband)");
    if(!w.started || !w.capture_pushed) return fail(h, MSK144_ESTATE, w.started ? "no wideband push has been made with capture on since it was last set" : "no wideband push has been made");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    static_assert(sizeof(msk144_wideband_capture_unit) == sizeof(msk144wb::CaptureUnit) && offsetof(msk144_wideband_capture_unit, hop) == offsetof(msk144wb::CaptureUnit, hop),
                  "the kernel writes msk144_wideband_capture_unit");
    msk144wb::CaptureHeader head{};
    HIP_TRY(h, hipMemcpy(&head, w.d_cap_header, sizeof(head), hipMemcpyDeviceToHost));
    // the push that left the header was made with capture_params (`set` ends the units of the push before it)
    if(head.count < 0 || head.count > w.capture_params.max_units || head.count > w.capture_rows) return fail(h, MSK144_EHIP, "msk144_wideband_capture: the device left a header out of range");
    // a quiet band costs the header alone
    if(head.count)
    {
        HIP_TRY(h, hipMemcpy(units, w.d_cap_units, sizeof(msk144wb::CaptureUnit) * static_cast<size_t>(head.count), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(data, w.d_cap_data, static_cast<size_t>(msk144wb::kCaptureUnitBytes) * static_cast<size_t>(head.count), hipMemcpyDeviceToHost));
    }
    *count = head.count;
    *total = head.total;
    return MSK144_OK;
}

int msk144_wideband_levels(msk144_handle* h, msk144_wideband_level* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    auto& w = h->wb;
    if(!w.configured) return fail(h, MSK144_EINVAL, "msk144_wideband_levels needs wideband mode (msk144_set_wideband)");
    if(!w.started) return fail(h, MSK144_ESTATE, "no wideband push has been made");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t C = w.gains.size();
    std::vector<unsigned long long> words(C);
    std::vector<int32_t> exps(C, 0);
    HIP_TRY(h, hipMemcpy(words.data(), w.d_levels, sizeof(unsigned long long) * C, hipMemcpyDeviceToHost));
    if(w.push_agc) HIP_TRY(h, hipMemcpy(exps.data(), w.d_used_exp, sizeof(int32_t) * C, hipMemcpyDeviceToHost));
    for(size_t c = 0; c < C; c++)
    {
        out[c].samples = w.last_first ? kWindowSamples : kHopSamples;
        out[c].sum_sq = msk144wb::level_sum_sq(words[c]);
        out[c].clipped = msk144wb::level_clipped(words[c]);
        out[c].gain = ldexpf(w.push_gains[c], exps[c]);
        out[c].exponent = exps[c];
    }
    return MSK144_OK;
}

}  // extern "C"
