// The handle behind the C ABI of libmsk144hip.so, and what its host files share: msk144_api.cpp (handle lifetime, the narrowband
// entries, the decode, and push_stream_hops, the one push behind msk144_push_hops and msk144_push_rate_hops),
// msk144_wideband_api.cpp (every msk144_*wideband* entry), msk144_input_rate_api.cpp (the resampler in front of the hop ring),
// msk144_stream_pings_api.cpp (levels and pings of the audio hops) and msk144_stream_gate_api.cpp (the gate on those pings); the
// last three each give the push one step.  Host code only: nothing here launches a kernel.
#pragma once

#include "../../include/msk144hip.h"

#include "input_rate.h"
#include "msk144_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <string>
#include <vector>

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

// Channel slots: without the bank slot c is channel c; with it, the channels of each occupied band (k mod 64, ascending) one after
// another, each band's group padded to whole waves, at the residual offset f_c - k Fs/64
struct WbSlots
{
    std::vector<int32_t> slot_channel;   // the channel of slot c; -1: padding
    std::vector<long long> slot_offset;  // its offset at the channeliser's rate
    std::vector<int32_t> wave_band;      // bank: the sub-band stream of each wave of 32 slots
    std::vector<int32_t> band_list;      // bank: the occupied band k mod 64 of stream j
};

// The shape of one push: 5184 output samples per channel for a first push, 2592 for a later one
struct WbPush
{
    bool first = false;
    int M = 0;        // output samples per channel
    int samples = 0;  // input samples: M Pin/Qin
    int frames = 0;   // the channeliser's input samples, M P/Q: with the bank, its frames of 32 input samples
};

// The wideband configuration of a handle (msk144_set_wideband): one block per option.  In every block `on` is what the next push
// does (set by the option's msk144_set_wideband_* entry), `pushed` whether the last push left the option's results (what its read
// entries test, wb_read_ready; set by the push), `restart` that the next push with the option on is its first since `set`; d_* are
// device buffers, allocated by `set` once per configuration (wb_ensure) and never in a push.  The exceptions are written at their
// block: bank.on is the rate's, no option; blanker; spectrum.pushed; capture.pushed.  Value-initialised is "not configured, all off".
struct Wideband
{
    Buffers mem;
    bool configured = false, started = false;  // started: a first push has been made since the configuration
    int channels = 0;      // the handle's
    WbPush last;           // the last push
    WbSlots layout;
    // the channeliser: Fs = 12000 P/Q in lowest terms at its input (Q = 1: decimation by D = P), 12000 Pin/Qin at the handle's
    struct Core
    {
        int P = 0, Q = 0, Pin = 0, Qin = 0, format = 0;
        int hist = 0, raw_hist = 0;  // samples kept between pushes: the channeliser's ceil(L/Q) - 1, the raw input's (the same without the bank)
        long long m_next = 0;        // output sample index of the next push
        size_t slot_bytes = 0;       // pinned bytes per slot: 5184 Pin/Qin samples
        uint8_t* pinned[MSK144_SLOTS] = {};
        uint8_t* d_raw = nullptr;    // history samples + the samples of one push, raw format
        uint8_t* d_in = nullptr;     // the running stream's input and its format there: d_raw in `format`, or d_blanked in cs16.  Derived
        int in_format = 0;           // from blanker.pushed alone, where a first push latches that (msk144_push_wideband); nothing else writes them
        float2* d_G = nullptr;       // one block per branch (WidebandBranch); Q = 1: the one block [ceil(slots/32)][D][K][32]
        msk144::WidebandBranch* d_branches = nullptr;  // [Q]
        int32_t* d_fmod = nullptr;
        float2* d_rot = nullptr;     // [12000]
        unsigned long long* d_clip = nullptr;
    } core;
    // two-stage bank (rates above 6.144 Msps): the channeliser runs at Fs/32 on the sub-band streams, one per layout.band_list
    struct Bank
    {
        bool on = false;
        int K1 = 0;
        long long stride = 0;  // float2 per sub-band stream: hist + 5184 P/Q frames
        long long n_next = 0;  // bank frame index of the next push
        float* d_h1 = nullptr;
        int32_t* d_bands = nullptr;
        float2* d_tw = nullptr;   // [64]
        float2* d_sub = nullptr;  // [bands][stride]
        int32_t* d_wave_band = nullptr;
        int32_t* d_slot_channel = nullptr;
    } bank;
    // per-channel levels (taken at every push), gains and the stepped AGC (msk144_set_wideband_agc), whose on / pushed these are
    struct Agc
    {
        bool on = false, pushed = false;
        msk144wb::AgcParams params;
        float gain = 0.0f;                       // the configured default, which msk144_set_wideband_gains(h, NULL) restores
        std::vector<float> gains, push_gains;    // base gain of every channel: of the next push, of the last one
        unsigned long long* d_levels = nullptr;  // [channels] msk144wb::pack_level of the last push
        float* d_scale = nullptr;                // [slots] what the next push is quantised with: 128 x gain x 2^exponent
        float* d_base_scale = nullptr;           // [slots] the same at exponent 0
        float* d_gains = nullptr;                // [channels]
        int32_t* d_exp = nullptr;                // [channels] AGC exponent of the next push
        int32_t* d_quiet = nullptr;              // [channels] pushes in a row below the window
        int32_t* d_used_exp = nullptr;           // [channels] AGC exponent of the last push
    } agc;
    // impulse-noise blanker (msk144_set_wideband_blanker).  Two-phase: on / next are what is set; a first push latches them into
    // pushed / params, the running stream's.  A blanked stream is cs16 in d_blanked (history + one push, as d_raw), made from d_stage
    struct Blanker
    {
        bool on = false, pushed = false;
        msk144wb::BlankerParams next, params;
        uint8_t *d_stage = nullptr, *d_blanked = nullptr;
        msk144::BlankerCounters* d_counters = nullptr;
        long long pushes = 0;   // of the running stream: its parity picks the carry word
        long long samples = 0;  // input samples since the first push
    } blanker;
    // power spectrum of the input stream (msk144_set_wideband_spectrum): tables and result for the largest B, allocated once
    struct Spectrum
    {
        int bins = 0;       // B of the next push; on: bins != 0
        int pushed = 0;     // B of the spectrum the last push left; 0: none
        int rows_bins = 0;  // the largest B set so far, which the partial sums hold
        float* d_window = nullptr;     // [B]
        float2* d_tw = nullptr;        // [B] e^{-j2pi m/B}
        double* d_partials = nullptr;  // [kSpectrumMaxGroups][rows_bins]
        double* d_out = nullptr;       // [B] ascending frequency
    } spectrum;
    // ping detection (msk144_set_wideband_pings)
    struct Pings
    {
        bool on = false, pushed = false, restart = false;
        msk144wb::PingParams params;
        msk144wb::PingHistory* d_state = nullptr;   // [channels]
        msk144wb::PingRecord* d_records = nullptr;  // [channels]
        int32_t* d_energies = nullptr;              // [channels][54]; the ping band's too, allocated by whichever `set` comes first
    } pings;
    // the ping band (msk144_set_wideband_ping_band): acts in a push made with the detector on, and restarts through pings.restart
    struct PingBand
    {
        bool on = false;
        int32_t shift = 0;
        int8_t* d_taps = nullptr;    // [64][2]
        uint8_t* d_tails = nullptr;  // [channels][128]: two zero bytes, then the 63 stored samples before the next push
    } ping_band;
    // the notch (msk144_set_wideband_notch): on = the table lists a channel.  pushed: the last push ran it and no `set` has come since
    struct Notch
    {
        bool on = false, pushed = false;
        int count = 0;                             // channels in the table = entries of d_list
        std::vector<uint8_t> listed;               // [channels] the channel is in the table, with ...
        std::vector<msk144wb::NotchParams> table;  // [channels] ... this entry
        int32_t* d_list = nullptr;     // [channels] the table's channels, ascending; the first `count` are read
        int8_t* d_taps = nullptr;      // [channels][64][2]
        int32_t* d_shifts = nullptr;   // [channels]
        uint8_t* d_tails = nullptr;    // [channels][128]: two zero bytes, then the 63 raw stored samples before the next push
        int32_t* d_clipped = nullptr;  // [channels] of the last push; 0 for a channel not in the table
    } notch;
    // per-channel waterfall (msk144_set_wideband_waterfall)
    struct Waterfall
    {
        bool on = false, pushed = false;
        float2* d_dft = nullptr;   // [3][96][32] the windowed DFT matrix in the kernel's order
        float* d_rows = nullptr;   // [channels][54][96]
        double* d_sums = nullptr;  // [channels][96]
    } waterfall;
    // per-ping capture (msk144_set_wideband_capture): descriptors and rows for the largest max_units set so far (`rows`; a larger
    // one frees them and allocates anew).  pushed: the last push left a header and no `set` has come since
    struct Capture
    {
        bool on = false, pushed = false, restart = false;
        msk144wb::CaptureParams params;
        int rows = 0;
        uint8_t* d_listed = nullptr;                  // [channels]
        msk144wb::CaptureState* d_state = nullptr;    // [channels]
        msk144wb::PlanHeader* d_header = nullptr;     // [1]
        msk144wb::CaptureUnit* d_units = nullptr;     // [rows]
        uint8_t* d_data = nullptr;                    // [rows][5184]
    } capture;
    // the audio (msk144_set_wideband_audio): the ring is written by every push made with it on; the dense rows are the capture's
    // units' and follow capture.rows (`rows`: what they hold; a larger one frees them and allocates anew, in whichever `set` brings
    // it).  pushed: the last push wrote the ring and no `set` has come since
    struct Audio
    {
        bool on = false, pushed = false, restart = false;
        int32_t shift = 0;
        int rows = 0;
        int8_t* d_taps = nullptr;          // [64][2]
        int16_t* d_phasor = nullptr;       // [96][2]
        uint8_t* d_tails = nullptr;        // [channels][128]: two zero bytes, then the 63 stored samples before the next push
        int16_t* d_ring = nullptr;         // [channels][2][2592]: the audio of hop k in row k & 1
        int32_t* d_clamped = nullptr;      // [channels][2]
        int16_t* d_rows = nullptr;         // [rows][2592]
        int32_t* d_row_clamped = nullptr;  // [rows]
    } audio;
    // the gate (msk144_set_wideband_gate).  pushed: the last push left a header and no `set` has come since.  `planned` is recorded
    // behind the copy of the header to `header`: what msk144_decode_stages and msk144_wideband_gate wait for, not the stream
    struct Gate
    {
        bool on = false, pushed = false, restart = false;
        msk144wb::GateParams params;
        uint8_t* d_always = nullptr;                // [channels]
        int32_t* d_since = nullptr;                 // [channels]
        msk144wb::PlanHeader* d_header = nullptr;   // [1]
        int32_t* d_list = nullptr;                  // [channels]
        float2* d_analytic = nullptr;               // [channels][5184]: row j is the window of channel list[j]
        msk144wb::PlanHeader* header = nullptr;     // pinned: the header, and behind it the list, int32 [channels]
        hipEvent_t planned = nullptr;
    } gate;
};

// The input-rate configuration of a handle (msk144_set_input_rate): one block, value-initialised is "off".  Its buffers are registered
// with the handle's own owner (msk144_handle::mem) and freed ahead of it by a new `set`.  d_* and slot_clamped are allocated by `set`,
// the pinned rows at the first msk144_rate_hop_slot.
struct InputRate
{
    bool on = false;
    bool pushed = false;          // a msk144_push_rate_hops has been made since `set`: what the two read entries test
    int64_t rate_hz = 0;
    msk144ir::Shape shape;
    int shift = 0;
    int hist_stride = 0;          // int16 per stream in d_hist: max(H, 1)
    std::vector<uint8_t> started; // [channels] the stream has had a first hop since `set`
    std::vector<uint8_t> last_first;  // [last_n] is_first of the last push
    int last_n = 0;
    int16_t* hops[MSK144_SLOTS] = {};          // pinned [channels][row]
    int16_t* first_halves[MSK144_SLOTS] = {};  // pinned [channels][row]
    int16_t* d_in_hops = nullptr;   // [channels][row]
    int16_t* d_in_first = nullptr;  // [channels][row]
    int16_t* d_hist = nullptr;      // [channels][hist_stride]: each stream's last H inputs, oldest first
    uint32_t* d_taps = nullptr;     // msk144ir::pack_taps
    int32_t* d_clamped = nullptr;   // [channels] by position of the last push
    int32_t* slot_clamped[MSK144_SLOTS] = {};  // pinned [channels]: the counts of the last push of each slot, copied behind its resampler
    int slot_n[MSK144_SLOTS] = {};             // n of that push; 0: none
};

// "The first listing since `set`": a stream's state on the device restarts at the first push that lists it after the option's
// `set`.  stage() fills the slot's pinned row, which the push copies to d_restart ahead of its kernel; commit() marks the streams
// seen, once the push's work has been enqueued - only a push that went out uses up a stream's restart.  The buffers are the
// option's `set` to allocate.
struct SinceSet
{
    std::vector<uint8_t> seen;             // [channels] the stream has been listed since `set`
    uint8_t* restart[MSK144_SLOTS] = {};   // pinned [channels] by position
    uint8_t* d_restart = nullptr;          // [channels] by position

    void reset(size_t channels) { seen.assign(channels, 0); }
    void stage(int32_t slot, const int32_t* streams, int32_t n)
    {
        uint8_t* row = restart[slot];
        for(int32_t j = 0; j < n; j++) row[j] = seen[static_cast<size_t>(streams[j])] ? 0 : 1;
    }
    void commit(const int32_t* streams, int32_t n)
    {
        for(int32_t j = 0; j < n; j++) seen[static_cast<size_t>(streams[j])] = 1;
    }
};

// Per-stream levels and pings on the audio hops (msk144_set_stream_pings): one block, value-initialised is "off".  Everything is
// allocated by the first `set` that switches it on, registered with the handle's own owner, and kept until the handle goes; a push
// allocates nothing.  The device results of a push are one block - records [n], levels [n], energies [n][54] - so that one copy takes
// them to the slot's pinned block of the same layout.
struct StreamPings
{
    bool on = false;              // what the next push does
    bool pushed = false;          // a push has left results since `set`: what the read entries test
    msk144sp::Params params;
    SinceSet since;               // which positions of a push restart their stream's history
    int last_slot = 0;            // the slot of the last push, ...
    int slot_n[MSK144_SLOTS] = {};  // ... n of each slot's last push since `set`; 0: none
    msk144wb::PingHistory* d_state = nullptr;  // [channels] by stream
    uint8_t* d_out = nullptr;                  // the results of the last push: channels x (32 + 32 + 54 x 4) bytes
    uint8_t* out[MSK144_SLOTS] = {};           // pinned, as d_out

    // the one layout of d_out and out[] for a push of n positions - records [n], levels [n], energies [n][54] - in bytes from the
    // start: what sp_push writes, the read entries take apart, and the stream gate reads its records and energies from
    static size_t levels_at(int n) { return sizeof(msk144wb::PingRecord) * static_cast<size_t>(n); }
    static size_t energies_at(int n) { return levels_at(n) + sizeof(msk144sp::Level) * static_cast<size_t>(n); }
    static size_t out_bytes(int n) { return energies_at(n) + sizeof(int32_t) * msk144sp::kMaxBlocks * static_cast<size_t>(n); }
};

// The stream gate (msk144_set_stream_gate): one block, value-initialised is "off".  Everything is allocated by `set`, registered with
// the handle's own owner and kept until the handle goes - the packed store for the largest row count set so far (`rows`; a larger
// one frees it and allocates anew); a push allocates nothing.  Each slot has its pinned header with the list behind it, and its
// event, recorded behind the copy of both: what msk144_decode_stages and the read entries wait for, not the stream.
struct StreamGate
{
    bool on = false;              // what the next push does
    bool pushed = false;          // a push has left a list since `set`: what msk144_stream_gate tests
    msk144sg::Params params;
    int rows = 0;                 // rows of d_analytic
    long long pushes = 0;         // gated pushes since `set`
    SinceSet since;               // which positions of a push restart their stream's count
    int last_slot = 0;            // the slot of the last push, ...
    bool slot_pushed[MSK144_SLOTS] = {};  // ... and whether each slot has had one since `set`
    uint8_t* d_always = nullptr;                // [channels] by stream
    int32_t* d_since = nullptr;                 // [channels] by stream
    unsigned long long* d_masks = nullptr;      // [channels] by position: the gate's own masks (ratio_q4 != 0)
    msk144wb::PlanHeader* d_header = nullptr;   // [1]
    int32_t* d_list = nullptr;                  // [channels]
    float2* d_analytic = nullptr;               // [rows][5184]: row i is the window of position list[i]
    msk144wb::PlanHeader* header[MSK144_SLOTS] = {};    // pinned: the header, and behind it the list, int32 [channels]
    hipEvent_t planned[MSK144_SLOTS] = {};
};

struct msk144_handle
{
    msk144_params params{};
    msk144::DeviceStore st{};
    msk144::SyncTemplate tpl{};
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
    bool gated = false;  // the current hop is a push made with a gate on (Wideband::Gate, StreamGate): the decode covers the listed windows ...
    int gated_n = 0;     // ... this many, which the last decode read from the gate's header
    // what the gate that made the current hop hands the decode and the dumps (set by wb_gate_gather, sg_gather)
    struct GatedHop
    {
        const msk144wb::PlanHeader* header = nullptr;  // pinned
        hipEvent_t planned = nullptr;                  // recorded behind the copy to it
        float2* analytic = nullptr;                    // the packed store
    } gate_of;
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
    Wideband wb;
    // resampler in front of the hop ring (msk144_set_input_rate)
    InputRate ir;
    // levels and pings of the audio hops (msk144_set_stream_pings)
    StreamPings sp;
    // the gate on those pings (msk144_set_stream_gate)
    StreamGate sg;

    std::string error;
};

// internal to the library: none of this is exported
#pragma GCC visibility push(hidden)

// defined in msk144_api.cpp
int fail(msk144_handle* h, int code, const std::string& msg);  // sets the handle's (h == nullptr: the thread's creation) error text; returns code
void ev_begin(msk144_handle* h);
void ev_end(msk144_handle* h, int stage);
int ensure_ring(msk144_handle* h);
int check_hop_slot(msk144_handle* h, int32_t slot);
int begin_hop(msk144_handle* h, int32_t slot, int32_t n);
int run_frontend(msk144_handle* h, const void* d_in);
// msk144_push_hops (rate = false) and msk144_push_rate_hops (rate = true): the checks, the staging copies, then the steps below
// and the hop ring and front end, in one order for both; `entry` is the exported name, the prefix of its messages
int push_stream_hops(msk144_handle* h, int32_t slot, int32_t n, const char* entry, bool rate);
// the two refusals every msk144_set_* entry of an audio-stream option shares - read_mode 2, wideband mode; `what` is the entry's own
// clause behind the semicolon of the first
int streams_only(msk144_handle* h, const char* entry, const char* what);
// defined in msk144_wideband_api.cpp: back to no wideband configuration, its buffers freed, every field reset
void wb_release(msk144_handle* h);
// The steps of push_stream_hops that the options own, each on the handle's stream, in the order it runs them.
// defined in msk144_input_rate_api.cpp: the n staged rows at the input rate to 12 kHz halves in d_first / d_hops, and the clamp counts
// to the slot's pinned row; behind the staging copies.  Only for the rate entry
int ir_resample(msk144_handle* h, int32_t slot, int32_t n, bool any_first);
// defined in msk144_stream_pings_api.cpp: the levels and pings of a push of n audio hops, behind the staging copy or the resampler
// and ahead of the hop ring.  Only while h->sp.on
int sp_push(msk144_handle* h, int32_t slot, int32_t n);
// defined in msk144_stream_gate_api.cpp.  sg_plan: the gate's list of a push of n audio hops, behind sp_push and ahead of the hop
// ring, its header and list to the slot's pinned block, and the event.  sg_gather: behind run_frontend, the listed positions'
// analytic windows into the gate's store; it makes the hop a gated one.  Only while h->sg.on.  sg_release: the events, which no
// owner frees
int sg_plan(msk144_handle* h, int32_t slot, int32_t n);
int sg_gather(msk144_handle* h, int32_t n);
void sg_release(msk144_handle* h);

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

// the same for one that host_alloc registered
template<typename T>
void host_free(Buffers& owner, T** p)
{
    const auto it = std::find(owner.pinned.begin(), owner.pinned.end(), static_cast<void*>(*p));
    if(it != owner.pinned.end())
    {
        (void)hipHostFree(*it);
        owner.pinned.erase(it);
    }
    *p = nullptr;
}

#pragma GCC visibility pop
