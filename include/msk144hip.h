/*
 * msk144hip - C ABI of the MI355X-native MSK144 hot path (libmsk144hip.so).
 *
 * The reference (alexander-sholohov/msk144cudecoder @ 2024_10_08) has no plugin/FFI interface: its
 * only external boundary is the process (raw samples on stdin, text on stdout).  This ABI is cut
 * along the reference's internal seams so that its main loop can call it instead of its own CUDA:
 *
 *   msk144_create            MSK144SearchContext ctor + ResultKeeper::init + LDPCContext::init +
 *                            Analytic(8192)                       msk_context.cuh:23-38, main.cu:211-226
 *   msk144_submit_audio      rms normalise, int16->complex, apply_shift_filter_shift<<<1,32>>> or
 *                            Analytic::execute                    main.cu:300-332
 *   msk144_submit_iq         int8 I/Q -> complex, apply_filter<<<1,32>>>   main.cu:365-380
 *   msk144_decode            clear_result + scan_kernel + softbits_kernel + index_kernel +
 *                            ldpc_kernel                          main.cu:461-468
 *   msk144_results           get_all_results() + the is_message_present filter of the host loop
 *                                                                 main.cu:477-484
 *   msk144_segment_power     the 8 segment powers SNRTracker::process_data sums from the analytic
 *                            window                               snr_tracker.cu:21-37, main.cu:388
 *   msk144_hop_slot,         the 50 %-overlap window ring kept on the device: 2592 new samples per stream and hop travel, not
 *   msk144_push_hops         5184-sample windows             main.cu:271-294, 337-359
 *   msk144_input_slot ..     the same hop, pipelined over two pinned staging slots (fread buffer -> H2D -> kernels ->
 *   msk144_fetch_wait        D2H of what the host loop consumes)  main.cu:261-422, 474-525
 *   msk144_dump_candidates   the raw ResultItem array (parity/debug)     result_keeper.cuh:17-32,123-130
 *   msk144_destroy           ~MSK144SearchContext / deinit        msk_context.cuh:81-120
 *   msk144_device_count      cudaGetDeviceCount behind cudaSetDeviceFlags (the reference drives device 0 only; the multi-device
 *                            stream program asks how many it may split its streams over)   main.cu:115
 *   msk144_llr_block_channels how many channels' softbits the handle keeps at a time (the reference keeps 512 B in every ResultItem of its one
 *                            stream, result_keeper.cuh:17-32; here a block of channels shares one LLR store)
 *   msk144_set_llr_retention whether the 128 softbits of every candidate stay readable after the decode, as in the reference's
 *                            ResultItem array (result_keeper.cuh:17-32, 105-115) - the stream program never reads them
 *   msk144_set_copy_handover whether slots that fold the same frames as a lower slot of their group are computed again, as
 *   msk144_copy_count        softbits_kernel / ldpc_kernel do for every slot (softbits_kernel.cuh:56-83, ldpc_kernel.cuh:100-249)
 *   msk144_set_wideband ..   the CPU decimation chain in front of --read-mode=2 (rtl_sdr | csdr fir_decimate_cc ... | convert_f_s8,
 *   msk144_push_wideband     README.md of the reference), for every channel of one wideband stream at once: a down-converter
 *                            bank on the device that writes the channels' int8 I/Q hops into the hop ring (no reference counterpart)
 *   msk144_wideband_levels,  what a bank of channels needs where a single csdr chain has one gain_ff stage: every channel's level and
 *   msk144_set_wideband_gains, clip count of the last push, a gain per channel, and a stepped AGC that runs on the device one
 *   msk144_set_wideband_agc  push behind the statistics (no reference counterpart)
 *   msk144_set_wideband_blanker, the noise blanker every SDR receiver chain has ahead of its channel filter, where an impulse is still a
 *   msk144_wideband_blanker_stats, few samples wide: on the device, ahead of the channeliser and the bank (no reference counterpart)
 *   msk144_dump_wideband_blanked
 *   msk144_set_wideband_spectrum, the spectrum display every SDR front end has: the power spectrum of each push's input samples at
 *   msk144_wideband_spectrum the input rate, on the device (no reference counterpart)
 *   msk144_set_wideband_waterfall, the fast graph every MSK144 operator knows, for every channel at once: a 96-point spectrum per
 *   msk144_wideband_waterfall, 8 ms block of each channel's int8 hop, on the device (no reference counterpart)
 *   msk144_wideband_waterfall_sums
 *   msk144_set_input_rate .. the `ffmpeg -ar 12000` step the reference's README puts in front of --read-mode=1, for every stream of a
 *   msk144_push_rate_hops    handle at once: an integer polyphase resampler on the device in front of the hop ring (no reference counterpart)
 *   msk144_clock_probe       gpu_timer.h's role for the one figure HIP events cannot give: the shader clock a running batch
 *                            actually gets (s_memtime / s_memrealtime), read beside it on a side stream
 *
 * One handle = one device + one HIP stream + `channels` independent input streams decoded per call
 * (the reference decodes one).  Plain pointers and sizes only; no exceptions cross the boundary:
 * every entry returns 0 or a negative MSK144_E* code, msk144_last_error() gives the text.
 * Handles are independent of each other; a handle is not re-entrant.
 */
#ifndef MSK144HIP_H
#define MSK144HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSK144_WINDOW_SAMPLES 5184 /* 6 frames of 864 samples (common.h:15) */
#define MSK144_HOP_SAMPLES 2592    /* 50 % overlap (main.cu:284) */
#define MSK144_CODE_BITS 128
#define MSK144_MESSAGE_BITS 77

enum
{
    MSK144_OK = 0,
    MSK144_EINVAL = -1,   /* bad argument / parameter */
    MSK144_EHIP = -2,     /* HIP runtime error (text in msk144_last_error) */
    MSK144_ENOMEM = -3,   /* device or host allocation failed */
    MSK144_ESTATE = -4,   /* call out of order (e.g. decode before submit) */
    MSK144_EOVERFLOW = -5, /* more decodes than max_results; results truncated */
    MSK144_ENOTRETAINED = -6 /* blocked staging does not retain what was asked for (LLR rows of an earlier block, or a partial
                                stage run); create the handle with llr_block_channels = channels */
};

/* msk144_decode_stages bits, in launch order (main.cu:463-467) */
enum
{
    MSK144_STAGE_SCAN = 1,
    MSK144_STAGE_SOFTBITS = 2,
    MSK144_STAGE_INDEX = 4,
    MSK144_STAGE_LDPC = 8,
    MSK144_STAGE_COLLECT = 16,
    MSK144_STAGE_ALL = 31
};

/* indices into msk144_stage_times */
enum
{
    MSK144_T_FRONTEND = 0,
    MSK144_T_SCAN = 1,
    MSK144_T_SOFTBITS = 2,
    MSK144_T_INDEX = 3,
    MSK144_T_LDPC = 4,
    MSK144_T_COLLECT = 5,
    MSK144_T_H2D = 6,  /* host -> device copy of the submitted windows (msk144_submit_audio/_iq/_slot) */
    MSK144_T_D2H = 7,  /* device -> host copy of count, records and segment powers (msk144_fetch_async) */
    MSK144_T_COUNT = 8
};

#define MSK144_SLOTS 2 /* pinned staging slots per handle (msk144_input_slot .. msk144_fetch_wait) */

typedef struct msk144_params
{
    float center_hz;        /* --center-frequency (1500 audio / 0 IQ) */
    float width_hz;         /* --search-width  (200) */
    float step_hz;          /* --search-step   (2)   */
    int32_t scan_depth;     /* --scan-depth    (4), clamped to 1..8 like msk_context.cuh:29-33 */
    int32_t nbadsync_threshold; /* --nbadsync-threshold (1) */
    int32_t read_mode;      /* --read-mode: 1 = int16 audio, 2 = int8 I/Q */
    int32_t analytic_method;/* --analytic-method: 1 = FFT, 2 = shift-filter-shift (audio only) */
    int32_t channels;       /* independent streams decoded per call (reference: 1) */
    int32_t device;         /* HIP device ordinal */
    int32_t max_results;    /* capacity of the compact result list; 0 = default */
    int32_t llr_block_channels; /* channels per softbits->index->LDPC block (reference: result_keeper.cuh:105-115 keeps every
                                   candidate's 128 softbits; ldpc_kernel.cuh:116-142 reads them back).  The LLR rows of a block
                                   (block x items x 512 B) are produced and consumed back to back, so the LLR store never grows
                                   with the batch (1.58 GB per 128-channel block at the deep config instead of 12.6 GB per 1024
                                   channels).  0 = automatic: min(channels, 128), the bottom of a flat valley on the 1024-channel bench
                                   step (48: +1.4 %, 64: +0.8 %, 96: +0.3 %, 160: +0.1 %, 192: +0.3 %, 256: +0.9 % step time).  With fewer channels per block than channels no row outlives
                                   its block, and a candidate the nbadsync gate drops (index_kernel.cuh:7-76) is not demodulated
                                   beyond its sync check.  Candidate dumps need every row retained:
                                   = channels: retain everything, every candidate in full (parity-dump mode) */
} msk144_params;

/* One accepted decode (CRC ok, < 18 hard errors), fields as the reference's host loop consumes them
 * (main.cu:484-522). */
typedef struct msk144_result
{
    int32_t channel;
    int32_t item;            /* k = block_idx*D*8 + pattern_idx*8 + slot inside the channel */
    float f0;                /* Hz */
    int32_t pattern_idx;
    int32_t num_avg;
    uint32_t pos;
    float xb;
    int32_t nbadsync;
    int32_t ldpc_iterations;
    int32_t ldpc_hard_errors;
    uint8_t message[10];     /* 77 payload bits, MSB first, zero padded */
    uint8_t reserved[2];
} msk144_result;

/* Same layout as the reference's ResultKeeper::ResultItem (result_keeper.cuh:17-32), 632 bytes. */
typedef struct msk144_candidate
{
    uint32_t block_idx;
    uint32_t pattern_idx;
    uint32_t pos;
    float f0;
    int32_t nbadsync;
    float xb;
    int32_t num_avg;
    float softbits_wo_sync[128];
    uint8_t is_message_present;
    int32_t ldpc_num_iterations;
    int32_t ldpc_num_hard_errors;
    char message[77];
} msk144_candidate;

typedef struct msk144_handle msk144_handle;

/* defaults exactly as main.cu:122-133 (NOT the help text) */
void msk144_default_params(msk144_params* p);

/* HIP devices visible to this process (0 and MSK144_EHIP when there is none): what msk144_params.device may range over.  The
 * reference binds the process to one device (main.cu:115); msk144hipdecoder --devices=... creates one handle per listed ordinal. */
int msk144_device_count(int32_t* n);

int msk144_create(const msk144_params* params, msk144_handle** out);
void msk144_destroy(msk144_handle* h);
/* h may be NULL: error text of the last failed msk144_create on this thread */
const char* msk144_last_error(const msk144_handle* h);

/* F frequency hypotheses, D patterns, items per channel = F*D*8 */
int msk144_geometry(const msk144_handle* h, int32_t* num_freqs, int32_t* scan_depth, int32_t* items_per_channel);
int msk144_frequency(const msk144_handle* h, int32_t block_idx, float* hz);

/* Run on a caller-owned HIP stream (hipStream_t passed as void*); NULL = the handle's own stream. */
int msk144_set_stream(msk144_handle* h, void* hip_stream);

/* Front end.  Host buffers are copied H2D on the handle's stream; *_device variants take device
 * pointers that must stay valid until the front-end kernel has run.
 *   audio: int16 [channels][5184];   iq: int8 [channels][2*5184] interleaved I,Q. */
int msk144_submit_audio(msk144_handle* h, const int16_t* windows);
int msk144_submit_iq(msk144_handle* h, const int8_t* windows);
int msk144_submit_audio_device(msk144_handle* h, const int16_t* d_windows);
int msk144_submit_iq_device(msk144_handle* h, const int8_t* d_windows);
/* bypass the front end: complex64 (re,im) [channels][5184], host memory (parity tests) */
int msk144_submit_analytic(msk144_handle* h, const float* windows);

/* Asynchronous: enqueues the kernels and returns. */
int msk144_decode(msk144_handle* h);
int msk144_decode_stages(msk144_handle* h, uint32_t stages);
int msk144_synchronize(msk144_handle* h);

/* Waits for the decode, copies the compact result list.  *n = number of decodes (<= cap copied). */
int msk144_results(msk144_handle* h, msk144_result* out, int32_t cap, int32_t* n);
int msk144_result_count(msk144_handle* h, int32_t* n);
/* device-side list for callers that gather on the GPU (RCCL): records + count stay valid until the
 * next decode */
int msk144_results_device(msk144_handle* h, const msk144_result** d_records, const int32_t** d_count);
/* Multi-GPU sharding (no reference counterpart: the reference decodes one stream on one GPU, main.cu:115):
 * msk144_result.channel = base + local channel, so that the records of a rank that owns channels
 * [base, base+channels) carry global channel ids when they are gathered.  Default 0. */
int msk144_set_channel_base(msk144_handle* h, int32_t base);

/* Copies (no reference counterpart: the reference demodulates and decodes every one of its F*D*8 slots, softbits_kernel.cuh:56-83,
 * ldpc_kernel.cuh:100-249).  Two slots of one (frequency, pattern) group whose scan positions are congruent modulo the 5184-sample
 * ring - or, for masks 111111 / 100100, modulo their period 864 / 2592 - fold the SAME frames.  In blocked staging
 * (llr_block_channels < channels: no LLR row outlives its block) such a slot is by default not computed again: it reports the
 * nbadsync, iterations, hard errors and payload of the LOWEST congruent slot of its group, with its own position and xb.
 *   msk144_set_copy_handover(h, 0)  every slot is demodulated and decoded on its own, as in the reference (still blocked staging,
 *                                   still no demodulation beyond the sync check for candidates the nbadsync gate drops);
 *   msk144_set_copy_handover(h, 1)  the default of a blocked handle; MSK144_ENOTRETAINED on a handle that retains every LLR row
 *                                   (such a handle always computes every slot: its dumps show each slot's own row).
 * Takes effect at the next decode.  msk144_copy_count: slots of the last decode that were handed over (0 when switched off). */
int msk144_set_copy_handover(msk144_handle* h, int32_t enable);
/* A handle whose one block covers all its channels (llr_block_channels = channels; the default up to 128 channels, e.g. the single
 * stream of the reference's program) keeps every candidate's 128 softbits readable after the decode, as the reference's ResultItem
 * array does (result_keeper.cuh:17-32): msk144_dump_candidates, partial stage runs and msk144_load_candidates work, and every slot is
 * demodulated in full.  A caller that only reads the result list - the stream program - says so with
 *   msk144_set_llr_retention(h, 0)  the handle behaves like a blocked one: a candidate the nbadsync gate drops stops after its sync
 *                                   check, copies are handed over (above), dumps / partial stage runs / loaded candidates are refused
 *                                   with MSK144_ENOTRETAINED - the kernels bench.py times at 1024 channels;
 *   msk144_set_llr_retention(h, 1)  back to retaining; MSK144_ENOTRETAINED on a handle created with fewer channels per block than
 *                                   channels.
 * Takes effect at the next decode. */
int msk144_set_llr_retention(msk144_handle* h, int32_t retain);
/* channels per softbits -> index -> LDPC block this handle decodes in (msk144_params.llr_block_channels after the automatic choice) */
int msk144_llr_block_channels(const msk144_handle* h, int32_t* channels_per_block);
int msk144_copy_handover(const msk144_handle* h, int32_t* enabled);
int msk144_copy_count(msk144_handle* h, int64_t* slots);

int msk144_segment_power(msk144_handle* h, float* out /*[channels][8]*/);

/* Pinned staging, two slots ("handle owns device + pinned host buffers").  The reference's loop is strictly serial
 * per hop - fread, H2D, kernels, cudaDeviceSynchronize, 15 MB D2H, host loop, print (main.cu:261-422, 461-525).  With the slots a
 * caller fills the windows of hop n+1 and reads the results of hop n-1 while the GPU decodes hop n, and one hop costs one
 * asynchronous H2D and one asynchronous D2H of exactly what the host loop consumes (count, compact records, 8 segment powers per
 * channel) instead of five blocking calls:
 *
 *     msk144_input_slot(h, s, &win, &bytes);   fill win[channels][5184] (int16) or [channels][2*5184] (int8), pinned
 *     msk144_submit_slot(h, s);                H2D + front end                      (asynchronous)
 *     msk144_decode(h);                        kernels; the record list of slot s   (asynchronous)
 *     msk144_fetch_async(h, s);                D2H into the slot's pinned output    (asynchronous)
 *     ... other work, e.g. the same four calls for slot 1 - s ...
 *     msk144_fetch_wait(h, s, &rec, &n, &seg); blocks until slot s has arrived; rec/seg point into the slot (valid until the slot
 *                                              is submitted again)
 *
 * Each slot has its own device-side record list, so the list of slot s stays intact while slot 1 - s decodes.  The asynchronous
 * copy covers a running estimate of the record count (twice the last count, at least 1024); msk144_fetch_wait copies a
 * remainder synchronously.  The buffers are allocated at the first msk144_input_slot / msk144_fetch_async call of a handle.
 * msk144_fetch_wait may be called from a second thread while the first thread submits the OTHER slot; everything else about a
 * handle stays single-threaded.  msk144_fetch_wait returns MSK144_EOVERFLOW (records truncated to max_results) like
 * msk144_results. */
int msk144_input_slot(msk144_handle* h, int32_t slot, void** host_windows, size_t* bytes);
int msk144_submit_slot(msk144_handle* h, int32_t slot);
/* The same for a hop that covers only the first n_channels windows of the slot (1..channels): every kernel, copy and result of
 * the hop is sized for n_channels, so a partial batch - streams that lag sit it out - costs what its streams cost, not what the
 * handle's capacity costs.  Record channel numbers are positions in the slot. */
int msk144_submit_slot_n(msk144_handle* h, int32_t slot, int32_t n_channels);
/* Library-side hop ring (the reference's host keeps the 50 %-overlap window itself: main.cu:284-288 / 349-353 copy the second half
 * over the first and fread 2592 new samples behind it; the first read fills all 5184, main.cu:271-283).  With these two calls the
 * DEVICE keeps every stream's window: per hop the caller writes, for each of the n streams that have one, the 2592 new samples into
 * hops[j], the stream's number (0 .. channels-1, ascending) into streams[j] and is_first[j] = 0 - or, for a stream's very first
 * hop, its first 2592 samples into first_halves[j], the second 2592 into hops[j] and is_first[j] = 1.  msk144_push_hops copies only
 * what the n hops need (half of what msk144_submit_slot_n copies), advances the rings of those streams on the device and runs the
 * front end on their n windows; msk144_decode / msk144_fetch_async / msk144_fetch_wait follow as after msk144_submit_slot_n (record
 * channel numbers are positions j).  A stream that is not listed keeps its window.  All four arrays are pinned, owned by the handle,
 * sized for `channels` entries, allocated at the first msk144_hop_slot call; sample units as in msk144_submit_audio / _iq. */
int msk144_hop_slot(msk144_handle* h, int32_t slot, void** hops /*[channels][2592 samples]*/, void** first_halves /*[channels][2592 samples]*/,
                    int32_t** streams /*[channels]*/, uint8_t** is_first /*[channels]*/);
int msk144_push_hops(msk144_handle* h, int32_t slot, int32_t n);
int msk144_fetch_async(msk144_handle* h, int32_t slot);
int msk144_fetch_wait(msk144_handle* h, int32_t slot, const msk144_result** records, int32_t* n, const float** seg_power /*[channels][8]*/);

/* parity / debug */
int msk144_dump_analytic(msk144_handle* h, int32_t channel, float* out /*[5184][2]*/);
/* row block_idx (0 .. num_freqs-1) of the handle's phasor table: (cos, sin) of the float phase by which the scan and softbits kernels
 * rotate sample n of a window for that frequency hypothesis.  The table is built once, in msk144_create. */
int msk144_dump_mix_table(msk144_handle* h, int32_t block_idx, float* out /*[5184][2]*/);
int msk144_dump_candidates(msk144_handle* h, int32_t channel, msk144_candidate* out /*[items_per_channel]*/);
int msk144_dump_indexes(msk144_handle* h, int32_t channel, int32_t* out /*[items_per_channel]*/, int32_t* n);
/* overwrite a channel's candidate store (pos, nbadsync, softbits) so later stages can be run on
 * known inputs */
int msk144_load_candidates(msk144_handle* h, int32_t channel, const msk144_candidate* items);

/* per-stage device time (HIP events recorded on the decode stream around every launch), summed over the launches of one
 * msk144_decode / msk144_submit_* call and averaged over the calls since the last reset; samples[s] = calls measured */
int msk144_set_profiling(msk144_handle* h, int32_t enable);
int msk144_stage_times(msk144_handle* h, float* avg_ms /*[MSK144_T_COUNT]*/, int32_t* samples /*[MSK144_T_COUNT] or NULL*/, int32_t reset);

/* Shader clock the handle's device runs at right now, in MHz: a one-wave kernel on a side stream of the handle spins for spin_us
 * microseconds of the constant 100 MHz counter (s_memrealtime) and divides the shader cycles that passed (s_memtime) by it.  It runs
 * BESIDE whatever the handle's stream is executing (one wave, no LDS), so calling it right after msk144_decode reads the clock the
 * decode kernels get - the number a sustained-throughput claim needs next to its step time (DVFS: a chip that has idled for a hop
 * period starts its next batch at a lower clock).  Blocks the caller for about spin_us.  spin_us 1..100000. */
int msk144_clock_probe(msk144_handle* h, int32_t spin_us, float* shader_mhz);

/* ---- Wideband channeliser (no reference counterpart) ----
 *
 * One wideband complex stream in, `channels` 12 ksps int8 I/Q streams out, each exactly what --read-mode=2 consumes: the
 * channeliser writes every channel's hop into the hop ring's device staging (as msk144_push_hops would have copied it), then the
 * hop ring and the IQ front end run unchanged.
 *
 *   Input:        interleaved I,Q samples at Fs = 12000 x P/Q Hz (P/Q in lowest terms), Fs an integer multiple of 125 with
 *                 24000 <= Fs <= 6144000, i.e. 2 <= P/Q <= 512; Q then divides 96.  Q = 1 is decimation by the integer D = P
 *                 (1.92 Msps: D = 160; 2.4 Msps: D = 200); otherwise e.g. 2.048 Msps = 12000 x 512/3, 250 ksps = 12000 x 125/6.
 *                 As cu8 (rtl_sdr, (u - 127.5) / 128), cs8 (s / 128) or cs16 (s / 32768).
 *   Offsets:      integer Hz, |f_c| <= Fs/2 - 6000, one per channel, no grid needed.
 *   Filter:       a real low-pass h[0..L), L = K x P, 1 <= K <= 64, at the upsampled rate Q x Fs = P x 12000, supplied by the
 *                 caller (num_taps = K x D for Q = 1).  The default design (K = 16, a Kaiser-windowed sinc: flat within 0.1 dB to
 *                 4 kHz, >= 60 dB down from 8 kHz) sums to Q, so that every branch h[r], h[r + Q], ... has about unit DC gain; it is
 *                 msk144host_wideband_taps_rate(rate, K) in libmsk144host.so (msk144host_wideband_taps(D, K) is that call at
 *                 rate = D x 12000), the taps msk144hipdecoder uses.
 *   Output:       y_c[m] = e^{-j2pi f_c m / 12000} . sum_{k<L} (h[k] e^{+j2pi f_c k / Fs}) . x[mD - k]
 *                 - mix, filter and decimate by D - with m the 64-bit output index from the first sample of the stream,
 *                 x[n < 0] = 0, and the phases reduced in integers, (f_c m) mod 12000 and (f_c k) mod Fs, so they do not drift.
 *                 For Q > 1, with n_m = floor(m P / Q) and r_m = (m P) mod Q - mix at Fs, upsample by Q, filter, keep every P-th:
 *                   y_c[m] = e^{-j2pi ((f_c n_m) mod Fs)/Fs} . sum_{k >= 0, r_m + kQ < L} h[r_m + kQ] e^{+j2pi ((f_c k) mod Fs)/Fs} x[n_m - k]
 *                 which is the formula above for Q = 1, as (f_c m D) mod (12000 D) = D ((f_c m) mod 12000); phases in 64-bit integers.
 *                 The library computes every rate in this form: Q polyphase branches, one of them at Q = 1.
 *                 I and Q are q = clamp(rint(128 . gain . y), -128, 127) each (default gain 100, the csdr gain_ff stage); a
 *                 component whose rounded value lies outside [-128, 127] counts as clipped.  f32 arithmetic on the device.
 *                 0 < gain <= 1e36, so that 128 . gain is finite in f32 (an infinite scale would turn an exact 0 into NaN).
 *   Hops:         a first push carries 5184 x P/Q wideband samples (5184 output samples per channel), every later push
 *                 2592 x P/Q (2592); whole numbers, as Q divides 2592.  The filter history (the last ceil(L/Q) - 1 input samples, L - 1
 *                 for Q = 1: what the longest branch needs) and m stay on the device between pushes; a first push restarts the stream
 *                 (m = 0, zero history).
 *
 *     msk144_set_wideband(h, &wp);                  read_mode 2 handle, num_offsets == channels; resets history and m
 *     msk144_wideband_slot(h, s, &buf, &bytes);     pinned, 5184 x P/Q samples; fill 5184 x P/Q (first) or 2592 x P/Q
 *     msk144_push_wideband(h, s, first);            H2D + channeliser + hop ring + IQ front end on the handle's stream
 *     msk144_decode / msk144_fetch_async / msk144_fetch_wait   as after msk144_push_hops (record channel = channel index)
 *
 * Above 6.144 Msps: a two-stage bank.  Fs a multiple of 8000 Hz with 6144000 < Fs <= 61440000.  Every rate up to 6144000 keeps the
 * path, contract and results above.
 *   Stage 1:      a 64-band, 2x oversampled analysis bank; for each band k some channel lies in, at rate Fs/32:
 *                   s_k[n] = (-1)^(k n) . sum_{l<L1} h1[l] e^{+j2pi (k l mod 64)/64} x[32n - l]
 *                 n from the first sample of the stream, x[n < 0] = 0, h1 real with L1 = 64 x K1 taps (1 <= K1 <= 16).  This is the
 *                 Q = 1 formula above with D = 32, offset k Fs/64 and output rate Fs/32 in place of 12000 (the float64 model relies on
 *                 it).  f32 on the device, kept there, never quantised.
 *   Channels:     f_c (|f_c| <= Fs/2 - 6000 as above) lies in band k_c = floor((64 f_c + Fs/2) / Fs), in integers, so -32 <= k_c <= 32
 *                 (band 32 is the stream of band -32), at the residual offset d_c = f_c - k_c Fs/64, an integer with
 *                 |d_c| <= Fs/128 < Fs/64 - 6000.
 *   Stage 2:      the contract above, unchanged, applied to s_{k_c} at the rate Fs/32 (a multiple of 250 from 192250 to 1920000, Q
 *                 dividing 96) with offset d_c, the caller's taps h (taps_per_phase x P taps for Fs/32 = 12000 P/Q), the same gain,
 *                 int8 quantiser and clip rule; output index m and hop sizes as above (a first push is 5184 Fs/12000 input samples,
 *                 a later one 2592 Fs/12000, a whole number of 32-sample frames).  The history of both stages stays on the device;
 *                 a first push restarts both.
 *   Bank filter:  the default (msk144_set_wideband, or msk144_set_wideband_ex with bank_taps NULL) is K1 = 8, 512 taps, a
 *                 Kaiser-windowed sinc summing to 1 (so the gain keeps its meaning): flat within 0.1 dB for |f| <= Fs/128 + 4 kHz, at
 *                 least 60 dB down for |f| >= 3 Fs/128 - 8 kHz, the range the decimation by 32 folds onto a channel's 8 kHz stop edge;
 *                 msk144host_wideband_bank_taps(rate, K1, out) in libmsk144host.so.
 *
 * Stage times: in wideband mode MSK144_T_FRONTEND includes the channeliser (and the bank), MSK144_T_H2D the wideband copy. */
enum
{
    MSK144_WB_CU8 = 0,
    MSK144_WB_CS8 = 1,
    MSK144_WB_CS16 = 2
};

typedef struct msk144_wideband_params
{
    int64_t rate_hz;          /* Fs = 12000 x P/Q (D x 12000 for Q = 1), or a bank rate (the taps are then for Fs/32) */
    int32_t format;           /* MSK144_WB_* */
    int32_t taps_per_phase;   /* K */
    float gain;               /* output gain before int8 (default 100), 0 < gain <= 1e36 */
    int32_t num_taps;         /* = K x P (K x D for Q = 1) */
    const double* taps;       /* h[0 .. num_taps) */
    const int32_t* offsets_hz;/* f_c of channel 0 .. num_offsets-1 */
    int32_t num_offsets;      /* = channels */
} msk144_wideband_params;

int msk144_set_wideband(msk144_handle* h, const msk144_wideband_params* params);
/* the general form: above 6144000 Hz bank_taps = h1[0 .. bank_num_taps), bank_num_taps = 64 x K1 with 1 <= K1 <= 16, or NULL (and
 * 0) for the default bank; at or below 6144000 Hz bank_taps must be NULL.  msk144_set_wideband(h, p) is
 * msk144_set_wideband_ex(h, p, NULL, 0). */
int msk144_set_wideband_ex(msk144_handle* h, const msk144_wideband_params* params, const double* bank_taps, int32_t bank_num_taps);
int msk144_wideband_slot(msk144_handle* h, int32_t slot, void** buf, size_t* bytes);
/* MSK144_ESTATE for a later push (first = 0) before any first push */
int msk144_push_wideband(msk144_handle* h, int32_t slot, int32_t first);
/* the channel's int8 I/Q pairs of the last push: 5184 after a first push, else 2592 */
int msk144_dump_wideband_hop(msk144_handle* h, int32_t channel, int8_t* out);
/* clipped I and Q components of the last push, all channels */
int msk144_wideband_clip_count(msk144_handle* h, int64_t* clipped);

/* ---- Per-channel levels, gains and a stepped AGC (no reference counterpart) ----
 *
 * Across a wide band the channels' levels differ by tens of dB, and int8 (the --read-mode=2 contract) has room for about 40.  The
 * quantiser therefore takes one scale per channel,
 *     q = clamp(rint(128 . g_c . 2^e_c . y), -128, 127)
 * with g_c the channel's base gain (msk144_wideband_params.gain until msk144_set_wideband_gains) and e_c its AGC exponent (0 while
 * the AGC is off, the default).  With nothing below called, every hop, clip count and decode is what it is without these entries.
 *
 *   Levels:   every push records, per channel and in integers, sum_sq = the sum of I*I + Q*Q over the int8 values actually stored
 *             (after the clamp) and clipped = its components that meet the clip rule above.  The numbers are exact and
 *             deterministic: they equal what msk144_dump_wideband_hop gives, and the clipped counts sum to msk144_wideband_clip_count.
 *   Gains:    msk144_set_wideband_gains sets g_c (NULL: back to params.gain, held to the same rule) and zeroes the exponents.  0 < g_c, and
 *             128 . g_c . 2^max_exp (max_exp = 0 while the AGC is off) finite in f32, for the reason given at the gain above.
 *   AGC:      msk144_set_wideband_agc(h, &p) switches it on, (h, NULL) off; either zeroes the exponents and hold counters.  After a
 *             push with n = samples, S = sum_sq, k = clipped, per channel, all in 64-bit integers (csrc/wideband.h agc_step):
 *               k . 10^6 > clip_ppm . 2n  or  S > hi_sq . 2n :  e <- max(e - 1, min_exp), quiet <- 0          (step down at once)
 *               else S < lo_sq . 2n :  quiet <- quiet + 1; when quiet >= hold: e <- min(e + 1, max_exp), quiet <- 0
 *               else :  quiet <- 0
 *             and the next push is quantised with ldexpf(128 . g_c, e), a 6 dB ladder that is exact in f32.  The step runs on the
 *             device right behind the channeliser: causal with one push of lag, no host round trip.  Only integers decide, so the
 *             trajectory is a pure function of the reported statistics; a step multiplies the power by 4, so hi_sq > 4 . lo_sq rules
 *             out a limit cycle on a stationary channel; fast down and slow up suits pings.  Defaults (design parameters, not
 *             measurements): lo_sq 64 (8 LSB rms per component), hi_sq 1024 (32 LSB rms: Gaussian noise there clips below 100 ppm),
 *             clip_ppm 1000 (0.1 %), hold 4 pushes (about 0.9 s), min_exp -20, max_exp 20.
 *             A gain step lands on a hop boundary, which lies inside the 50 %-overlapped decode window: a window that spans a step
 *             sees a 6 dB jump in its middle.  This applies only while the AGC is on.
 *   Order:    gains and AGC take effect from the next push.  msk144_set_wideband resets to the scalar gain with the AGC off.  A first
 *             push (stream restart) zeroes exponents and hold counters, so the same stream pushed twice gives the same bytes.
 *   Refused:  MSK144_EINVAL outside wideband mode, for hi_sq <= 4 . lo_sq, hold < 1, min_exp > max_exp (or outside -126..126), a
 *             negative lo_sq or clip_ppm, and for any 128 . g_c . 2^max_exp that is not finite in f32. */
typedef struct msk144_wideband_level
{
    int64_t samples;   /* complex outputs of the last push: 5184 after a first push, else 2592 */
    int64_t sum_sq;    /* sum of I*I + Q*Q over the stored int8 values */
    int64_t clipped;   /* clipped components, the existing rule */
    float gain;        /* the gain this push was quantised with (base gain x 2^exponent) */
    int32_t exponent;  /* AGC exponent used for this push; 0 when AGC is off */
} msk144_wideband_level;

typedef struct msk144_wideband_agc
{
    int32_t lo_sq, hi_sq; /* mean-square window per component, LSB^2 (defaults 64, 1024) */
    int32_t clip_ppm;     /* clipped components per million that force a step down (1000) */
    int32_t hold;         /* pushes in a row below the window before a step up (4) */
    int32_t min_exp, max_exp; /* (-20, 20) */
} msk144_wideband_agc;

/* the levels of the last push, out[channels], with the gain and exponent that push was quantised with, whatever was set since;
 * synchronises like msk144_wideband_clip_count.  MSK144_ESTATE before any push */
int msk144_wideband_levels(msk144_handle* h, msk144_wideband_level* out);
/* gains[channels], each 0 < g; NULL: back to params.gain */
int msk144_set_wideband_gains(msk144_handle* h, const float* gains);
/* NULL: off */
int msk144_set_wideband_agc(msk144_handle* h, const msk144_wideband_agc* p);

/* ---- Impulse-noise blanker on the input stream (no reference counterpart) ----
 *
 * Power-line arcing, ignition and switching supplies put impulses on the stream that are a few input samples long, tens of dB over
 * the floor and white, so they land in every channel at once.  The blanker zeroes them at the input rate Fs, ahead of the channeliser
 * (and of stage 1 at a bank rate): behind the decimation an impulse is smeared over the whole filter.  It is written in integers, a
 * pure function of the raw samples, and it is a contract per push, as the AGC is.
 *
 * Let the N new samples of a push be n = 0 .. N-1 (N = 5184 Fs/12000 for a first push, else 2592 Fs/12000).
 *   Power:      p[n] = cI^2 + cQ^2 in integer component units of the input format: cu8 c = 2u - 255, cs8 c = s, cs16 c = s.
 *   Threshold:  one per push, from that push's own samples: S = sum p[n], M = floor(S / N), T = (M . threshold_q4) >> 4; sample n is a
 *               hit iff p[n] > T (strictly).  S <= 2^56 and M . threshold_q4 < 2^47: unsigned 64 bits hold everything
 *               (csrc/wideband.h blanker_threshold).  The mean includes the impulses, on purpose: 1 % of the samples at +30 dB raise T
 *               by 10 dB, and the impulses are still 20 dB over it.
 *   Guard:      sample n is blanked iff some hit h of this push has h - pre <= n <= h + post, or n < carry_in.  carry_in is what the
 *               previous push's last hit still owes, max(0, h_last + post - (N_prev - 1)); 0 if that push had no hit, and for a first
 *               push.  The pre-guard does not reach back across a push boundary: those samples are already channelised.
 *   Effect:     a blanked sample enters the channeliser or the bank as exactly 0 + 0j, every other sample as exactly the value it has
 *               without the blanker; the filter history taken from a previous push is the blanked stream.  (cu8 has no byte that means
 *               zero, so the device keeps a blanked stream as cs16: cu8 (2u - 255) . 128, cs8 s . 256 - the same real numbers, each
 *               within int16 - which msk144_dump_wideband_blanked returns.)
 *   Parameters: 16 <= threshold_q4 <= 65535 (the power ratio to the mean in 1/16), 0 <= pre, post <= 4096.  Defaults 256 / 2 / 8: 16 x
 *               the mean power, which complex Gaussian noise exceeds with probability e^-16, about 1.1e-7, per sample.  The defaults
 *               are design parameters, not measurements.
 *   Order:      msk144_set_wideband_blanker(h, &p) sets the blanker, (h, NULL) switches it off; either takes effect at the next first
 *               push (stream restart).  A running stream keeps what it started with, so the same stream pushed twice gives the same
 *               bytes.  msk144_set_wideband resets the blanker to off.  With none of these entries called, every hop, clip count,
 *               level and decode is what it is without them.
 *   Refused:    MSK144_EINVAL outside wideband mode and for parameters out of range. */
typedef struct msk144_wideband_blanker
{
    int32_t threshold_q4; /* 16 x the power ratio to the push's mean power (256) */
    int32_t pre, post;    /* samples blanked ahead of and behind every hit (2, 8) */
} msk144_wideband_blanker;

typedef struct msk144_wideband_blanker_counts
{
    /* the last push */
    int64_t samples;    /* N */
    int64_t sum_power;  /* S */
    int64_t threshold;  /* T */
    int64_t hits;
    int64_t blanked;    /* samples zeroed, those owed by the push before included */
    int64_t carry_out;  /* guard samples its last hit owes to the next push */
    /* since the first push */
    int64_t total_samples, total_hits, total_blanked;
} msk144_wideband_blanker_counts;

/* NULL: off */
int msk144_set_wideband_blanker(msk144_handle* h, const msk144_wideband_blanker* p);
/* synchronises like msk144_wideband_levels.  MSK144_ESTATE before any push, and while the running stream has no blanker */
int msk144_wideband_blanker_stats(msk144_handle* h, msk144_wideband_blanker_counts* out);
/* test and debug, like msk144_dump_wideband_hop: the N new samples of the last push as the channeliser (or the bank) saw them, cs16 I,Q
 * pairs.  MSK144_ESTATE as above */
int msk144_dump_wideband_blanked(msk144_handle* h, int16_t* out);

/* ---- Power spectrum of the input stream (no reference counterpart) ----
 *
 * Where in the band the energy lies - the tuner's ppm error against the grid, the birdie that drives one channel's AGC down, the
 * distance of the noise floor from full scale, what the blanker did to the floor - is what every SDR front end shows as a spectrum.
 * The whole stream is on the device at Fs, so the spectrum of a push is computed there, from one more read of its samples.
 *
 *   Input:      the N new samples x[0..N) of a push (N = 5184 Fs/12000 for a first push, else 2592 Fs/12000) exactly as the
 *               channeliser (or stage 1 at a bank rate) reads them: the blanked stream when the running stream has a blanker, else
 *               the raw one; cu8 (u - 127.5)/128, cs8 s/128, cs16 s/32768, so full scale is 1.0.  The filter history is no part of it.
 *   Segments:   S = floor(N / B) segments of B = bins samples, not overlapped: segment s is x[sB .. sB + B - 1]; the last N mod B
 *               samples are not used, and nothing is carried from push to push: a push's spectrum is a pure function of its samples.
 *   Output:     X_s[k] = sum_i w[i] x[sB + i] e^{-j 2 pi i k / B},  P[k] = sum_s |X_s[k]|^2,  in ascending frequency: power[j] is bin
 *               k = (j - B/2) mod B, at (j - B/2) Fs / B Hz from the centre; *segments = S.  A full-scale complex tone on a bin centre
 *               reads S (sum w)^2: that is 0 dBFS, dBFS[j] = 10 log10(power[j] / (S (sum w)^2)).
 *   Window:     w[0..B) real and finite; NULL selects the periodic Hann window 0.5 - 0.5 cos(2 pi i / B)
 *               (msk144host_wideband_spectrum_window).  Formed in double, stored f32, as the taps are.
 *   Arithmetic: the transform and |X|^2 in f32, the sum over the segments in double.  Segments are assigned to workgroups and the
 *               partial sums added in a fixed order, without atomics: the same stream pushed twice gives the same bytes.
 *   Error:      against the exact P of the f32 window and samples, with T = sum_k P[k]:
 *                   |power[k] - P[k]| <= 2 u sqrt(P[k] T) + u^2 T + v P[k],   v = 4 x 2^-24 (the rounding of re^2 + im^2),
 *               u = MSK144_SPECTRUM_U the relative l2 error of one f32 transform (|dX_s[k]| <= ||dX_s||_2 <= u ||X_s||_2, then
 *               Cauchy-Schwarz over the segments): 4 x the largest value any bin needed on an MI355X against a float64 model over
 *               B = 256..8192 and the three formats (3.9e-8), rounded up; far below the textbook ceiling 8 x 2^-24 x log2 B.
 *   Parameters: bins a power of two, 256 <= bins <= 8192, and bins <= 2592 Fs/12000, so that every push has a segment.
 *   Order:      msk144_set_wideband_spectrum(h, &p) takes effect from the next push and allocates everything it needs - a push
 *               allocates nothing; (h, NULL) switches the spectrum off, as msk144_set_wideband does.  msk144_wideband_spectrum reports
 *               the last push and synchronises like msk144_wideband_levels.  With none of these entries called, every hop, clip
 *               count, level, blanker statistic and decode is byte for byte what it is without them.
 *   Refused:    MSK144_EINVAL outside wideband mode, for bins not a power of two, out of range or longer than a later push, and for a
 *               window value that is not finite; MSK144_ESTATE from msk144_wideband_spectrum before any push made with the spectrum on. */
#define MSK144_SPECTRUM_U 2e-7
/* (a typedef and a function share C's one name space, so the structure cannot be called msk144_wideband_spectrum as well) */
typedef struct msk144_wideband_spectrum_params
{
    int32_t bins;          /* B (1024 is what the program and the Python view default to) */
    const double* window;  /* [bins], or NULL: periodic Hann */
} msk144_wideband_spectrum_params;

/* NULL: off */
int msk144_set_wideband_spectrum(msk144_handle* h, const msk144_wideband_spectrum_params* p);
int msk144_wideband_spectrum(msk144_handle* h, double* power /*[bins]*/, int64_t* segments);

/* ---- Per-channel ping detection (no reference counterpart) ----
 *
 * What a meteor-scatter operator looks for first is whether, when and where something burst out of the noise; a decode line appears
 * only when a ping was long and strong enough to decode.  Every channel's int8 hop sits on the device right behind the channeliser,
 * so a short-time energy profile per channel and an integer detection rule are evaluated there, and the program turns the reports
 * into an event log.  The detector only reads the staged hops.  Everything below is per channel and per push, in integers.
 *
 *   Input:      the int8 I/Q values of the channel's push exactly as stored, what msk144_dump_wideband_hop returns: M = 5184 after a
 *               first push, else 2592.
 *   Blocks:     one block is B = 96 samples, 8 ms (a 72 ms MSK144 frame is 9 blocks); nb = M / 96 is 54 or 27.
 *               E[b] = sum of I*I + Q*Q over samples 96b .. 96b + 95, at most 96 . 2 . 128^2 = 3145728 < 2^22.
 *   Quiet:      q = the value at rank floor(nb / 4), counted from 0, of E sorted in ascending order (rank 6 of 27, rank 13 of 54): a
 *               lower quartile, which a ping of up to about 3/4 of a push does not move.
 *   Reference:  R = max(min(q, the q of the last h earlier pushes of this stream), min_ref), h = min(memory, pushes since the history
 *               last restarted).  The history restarts at a first push, at the first push after msk144_set_wideband_pings, and at any
 *               push whose quantiser scale differs from the previous push's - the f32 `gain` msk144_wideband_levels reports for the
 *               push, compared for equality - so that an AGC step or new gains restart the memory instead of rescaling it.
 *   Up:         block b is up iff E[b] . 16 > R . ratio_q4, strictly, in 64-bit arithmetic (csrc/wideband.h ping_up).
 *   Parameters: 16 <= ratio_q4 <= 65535 (default 32: 2.0 x the reference), 0 <= memory <= 16 pushes (default 8, about 1.7 s of hops),
 *               1 <= min_ref <= 2^22 (default 96: a mean of 1 LSB^2 per sample; below it the channel is under-driven and R is held
 *               there).  The defaults are design parameters, not measurements.
 *   Sensitivity: this is a strong-ping detector, less sensitive than the decoder.  A ping at S dB in 2500 Hz lifts a 12 kHz channel by
 *               1 + 10^(S/10) . 2500/12000, so the defaults see pings from roughly +7 dB up.  In a CPU simulation of the model (no
 *               GPU measurement stands behind these figures) white int8 noise at 3 and at 20 LSB rms, 1.66 M blocks each with memory
 *               8, put 0 blocks up at ratio 2.0, 2-3 at 1.75 and about 2600 at 1.5; in a 240 ksps scene with noise at about 20 LSB rms
 *               every block wholly inside a +10 dB ping was up, most at +7 dB, almost none at +4 dB.  The ping band below
 *               (msk144_set_wideband_ping_band) compares in-band energy instead and sees pings some 2.5 to 3 dB weaker.
 *   Events:     the program (and wideband.PingEvents) joins up blocks into events: with g = (blocks of all earlier pushes) + b, an
 *               event is a maximal run of consecutive up blocks in g; a run that reaches a push's last block stays open into the
 *               next push, a history restart does not close it, the end of the stream does (csrc/wideband.h PingTracker).
 *   Order:      msk144_set_wideband_pings(h, &p) switches the detector on from the next push and allocates everything it needs - a
 *               push allocates nothing; (h, NULL) switches it off, as msk144_set_wideband does.  msk144_wideband_pings reports the last
 *               push and synchronises like msk144_wideband_levels.  The same stream pushed twice gives the same bytes: a first push
 *               clears the history.  Whether the detector is on or off, every hop, clip count, level, AGC step, blanker statistic,
 *               spectrum and decode is byte for byte the same.
 *   Refused:    MSK144_EINVAL outside wideband mode and for parameters out of range; MSK144_ESTATE from either read entry before a
 *               push made with the detector on. */
typedef struct msk144_wideband_ping
{
    uint64_t up_mask;   /* bit b is set iff block b is up */
    int32_t blocks;     /* nb */
    int32_t history;    /* h, the number of earlier pushes R drew on */
    int32_t quiet;      /* q */
    int32_t reference;  /* R */
    int32_t peak;       /* max E */
    int32_t peak_block; /* the lowest b at the maximum */
} msk144_wideband_ping;

typedef struct msk144_wideband_pings_params
{
    int32_t ratio_q4; /* 16 x the ratio to the reference (32) */
    int32_t memory;   /* earlier pushes whose quiet level bounds the reference (8) */
    int32_t min_ref;  /* floor of the reference (96) */
} msk144_wideband_pings_params;

#define MSK144_PING_MAX_BLOCKS 54

/* NULL: off */
int msk144_set_wideband_pings(msk144_handle* h, const msk144_wideband_pings_params* p);
/* out[channels]: the last push */
int msk144_wideband_pings(msk144_handle* h, msk144_wideband_ping* out);
/* test and debug, like msk144_dump_wideband_hop: E of the channel's last push in energies[0 .. *n), energies[54]; the rest is 0.
 * channel = -1: every channel's, energies[channels][54] (what the program's event log reads, in one copy) */
int msk144_wideband_ping_blocks(msk144_handle* h, int32_t channel, int32_t* energies, int32_t* n);

/* ---- The ping band: an in-band filter ahead of the ping detector's block energies (no reference counterpart) ----
 *
 * E above is the energy of a whole 12 kHz channel; an MSK144 signal fills about 2.4 kHz of it.  With the band on, a 64-tap complex
 * band-pass runs on the stored int8 values ahead of the block energies, and the detector - quiet level, reference, up mask, peak -
 * runs unchanged on the in-band energies Ef.  Exact integer arithmetic throughout (csrc/pingband.hip; the same rule on the host is
 * csrc/wideband.h ping_band_energies).  Per channel, with x[n] = I + jQ the stored int8 values as integers:
 *
 *   Taps:       64 complex int8 taps b[k] = (br[k], bi[k]), k = 0..63; any int8 values are valid, a shorter filter is zero-padded.
 *   Filter:     z[n] = sum over k < 64 of b[k] . x[n - k], a complex integer product; |Re z| and |Im z| are at most
 *               128 . 64 . 2 . 128 = 2^21, so int32 is exact.
 *   Tail:       x[n - k] reaches into the channel's previous 63 stored samples, which the filter keeps per channel on the device.
 *               The tail is all zero whenever the ping history restarts by order of the library: at a first push, and at the first
 *               push after msk144_set_wideband_pings or msk144_set_wideband_ping_band.  A change of quantiser scale (an AGC step, new
 *               gains) restarts the reference history but not the tail: it holds the stored values as they are.  The tail advances
 *               only on pushes made with the detector and the band both on.
 *   Energy:     Ef[b] = min((sum over samples 96b .. 96b + 95 of Re z^2 + Im z^2) >> shift, 2^22 - 1), 0 <= shift <= 40.  The sum is
 *               below 2^50; the clamp keeps Ef inside the 22 bits of E.
 *   Use:        with the band on, Ef stands for E everywhere in the ping contract above: msk144_wideband_ping_blocks returns Ef,
 *               msk144_wideband_ping keeps its layout (quiet, reference and peak are then in-band), the events, the frequency of a
 *               ping, the waterfall's `pings` mode and the capture follow the same up masks.
 *   Default design (msk144host_wideband_ping_band_design in libmsk144host.so, csrc/wideband.h ping_band_design; the program and the
 *               Python side both take it from there): integer centre_hz and 500 <= halfwidth_hz <= 3000 with
 *               |centre_hz| + halfwidth_hz <= 6000.  In double: a Hamming-windowed sinc low-pass with cutoff halfwidth_hz centred on
 *               k = 31.5, turned by e^{+j 2 pi centre (k - 31.5) / 12000}, scaled so that the largest |component| is 127, rounded
 *               with rint.  shift = rint(log2 |B(centre)|^2), B the response of the rounded taps, so that a signal inside the band
 *               comes out near the level it went in with and min_ref keeps its meaning.
 *   Ratio:      Ef has about a quarter of E's degrees of freedom per block, so noise alone swings it further and the ratio must rise
 *               with the band on.  In a CPU simulation of the model (tools/pingband_sim.py; no GPU measurement stands behind these
 *               figures), set up as the one above - white int8 noise at 3 and at 20 LSB rms, 1.66 M blocks each, memory 8 - and with
 *               the default band, the blocks up were 14375 and 13813 at ratio 2.0, 232 and 206 at 2.5, 17 and 18 at 2.75, 2 and 0 at
 *               3.0, 0 and 0 at 3.25 and above.  MSK144_PING_BAND_RATIO_Q4 = 52, ratio 3.25, the smallest multiple of 0.25 with no
 *               block up in either, is the default the program uses with the band on.
 *   Sensitivity: CPU simulation again, the 240 ksps scene of the ping detector's paragraph with synthesised MSK144 pings through the
 *               float64 channeliser model, eight seeds, 552 blocks wholly inside a ping.  Share of them up, whole channel at ratio
 *               2.0 / default band at 3.25: +10 dB 100 / 100 %, +7 dB 86.1 / 100 %, +4 dB 2.2 / 74.1 %, +2 dB 0 / 14.1 %, 0 dB 0 / 1.1 %
 *               (+6 dB 42.9 / 99.8 %, +5 dB 12.9 / 94.9 %, +3 dB 0 / 37.9 %); no block away from a ping was up in either.  Half the
 *               blocks are up at about +6.2 dB without and +3.4 dB with the band: a gain of 2.5 to 3 dB, less than the 6 dB of the
 *               bandwidth ratio because of the higher ratio.
 *   Order:      msk144_set_wideband_ping_band(h, &p) takes effect from the next push, allocates everything it needs - a push
 *               allocates nothing - and restarts the ping history; (h, NULL) switches the band off, likewise from the next push and
 *               with a restart, as msk144_set_wideband does.  It is valid in wideband mode whether or not the detector is on and acts
 *               only on pushes made with the detector on; msk144_set_wideband_pings(h, NULL) leaves it configured.  No atomics: the
 *               same stream pushed twice gives the same bytes.  Whether the band is on or off, every hop, clip count, level, AGC
 *               step, blanker statistic, spectrum, waterfall row of a listed channel and decode is byte for byte the same.
 *   Refused:    MSK144_EINVAL outside wideband mode and for shift outside 0..40. */
typedef struct msk144_wideband_ping_band_params
{
    int8_t taps[64][2]; /* (br, bi) of b[0] .. b[63] */
    int32_t shift;
} msk144_wideband_ping_band_params;

#define MSK144_PING_BAND_RATIO_Q4 52

/* NULL: off */
int msk144_set_wideband_ping_band(msk144_handle* h, const msk144_wideband_ping_band_params* p);

/* ---- Per-channel waterfall (no reference counterpart) ----
 *
 * Levels, the input spectrum and the ping detector do not show what is inside a 12 kHz channel: where in the channel a ping sat,
 * whether a steady carrier sits in the passband, what a ping looked like in time x frequency.  At bank rates a bin of the input
 * spectrum is wider than that.  Every channel's int8 hop sits on the device behind the channeliser, so the short-time spectra of
 * all channels are one more read of the staged hops and one small transform per 8 ms block.  The waterfall only reads the hops: it is
 * a display and a per-event frequency estimate at 125 Hz resolution from 8 ms blocks, and does not feed the decoder.
 *
 *   Input:      the int8 I/Q values of the channel's push exactly as stored, what msk144_dump_wideband_hop returns, taken as
 *               integers x = I + jQ in LSB: M = 5184 after a first push, else 2592.
 *   Rows:       one row per block of the ping detector: B = 96 samples, nb = M / 96 = 54 or 27, row b covers samples 96b .. 96b + 95
 *               (block b of msk144_wideband_ping is row b).  Nothing is carried from push to push: a push's rows are a pure
 *               function of its hops.
 *   Output:     X_b[k] = sum_{i<96} w[i] x[96b + i] e^{-j 2 pi i k / 96},  P_b[k] = |X_b[k]|^2, in ascending frequency: rows[b][j] is
 *               bin k = (j - 48) mod 96, at (j - 48) x 125 Hz from the channel's offset.
 *   Window:     w[0..96) real and finite; NULL selects the periodic Hann window 0.5 - 0.5 cos(2 pi i / 96)
 *               (msk144host_wideband_waterfall_window).  Formed in double, stored f32, as the spectrum's window and the taps are.
 *   Scale:      a tone of amplitude A LSB on a bin centre reads (A sum w)^2; the program's 0 dB is A = 1:
 *               dB = 10 log10(max(P / (sum w)^2, 1e-10)), the sum taken over the f32 window.
 *   Sums:       sums[c][j] = sum_b (double) rows[c][b][j] over the f32 values actually stored, b ascending, added one after another
 *               in double.
 *   Arithmetic: the transform and |X|^2 in f32; no atomics and a fixed order everywhere: the same stream pushed twice gives the
 *               same bytes in rows and sums.
 *   Error:      per row, against the exact P_b of the f32 window and the integer samples, with T_b = sum_k P_b[k]:
 *                   |rows[b][j] - P_b[k]| <= 2 u sqrt(P_b[k] T_b) + u^2 T_b + v P_b[k],   v = 4 x 2^-24 (the rounding of re^2 + im^2),
 *               u = MSK144_WATERFALL_U: 4 x the largest value any row needed on an MI355X against a float64 model over 1 .. 130
 *               channels, cu8 and cs16, the Hann, an all-ones and a random window, silence and all-clipped hops (6.9e-7),
 *               rounded up to one significant digit; below the worst case of a 96-term f32 sum with rounded twiddles and window,
 *               98 x 2^-24 = 5.8e-6.
 *   Order:      msk144_set_wideband_waterfall(h, &p) takes effect from the next push and allocates everything a push needs - a push
 *               allocates nothing; (h, NULL) switches it off, as msk144_set_wideband does.  The read entries report the last push and
 *               synchronise like msk144_wideband_levels.  Whether the waterfall is on or off, every hop, clip count, level, AGC
 *               step, blanker statistic, spectrum, ping record and decode is byte for byte the same.
 *   Refused:    MSK144_EINVAL outside wideband mode, for a window value that is not finite and for a channel outside
 *               -1 .. channels - 1; MSK144_ESTATE from the read entries before a push made with the waterfall on. */
#define MSK144_WATERFALL_BINS 96
#define MSK144_WATERFALL_U 3e-6 /* largest needed: 6.9e-7 */
typedef struct msk144_wideband_waterfall_params
{
    const double* window; /* [96], or NULL: periodic Hann */
} msk144_wideband_waterfall_params;

/* NULL: off */
int msk144_set_wideband_waterfall(msk144_handle* h, const msk144_wideband_waterfall_params* p);
/* rows[54][96] of the channel's last push, *n = nb of them, the rows past *n are 0; channel = -1: every channel's, rows[channels][54][96] */
int msk144_wideband_waterfall(msk144_handle* h, int32_t channel, float* rows, int32_t* n);
/* sums[channels][96] of the last push */
int msk144_wideband_waterfall_sums(msk144_handle* h, double* sums);

/* ---- The notch: steady carriers taken out of a channel (no reference counterpart) ----
 *
 * A spur of the SDR, a birdie or a beacon inside a channel's 2.4 kHz band goes straight into the decoder's int8 I/Q and costs
 * decodes.  With a notch on a channel, a 64-tap complex band-pass estimates the carriers from the stored int8 values and the stage
 * takes the estimate from the delayed input.  Exact integer arithmetic throughout (csrc/notch.hip; the same rule on the host is
 * csrc/wideband.h notch_filter).  Per notched channel, with x[n] = I + jQ the stored int8 values as integers, in stream order:
 *
 *   Taps:       64 complex int8 taps b[k] = (br[k], bi[k]), k = 0..63, and a shift s, 0 <= s <= 15; any int8 values are valid.
 *   Filter:     z[n] = sum over k < 64 of b[k] . x[n - k], in int32 as the ping band's z;
 *               y[n] = sat8(((x[n - 31] << s) - z[n] + r) >> s) per component, r = s ? 1 << (s - 1) : 0, the shift right an
 *               arithmetic shift of int32, sat8 a clamp to -128..127.  y replaces x in the staged rows.
 *   Delay:      the output is the input delayed by 31 samples (2.6 ms) minus the band-passed estimate of the carriers.  The delay
 *               is part of the contract: a notched channel's pings, waterfall rows and decode times lie 31 samples late.
 *   Tail:       x[n - k] reaches into the channel's previous 63 raw (pre-notch) stored samples, which the stage keeps per channel
 *               on the device.  x before the channel's first filtered sample is 0: the tail is all zero at a first push, and on
 *               the next push of a channel whose entry is new or differs from the one it had.  A channel whose entry is unchanged
 *               by a new table keeps its tail.
 *   Place:      directly behind the channeliser and the AGC step, ahead of everything that reads the staged hops.  So
 *               msk144_dump_wideband_hop, the ping band, the pings, the waterfall, the hop ring, the capture and the decode all
 *               see the notched channel; msk144_wideband_levels and the clip count stay the channeliser's own, so that the AGC
 *               keeps acting on the level with the carrier in it.  The channels not in the table are not touched.
 *   Default design (msk144host_wideband_notch_design in libmsk144host.so, csrc/wideband.h notch_design; the Python side takes it
 *               from there): 1 or 2 integer frequencies per channel, relative to the channel's offset, 50 <= halfwidth_hz <= 500
 *               (default 100), |f| + halfwidth_hz <= 6000, two frequencies at least 1000 Hz apart (closer ones over-subtract in a
 *               CPU check, because the two pass bands add).  In double: a 63-tap Hamming-windowed sinc low-pass with cutoff
 *               halfwidth_hz centred on k = 31, scaled to unit DC gain, turned by e^{+j 2 pi f (k - 31) / 12000} to each frequency
 *               and summed; s = min(15, floor(log2(127 / largest |component|))), taps rint(value x 2^s), tap 63 = 0.  In a CPU
 *               check of the rounded default design (W = 100) a component 62 Hz from the notch comes out 23.0 dB down, one 400 Hz
 *               away 0.1 dB down.
 *   Cost:       CPU simulation with the reference decoder on synthetic int8 windows (no GPU measurement stands behind these
 *               figures; DESIGN 4.4 has the table): the notch recovers nearly every decode a carrier takes away (+6 dB pings, two
 *               tones of 50 LSB: 5 of 24 decoded without, 24 of 24 with), and costs sensitivity on a weak ping where there is no
 *               carrier (0 dB, no carrier: 24 of 24 without, 21 of 24 with).  Hence per channel, and only where a carrier sits.
 *   Order:      msk144_set_wideband_notch(h, channels, count, params) replaces the whole table from the next push on and allocates
 *               everything it needs - a push allocates nothing; count = 0 or channels = NULL switches the notch off, as
 *               msk144_set_wideband does.  With no channel notched a push launches nothing.  No atomics: the same stream pushed
 *               twice gives the same bytes.  msk144_wideband_notch_stats reports the last push - on[c] and the components of it
 *               that sat8 clamped - and synchronises like msk144_wideband_levels.
 *   Refused:    MSK144_EINVAL outside wideband mode, for a channel listed twice or out of range, for count outside 0..channels,
 *               for a missing params and for a shift outside 0..15; MSK144_ESTATE from msk144_wideband_notch_stats before a push
 *               made with the notch on since the table was last set. */
typedef struct msk144_wideband_notch_params
{
    int8_t taps[64][2]; /* (br, bi) of b[0] .. b[63] */
    int32_t shift;
} msk144_wideband_notch_params;

typedef struct msk144_wideband_notch_count
{
    int32_t on;      /* 1: the channel was notched in the last push */
    int32_t clipped; /* components of the last push that sat8 clamped */
} msk144_wideband_notch_count;

#define MSK144_NOTCH_DELAY 31

/* params[count], one per listed channel; count = 0 or channels = NULL: off */
int msk144_set_wideband_notch(msk144_handle* h, const int32_t* channels, int32_t count, const msk144_wideband_notch_params* params);
/* out[channels]: the last push */
int msk144_wideband_notch_stats(msk144_handle* h, msk144_wideband_notch_count* out);

/* ---- Per-ping capture of a channel's hops, for replay (no reference counterpart) ----
 *
 * A ping that did not decode is gone 216 ms later, when the hop ring advances.  Every channel's 12 ksps int8 I/Q stream - exactly
 * what a read_mode 2 handle, or msk144hipdecoder --read-mode=2, reads - sits on the device behind the channeliser, and the ring
 * also holds the hop before the newest one.  The capture picks the few (channel, hop) pairs worth keeping, packs them densely on the
 * device and hands the host only those bytes: a quiet band costs a 16-byte header, a busy one 5184 bytes per kept hop.  The
 * capture only reads the ping records and the ring.
 *
 *   Input:      per channel c, the ping record of every push (msk144_wideband_pings; all zero while the detector is off) and the
 *               channel's ring window behind the push.  A stream's hops are numbered k = 0, 1, 2, ...: the first push carries hops
 *               0 and 1, the p-th later push hop p + 1.  One hop is 2592 int8 I/Q pairs, 5184 bytes: one unit.
 *   Rule:       a(k) = 1 iff the record of the push that carried hop k has an up block among hop k's 27 (first push: bits 0..26 are
 *               hop 0, bits 27..53 hop 1; later push: bits 0..26).  L = c is in the list.
 *               W(k) = L, or a(j) = 1 for some max(0, k - post) <= j <= k: active, within `post` hops after activity, or listed.
 *               P(k) = pre = 1 and not W(k) and a(k + 1) = 1: the one hop of pre-roll the ring holds.
 *               Hop k is emitted in the push that carries k if W(k), in the push that carries k + 1 if P(k) (for k = 0 both are the
 *               first push), otherwise never; no hop is emitted twice.  csrc/wideband.h capture_step is the rule for device and host.
 *   Parameters: pre 0 or 1 (default 1), 0 <= post <= 16 hops (default 1), 1 <= max_units <= 16384, up to 16 listed channels.  The
 *               defaults are design parameters, not measurements.
 *   Order:      a push's units come by channel ascending, then by hop ascending.  Of `total` units the first min(total, max_units)
 *               are stored, the rest dropped and only counted; the rule never depends on what was dropped.  The state is per
 *               channel - hops since the last active one, saturating, and whether the newest hop was emitted.  A first push clears
 *               it: the same stream pushed twice gives the same bytes.  msk144_set_wideband_capture(h, &p) takes effect from the
 *               next push, allocates everything - a push allocates nothing - and clears the state as well: activity before it counts
 *               as none, and the pre-roll hop is used when the stream already has one.  (h, NULL) switches capture off, as
 *               msk144_set_wideband does.  With capture off a push issues the calls it issues without it; on or off, every hop,
 *               clip count, level, AGC step, blanker statistic, spectrum, ping record, waterfall row and decode is byte for byte the
 *               same.
 *   Output:     msk144_wideband_capture reports the last push and synchronises like msk144_wideband_levels: *count descriptors in
 *               units[], *count rows of 5184 bytes in data[] (nothing past them is written), *total = all units of the push.
 *               *count <= the max_units that push was made with, which is the last one set: every call of
 *               msk144_set_wideband_capture that is accepted, (h, NULL) too, ends the last push's units, and the read entry answers
 *               MSK144_ESTATE until the next push made with capture on.  So buffers for the max_units last set always suffice.
 *               A larger max_units than any set before frees the device rows and allocates larger ones; a smaller one keeps them.
 *               A unit's bytes are the bytes msk144_dump_wideband_hop returned for that hop in the push that carried it.
 *               flags: bit 0 a(k); bit 1 L; bit 2 emitted as P(k), one push late; bit 3 tail: not active, but within `post` hops
 *               after activity.
 *   Refused:    MSK144_EINVAL outside wideband mode, for parameters out of range and for a listed channel that is out of range or
 *               repeated (a refused call changes nothing); MSK144_ESTATE from msk144_wideband_capture before a push made with capture
 *               on, and between an accepted msk144_set_wideband_capture and the next such push. */
#define MSK144_CAPTURE_UNIT_BYTES 5184
typedef struct msk144_wideband_capture_params
{
    int32_t pre;        /* hops of pre-roll, 0 or 1 (1) */
    int32_t post;       /* hops kept after the last active one (1) */
    int32_t max_units;  /* units stored per push; the program takes min(2 x channels, 512) */
    int32_t num_listed; /* channels captured whether active or not */
    int32_t listed[16];
} msk144_wideband_capture_params;

typedef struct msk144_wideband_capture_unit
{
    int32_t channel;
    int32_t flags; /* bit 0 active, 1 listed, 2 pre-roll, 3 tail */
    int64_t hop;   /* k */
} msk144_wideband_capture_unit;

/* NULL: off */
int msk144_set_wideband_capture(msk144_handle* h, const msk144_wideband_capture_params* p);
/* units[max_units], data[max_units][5184], max_units as last set: the last push, made since then */
int msk144_wideband_capture(msk144_handle* h, msk144_wideband_capture_unit* units, int8_t* data /*[max_units][5184]*/, int32_t* count, int32_t* total);

/* ---- Each captured hop as 12 kHz audio (no reference counterpart) ----
 *
 * The capture's units are complex int8 I/Q, which only a read_mode 2 handle reads back.  What the rest of the MSK144 world takes -
 * WSJT-X's File > Open, the reference's default read mode, this library's own audio front end - is real 16-bit audio at 12000
 * samples per second with the signal around 1500 Hz.  With the audio on, a 64-tap complex band-pass runs on every channel's stored
 * int8 values, a 96-entry integer phasor table takes the result to a real tone frequency, and the audio of the capture's units can be
 * read beside them.  Exact integer arithmetic throughout (csrc/audio.hip; the same rule on the host is csrc/wideband.h audio_push).
 * Per channel, with x[n] = I + jQ the stored int8 values as integers - what msk144_dump_wideband_hop returns, behind the notch - and
 * n counted from the stream's first stored sample:
 *
 *   Filter:     z[n] = sum over k < 64 of b[k] . x[n - k], the ping band's filter: |Re z|, |Im z| <= 2^21, int32 is exact.
 *   Mix:        a[n] = Re z[n] . pr[n mod 96] - Im z[n] . pi[n mod 96] in int64, |a| <= 2^37: the real part of z[n] w[n mod 96].
 *               A hop is 2592 = 27 x 96 samples, so n mod 96 is the index inside the hop mod 96, and there is no phase state.
 *   Output:     y[n] = clamp((a[n] + 2^(shift - 1)) >> shift, -32768, 32767), 1 <= shift <= 40, the shift right an arithmetic
 *               shift (floor).  `clamped` counts the samples of a hop that the clamp changed.
 *   Tail:       x[n - k] reaches into the channel's previous 63 stored samples, kept per channel on the device as the ping band's.
 *               A first push starts from an all-zero tail and filters hops 0 and 1.  The first push after an accepted
 *               msk144_set_wideband_audio starts from an all-zero tail as well and filters both hops the ring window then holds,
 *               the hop before the newest and then the newest, so that every unit a push can emit, the pre-roll unit included, has
 *               audio.  Every other push filters its newest hop and continues the tail.  A change of gain or an AGC step does not
 *               touch the tail.
 *   Ring:       the audio of hop k lies in slot k & 1 of a device ring [channels][2][2592] int16, with its clamp count beside it;
 *               written on every push made with the audio on, whether or not the capture is on.
 *   Read:       msk144_wideband_capture_audio reports the last push and synchronises like msk144_wideband_capture.  Row u is the
 *               audio of unit u of msk144_wideband_capture for that push - the same count, order and drop rule - and clamped[u]
 *               that hop's count.  Nothing past row *count - 1 is written.
 *   Delay:      the filter's group delay of 31.5 samples (2.6 ms): the audio lags the unit's I/Q by that much.
 *   Default design (msk144host_wideband_audio_design in libmsk144host.so, csrc/wideband.h audio_design; the program and the Python
 *               side both take it from there): the taps of the ping band's design for (centre_hz, halfwidth_hz);
 *               w[m] = (rint(16384 cos t), rint(16384 sin t)), t = 2 pi (tone_hz - centre_hz) m / 12000;
 *               shift = rint(log2 |B(centre)| + 6), B the response of the rounded taps.  A tone of amplitude A at f inside the band
 *               comes out at tone + (f - centre) Hz with amplitude near 256 A: an int8 full scale maps near an int16 full scale.
 *               The figure 256 is a design parameter, not a measurement.  500 <= halfwidth <= 3000, |centre| + halfwidth <= 6000,
 *               halfwidth <= tone <= 6000 - halfwidth, and tone - centre a multiple of 125 Hz, because the table has 96 entries.
 *               Defaults: halfwidth 1250, centre 0, tone 1500 (the program takes --center-frequency as the centre).  The band's
 *               skirt reaches the stop band about 310 Hz outside the half-width; with halfwidth > tone - 310 part of the skirt
 *               folds over 0 Hz, which is the caller's choice.  In a CPU check of the integer model (no GPU measurement stands
 *               behind these figures, nor behind the default half-width) tones inside the band came out within +0.7 .. +2.4 dB of
 *               256 A, and a tone 700 to 3500 Hz outside the band edge at least 36.1 dB below it (tests/test_wideband_audio_model.py).
 *   Order:      msk144_set_wideband_audio(h, &p) takes effect from the next push and allocates everything it needs - a push
 *               allocates nothing; the dense rows follow the capture's max_units, and a larger one reallocates them in whichever
 *               `set` brings it.  (h, NULL) switches the audio off, as msk144_set_wideband does.  With the audio off a push issues
 *               the calls it issues without it; on or off, every hop, level, ping record, capture unit and decode is byte for byte
 *               the same.  No atomics: the same stream pushed twice gives the same bytes.
 *   Refused:    MSK144_EINVAL outside wideband mode and for a shift outside 1..40 (a refused call changes nothing);
 *               MSK144_ESTATE from msk144_wideband_capture_audio wherever msk144_wideband_capture answers it, and when the last
 *               push was made without the audio. */
#define MSK144_AUDIO_PHASORS 96
typedef struct msk144_wideband_audio_params
{
    int8_t taps[64][2];    /* (br, bi) of b[0] .. b[63]; any int8 values are valid */
    int16_t phasor[96][2]; /* (pr, pi) of w[0] .. w[95]; any int16 values are valid */
    int32_t shift;         /* 1..40 */
} msk144_wideband_audio_params;

/* NULL: off */
int msk144_set_wideband_audio(msk144_handle* h, const msk144_wideband_audio_params* p);
/* audio[max_units][2592], clamped[max_units], max_units as last set for the capture: the last push, made since then */
int msk144_wideband_capture_audio(msk144_handle* h, int16_t* audio /*[max_units][2592]*/, int32_t* clamped /*[max_units]*/, int32_t* count);

/* ---- The gate: only the channels with activity are decoded (no reference counterpart) ----
 *
 * A meteor-scatter channel is noise for minutes and carries a ping for a fraction of a second, yet every channel's window goes
 * through scan, softbits and LDPC on every push.  With the gate on, the ping detector's up masks pick the channels whose window is
 * decoded, on the device; the decode then runs on those alone.  The channeliser, AGC, notch, ping detector, waterfall, hop ring,
 * capture and the IQ front end run for every channel as without it, so levels, ping records, captures and the eight segment
 * powers of every channel are those of an ungated push.  The detector is less sensitive than the decoder: a ping
 * the detector does not see is not decoded.  An opt-in extra; with the gate off every byte is what it is without this entry.
 *
 *   Rule:       per channel `since`, the hops since the last active one, saturating at 17.  A push carries one hop (up_mask bits
 *               0..26), a first push hops 0 and 1 (bits 0..26 and 27..53), walked in that order.  A hop is active iff at least
 *               min_up of its 27 blocks are up; since = active ? 0 : min(since + 1, 17).  After the walk the channel's window is
 *               decoded iff always[c] or since <= hold.  A first push, and the first push after msk144_set_wideband_gate, start
 *               from since = 17.  up_mask is 0 while the detector is off: then only the `always` channels are decoded.  The window
 *               of push k covers hops k - 1 and k, so with hold >= 1 every window that contains an active hop is decoded, and no
 *               window is decoded because of activity more than `hold` hops old; hold = 0 decodes only windows whose newest hop is
 *               active.  csrc/wideband.h gate_step is the rule for device and host.
 *   Parameters: 0 <= hold <= 16 hops (default 1), 1 <= min_up <= 27 blocks (default 1), 1 <= max_channels <= channels or 0 = all,
 *               and an `always` flag per channel, any subset.  The defaults are design parameters, not measurements.
 *   Order:      the qualifying channels in ascending order.  Of `total` the first min(total, max_channels) are listed and decoded,
 *               the rest dropped and only counted; `since` moves the same for every channel either way.  On the stream: the plan
 *               behind the ping detector, its header and list to pinned memory, an event; then the hop ring, the capture and the
 *               front end; then the gather of the listed channels' analytic windows into a store of the gate's own.
 *               msk144_set_wideband_gate(h, &p, always) takes effect from the next push and allocates everything - a push
 *               allocates nothing; (h, NULL, NULL) switches the gate off, as msk144_set_wideband does.
 *   Decode:     msk144_decode_stages on a push made with the gate on waits for that event - the one host wait the gate adds: the
 *               decode's launches are sized by the count, and the hot kernels are given neither an indirection nor an early exit -
 *               and runs scan .. collect on `count` channels.  count = 0 launches nothing and leaves 0 records.  A record's channel
 *               is the position j in the list, as after msk144_push_hops; msk144_copy_count and the dumps are by position too.
 *               msk144_fetch_wait returns seg_power[channels][8] by channel, for all channels.
 *   Output:     msk144_wideband_gate reports the last push: channels_out[0 .. *count) the listed channels, *total all that
 *               qualified.  It waits for the gate's event only, not for the stream.
 *   Refused:    MSK144_EINVAL outside wideband mode and for parameters out of range (a refused call changes nothing);
 *               MSK144_ESTATE from msk144_wideband_gate before a push made with the gate on, and between an accepted
 *               msk144_set_wideband_gate and the next such push. */
typedef struct msk144_wideband_gate_params
{
    int32_t hold;          /* hops a channel stays in after its last active one (1) */
    int32_t min_up;        /* up blocks that make a hop active (1) */
    int32_t max_channels;  /* channels decoded per push; 0: all */
} msk144_wideband_gate_params;

/* params NULL: off.  always[channels], nonzero = decoded on every push, or NULL: none */
int msk144_set_wideband_gate(msk144_handle* h, const msk144_wideband_gate_params* params, const uint8_t* always);
/* channels_out[max_channels as last set; channels when 0]: the last push, made since then */
int msk144_wideband_gate(msk144_handle* h, int32_t* channels_out, int32_t* count, int32_t* total);

/* bank rates only: band k's (-32..32, a band some channel lies in) complex f32 samples s_k[n] of the last push, re,im interleaved:
 * 5184 x P/Q after a first push, else 2592 x P/Q, with P/Q the ratio of the sub-band rate Fs/32 to 12000 */
int msk144_dump_wideband_band(msk144_handle* h, int32_t band, float* out);

/* ---- Audio input at 24 to 192 kHz: a resampler in front of the hop ring (no reference counterpart) ----
 *
 * The reference reads int16 audio at 12000 samples per second and sends its users through `ffmpeg -ar 12000` first; sound cards
 * and SDR applications record at 48 kHz.  With an input rate set, a read_mode 1 handle takes every stream's hop at Fs and resamples
 * it to 12 kHz on the device, in exact integers, into the hop ring's staging - what msk144_push_hops would have been handed.  The hop
 * ring, the audio front end and the decode run unchanged.
 *
 *   Input:   real int16 samples per stream at Fs = 12000 x P/Q (lowest terms), Fs a multiple of 125 Hz, 24000 <= Fs <= 192000: Q
 *            divides 96, hence 2592.  A stream's first hop is 5184 x P/Q input samples, every later one 2592 x P/Q, whole numbers.
 *   Filter:  integer taps h[0..L), int16, L = K x P, 1 <= K <= 64, at the upsampled rate 12000 x P, and a shift s, 1 <= s <= 15.
 *            The default is s = 14 and h[k] = rint(2^14 d[k]), d the channel filter's Kaiser-sinc of msk144host_wideband_taps_rate(Fs, K)
 *            (it sums to Q), K = 16: msk144host_input_rate_taps(rate, K, out) in libmsk144host.so.  Read as h / 2^14 / Q the K = 16
 *            taps are flat within 0.1 dB to 4 kHz and at least 60 dB down from 8 kHz (a numpy evaluation of the integer taps, no
 *            measurement on the air stands behind it).
 *   Headroom: checked when the taps are set: every polyphase branch has sum_k |h[r + kQ]| <= 65535.  Then |acc| <= 65535 x 32768 =
 *            2^31 - 32768, the rounding term fits, and a 32-bit accumulator is exact for any int16 input.
 *   Output:  per stream, m counting output samples from the stream's first sample, n_m = floor(mP/Q), r_m = (mP) mod Q, x[n < 0] = 0:
 *                acc[m] = sum over k >= 0 with r_m + kQ < L of h[r_m + kQ] . x[n_m - k]            (exact, 32-bit)
 *                y[m]   = clamp((acc[m] + 2^(s-1)) >> s, -32768, 32767)                             (arithmetic shift: floor)
 *            - the wideband Q-branch formula at f_c = 0.  A value outside the int16 range is clamped and counted.  y[0..2591] goes
 *            to the first half and y[2592..5183] to the hop on a first hop, 2592 samples to the hop afterwards.
 *   Delay:   the filter delays the signal by (L - 1)/(2P) output samples: 8 at K = 16, 0.67 ms.
 *   State:   the stream's last H = ceil(L/Q) - 1 input samples, kept on the device; H is shorter than a hop.  A first hop starts from
 *            zero history.  Streams that a push does not list keep window and history.
 *
 *     msk144_set_input_rate(h, &p);                 resets every stream's history: each stream's next hop must be a first one, else
 *                                                   MSK144_ESTATE.  NULL switches the resampler off and frees what it held.
 *     msk144_rate_hop_slot(h, s, &hops, &first_halves, &streams, &is_first, &row);   the four pinned arrays of msk144_hop_slot with
 *                                                   rows of row = 2592 x P/Q int16; allocated at the first call after a `set`
 *     msk144_push_rate_hops(h, s, n);               the rules of msk144_push_hops: n listed streams, ascending.  H2D, resampler,
 *                                                   history, hop ring and front end on the handle's stream
 *     msk144_decode / msk144_fetch_async / msk144_fetch_wait   as after msk144_push_hops
 *
 * msk144_hop_slot / msk144_push_hops / msk144_submit_* stay what they are on such a handle and advance no history.
 * Stage times: MSK144_T_FRONTEND includes the resampler, MSK144_T_H2D its copy.
 * Refused: MSK144_EINVAL for a read_mode 2 handle (its input is complex int8 I/Q) or one in wideband mode, for 12000 Hz, a rate that
 * is no multiple of 125 Hz (the 44.1 kHz family) or outside 24000..192000, L not K x P with 1 <= K <= 64, a shift outside 1..15 and a
 * branch sum above 65535. */
typedef struct msk144_input_rate_params
{
    int64_t rate_hz;      /* Fs */
    int32_t shift;        /* s */
    int32_t num_taps;     /* L = K x P */
    const int16_t* taps;  /* h[0 .. num_taps) */
} msk144_input_rate_params;

/* NULL: off */
int msk144_set_input_rate(msk144_handle* h, const msk144_input_rate_params* params);
int msk144_rate_hop_slot(msk144_handle* h, int32_t slot, void** hops /*[channels][row]*/, void** first_halves /*[channels][row]*/, int32_t** streams /*[channels]*/,
                         uint8_t** is_first /*[channels]*/, int32_t* row_samples);
int msk144_push_rate_hops(msk144_handle* h, int32_t slot, int32_t n);
/* test and debug: the resampled samples of position j of the last msk144_push_rate_hops, *n = 5184 (a first hop) or 2592; out[5184].
 * They are read from the hop ring's staging: call it before the handle's next hop entry.  MSK144_ESTATE before any such push */
int msk144_dump_rate_hop(msk144_handle* h, int32_t j, int16_t* out, int32_t* n);
/* clamped outputs of every position of the last msk144_push_rate_hops; waits for it.  MSK144_ESTATE before any such push */
int msk144_input_rate_clamped(msk144_handle* h, int32_t* clamped /*[n of the last push]*/);
/* the same for pipelined callers, without a wait: the counts of the slot's last msk144_push_rate_hops, *n of them, in pinned memory the
 * handle owns.  The copy runs on the handle's stream right behind the resampler, so the counts are there once msk144_fetch_wait of
 * that hop has returned, and stay until the slot is pushed again.  MSK144_ESTATE before any such push on the slot */
int msk144_input_rate_slot_clamped(msk144_handle* h, int32_t slot, const int32_t** clamped, int32_t* n);

/* ---- Stream levels and pings: per-stream levels and a ping record of the audio hops (no reference counterpart) ----
 *
 * For the audio streams of msk144_push_hops and msk144_push_rate_hops the decoder reports decodes and nothing else: not whether a
 * stream is dead, clipping, far too quiet, or full of pings that did not decode.  With the option on, every push also leaves, per
 * listed position, the levels of its new samples and the record of the wideband ping detector run on their block energies.  read_mode
 * 1 handles only.  The arithmetic is csrc/stream_pings.h, the kernel csrc/stream_pings.hip, the Python model
 * msk144cudecoder_amd/stream_pings.py; all integers, nothing has a tolerance.
 *
 *   Input:    per listed position j of a push, for stream s = streams[j], the new 12 kHz int16 samples x of that push as the hop
 *             ring's staging holds them - behind the resampler when an input rate is set.  A later hop has 2592 samples, nb = 27
 *             blocks of 96; a first hop (is_first[j]) has 5184, nb = 54: the first-half row, then the hop row.
 *   Energy:   E[b] = min(2^22 - 1, (sum over n < 96 of x[96b + n]^2) >> shift).  The sum is exact: it reaches 96 x 2^30 and is
 *             kept in 64 bits.  shift is 0..24; the default 12 follows from the cap: audio of 30 to about 13 000 LSB rms stays inside
 *             the range, and at 30 LSB the quiet level is still about 17.  Louder audio saturates; the saturated blocks are counted.
 *   Rule:     the wideband ping detector's, unchanged (above; csrc/wideband.h ping_rank, ping_history_min, ping_reference, ping_up,
 *             ping_history_put), on E with the scale fixed at 1.0f: quiet level at rank nb/4, R = max(min(quiet, the quiet levels of
 *             the last `memory` pushes of the stream), min_ref), block b up iff E[b] x 16 > R x ratio_q4.  The record is
 *             msk144_wideband_ping.  ratio_q4, memory and min_ref have the ranges of msk144_set_wideband_pings; the default ratio
 *             3.5 x (ratio_q4 = 56) is the smallest multiple of 0.25 at which no block of band-limited noise was up in a run of the
 *             model (the table in csrc/stream_pings.h; a CPU simulation, nothing measured on the air).
 *   State:    one history per stream, indexed by stream number.  It restarts on the stream's is_first hop and on its first listed
 *             hop after msk144_set_stream_pings (msk144_set_input_rate forces first hops already).  Streams that a push does not
 *             list keep their state.
 *   Levels:   msk144_stream_level per position, exact integers over the same samples.  With an input rate set these are the
 *             levels of the resampled stream: clipping of the input at Fs is smeared by the filter, and the resampler's clamp count
 *             (msk144_input_rate_clamped) is a separate figure.
 *   Order:    msk144_set_stream_pings(h, &p) takes effect from the next push and allocates everything it needs - a push allocates
 *             nothing; (h, NULL) switches it off.  Never set, or switched off again, every launch, copy and record of a push is
 *             what it is without the option.  The kernel runs on the handle's stream behind the staging copy (and the resampler)
 *             and ahead of the hop ring; it reads the staging, never the ring; one copy on the same stream then takes records,
 *             levels and energies to pinned memory of the slot.  No atomics: the same hops give the same bytes.
 *             msk144_submit_* pushes carry whole windows: they leave no records and change no state.
 *   Refused:  MSK144_EINVAL on a read_mode 2 handle, on a handle in wideband mode and for parameters out of range; MSK144_ESTATE
 *             from the read entries while the option is off or before a push since the `set`.
 *   Not covered: read_mode 2 streams, a capture on these records, levels at the input rate, a band filter.  The gate on these
 *             records is the next section. */
typedef struct msk144_stream_level
{
    int64_t sum;               /* sum of x */
    int64_t sum_sq;            /* sum of x^2 */
    int32_t peak;              /* max |x|, 0..32768 */
    int32_t full_scale;        /* samples equal to 32767 or -32768 */
    int32_t samples;           /* 2592 or 5184 */
    int32_t saturated_blocks;  /* blocks whose E is the cap 2^22 - 1 */
} msk144_stream_level;

#define MSK144_STREAM_PINGS_RATIO_Q4 56
#define MSK144_STREAM_PINGS_SHIFT 12

typedef struct msk144_stream_pings_params
{
    int32_t ratio_q4;  /* 16..65535 (56) */
    int32_t memory;    /* 0..16 pushes (8) */
    int32_t min_ref;   /* 1..4194304 (96) */
    int32_t shift;     /* 0..24 (12) */
} msk144_stream_pings_params;

/* NULL: off */
int msk144_set_stream_pings(msk144_handle* h, const msk144_stream_pings_params* params);
/* records[channels], levels[channels]: the first *n, by position, of the last push; waits for it */
int msk144_stream_pings(msk144_handle* h, msk144_wideband_ping* records, msk144_stream_level* levels, int32_t* n);
/* out[54]: the block energies of position j of the last push, *nb = 27 or 54 of them, zeros behind; waits for it */
int msk144_stream_ping_blocks(msk144_handle* h, int32_t j, int32_t* out, int32_t* nb);
/* for pipelined callers, without a wait: records [*n], levels [*n] and energies [*n][54] of the slot's last push, in pinned memory
 * the handle owns.  The copy runs on the handle's stream right behind the kernel, so they are there once msk144_fetch_wait of that hop
 * has returned, and stay until the slot is pushed again.  MSK144_ESTATE before a push on the slot since the `set` */
int msk144_stream_pings_slot(msk144_handle* h, int32_t slot, const msk144_wideband_ping** records, const msk144_stream_level** levels, const int32_t** energies, int32_t* n);

/* ---- Stream gate: only the streams with activity are decoded (no reference counterpart) ----
 *
 * The wideband gate (above) for the audio streams of msk144_push_hops and msk144_push_rate_hops: a stream is noise for minutes and
 * carries a ping for a fraction of a second, yet every listed stream's window goes through scan, softbits and LDPC on every push.
 * With the stream gate on, the stream-ping records of a push pick the listed positions whose window is decoded, on the device; the
 * decode then runs on those alone.  Staging copy, resampler, stream pings, hop ring and the audio front end run for every listed
 * position as without it, so levels, ping records and the eight segment powers of every position are those of an ungated push.  The
 * detector is less sensitive than the decoder: a ping it does not see is not decoded.  read_mode 1 handles only.  An opt-in extra:
 * never set, or switched off again, every launch, copy and record of a push is what it is without this entry.  The rule is
 * csrc/stream_gate.h on csrc/wideband.h gate_step, the kernels csrc/stream_gate.hip, the Python model stream_pings.StreamGate.
 *
 *   Rule:       per listed position j of a push, s = streams[j].
 *               Mask: with ratio_q4 = 0, records[j].up_mask of the push's stream-ping record.  Otherwise bit b < records[j].blocks
 *               is E[j][b] . 16 > records[j].reference . ratio_q4 (ping_up) on the block energies and the reference the detector
 *               left for this push - the gate's own ratio, so that the log keeps a strict ratio while the gate triggers on a looser
 *               one (the table in csrc/stream_gate.h: a CPU simulation, nothing measured on the air).  While stream pings are off
 *               the mask is 0 whatever the ratio: then only the `always` streams are decoded.
 *               Step: the wideband gate's, unchanged, on since[s]: a later hop walks bits 0..26, a first hop (is_first[j]) hops 0 and 1,
 *               bits 0..26 and 27..53; a hop is active iff at least min_up of its 27 blocks are up; since = active ? 0 :
 *               min(since + 1, 17); the window is decoded iff always[s] or since <= hold.  A first hop, and the stream's first listed hop
 *               since msk144_set_stream_gate, start from since = 17.
 *   State:      `since` is indexed by stream number.  A stream that a push does not list keeps it: it had no hop, its window did
 *               not move.
 *   Parameters: 0 <= hold <= 16 hops (default 1), 1 <= min_up <= 27 blocks (default 1), 1 <= max_streams <= channels or 0 = all,
 *               ratio_q4 0 or 16..65535 (default 0: no new number), and an `always` flag per stream number, any subset.  hold and
 *               min_up are the wideband gate's design parameters, not measurements.
 *   Order:      the positions that are in, in ascending j.  Of `total` the first min(total, max_streams) are listed and decoded,
 *               the rest dropped and only counted; `since` moves the same for every position either way.  The header is {count,
 *               total, hop}, hop the number of gated pushes since the `set`, minus 1.  On the handle's stream: the staging copy, the
 *               resampler where one is set, the stream-pings kernel and its copy, the gate's mask where ratio_q4 != 0, the plan, one
 *               copy of header and list to the slot's pinned block, an event; then the hop ring and the front end for all n positions;
 *               then the gather of the listed positions' analytic windows into a store of the gate's own: max_streams rows, or
 *               `channels` rows when max_streams is 0, of 41 472 bytes each.  msk144_set_stream_gate allocates everything - a push
 *               allocates nothing - and takes effect from the next push; (h, NULL, NULL) switches the gate off.
 *   Decode:     msk144_decode_stages on such a push waits for that event - the one host wait the gate adds, as for the wideband
 *               gate - and runs scan .. collect on `count` windows.  count = 0 launches nothing and leaves 0 records.  A record's
 *               channel is its index i in the list: the caller maps index -> position -> stream.  msk144_copy_count,
 *               msk144_dump_analytic and the candidate dumps go by list index too.  msk144_fetch_wait returns seg_power[n][8] by
 *               position, for all n positions.  msk144_submit_* pushes carry whole windows: they are not gated and move no state.
 *   Refused:    MSK144_EINVAL on a read_mode 2 handle, on a handle in wideband mode and for parameters out of range (a refused call
 *               changes nothing, and a `set` that fails to allocate leaves the gate as it was); MSK144_ESTATE from the read entries
 *               while the gate is off, and between an accepted
 *               msk144_set_stream_gate and the next gated push (msk144_stream_gate_slot: the next one on that slot).
 *   Not covered: read_mode 2 streams, a capture, a band filter, skipping the front end of unlisted streams (their segment powers
 *               feed the SNR), rotating which streams are dropped over max_streams. */
typedef struct msk144_stream_gate_params
{
    int32_t hold;         /* hops a stream stays in after its last active one, 0..16 (1) */
    int32_t min_up;       /* up blocks that make a hop active, 1..27 (1) */
    int32_t max_streams;  /* stream windows decoded per push, 1..channels; 0: all */
    int32_t ratio_q4;     /* 0: the detector's own up mask; else 16..65535, the gate's own ratio (above) */
} msk144_stream_gate_params;

/* params NULL: off.  always[channels] BY STREAM NUMBER, nonzero = decoded on every push that lists the stream; NULL: none */
int msk144_set_stream_gate(msk144_handle* h, const msk144_stream_gate_params* params, const uint8_t* always);
/* the last push: positions_out[0 .. *count) the listed POSITIONS j (ascending), *total all that qualified; positions_out holds
 * max_streams as last set, channels when 0.  Waits for the gate's event only, not for the stream */
int msk144_stream_gate(msk144_handle* h, int32_t* positions_out, int32_t* count, int32_t* total);
/* pipelined callers, no wait: the slot's last push, in pinned memory the handle owns; valid once msk144_fetch_wait of that hop
 * has returned, until the slot is pushed again */
int msk144_stream_gate_slot(msk144_handle* h, int32_t slot, const int32_t** positions, int32_t* count, int32_t* total);

#ifdef __cplusplus
}
#endif

#endif /* MSK144HIP_H */
