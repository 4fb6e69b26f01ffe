// Internal interface between the C-ABI host code (msk144_api.cpp, msk144_wideband_api.cpp) and the gfx950 kernels.
// One launcher per reference kernel; every launcher only enqueues work on `stream`.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msk144_protocol.h"
#include "stream_gate.h"
#include "stream_pings.h"
#include "wideband.h"

namespace msk144
{

// 42-tap sync template and the 12-sample half-sine, built on the host exactly like
// msk_context.cuh:137-196 and handed to kernels by value (kernarg -> SGPRs).
struct SyncTemplate
{
    float re[kSyncTaps];
    float im[kSyncTaps];
    float pp[12];
};

// Candidate store, structure-of-arrays, [channel][item] with item k = b*D*8 + p*8 + slot
// (result_keeper.cuh:85-91).  Replaces the reference's 632-byte array-of-structs ResultItem.
struct DeviceStore
{
    int32_t channels;
    int32_t F;                // frequency hypotheses
    int32_t D;                // scan depth (patterns)
    int32_t K;                // items per channel = F*D*8
    int32_t nbadsync_threshold;
    int32_t max_results;
    int32_t channel_base;     // added to the channel number in result records (multi-GPU sharding)
    // Blocked staging: softbits / index / LDPC are launched per block of channels [ch0, ch0 + nch), so the LLR store is
    // llr_block x K x 512 B however large the batch is (a 128-channel block: 1.58 GB at the deep config; the reference keeps
    // 512 B of softbits in every 632-byte item).  llr is indexed by (channel - ch0), every other array by the absolute
    // channel.  scan, front ends and collect always cover all `channels`.
    int32_t ch0;
    int32_t nch;
    // LLR rows do not outlive their block (the handle's block is smaller than its channel capacity): a candidate the nbadsync
    // gate is going to drop is not demodulated beyond its sync check (softbits_kernel<true>)
    int32_t gate_early;
    // Copies handed over (only with gate_early; msk144_set_copy_handover): a slot whose position folds the same frames as a LOWER slot
    // of its (frequency, pattern) group is not demodulated or decoded, it reports that slot's result.  0: every slot is computed on its
    // own, as the reference does (softbits_kernel.cuh:56-83, ldpc_kernel.cuh:100-249)
    int32_t handover;

    const float* freq;        // [F] Hz, host-computed as msk_context.cuh:135
    const float2* cb42;       // [42] sync template (re, im), for kernels that index it per lane
    float2* mix_table;        // [F][5184] (cos, sin) of the mixers' phase at (freq[b], sample n): launch_mix_table, once per handle
    float2* analytic;         // [channels][5184] front-end output
    float* seg_power;         // [channels][8]

    uint32_t* pos;            // [channels][K]
    float* xb;                // [channels][K]
    int32_t* nbadsync;        // [channels][K]
    float* llr;               // [llr_block][K][128], row of (channel, item) = ((channel - ch0) * K + item) * 128
    int32_t* idx;             // [channels][K] gated item numbers, ascending
    int32_t* n_idx;           // [channels]
    uint8_t* dec_flag;        // [channels][K] is_message_present
    uint8_t* dec_iter;        // [channels][K]
    uint8_t* dec_nhard;       // [channels][K]
    uint32_t* dec_msg;        // [channels][K][3]  77 bits MSB first in 96

    int32_t* dec_count;       // [channels] decodes per channel
    int32_t* copy_count;      // [channels] slots of the last decode that were handed to a lower slot (collect stage)
    int32_t* result_count;    // [1]
    void* results;            // [max_results] msk144_result
};

// front ends (frontend.hip)
void launch_frontend_audio(const DeviceStore& st, const int16_t* d_in, int analytic_method, const float2* d_twiddle, const float* d_fft_mask,
                           hipStream_t stream);
void launch_frontend_iq(const DeviceStore& st, const int8_t* d_in, hipStream_t stream);

// device-side window ring of every stream (hopring.hip): ring[streams[j]] advances by the hop at position j (or is filled from
// first_halves[j] + hops[j] when is_first[j]); windows[j] = the stream's new window.  Halves and windows in raw input bytes.
void launch_hop_ring(void* ring, const void* hops, const void* first_halves, const int32_t* streams, const uint8_t* is_first, void* windows, int n, hipStream_t stream);

// the resampler in front of the hop ring (resample.hip; contract in include/msk144hip.h): position j of a batch of n is stream
// streams[j]; its inputs are row j of in_hops (and of in_first on a first hop), rows of `row` = 2592 P/Q int16; its 12 kHz samples go
// to row j of out_hops (and out_first), rows of 2592 int16, what launch_hop_ring reads.  hist[channels][hist_stride] holds each
// stream's last H inputs; taps is msk144ir::pack_taps.  clamped[j] is added to: zero it ahead of the launch.
struct ResampleArgs
{
    const int16_t* in_first;
    const int16_t* in_hops;
    const int32_t* streams;
    const uint8_t* is_first;
    const uint32_t* taps;
    const int16_t* hist;
    int16_t* out_first;
    int16_t* out_hops;
    int32_t* clamped;
    int P, Q, H, hist_stride, row, dwords, shift;
};
// the resampler, then the new history of the n streams.  any_first: some is_first[j] is set (the grid then covers both halves)
void launch_resample(const ResampleArgs& a, int n, bool any_first, hipStream_t stream);

// Above 6.144 Msps the channeliser reads the analysis bank's sub-band streams (format kSubbandFormat: complex f32, one stream per
// occupied band, stride float2 apart) and its `channels` are channel slots: slot c belongs to channel slot_channel[c] (-1: a padding
// slot, written nowhere), and wave w (slots 32w .. 32w+31) reads stream wave_band[w].  Unused at the raw formats.
constexpr int kSubbandFormat = 3;
struct WidebandBands
{
    const int32_t* wave_band = nullptr;
    const int32_t* slot_channel = nullptr;
    long long stride = 0;
};

// one polyphase branch of the channeliser at Fs = 12000 P/Q: the outputs m = mr + Q a of a push read inputs n0 + a P - k, k < taps,
// with the taps h[r + k Q] (r = mr P mod Q) of its G block, which starts at float2 offset g_off.  An integer rate (Q = 1, D = P) has
// the one branch {0, 0, L}.
struct WidebandBranch
{
    long long g_off;  // G block: [ceil(channels/32)][taps in phase-major order, k = p + P q][32], zero rows past `channels`
    int n0;           // floor(mr P / Q)
    int taps;         // ceil((L - r) / Q)
};

// wideband down-converter bank (channelise.hip) at Fs = 12000 P/Q, Q >= 1: raw = `hist` history samples then M*P/Q new ones (format
// 0 cu8, 1 cs8, 2 cs16); branches[0..Q) by output residue mr, G their blocks one after another; fmod[c] = f_c mod 12000 in 0..11999;
// rot[r] = e^{-j2pi r/12000}.  G carries each branch's constant output rotation e^{-j2pi (f_c n0 mod Fs)/Fs}, so the kernel rotates
// by (f_c (m - mr)) mod 12000.  Writes the int8 I/Q of output samples m_base .. m_base+M-1 of every channel into the hop ring
// staging (M = 5184 with first != 0: the first 2592 into first_halves), quantised with scale[c] (128 x the gain of slot c), and adds
// the clipped components to *clip_count and every channel's statistics to levels[channel] (msk144wb::pack_level; csrc/wideband.h).
void launch_channelise(const void* raw, int format, const float2* G, const WidebandBranch* branches, const int32_t* fmod, const float2* rot, int8_t* first_halves,
                       int8_t* hops, unsigned long long* clip_count, int channels, int P, int Q, int hist, int M, int first, long long m_base,
                       const float* scale, unsigned long long* levels, hipStream_t stream, WidebandBands bands = {});

// the AGC step after a push of `samples` outputs per channel (channelise.hip): used_exps[ch] = exps[ch], then msk144wb::agc_step on
// levels[ch] moves (exps[ch], quiet[ch]) and scale[slot] = 128 gains[ch] 2^exps[ch] is what the next push is quantised with.
// slot_channel: the channel of each slot (NULL: slot c is channel c).
void launch_agc_step(const unsigned long long* levels, const int32_t* slot_channel, const float* gains, int32_t* exps, int32_t* quiet, int32_t* used_exps, float* scale,
                     int slots, int samples, const msk144wb::AgcParams& p, hipStream_t stream);

// the notch of a push (notch.hip; contract in include/msk144hip.h), behind the channeliser and the AGC step on the same stream and
// ahead of every reader of the staged hops, which it rewrites in place: list[count] the notched channels, count >= 1;
// taps[channels][64][2] int8 and shifts[channels], read for the listed channels; tails[channels][128] bytes, a channel's 63 raw stored
// samples before the push behind two zero bytes, moved on to the push's last 63 raw ones.  Writes clipped[c] for the listed channels.
void launch_notch(int8_t* first_halves, int8_t* hops, int first, const int32_t* list, int count, const int8_t* taps, const int32_t* shifts, uint8_t* tails, int32_t* clipped,
                  hipStream_t stream);

// ping detection on the staged hops of a push (pings.hip; contract in include/msk144hip.h), behind the channeliser and the AGC step:
// first_halves and hops are the hop ring's staging, [channels][5184] bytes each (with first != 0 a channel's push is its row of
// first_halves followed by its row of hops).  gains[channels] and used_exps[channels] (NULL without the AGC: exponent 0) give the
// scale each channel's push was quantised with; restart != 0 restarts every channel's history.  Writes records[channels] and
// energies[channels][54] (0 past the push's blocks) and moves state[channels].  band: the push's energies are taken from `energies`
// as launch_pingband left them, not summed from the hops.
void launch_pings(const int8_t* first_halves, const int8_t* hops, int first, int channels, const float* gains, const int32_t* used_exps, const msk144wb::PingParams& p,
                  int restart, msk144wb::PingHistory* state, msk144wb::PingRecord* records, int32_t* energies, bool band, hipStream_t stream);

// per-stream levels and pings of a push of audio hops (stream_pings.hip; contract in include/msk144hip.h and stream_pings.h), on the
// hop ring's staging behind the copy or the resampler: first_halves, hops [n][2592] int16 by position; streams[n], is_first[n] and
// restart[n] on the device; state[channels] by stream number; records[n], levels[n] and energies[n][54] by position.
void launch_stream_pings(const void* first_halves, const void* hops, const int32_t* streams, const uint8_t* is_first, const uint8_t* restart, int n, const msk144sp::Params& p,
                         msk144wb::PingHistory* state, msk144wb::PingRecord* records, msk144sp::Level* levels, int32_t* energies, hipStream_t stream);

// the ping band of a push (pingband.hip; contract in include/msk144hip.h), ahead of launch_pings on the same stream and on the same
// staged hops: taps[64][2] int8 on the device; tails[channels][128] bytes, a channel's 63 stored samples before the push behind two
// zero bytes, read unless restart != 0 (then all zero) and moved on to the push's last 63.  Writes energies[channels][b] for the
// push's blocks, 27 or with first != 0 54.
void launch_pingband(const int8_t* first_halves, const int8_t* hops, int first, int channels, const int8_t* taps, int shift, int restart, uint8_t* tails, int32_t* energies,
                     hipStream_t stream);

// the per-channel waterfall of a push (waterfall.hip; contract in include/msk144hip.h), on the staged hops like launch_pings:
// dft[t][i][c] = w[i] e^{-j2pi i k/96} of slot j = 32 t + c, k = (j - 48) mod 96, f32 (kWaterfallDftSize values).  Writes
// rows[channels][54][96] - only the rows of the push's blocks, 27 or with first != 0 54 - and sums[channels][96], the sum of a
// channel's rows in ascending block order in double.
constexpr size_t kWaterfallDftSize = static_cast<size_t>(msk144wb::kWaterfallBins) * msk144wb::kWaterfallBins;
void launch_waterfall(const int8_t* first_halves, const int8_t* hops, int first, int channels, const float2* dft, float* rows, double* sums, hipStream_t stream);

// the capture of a push (capture.hip; contract in include/msk144hip.h), behind launch_hop_ring: ring[channels] the 10368-byte
// windows, records[channels] the push's ping records or nullptr (the detector was off), listed[channels] the list flags.  `newest`
// is the newest hop of the push; `clear`: a first push or the first one after msk144_set_wideband_capture.  Moves state[channels]
// and writes the header, the first min(total, max_units) descriptors and their rows data[.][5184].
void launch_capture(const void* ring, const msk144wb::PingRecord* records, const uint8_t* listed, msk144wb::CaptureState* state, int channels, int first, int clear,
                    const msk144wb::CaptureParams& p, long long newest, msk144wb::PlanHeader* header, msk144wb::CaptureUnit* units, void* data, hipStream_t stream);

// the audio of a push (audio.hip; contract in include/msk144hip.h), behind launch_hop_ring and ahead of launch_capture: ring[channels]
// the 10368-byte windows; taps[64][2] int8 and phasor[96][2] int16 on the device; tails[channels][128] bytes as launch_pingband's.
// `newest` is the newest hop of the push.  With both != 0 - a first push, or the first one after msk144_set_wideband_audio - the tail
// is taken as all zero and both hops of the window are filtered, else the newest alone.  Writes the audio of hop k to row k & 1 of
// audio[channels][2][2592] int16 and its clamp count to clamped[channels][2].
void launch_audio(const void* ring, int channels, int both, long long newest, const int8_t* taps, const int16_t* phasor, int shift, uint8_t* tails, int16_t* audio,
                  int32_t* clamped, hipStream_t stream);
// ... and behind launch_capture on the same stream: row u of rows[max_units][2592] and row_clamped[u] for the header's first `count`
// units, from row (channel, hop & 1) of audio and clamped.
void launch_audio_copy(const int16_t* audio, const int32_t* clamped, const msk144wb::PlanHeader* header, const msk144wb::CaptureUnit* units, int max_units, int16_t* rows,
                       int32_t* row_clamped, hipStream_t stream);

// the gate of a push (gate.hip; contract in include/msk144hip.h).  Plan, behind launch_pings: records[channels] the push's ping
// records or nullptr (the detector was off), always[channels] the always flags; `newest` is the newest hop of the push; `clear`: a
// first push or the first one after msk144_set_wideband_gate.  Moves since[channels] and writes the header and the first
// min(total, max_channels) channels of list[channels].  Gather, behind the IQ front end: a grid of `channels` workgroups, of which
// the first header->count move row list[j] of analytic[channels][5184] to row j of packed[channels][5184].
void launch_gate_plan(const msk144wb::PingRecord* records, const uint8_t* always, int32_t* since, int channels, int first, int clear, const msk144wb::GateParams& p,
                      long long newest, msk144wb::PlanHeader* header, int32_t* list, hipStream_t stream);
void launch_gate_gather(const float2* analytic, const msk144wb::PlanHeader* header, const int32_t* list, int channels, float2* packed, hipStream_t stream);

// the stream gate of a push of n audio hops (stream_gate.hip; contract in include/msk144hip.h and stream_gate.h), behind
// launch_stream_pings on the same stream.  Mask, only with a ratio of the gate's own: masks[j] from records[n] and energies[n][54]
// as the detector left them.  Plan: streams[n], is_first[n] and restart[n] by position on the device; records[n] or nullptr (the
// detector is off), masks[n] or nullptr (the record's up mask decides); always[channels] and since[channels] by stream number;
// writes the header {count, total, hop} and the first min(total, cap) positions of list.  The gather is launch_gate_gather with n.
void launch_stream_gate_mask(const msk144wb::PingRecord* records, const int32_t* energies, int n, int ratio_q4, unsigned long long* masks, hipStream_t stream);
void launch_stream_gate_plan(const int32_t* streams, const uint8_t* is_first, const uint8_t* restart, const msk144wb::PingRecord* records, const unsigned long long* masks,
                             const uint8_t* always, int32_t* since, int n, const msk144sg::Params& p, int cap, long long hop, msk144wb::PlanHeader* header, int32_t* list,
                             hipStream_t stream);

// what the blanker counts on the device (blanker.hip): the last push's sum of powers, hits and blanked samples (zeroed by the host
// before every push), the guard samples a push's last hit owes to the next one, by push parity, and the totals since the first push
struct BlankerCounters
{
    unsigned long long sum_power, hits, blanked;
    unsigned long long carry[2];
    unsigned long long total_hits, total_blanked;
};

// the impulse-noise blanker ahead of the channeliser or the bank (blanker.hip; contract in include/msk144hip.h): raw = the N new
// samples of a push (format 0 cu8, 1 cs8, 2 cs16, 16-byte aligned), out = the same N samples as cs16 with every blanked one 0 + 0j.
// counters->sum_power, hits and blanked must be 0; carry[parity ^ 1] is what the previous push owes (0 for a first push), and
// carry[parity] receives what this one owes.
void launch_blanker(const void* raw, int format, short2* out, int N, const msk144wb::BlankerParams& p, int parity, BlankerCounters* counters, hipStream_t stream);

// the power spectrum of a push's input samples (spectrum.hip; contract in include/msk144hip.h): raw = the N new samples of a push
// (format 0 cu8, 1 cs8, 2 cs16; 16-byte loads when it is 16-byte aligned), B = the bins, a power of two within 256..8192 and <= N;
// window[B] f32; twiddles[m] = e^{-j2pi m/B}, m < B.  Workgroup g of G <= kSpectrumMaxGroups (a function of floor(N / B) alone) leaves
// its segments' sums in partials[g][B]; out[j] = their sum in row order, bin (j - B/2) mod B: ascending frequency.
constexpr int kSpectrumMaxGroups = 512;   // two workgroups on each of 256 CUs
void launch_spectrum(const void* raw, int format, int N, int B, const float* window, const float2* twiddles, double* partials, double* out, hipStream_t stream);

// the analysis bank in front of the channeliser above 6.144 Msps (bank.hip): raw = the L1-1 history samples then 32 x frames new
// ones (format 0 cu8, 1 cs8, 2 cs16); h1 = the L1 = 64 K1 bank taps (f32); bands[j] = the occupied band k mod 64 of stream j;
// tw[t] = e^{+j2pi t/64}.  Writes s_{bands[j]}[n_base + f] of frames f < frames to sub[j * stride + off + f] (complex f32).
void launch_bank(const void* raw, int format, const float* h1, const int32_t* bands, const float2* tw, float2* sub, int n_bands, int K1, int frames,
                 long long stride, int off, int first, long long n_base, hipStream_t stream);

// one wave that spins for `ticks` of the 100 MHz counter; out[0] = shader cycles elapsed, out[1] = 100 MHz ticks elapsed (hopring.hip)
void launch_clock_probe(uint64_t* out, uint32_t ticks, hipStream_t stream);

// the phasor table scan and softbits mix from (scan.hip, mix.h): table[b][n] for the F frequencies of freq, n < 5184
void launch_mix_table(const float* freq, float2* table, int F, hipStream_t stream);

// hot kernels
void launch_scan(const DeviceStore& st, const SyncTemplate& tpl, hipStream_t stream);
void launch_softbits(const DeviceStore& st, const SyncTemplate& tpl, hipStream_t stream);
void launch_index(const DeviceStore& st, hipStream_t stream);
void launch_ldpc(const DeviceStore& st, hipStream_t stream);
void launch_collect(const DeviceStore& st, hipStream_t stream);

}  // namespace msk144
