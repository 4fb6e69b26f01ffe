// The wideband half of the C ABI of libmsk144hip.so (include/msk144hip.h): every msk144_*wideband* entry; the handle and what is
// shared with msk144_api.cpp are in api_handle.h.  Compiled with -ffp-contract=off like that file: the tap tables and unit circles
// are formed in double and rounded to f32 once.
#include "api_handle.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <numeric>

using namespace msk144;

void wb_release(msk144_handle* h)
{
    // the gate's event and store go with the configuration: a window pushed through them can no longer be decoded
    if(h->wb.gate.planned) (void)hipEventDestroy(h->wb.gate.planned);
    if(h->gated) h->have_window = false;
    h->gated = false;
    h->wb.mem.release();
    h->wb = {};
}

namespace
{

// Every rule a configuration must meet (csrc/wideband.h check_config and the ones that need the handle); h1 = the bank prototype
// above 6.144 Msps, the caller's or the default one
int wb_validate(msk144_handle* h, const msk144_wideband_params* wp, const double* bank_taps, int32_t bank_num_taps, std::vector<double>& h1)
{
    if(!h || !wp) return fail(h, MSK144_EINVAL, "null argument");
    if(h->params.read_mode != 2) return fail(h, MSK144_EINVAL, "wideband input needs an IQ handle (read_mode 2)");
    if(wp->num_offsets != h->params.channels) return fail(h, MSK144_EINVAL, "the number of channel offsets must equal the handle's channels");
    if(const std::string why = msk144wb::check_config(wp->rate_hz, wp->format, wp->taps_per_phase, wp->gain, wp->offsets_hz, wp->num_offsets); !why.empty()) return fail(h, MSK144_EINVAL, why);
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

WbSlots wb_slot_layout(const msk144_wideband_params* wp, bool bank)
{
    WbSlots sl;
    const int C = wp->num_offsets;
    if(!bank)
    {
        sl.slot_channel.resize(static_cast<size_t>(C));
        std::iota(sl.slot_channel.begin(), sl.slot_channel.end(), 0);
        sl.slot_offset.assign(wp->offsets_hz, wp->offsets_hz + C);
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
    if(dev_alloc(h, h->wb.mem, d, v.size())) return MSK144_ENOMEM;
    HIP_TRY(h, hipMemcpy(*d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return MSK144_OK;
}

// A device buffer of the configuration: allocated by the first `set` that needs it, once per configuration and never in a push.
// Fails with MSK144_ENOMEM alone (alloc), the text set
template<typename T>
int wb_ensure(msk144_handle* h, T** d, size_t count)
{
    return *d ? MSK144_OK : dev_alloc(h, h->wb.mem, d, count);
}

WbPush wb_push_shape(const Wideband& w, bool first)
{
    const int M = first ? kWindowSamples : kHopSamples;
    return WbPush{first, M, M / w.core.Qin * w.core.Pin, M / w.core.Q * w.core.P};
}

// The base gains to the device: every slot's scale at exponent 0 (a padding slot's is never read; it gets 0), which is also what
// the next push is quantised with, and the AGC state back to exponent 0 with no quiet pushes counted.  What the last push was
// quantised with (push_gains, d_used_exp) stays, for msk144_wideband_levels.
int wb_upload_gains(msk144_handle* h)
{
    auto& a = h->wb.agc;
    const std::vector<int32_t>& slot_channel = h->wb.layout.slot_channel;
    std::vector<float> scale(slot_channel.size(), 0.0f);
    for(size_t c = 0; c < scale.size(); c++)
        if(slot_channel[c] >= 0) scale[c] = msk144wb::agc_scale(a.gains[static_cast<size_t>(slot_channel[c])], 0);
    // on the handle's stream, so that the next push is ordered behind them; waited for, as the sources live on this stack
    const size_t C = static_cast<size_t>(h->wb.channels);
    HIP_TRY(h, hipMemcpyAsync(a.d_base_scale, scale.data(), sizeof(float) * scale.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(a.d_scale, scale.data(), sizeof(float) * scale.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(a.d_gains, a.gains.data(), sizeof(float) * C, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(a.d_exp, 0, sizeof(int32_t) * C, h->stream));
    HIP_TRY(h, hipMemsetAsync(a.d_quiet, 0, sizeof(int32_t) * C, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MSK144_OK;
}

// The gate of every read entry, and through wb_quiesce of every `set` entry.  Each text stands for one test, made in this order,
// and a null text for a test that is not made (it is never read then): who - wideband mode, MSK144_EINVAL naming the entry;
// no_config - a configuration, MSK144_ESTATE (the clip count); text_when_not - a push, and one that left the option's results
// (option_pushed; the text says what it was made without).  Then the handle's device is selected and its stream waited for
int wb_read_ready(msk144_handle* h, const char* who, bool option_pushed, const char* text_when_not, const char* no_config = nullptr)
{
    if(who && !h->wb.configured) return fail(h, MSK144_EINVAL, std::string(who) + " needs wideband mode (msk144_set_wideband)");
    if(no_config && !h->wb.configured) return fail(h, MSK144_ESTATE, no_config);
    if(text_when_not && (!h->wb.started || !option_pushed)) return fail(h, MSK144_ESTATE, h->wb.started ? text_when_not : "no wideband push has been made");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MSK144_OK;
}

// the `set` entries of the options change what the next push does: configured, and nothing of an earlier push still running
int wb_quiesce(msk144_handle* h, const char* who)
{
    return h ? wb_read_ready(h, who, true, nullptr) : fail(h, MSK144_EINVAL, "null argument");
}

// Every buffer of the configuration whose shape h->wb already holds; on failure the caller releases what was allocated
int wb_allocate(msk144_handle* h, const WbTables& t, const std::vector<double>& h1)
{
    auto& w = h->wb;
    auto& k = w.core;
    auto& a = w.agc;
    const WbSlots& sl = w.layout;
    const size_t sb = static_cast<size_t>(msk144wb::sample_bytes(k.format));
    k.slot_bytes = static_cast<size_t>(wb_push_shape(w, true).samples) * sb;
    int rc = MSK144_OK;
    for(uint8_t*& p : k.pinned)
        if((rc = host_alloc(h, w.mem, &p, k.slot_bytes)) != MSK144_OK) return rc;
    if(wb_ensure(h, &k.d_raw, static_cast<size_t>(k.raw_hist) * sb + k.slot_bytes) || wb_ensure(h, &k.d_clip, 1)) return MSK144_ENOMEM;
    if((rc = wb_table(h, &k.d_G, t.G)) || (rc = wb_table(h, &k.d_branches, t.branches)) || (rc = wb_table(h, &k.d_fmod, t.fmod)) || (rc = wb_table(h, &k.d_rot, unit_circle(msk144wb::kOutRate, -1.0))))
        return rc;
    HIP_TRY(h, hipMemset(k.d_clip, 0, sizeof(unsigned long long)));
    const size_t C = static_cast<size_t>(w.channels), S = sl.slot_channel.size();
    if(wb_ensure(h, &a.d_levels, C) || wb_ensure(h, &a.d_scale, S) || wb_ensure(h, &a.d_base_scale, S) || wb_ensure(h, &a.d_gains, C) || wb_ensure(h, &a.d_exp, C) ||
       wb_ensure(h, &a.d_quiet, C) || wb_ensure(h, &a.d_used_exp, C))
        return MSK144_ENOMEM;
    HIP_TRY(h, hipMemset(a.d_levels, 0, sizeof(unsigned long long) * C));
    HIP_TRY(h, hipMemset(a.d_used_exp, 0, sizeof(int32_t) * C));
    if((rc = wb_upload_gains(h)) != MSK144_OK) return rc;
    auto& b = w.bank;
    if(!b.on) return MSK144_OK;
    if((rc = wb_table(h, &b.d_h1, std::vector<float>(h1.begin(), h1.end()))) || (rc = wb_table(h, &b.d_bands, sl.band_list)) || (rc = wb_table(h, &b.d_tw, unit_circle(msk144wb::kBankBands, 1.0))) ||
       (rc = wb_table(h, &b.d_wave_band, sl.wave_band)) || (rc = wb_table(h, &b.d_slot_channel, sl.slot_channel)))
        return rc;
    return dev_alloc(h, w.mem, &b.d_sub, sl.band_list.size() * static_cast<size_t>(b.stride));
}

// msk144_push_wideband, step by step.  Stage the input: the histories of the last push moved to the front, the slot's samples to the device, the counters of a push
// and (first push) of a stream back to 0
int wb_stage_input(msk144_handle* h, int32_t slot, const WbPush& p)
{
    auto& w = h->wb;
    const auto& k = w.core;
    const int C = w.channels;
    const size_t sb = static_cast<size_t>(msk144wb::sample_bytes(k.in_format)), hist_bytes = static_cast<size_t>(k.raw_hist) * sb;
    msk144_handle::Slot& sl = h->slots[slot];
    std::iota(sl.streams, sl.streams + C, 0);
    std::memset(sl.is_first, p.first ? 1 : 0, static_cast<size_t>(C));
    ev_begin(h);
    hipError_t e = hipSuccess;
    // the filter history: the last raw_hist samples of the previous push (a push has >= 2592*P/Q samples, raw_hist < ceil(64*P/Q)
    // without the bank and 1024 with it, so the ranges do not overlap)
    if(!p.first) e = hipMemcpyAsync(k.d_in, k.d_in + static_cast<size_t>(w.last.samples) * sb, hist_bytes, hipMemcpyDeviceToDevice, h->stream);
    // the bank's sub-band streams: the channeliser's history, the last hist frames of the previous push, likewise apart
    if(e == hipSuccess && !p.first && w.bank.on && k.hist > 0)
        e = hipMemcpy2DAsync(w.bank.d_sub, w.bank.stride * sizeof(float2), w.bank.d_sub + w.last.frames, w.bank.stride * sizeof(float2), k.hist * sizeof(float2),
                             w.layout.band_list.size(), hipMemcpyDeviceToDevice, h->stream);
    if(w.blanker.pushed)
    {
        // the raw push to the staging buffer; the counters of a push start at 0, those of a stream (totals, carry) with its first push
        if(e == hipSuccess) e = hipMemcpyAsync(w.blanker.d_stage, k.pinned[slot], static_cast<size_t>(p.samples) * msk144wb::sample_bytes(k.format), hipMemcpyHostToDevice, h->stream);
        if(e == hipSuccess) e = hipMemsetAsync(w.blanker.d_counters, 0, p.first ? sizeof(BlankerCounters) : offsetof(BlankerCounters, carry), h->stream);
    }
    else if(e == hipSuccess) e = hipMemcpyAsync(k.d_in + hist_bytes, k.pinned[slot], static_cast<size_t>(p.samples) * sb, hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess) e = hipMemcpyAsync(h->d_streams, sl.streams, sizeof(int32_t) * C, hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess) e = hipMemcpyAsync(h->d_isfirst, sl.is_first, C, hipMemcpyHostToDevice, h->stream);
    if(e == hipSuccess) e = hipMemsetAsync(k.d_clip, 0, sizeof(unsigned long long), h->stream);
    if(e == hipSuccess) e = hipMemsetAsync(w.agc.d_levels, 0, sizeof(unsigned long long) * C, h->stream);
    if(w.agc.on && p.first)
    {
        // a stream restart: exponent 0 and no quiet pushes counted, so that the same stream pushed twice gives the same bytes
        if(e == hipSuccess) e = hipMemcpyAsync(w.agc.d_scale, w.agc.d_base_scale, sizeof(float) * w.layout.slot_channel.size(), hipMemcpyDeviceToDevice, h->stream);
        if(e == hipSuccess) e = hipMemsetAsync(w.agc.d_exp, 0, sizeof(int32_t) * C, h->stream);
        if(e == hipSuccess) e = hipMemsetAsync(w.agc.d_quiet, 0, sizeof(int32_t) * C, h->stream);
    }
    // the notch starts from silence with a stream: x before the first filtered sample is 0
    if(w.notch.on && p.first && e == hipSuccess) e = hipMemsetAsync(w.notch.d_tails, 0, static_cast<size_t>(C) * 2 * msk144wb::kNotchTaps, h->stream);
    ev_end(h, MSK144_T_H2D);
    return e == hipSuccess ? MSK144_OK : fail(h, MSK144_EHIP, std::string("msk144_push_wideband: ") + hipGetErrorString(e));
}

// The front end: blanker and spectrum on the input, the bank, the channeliser into the staged hops, the AGC's step, the notch on
// the staged hops of the table's channels
void wb_launch_frontend(msk144_handle* h, const WbPush& p)
{
    auto& w = h->wb;
    const auto& k = w.core;
    const auto& a = w.agc;
    const auto& b = w.bank;
    uint8_t* fresh = k.d_in + static_cast<size_t>(k.raw_hist) * msk144wb::sample_bytes(k.in_format);  // the push, behind the history
    const int slots = static_cast<int>(w.layout.slot_channel.size());
    if(w.blanker.pushed)
    {
        launch_blanker(w.blanker.d_stage, k.format, reinterpret_cast<short2*>(fresh), p.samples, w.blanker.params, static_cast<int>(w.blanker.pushes & 1), w.blanker.d_counters, h->stream);
        w.blanker.pushes++;
        w.blanker.samples += p.samples;
    }
    const auto& sp = w.spectrum;
    if(sp.bins) launch_spectrum(fresh, k.in_format, p.samples, sp.bins, sp.d_window, sp.d_tw, sp.d_partials, sp.d_out, h->stream);
    w.spectrum.pushed = sp.bins;
    if(b.on)
        launch_bank(k.d_in, k.in_format, b.d_h1, b.d_bands, b.d_tw, b.d_sub, static_cast<int>(w.layout.band_list.size()), b.K1, p.frames, b.stride, k.hist, p.first ? 1 : 0, b.n_next,
                    h->stream);
    const WidebandBands bands{b.d_wave_band, b.d_slot_channel, b.stride};  // without the bank these are null and 0, as WidebandBands' own defaults
    launch_channelise(b.on ? static_cast<const void*>(b.d_sub) : k.d_in, b.on ? kSubbandFormat : k.in_format, k.d_G, k.d_branches, k.d_fmod, k.d_rot, reinterpret_cast<int8_t*>(h->d_first),
                      reinterpret_cast<int8_t*>(h->d_hops), k.d_clip, slots, k.P, k.Q, k.hist, p.M, p.first ? 1 : 0, k.m_next, a.d_scale, a.d_levels, h->stream, bands);
    if(a.on) launch_agc_step(a.d_levels, b.on ? b.d_slot_channel : nullptr, a.d_gains, a.d_exp, a.d_quiet, a.d_used_exp, a.d_scale, slots, p.M, a.params, h->stream);
    auto& n = w.notch;
    if(n.on)
        launch_notch(reinterpret_cast<int8_t*>(h->d_first), reinterpret_cast<int8_t*>(h->d_hops), p.first ? 1 : 0, n.d_list, n.count, n.d_taps, n.d_shifts, n.d_tails, n.d_clipped, h->stream);
    n.pushed = n.on;
}

// The observers of the staged hops: the ping band ahead of the detector, the waterfall
void wb_launch_observers(msk144_handle* h, const WbPush& p)
{
    auto& w = h->wb;
    auto& pg = w.pings;
    const int8_t* first_halves = reinterpret_cast<int8_t*>(h->d_first);
    const int8_t* hops = reinterpret_cast<int8_t*>(h->d_hops);
    const int first = p.first ? 1 : 0, restart = p.first || pg.restart ? 1 : 0;
    if(pg.on && w.ping_band.on)
        launch_pingband(first_halves, hops, first, w.channels, w.ping_band.d_taps, w.ping_band.shift, restart, w.ping_band.d_tails, pg.d_energies, h->stream);
    if(pg.on)
        launch_pings(first_halves, hops, first, w.channels, w.agc.d_gains, w.agc.on ? w.agc.d_used_exp : nullptr, pg.params, restart, pg.d_state, pg.d_records, pg.d_energies,
                     w.ping_band.on, h->stream);
    if(pg.on) pg.restart = false;
    pg.pushed = pg.on;
    if(w.waterfall.on) launch_waterfall(first_halves, hops, first, w.channels, w.waterfall.d_dft, w.waterfall.d_rows, w.waterfall.d_sums, h->stream);
    w.waterfall.pushed = w.waterfall.on;
}

// The frame of a push's plan (capture, gate), around the option's launch: launch(records, first, clear) gets the ping records of
// the push (null: the detector is off), whether the push is a first one, and whether the option's state starts afresh - a first
// push, or the first push after the option's `set`
template<class Option, class Launch>
int wb_plan(msk144_handle* h, const WbPush& p, Option& o, Launch launch)
{
    o.pushed = o.on;
    if(!o.on) return MSK144_OK;
    ev_begin(h);
    launch(h->wb.pings.on ? h->wb.pings.d_records : nullptr, p.first ? 1 : 0, p.first || o.restart ? 1 : 0);
    ev_end(h, MSK144_T_FRONTEND);
    o.restart = false;
    HIP_TRY(h, hipGetLastError());
    return MSK144_OK;
}

// The audio, behind the ring kernel: the ring now holds the push's newest hop, number m_next / 2592 - 1, and the one before it.
// A first push and the first one after msk144_set_wideband_audio filter both from an all-zero tail, every other push the newest
int wb_audio(msk144_handle* h, const WbPush& p)
{
    auto& a = h->wb.audio;
    a.pushed = a.on;
    if(!a.on) return MSK144_OK;
    ev_begin(h);
    launch_audio(h->d_ring, h->wb.channels, p.first || a.restart ? 1 : 0, h->wb.core.m_next / kHopSamples - 1, a.d_taps, a.d_phasor, a.shift, a.d_tails, a.d_ring, a.d_clamped, h->stream);
    ev_end(h, MSK144_T_FRONTEND);
    a.restart = false;
    HIP_TRY(h, hipGetLastError());
    return MSK144_OK;
}

// The dense audio rows follow the capture's: with the audio on and more capture rows than they hold, the old ones, which nothing
// reads any more, are freed and larger ones take their place (the caller's wb_quiesce has waited for the kernels that wrote them)
int wb_audio_rows(msk144_handle* h)
{
    auto& w = h->wb;
    auto& a = w.audio;
    if(!a.on || w.capture.rows <= a.rows) return MSK144_OK;
    a.rows = 0;
    dev_free(w.mem, &a.d_rows);
    dev_free(w.mem, &a.d_row_clamped);
    if(wb_ensure(h, &a.d_rows, static_cast<size_t>(w.capture.rows) * msk144wb::kAudioHopSamples) || wb_ensure(h, &a.d_row_clamped, static_cast<size_t>(w.capture.rows))) return MSK144_ENOMEM;
    a.rows = w.capture.rows;
    return MSK144_OK;
}

// Capture, behind the ring kernel and the audio: the plan and the copy of the units' I/Q, and with the audio on the copy of their audio
int wb_capture(msk144_handle* h, const WbPush& p)
{
    auto& c = h->wb.capture;
    const auto& a = h->wb.audio;
    return wb_plan(h, p, c, [&](const msk144wb::PingRecord* records, int first, int clear) {
        launch_capture(h->d_ring, records, c.d_listed, c.d_state, h->wb.channels, first, clear, c.params, h->wb.core.m_next / kHopSamples - 1, c.d_header, c.d_units, c.d_data, h->stream);
        if(a.on) launch_audio_copy(a.d_ring, a.d_clamped, c.d_header, c.d_units, c.params.max_units, a.d_rows, a.d_row_clamped, h->stream);
    });
}

// The gate's plan, behind the ping detector: the list of the channels whose window this push decodes, its header to the pinned
// copy, and the event the decode waits for.  The ring, the capture and the front end follow it on the stream
int wb_gate_plan(msk144_handle* h, const WbPush& p)
{
    auto& g = h->wb.gate;
    const int C = h->wb.channels;
    const int rc = wb_plan(h, p, g, [&](const msk144wb::PingRecord* records, int first, int clear) {
        launch_gate_plan(records, g.d_always, g.d_since, C, first, clear, g.params, (h->wb.core.m_next + p.M) / kHopSamples - 1, g.d_header, g.d_list, h->stream);
    });
    if(rc != MSK144_OK || !g.on) return rc;
    // header and list in one pinned block: a quiet band reads 16 bytes of it, a busy one the listed channels behind them
    HIP_TRY(h, hipMemcpyAsync(g.header, g.d_header, sizeof(msk144wb::PlanHeader), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(g.header + 1, g.d_list, sizeof(int32_t) * static_cast<size_t>(C), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipEventRecord(g.planned, h->stream));
    return MSK144_OK;
}

// ... and its gather, behind the IQ front end: the listed channels' analytic windows, densely, for the decode
int wb_gate_gather(msk144_handle* h)
{
    auto& g = h->wb.gate;
    h->gated = g.on;
    if(!g.on) return MSK144_OK;
    h->gate_of = {g.header, g.planned, g.d_analytic};
    ev_begin(h);
    launch_gate_gather(h->st.analytic, g.d_header, g.d_list, h->wb.channels, g.d_analytic, h->stream);
    ev_end(h, MSK144_T_FRONTEND);
    HIP_TRY(h, hipGetLastError());
    return MSK144_OK;
}

// The end of an accepted `set` of a planning option (capture, gate): its flag per channel on the device, its per-channel state
// cleared, the option on, and its next push one that starts the state afresh
template<class Option>
int wb_plan_on(msk144_handle* h, Option& o, uint8_t* d_flags, const std::vector<uint8_t>& flags, void* d_state, size_t state_bytes)
{
    HIP_TRY(h, hipMemcpy(d_flags, flags.data(), flags.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemset(d_state, 0, state_bytes));
    o.on = true;
    o.restart = true;
    return MSK144_OK;
}

// the header a plan left, as a read entry takes it: a count within 0..most
int wb_plan_header(msk144_handle* h, const char* who, const msk144wb::PlanHeader& head, int most)
{
    return head.count < 0 || head.count > most ? fail(h, MSK144_EHIP, std::string(who) + ": the device left a header out of range") : MSK144_OK;
}

}  // namespace

extern "C" {

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
    const int64_t rate2 = msk144wb::stage2_rate(wp->rate_hz);  // the channeliser's input rate
    const msk144wb::RateRatio rr = msk144wb::rate_ratio(rate2), rin = msk144wb::rate_ratio(wp->rate_hz);
    auto& w = h->wb;
    auto& k = w.core;
    w.channels = wp->num_offsets;
    w.bank.on = msk144wb::is_bank_rate(wp->rate_hz);
    w.layout = wb_slot_layout(wp, w.bank.on);
    const WbTables t = wb_tap_tables(wp, w.layout, rate2, rr.P, rr.Q);
    k.P = rr.P;
    k.Q = rr.Q;
    k.hist = (wp->num_taps + k.Q - 1) / k.Q - 1;
    k.Pin = rin.P;
    k.Qin = rin.Q;
    k.raw_hist = w.bank.on ? static_cast<int>(h1.size()) - 1 : k.hist;
    k.format = wp->format;
    w.bank.K1 = static_cast<int>(h1.size()) / msk144wb::kBankBands;
    w.bank.stride = w.bank.on ? k.hist + static_cast<long long>(wb_push_shape(w, true).frames) : 0;
    w.agc.gain = wp->gain;
    w.agc.gains.assign(static_cast<size_t>(w.channels), wp->gain);
    if((rc = wb_allocate(h, t, h1)) != MSK144_OK)
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
    *buf = h->wb.core.pinned[slot];
    *bytes = h->wb.core.slot_bytes;
    return MSK144_OK;
}

int msk144_push_wideband(msk144_handle* h, int32_t slot, int32_t first)
{
    int rc = check_hop_slot(h, slot);
    if(rc != MSK144_OK) return rc;
    auto& w = h->wb;
    if(!w.configured) return fail(h, MSK144_ESTATE, "msk144_push_wideband before msk144_set_wideband");
    if(!first && !w.started) return fail(h, MSK144_ESTATE, "a later wideband push before the first one");
    if((rc = begin_hop(h, slot, w.channels)) != MSK144_OK) return rc;
    const WbPush p = wb_push_shape(w, first != 0);
    if(p.first)
    {
        w.blanker.pushed = w.blanker.on;
        w.blanker.params = w.blanker.next;
        w.blanker.pushes = 0;
        w.blanker.samples = 0;
        w.core.d_in = w.blanker.on ? w.blanker.d_blanked : w.core.d_raw;
        w.core.in_format = w.blanker.on ? static_cast<int>(msk144wb::kCs16) : w.core.format;
        w.core.m_next = 0;
        w.bank.n_next = 0;
    }
    if((rc = wb_stage_input(h, slot, p)) != MSK144_OK) return rc;
    ev_begin(h);
    wb_launch_frontend(h, p);
    wb_launch_observers(h, p);
    ev_end(h, MSK144_T_FRONTEND);
    HIP_TRY(h, hipGetLastError());
    if((rc = wb_gate_plan(h, p)) != MSK144_OK) return rc;
    w.agc.push_gains = w.agc.gains;
    w.agc.pushed = w.agc.on;
    w.core.m_next += p.M;
    w.bank.n_next += p.frames;
    w.started = true;
    w.last = p;
    launch_hop_ring(h->d_ring, h->d_hops, h->d_first, h->d_streams, h->d_isfirst, h->d_input, w.channels, h->stream);
    if((rc = wb_audio(h, p)) != MSK144_OK) return rc;
    if((rc = wb_capture(h, p)) != MSK144_OK) return rc;
    if((rc = run_frontend(h, h->d_input)) != MSK144_OK) return rc;
    return wb_gate_gather(h);
}

int msk144_dump_wideband_hop(msk144_handle* h, int32_t channel, int8_t* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    if(channel < 0 || channel >= h->params.channels) return fail(h, MSK144_EINVAL, "channel out of range");
    if(const int rc = wb_read_ready(h, nullptr, true, ""); rc != MSK144_OK) return rc;
    const size_t half = 2 * static_cast<size_t>(kHopSamples);
    if(h->wb.last.first)
    {
        HIP_TRY(h, hipMemcpy(out, h->d_first + half * channel, half, hipMemcpyDeviceToHost));
        out += half;
    }
    HIP_TRY(h, hipMemcpy(out, h->d_hops + half * channel, half, hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_dump_wideband_band(msk144_handle* h, int32_t band, float* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(const int rc = wb_read_ready(h, nullptr, true, ""); rc != MSK144_OK) return rc;
    if(!w.bank.on) return fail(h, MSK144_ESTATE, "the wideband configuration has no bank (rate <= 6144000 Hz)");
    if(band < -msk144wb::kBankBands / 2 || band > msk144wb::kBankBands / 2) return fail(h, MSK144_EINVAL, "band out of range (-32..32)");
    const std::vector<int32_t>& bands = w.layout.band_list;
    const auto j = std::find(bands.begin(), bands.end(), band & (msk144wb::kBankBands - 1)) - bands.begin();
    if(j == static_cast<long>(bands.size())) return fail(h, MSK144_EINVAL, "no channel lies in band " + std::to_string(band));
    HIP_TRY(h, hipMemcpy(out, w.bank.d_sub + static_cast<long long>(j) * w.bank.stride + w.core.hist, sizeof(float2) * w.last.frames, hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_wideband_clip_count(msk144_handle* h, int64_t* clipped)
{
    if(!h || !clipped) return fail(h, MSK144_EINVAL, "null argument");
    if(const int rc = wb_read_ready(h, nullptr, true, nullptr, "no wideband configuration"); rc != MSK144_OK) return rc;
    unsigned long long v = 0;
    HIP_TRY(h, hipMemcpy(&v, h->wb.core.d_clip, sizeof(v), hipMemcpyDeviceToHost));
    *clipped = static_cast<int64_t>(v);
    return MSK144_OK;
}

int msk144_set_wideband_gains(msk144_handle* h, const float* gains)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_gains"); rc != MSK144_OK) return rc;
    auto& a = h->wb.agc;
    const int32_t top = a.on ? a.params.max_exp : 0;
    const std::vector<float> next = gains ? std::vector<float>(gains, gains + a.gains.size()) : std::vector<float>(a.gains.size(), a.gain);
    for(size_t c = 0; c < next.size(); c++)
        if(!msk144wb::gain_ok(next[c], top))
            return fail(h, MSK144_EINVAL, gains ? "gain of channel " + std::to_string(c) + " must be positive with 128 x gain x 2^max_exp finite in f32"
                                                : "the configured gain cannot be restored while the AGC is on: 128 x gain x 2^max_exp is not finite in f32");
    a.gains = next;
    return wb_upload_gains(h);
}

int msk144_set_wideband_agc(msk144_handle* h, const msk144_wideband_agc* p)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_agc"); rc != MSK144_OK) return rc;
    auto& a = h->wb.agc;
    if(p)
    {
        const msk144wb::AgcParams ap{p->lo_sq, p->hi_sq, p->clip_ppm, p->hold, p->min_exp, p->max_exp};
        if(const std::string why = msk144wb::check_agc(ap); !why.empty()) return fail(h, MSK144_EINVAL, why);
        for(size_t c = 0; c < a.gains.size(); c++)
            if(!msk144wb::gain_ok(a.gains[c], ap.max_exp))
                return fail(h, MSK144_EINVAL, "128 x gain x 2^max_exp of channel " + std::to_string(c) + " is not finite in f32");
        a.params = ap;
    }
    a.on = p != nullptr;
    return wb_upload_gains(h);  // exponent 0, nothing counted: the AGC starts, or the base gains hold again
}

int msk144_set_wideband_blanker(msk144_handle* h, const msk144_wideband_blanker* p)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_blanker"); rc != MSK144_OK) return rc;
    auto& w = h->wb;
    auto& b = w.blanker;
    if(p)
    {
        const msk144wb::BlankerParams bp{p->threshold_q4, p->pre, p->post};
        if(const std::string why = msk144wb::check_blanker(bp); !why.empty()) return fail(h, MSK144_EINVAL, why);
        const size_t blanked = (static_cast<size_t>(w.core.raw_hist) + static_cast<size_t>(wb_push_shape(w, true).samples)) * msk144wb::sample_bytes(msk144wb::kCs16);
        if(wb_ensure(h, &b.d_stage, w.core.slot_bytes) || wb_ensure(h, &b.d_blanked, blanked) || wb_ensure(h, &b.d_counters, 1)) return MSK144_ENOMEM;
        b.next = bp;
    }
    b.on = p != nullptr;
    return MSK144_OK;
}

int msk144_wideband_blanker_stats(msk144_handle* h, msk144_wideband_blanker_counts* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(const int rc = wb_read_ready(h, "msk144_wideband_blanker_stats", w.blanker.pushed, "the running wideband stream has no blanker"); rc != MSK144_OK) return rc;
    BlankerCounters c;
    HIP_TRY(h, hipMemcpy(&c, w.blanker.d_counters, sizeof(c), hipMemcpyDeviceToHost));
    out->samples = w.last.samples;
    out->sum_power = static_cast<int64_t>(c.sum_power);
    out->threshold = static_cast<int64_t>(msk144wb::blanker_threshold(c.sum_power, static_cast<uint64_t>(out->samples), static_cast<uint32_t>(w.blanker.params.threshold_q4)));
    out->hits = static_cast<int64_t>(c.hits);
    out->blanked = static_cast<int64_t>(c.blanked);
    out->carry_out = static_cast<int64_t>(c.carry[(w.blanker.pushes - 1) & 1]);
    out->total_samples = w.blanker.samples;
    out->total_hits = static_cast<int64_t>(c.total_hits);
    out->total_blanked = static_cast<int64_t>(c.total_blanked);
    return MSK144_OK;
}

int msk144_dump_wideband_blanked(msk144_handle* h, int16_t* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    if(const int rc = wb_read_ready(h, nullptr, h->wb.blanker.pushed, "the running wideband stream has no blanker"); rc != MSK144_OK) return rc;
    const size_t cs16 = static_cast<size_t>(msk144wb::sample_bytes(msk144wb::kCs16));
    HIP_TRY(h, hipMemcpy(out, h->wb.blanker.d_blanked + static_cast<size_t>(h->wb.core.raw_hist) * cs16, static_cast<size_t>(h->wb.last.samples) * cs16, hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_set_wideband_spectrum(msk144_handle* h, const msk144_wideband_spectrum_params* p)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_spectrum"); rc != MSK144_OK) return rc;
    auto& sp = h->wb.spectrum;
    if(p)
    {
        if(const std::string why = msk144wb::check_spectrum(p->bins, p->window, static_cast<int64_t>(wb_push_shape(h->wb, false).samples)); !why.empty()) return fail(h, MSK144_EINVAL, why);
        const int B = p->bins;
        constexpr size_t kMax = msk144wb::kSpectrumMaxBins;
        if(wb_ensure(h, &sp.d_window, kMax) || wb_ensure(h, &sp.d_tw, kMax) || wb_ensure(h, &sp.d_out, kMax)) return MSK144_ENOMEM;
        // a larger B than any before: new rows (the old ones stay with the configuration's owner until it is released)
        if(B > sp.rows_bins && dev_alloc(h, h->wb.mem, &sp.d_partials, static_cast<size_t>(B) * kSpectrumMaxGroups)) return MSK144_ENOMEM;
        sp.rows_bins = std::max(sp.rows_bins, B);
        // window and twiddles: formed in double, stored f32
        const std::vector<double> hann = p->window ? std::vector<double>() : msk144wb::spectrum_window(B);
        const double* win = p->window ? p->window : hann.data();
        const std::vector<float> wf(win, win + B);
        const std::vector<float2> tw = unit_circle(B, -1.0);
        HIP_TRY(h, hipMemcpy(sp.d_window, wf.data(), sizeof(float) * wf.size(), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(sp.d_tw, tw.data(), sizeof(float2) * tw.size(), hipMemcpyHostToDevice));
    }
    sp.bins = p ? p->bins : 0;
    return MSK144_OK;
}

int msk144_wideband_spectrum(msk144_handle* h, double* power, int64_t* segments)
{
    if(!h || !power || !segments) return fail(h, MSK144_EINVAL, "null argument");
    if(const int rc = wb_read_ready(h, "msk144_wideband_spectrum", h->wb.spectrum.pushed != 0, "the last wideband push was made without a spectrum"); rc != MSK144_OK) return rc;
    HIP_TRY(h, hipMemcpy(power, h->wb.spectrum.d_out, sizeof(double) * static_cast<size_t>(h->wb.spectrum.pushed), hipMemcpyDeviceToHost));
    *segments = static_cast<int64_t>(h->wb.last.samples) / h->wb.spectrum.pushed;
    return MSK144_OK;
}

int msk144_set_wideband_pings(msk144_handle* h, const msk144_wideband_pings_params* p)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_pings"); rc != MSK144_OK) return rc;
    auto& pg = h->wb.pings;
    if(p)
    {
        const msk144wb::PingParams pp{p->ratio_q4, p->memory, p->min_ref};
        if(const std::string why = msk144wb::check_pings(pp); !why.empty()) return fail(h, MSK144_EINVAL, why);
        const size_t C = static_cast<size_t>(h->wb.channels);
        if(wb_ensure(h, &pg.d_state, C) || wb_ensure(h, &pg.d_records, C) || wb_ensure(h, &pg.d_energies, C * msk144wb::kPingMaxBlocks)) return MSK144_ENOMEM;
        HIP_TRY(h, hipMemset(pg.d_state, 0, sizeof(msk144wb::PingHistory) * C));
        pg.params = pp;
        pg.restart = true;
    }
    pg.on = p != nullptr;
    return MSK144_OK;
}

int msk144_set_wideband_ping_band(msk144_handle* h, const msk144_wideband_ping_band_params* p)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_ping_band"); rc != MSK144_OK) return rc;
    auto& pb = h->wb.ping_band;
    static_assert(sizeof(msk144_wideband_ping_band_params) == sizeof(msk144wb::PingBandParams) && offsetof(msk144_wideband_ping_band_params, shift) == offsetof(msk144wb::PingBandParams, shift),
                  "msk144wb::PingBandParams is msk144_wideband_ping_band_params");
    if(p)
    {
        msk144wb::PingBandParams bp;
        std::memcpy(&bp, p, sizeof(bp));
        if(const std::string why = msk144wb::check_ping_band(bp); !why.empty()) return fail(h, MSK144_EINVAL, why);
        const size_t C = static_cast<size_t>(h->wb.channels);
        if(wb_ensure(h, &pb.d_taps, sizeof(bp.taps)) || wb_ensure(h, &pb.d_tails, C * 2 * msk144wb::kPingBandTaps) || wb_ensure(h, &h->wb.pings.d_energies, C * msk144wb::kPingMaxBlocks))
            return MSK144_ENOMEM;
        HIP_TRY(h, hipMemcpy(pb.d_taps, bp.taps, sizeof(bp.taps), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemset(pb.d_tails, 0, C * 2 * msk144wb::kPingBandTaps));
        pb.shift = bp.shift;
    }
    pb.on = p != nullptr;
    // E and Ef do not share a history: the next push with the detector on restarts it, and finds the tail all zero
    h->wb.pings.restart = true;
    return MSK144_OK;
}

int msk144_set_wideband_notch(msk144_handle* h, const int32_t* channels, int32_t count, const msk144_wideband_notch_params* params)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_notch"); rc != MSK144_OK) return rc;
    auto& n = h->wb.notch;
    static_assert(sizeof(msk144_wideband_notch_params) == sizeof(msk144wb::NotchParams) && offsetof(msk144_wideband_notch_params, shift) == offsetof(msk144wb::NotchParams, shift),
                  "msk144wb::NotchParams is msk144_wideband_notch_params");
    const int C = h->wb.channels;
    if(!channels) count = 0;
    if(count < 0 || count > C) return fail(h, MSK144_EINVAL, "the notch table holds 0.." + std::to_string(C) + " channels");
    if(count && !params) return fail(h, MSK144_EINVAL, "null argument");
    std::vector<uint8_t> listed(static_cast<size_t>(C), 0);
    std::vector<msk144wb::NotchParams> table(static_cast<size_t>(C));
    for(int i = 0; i < count; i++)
    {
        const int32_t c = channels[i];
        if(c < 0 || c >= C) return fail(h, MSK144_EINVAL, "notch channel " + std::to_string(c) + " is out of range");
        if(listed[static_cast<size_t>(c)]) return fail(h, MSK144_EINVAL, "notch channel " + std::to_string(c) + " is listed twice");
        listed[static_cast<size_t>(c)] = 1;
        std::memcpy(&table[static_cast<size_t>(c)], &params[i], sizeof(msk144wb::NotchParams));
        if(const std::string why = msk144wb::check_notch(table[static_cast<size_t>(c)].shift); !why.empty()) return fail(h, MSK144_EINVAL, why);
    }
    n.pushed = false;
    if(count)
    {
        const size_t Cs = static_cast<size_t>(C), row = 2 * msk144wb::kNotchTaps;
        if(wb_ensure(h, &n.d_list, Cs) || wb_ensure(h, &n.d_taps, Cs * row) || wb_ensure(h, &n.d_shifts, Cs) || wb_ensure(h, &n.d_clipped, Cs)) return MSK144_ENOMEM;
        if(!n.d_tails)
        {
            if(wb_ensure(h, &n.d_tails, Cs * row)) return MSK144_ENOMEM;
            HIP_TRY(h, hipMemset(n.d_tails, 0, Cs * row));
        }
        if(n.listed.empty()) n.listed.assign(Cs, 0), n.table.assign(Cs, msk144wb::NotchParams{});
        std::vector<int32_t> list, shifts(Cs, 0);
        std::vector<int8_t> taps(Cs * row, 0);
        for(size_t c = 0; c < Cs; c++)
        {
            if(!listed[c]) continue;
            list.push_back(static_cast<int32_t>(c));
            shifts[c] = table[c].shift;
            std::memcpy(&taps[c * row], table[c].taps, row);
            // a new or a changed entry starts from silence; an unchanged one keeps its tail
            if(!n.listed[c] || std::memcmp(&n.table[c], &table[c], sizeof(msk144wb::NotchParams)) != 0) HIP_TRY(h, hipMemset(n.d_tails + c * row, 0, row));
        }
        HIP_TRY(h, hipMemcpy(n.d_list, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(n.d_taps, taps.data(), taps.size(), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(n.d_shifts, shifts.data(), sizeof(int32_t) * Cs, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemset(n.d_clipped, 0, sizeof(int32_t) * Cs));
    }
    n.listed = count ? listed : std::vector<uint8_t>();
    n.table = count ? table : std::vector<msk144wb::NotchParams>();
    n.count = count;
    n.on = count > 0;
    return MSK144_OK;
}

int msk144_wideband_notch_stats(msk144_handle* h, msk144_wideband_notch_count* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    const auto& n = h->wb.notch;
    if(const int rc = wb_read_ready(h, "msk144_wideband_notch_stats", n.pushed, "no wideband push has been made with the notch on since it was last set"); rc != MSK144_OK) return rc;
    const size_t C = static_cast<size_t>(h->wb.channels);
    std::vector<int32_t> clipped(C);
    HIP_TRY(h, hipMemcpy(clipped.data(), n.d_clipped, sizeof(int32_t) * C, hipMemcpyDeviceToHost));
    for(size_t c = 0; c < C; c++) out[c] = msk144_wideband_notch_count{n.listed[c], clipped[c]};
    return MSK144_OK;
}

int msk144_wideband_pings(msk144_handle* h, msk144_wideband_ping* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    if(const int rc = wb_read_ready(h, "msk144_wideband_pings", h->wb.pings.pushed, "the last wideband push was made without the ping detector"); rc != MSK144_OK) return rc;
    static_assert(sizeof(msk144_wideband_ping) == sizeof(msk144wb::PingRecord) && offsetof(msk144_wideband_ping, peak_block) == offsetof(msk144wb::PingRecord, peak_block),
                  "the kernel writes msk144_wideband_ping");
    HIP_TRY(h, hipMemcpy(out, h->wb.pings.d_records, sizeof(msk144_wideband_ping) * static_cast<size_t>(h->wb.channels), hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_wideband_ping_blocks(msk144_handle* h, int32_t channel, int32_t* energies, int32_t* n)
{
    if(!h || !energies || !n) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(w.configured && (channel < -1 || channel >= w.channels)) return fail(h, MSK144_EINVAL, "channel out of range");
    if(const int rc = wb_read_ready(h, "msk144_wideband_ping_blocks", w.pings.pushed, "the last wideband push was made without the ping detector"); rc != MSK144_OK) return rc;
    const size_t row = msk144wb::kPingMaxBlocks;
    if(channel < 0) HIP_TRY(h, hipMemcpy(energies, w.pings.d_energies, sizeof(int32_t) * row * static_cast<size_t>(w.channels), hipMemcpyDeviceToHost));
    else HIP_TRY(h, hipMemcpy(energies, w.pings.d_energies + row * static_cast<size_t>(channel), sizeof(int32_t) * row, hipMemcpyDeviceToHost));
    *n = w.last.M / msk144wb::kPingBlock;
    return MSK144_OK;
}

int msk144_set_wideband_waterfall(msk144_handle* h, const msk144_wideband_waterfall_params* p)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_waterfall"); rc != MSK144_OK) return rc;
    auto& wf = h->wb.waterfall;
    if(p)
    {
        if(const std::string why = msk144wb::check_waterfall(p->window); !why.empty()) return fail(h, MSK144_EINVAL, why);
        constexpr int B = msk144wb::kWaterfallBins;
        const size_t C = static_cast<size_t>(h->wb.channels);
        if(wb_ensure(h, &wf.d_dft, kWaterfallDftSize) || wb_ensure(h, &wf.d_rows, C * msk144wb::kWaterfallRows * B) || wb_ensure(h, &wf.d_sums, C * B)) return MSK144_ENOMEM;
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
        HIP_TRY(h, hipMemcpy(wf.d_dft, dft.data(), sizeof(float2) * dft.size(), hipMemcpyHostToDevice));
    }
    wf.on = p != nullptr;
    return MSK144_OK;
}

int msk144_wideband_waterfall(msk144_handle* h, int32_t channel, float* rows, int32_t* n)
{
    if(!h || !rows || !n) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(w.configured && (channel < -1 || channel >= w.channels)) return fail(h, MSK144_EINVAL, "channel out of range");
    if(const int rc = wb_read_ready(h, "msk144_wideband_waterfall", w.waterfall.pushed, "the last wideband push was made without the waterfall"); rc != MSK144_OK) return rc;
    constexpr size_t B = msk144wb::kWaterfallBins, R = msk144wb::kWaterfallRows;
    const size_t nb = static_cast<size_t>(w.last.M) / B;
    const size_t count = channel < 0 ? static_cast<size_t>(w.channels) : 1;
    const float* d_rows = w.waterfall.d_rows + (channel < 0 ? 0 : R * B * static_cast<size_t>(channel));
    // the device holds the rows of the push's blocks; what lies past them (an earlier first push's) is not part of this push
    if(nb == R) HIP_TRY(h, hipMemcpy(rows, d_rows, sizeof(float) * R * B * count, hipMemcpyDeviceToHost));
    else
    {
        HIP_TRY(h, hipMemcpy2D(rows, sizeof(float) * R * B, d_rows, sizeof(float) * R * B, sizeof(float) * nb * B, count, hipMemcpyDeviceToHost));
        for(size_t c = 0; c < count; c++) std::fill(rows + (c * R + nb) * B, rows + (c + 1) * R * B, 0.0f);
    }
    *n = static_cast<int32_t>(nb);
    return MSK144_OK;
}

int msk144_wideband_waterfall_sums(msk144_handle* h, double* sums)
{
    if(!h || !sums) return fail(h, MSK144_EINVAL, "null argument");
    if(const int rc = wb_read_ready(h, "msk144_wideband_waterfall_sums", h->wb.waterfall.pushed, "the last wideband push was made without the waterfall"); rc != MSK144_OK) return rc;
    HIP_TRY(h, hipMemcpy(sums, h->wb.waterfall.d_sums, sizeof(double) * msk144wb::kWaterfallBins * static_cast<size_t>(h->wb.channels), hipMemcpyDeviceToHost));
    return MSK144_OK;
}

int msk144_set_wideband_capture(msk144_handle* h, const msk144_wideband_capture_params* p)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_capture"); rc != MSK144_OK) return rc;
    auto& w = h->wb;
    auto& c = w.capture;
    if(!p)
    {
        c.on = c.pushed = false;
        return MSK144_OK;
    }
    static_assert(sizeof(p->listed) / sizeof(p->listed[0]) == msk144wb::kCaptureMaxListed, "the list holds 16 channels");
    const msk144wb::CaptureParams cp{p->pre, p->post, p->max_units};
    const size_t C = static_cast<size_t>(w.channels);
    if(const std::string why = msk144wb::check_capture(cp, p->listed, p->num_listed, w.channels); !why.empty()) return fail(h, MSK144_EINVAL, why);
    // An accepted `set` ends the last push's units: the read entry answers MSK144_ESTATE until the next push made with capture on.
    // So it never meets a count above the caller's max_units, nor rows that no push has written.
    c.on = c.pushed = false;
    if(wb_ensure(h, &c.d_listed, C) || wb_ensure(h, &c.d_state, C) || wb_ensure(h, &c.d_header, 1)) return MSK144_ENOMEM;
    if(cp.max_units > c.rows)
    {
        // more units than any set before: the old rows, which nothing reads any more, are freed and larger ones take their place
        // (wb_quiesce has waited for the kernels that wrote them).  If that fails capture stays off, with no rows.
        c.rows = 0;
        dev_free(w.mem, &c.d_units);
        dev_free(w.mem, &c.d_data);
        if(wb_ensure(h, &c.d_units, static_cast<size_t>(cp.max_units)) || wb_ensure(h, &c.d_data, static_cast<size_t>(cp.max_units) * msk144wb::kCaptureUnitBytes)) return MSK144_ENOMEM;
        c.rows = cp.max_units;
    }
    if(const int rc = wb_audio_rows(h); rc != MSK144_OK) return rc;  // capture stays off
    std::vector<uint8_t> listed(C, 0);
    for(int i = 0; i < p->num_listed; i++) listed[static_cast<size_t>(p->listed[i])] = 1;
    c.params = cp;
    return wb_plan_on(h, c, c.d_listed, listed, c.d_state, sizeof(msk144wb::CaptureState) * C);
}

int msk144_wideband_capture(msk144_handle* h, msk144_wideband_capture_unit* units, int8_t* data, int32_t* count, int32_t* total)
{
    if(!h || !units || !data || !count || !total) return fail(h, MSK144_EINVAL, "null argument");
    const auto& c = h->wb.capture;
    if(const int rc = wb_read_ready(h, "msk144_wideband_capture", c.pushed, "no wideband push has been made with capture on since it was last set"); rc != MSK144_OK) return rc;
    static_assert(sizeof(msk144_wideband_capture_unit) == sizeof(msk144wb::CaptureUnit) && offsetof(msk144_wideband_capture_unit, hop) == offsetof(msk144wb::CaptureUnit, hop),
                  "the kernel writes msk144_wideband_capture_unit");
    msk144wb::PlanHeader head{};
    HIP_TRY(h, hipMemcpy(&head, c.d_header, sizeof(head), hipMemcpyDeviceToHost));
    // the push that left the header was made with c.params (`set` ends the units of the push before it)
    if(const int rc = wb_plan_header(h, "msk144_wideband_capture", head, std::min(c.params.max_units, c.rows)); rc != MSK144_OK) return rc;
    // a quiet band costs the header alone
    if(head.count)
    {
        HIP_TRY(h, hipMemcpy(units, c.d_units, sizeof(msk144wb::CaptureUnit) * static_cast<size_t>(head.count), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(data, c.d_data, static_cast<size_t>(msk144wb::kCaptureUnitBytes) * static_cast<size_t>(head.count), hipMemcpyDeviceToHost));
    }
    *count = head.count;
    *total = head.total;
    return MSK144_OK;
}

int msk144_set_wideband_audio(msk144_handle* h, const msk144_wideband_audio_params* p)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_audio"); rc != MSK144_OK) return rc;
    auto& a = h->wb.audio;
    static_assert(sizeof(msk144_wideband_audio_params) == sizeof(msk144wb::AudioParams) && offsetof(msk144_wideband_audio_params, shift) == offsetof(msk144wb::AudioParams, shift) &&
                      offsetof(msk144_wideband_audio_params, phasor) == offsetof(msk144wb::AudioParams, phasor),
                  "msk144wb::AudioParams is msk144_wideband_audio_params");
    if(!p)
    {
        a.on = a.pushed = false;
        return MSK144_OK;
    }
    msk144wb::AudioParams ap;
    std::memcpy(&ap, p, sizeof(ap));
    if(const std::string why = msk144wb::check_audio(ap); !why.empty()) return fail(h, MSK144_EINVAL, why);
    // an accepted `set` ends the last push's rows, as the capture's does: the read entry answers MSK144_ESTATE until the next push
    a.on = a.pushed = false;
    const size_t C = static_cast<size_t>(h->wb.channels);
    if(wb_ensure(h, &a.d_taps, sizeof(ap.taps)) || wb_ensure(h, &a.d_phasor, 2 * static_cast<size_t>(msk144wb::kAudioPhasors)) || wb_ensure(h, &a.d_tails, C * 2 * msk144wb::kFirTaps) ||
       wb_ensure(h, &a.d_ring, C * 2 * msk144wb::kAudioHopSamples) || wb_ensure(h, &a.d_clamped, C * 2))
        return MSK144_ENOMEM;
    HIP_TRY(h, hipMemcpy(a.d_taps, ap.taps, sizeof(ap.taps), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(a.d_phasor, ap.phasor, sizeof(ap.phasor), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemset(a.d_tails, 0, C * 2 * msk144wb::kFirTaps));
    HIP_TRY(h, hipMemset(a.d_clamped, 0, sizeof(int32_t) * C * 2));
    a.shift = ap.shift;
    a.on = true;
    if(const int rc = wb_audio_rows(h); rc != MSK144_OK)
    {
        a.on = false;
        return rc;
    }
    a.restart = true;
    return MSK144_OK;
}

int msk144_wideband_capture_audio(msk144_handle* h, int16_t* audio, int32_t* clamped, int32_t* count)
{
    if(!h || !audio || !clamped || !count) return fail(h, MSK144_EINVAL, "null argument");
    const auto& c = h->wb.capture;
    const auto& a = h->wb.audio;
    const char* why = !c.pushed ? "no wideband push has been made with capture on since it was last set" : "the last wideband push was made without the audio";
    if(const int rc = wb_read_ready(h, "msk144_wideband_capture_audio", c.pushed && a.pushed, why); rc != MSK144_OK) return rc;
    msk144wb::PlanHeader head{};
    HIP_TRY(h, hipMemcpy(&head, c.d_header, sizeof(head), hipMemcpyDeviceToHost));
    if(const int rc = wb_plan_header(h, "msk144_wideband_capture_audio", head, std::min(c.params.max_units, a.rows)); rc != MSK144_OK) return rc;
    if(head.count)
    {
        HIP_TRY(h, hipMemcpy(audio, a.d_rows, sizeof(int16_t) * msk144wb::kAudioHopSamples * static_cast<size_t>(head.count), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(clamped, a.d_row_clamped, sizeof(int32_t) * static_cast<size_t>(head.count), hipMemcpyDeviceToHost));
    }
    *count = head.count;
    return MSK144_OK;
}

int msk144_set_wideband_gate(msk144_handle* h, const msk144_wideband_gate_params* p, const uint8_t* always)
{
    if(const int rc = wb_quiesce(h, "msk144_set_wideband_gate"); rc != MSK144_OK) return rc;
    auto& w = h->wb;
    auto& g = w.gate;
    if(!p)
    {
        g.on = g.pushed = false;
        return MSK144_OK;
    }
    const msk144wb::GateParams gp{p->hold, p->min_up, p->max_channels};
    const size_t C = static_cast<size_t>(w.channels);
    if(const std::string why = msk144wb::check_gate(gp, w.channels); !why.empty()) return fail(h, MSK144_EINVAL, why);
    // an accepted `set` ends the last push's list: the read entry answers MSK144_ESTATE until the next push made with the gate on
    g.on = g.pushed = false;
    if(wb_ensure(h, &g.d_always, C) || wb_ensure(h, &g.d_since, C) || wb_ensure(h, &g.d_header, 1) || wb_ensure(h, &g.d_list, C) || wb_ensure(h, &g.d_analytic, C * kWindowSamples))
        return MSK144_ENOMEM;
    if(!g.header)
    {
        // the pinned header with the list behind it: 16 bytes are four int32
        int32_t* block = nullptr;
        if(const int rc = host_alloc(h, w.mem, &block, sizeof(msk144wb::PlanHeader) / sizeof(int32_t) + C); rc != MSK144_OK) return rc;
        g.header = reinterpret_cast<msk144wb::PlanHeader*>(block);
    }
    if(!g.planned) HIP_TRY(h, hipEventCreateWithFlags(&g.planned, hipEventBlockingSync | hipEventDisableTiming));
    std::vector<uint8_t> flags(C, 0);
    for(size_t c = 0; always && c < C; c++) flags[c] = always[c] != 0;
    g.params = gp;
    return wb_plan_on(h, g, g.d_always, flags, g.d_since, sizeof(int32_t) * C);
}

int msk144_wideband_gate(msk144_handle* h, int32_t* channels_out, int32_t* count, int32_t* total)
{
    if(!h || !channels_out || !count || !total) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    const auto& g = w.gate;
    // as wb_read_ready, but it waits for the gate's event alone: the list is ready long before the push's front end is
    if(!w.configured) return fail(h, MSK144_EINVAL, "msk144_wideband_gate needs wideband mode (msk144_set_wideband)");
    if(!w.started || !g.pushed) return fail(h, MSK144_ESTATE, w.started ? "no wideband push has been made with the gate on since it was last set" : "no wideband push has been made");
    HIP_TRY(h, hipSetDevice(h->params.device));
    HIP_TRY(h, hipEventSynchronize(g.planned));
    const msk144wb::PlanHeader head = *g.header;
    if(const int rc = wb_plan_header(h, "msk144_wideband_gate", head, w.channels); rc != MSK144_OK) return rc;
    std::memcpy(channels_out, g.header + 1, sizeof(int32_t) * static_cast<size_t>(head.count));
    *count = head.count;
    *total = head.total;
    return MSK144_OK;
}

int msk144_wideband_levels(msk144_handle* h, msk144_wideband_level* out)
{
    if(!h || !out) return fail(h, MSK144_EINVAL, "null argument");
    const auto& w = h->wb;
    if(const int rc = wb_read_ready(h, "msk144_wideband_levels", true, ""); rc != MSK144_OK) return rc;
    const size_t C = static_cast<size_t>(w.channels);
    std::vector<unsigned long long> words(C);
    std::vector<int32_t> exps(C, 0);
    HIP_TRY(h, hipMemcpy(words.data(), w.agc.d_levels, sizeof(unsigned long long) * C, hipMemcpyDeviceToHost));
    if(w.agc.pushed) HIP_TRY(h, hipMemcpy(exps.data(), w.agc.d_used_exp, sizeof(int32_t) * C, hipMemcpyDeviceToHost));
    for(size_t c = 0; c < C; c++)
    {
        out[c].samples = w.last.M;
        out[c].sum_sq = msk144wb::level_sum_sq(words[c]);
        out[c].clipped = msk144wb::level_clipped(words[c]);
        out[c].gain = ldexpf(w.agc.push_gains[c], exps[c]);
        out[c].exponent = exps[c];
    }
    return MSK144_OK;
}

}  // extern "C"
