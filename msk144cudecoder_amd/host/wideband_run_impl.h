// The member functions of WidebandRun.  wideband_run.h includes this file at its end: the class is header-only, like
// wideband_cli.h, so the program's list of sources stays what it was, and every definition here is `inline`.
#pragma once

#include "wideband_run.h"

#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <iostream>

namespace msk144host
{

// the one "open FILE or give up" of the options that append to a file
inline FILE* WidebandRun::open_to_append(const char* option, const std::string& path)
{
    FILE* f = fopen(path.c_str(), "a");
    if(!f) std::cerr << option << ": cannot open '" << path << "': " << strerror(errno) << std::endl;
    return f;
}

// the one report of a `set` call the library refused
inline bool WidebandRun::set_failed(msk144_handle* h)
{
    std::cerr << "msk144hip: " << msk144_last_error(h) << std::endl;
    return false;
}

inline double WidebandRun::spectrum_dbfs(double power, double full)
{
    const double db = power > 0.0 && full > 0.0 ? 10.0 * std::log10(power / full) : -200.0;
    return db < -200.0 ? -200.0 : std::round(db * 100.0) / 100.0 + 0.0;  // two decimals, and no "-0.00"
}

inline double WidebandRun::Levels::Channel::rms() const
{
    return samples ? std::sqrt(static_cast<double>(sum_sq) / (2.0 * static_cast<double>(samples))) : 0.0;
}

inline WidebandRun::~WidebandRun()
{
    for(FILE* f : {spectrum_.file, pings_.file, waterfall_.file})
        if(f) fclose(f);
}

inline bool WidebandRun::prepare()
{
    std::string err;
    if(!api_.resolve(opt_, err))
    {
        std::cerr << "msk144hip: " << err << std::endl;
        return false;
    }
    // the files are opened once the entries are known to exist, and still before any library call
    if(opt_.spectrum && !(spectrum_.file = open_to_append("--wideband-spectrum", opt_.spectrum_file))) return false;
    if(opt_.pings && !(pings_.file = open_to_append("--wideband-pings", opt_.pings_file))) return false;
    if(opt_.waterfall && !(waterfall_.file = open_to_append("--wideband-waterfall", opt_.waterfall_file))) return false;
    // --wideband-capture: its directory is made if it is not there, and capture.log must be writable in it.  A run starts the log
    // afresh: a segment's first write truncates a file of the same name that an earlier run left, so that run's lines would name
    // files whose content is no longer theirs.
    if(opt_.capture)
    {
        FILE* log = nullptr;
        if((mkdir(opt_.capture_dir.c_str(), 0777) != 0 && errno != EEXIST) || !(log = fopen((opt_.capture_dir + "/capture.log").c_str(), "w")))
        {
            std::cerr << "--wideband-capture: cannot write under '" << opt_.capture_dir << "': " << strerror(errno) << std::endl;
            return false;
        }
        fclose(log);
        opt_.capture_params.max_units = capture_default_max_units(opt_.offsets.size());
    }

    const size_t C = opt_.offsets.size();
    if(opt_.spectrum)
    {
        // 0 dBFS is S (sum w)^2 of the window the device holds: the default one, rounded to f32
        double sum = 0.0;
        for(double v : msk144wb::spectrum_window(opt_.spectrum_bins)) sum += static_cast<double>(static_cast<float>(v));
        spectrum_.full = sum * sum;
        spectrum_.buf.assign(static_cast<size_t>(opt_.spectrum_bins), 0.0);
        spectrum_.group = spectrum_.run = spectrum_.buf;
    }
    if(opt_.pings)
    {
        pings_.tracker.reset(new msk144wb::PingTracker(static_cast<int>(C), opt_.ping_min_blocks));
        pings_.buf.resize(C);
        pings_.energies.resize(C * msk144wb::kPingMaxBlocks);
    }
    if(opt_.waterfall)
    {
        if(opt_.pings) waterfall_.spectra.reset(new msk144wb::PingSpectra(static_cast<int>(C), opt_.ping_min_blocks));
        waterfall_.full = msk144wb::waterfall_full(nullptr);
        waterfall_.rows.assign(C * msk144wb::kWaterfallRows * msk144wb::kWaterfallBins, 0.0f);
        waterfall_.sums.assign(C * msk144wb::kWaterfallBins, 0.0);
        waterfall_.run = waterfall_.sums;
    }
    if(opt_.notch)
    {
        notch_.table.assign(C, std::vector<int32_t>());
        notch_.counts.resize(C);
        for(const auto& e : opt_.notch_table) notch_.table[static_cast<size_t>(e.first)] = e.second;
        if(opt_.notch_auto) notch_.planner.reset(new msk144wb::NotchPlanner(static_cast<int>(C), opt_.notch_plan, opt_.notch_halfwidth));
        if(opt_.notch_auto && !opt_.waterfall) notch_.sums.assign(C * msk144wb::kWaterfallBins, 0.0);
    }
    if(opt_.gate) gate_.list.resize(C);
    if(opt_.capture)
    {
        capture_.segments.reset(new msk144wb::CaptureSegments(opt_.capture_dir, opt_.offsets));
        capture_.units.resize(static_cast<size_t>(opt_.capture_params.max_units));
        capture_.data.resize(static_cast<size_t>(opt_.capture_params.max_units) * msk144wb::kCaptureUnitBytes);
    }
    if(opt_.audio)
    {
        audio_.rows.resize(static_cast<size_t>(opt_.capture_params.max_units) * msk144wb::kAudioHopSamples);
        audio_.clamped.resize(static_cast<size_t>(opt_.capture_params.max_units));
    }
    return true;
}

inline bool WidebandRun::configure(msk144_handle* h)
{
    const int nch = channels();
    const int64_t rate2 = msk144wb::stage2_rate(opt_.rate_hz);  // the channeliser's rate: Fs, or Fs/32 behind the bank
    const msk144wb::RateRatio rr = msk144wb::rate_ratio(rate2);
    static const char* fmt_names[] = {"cu8", "cs8", "cs16"};
    std::cerr << "msk144hipdecoder: wideband input " << opt_.rate_hz << " sps " << fmt_names[opt_.format] << " on stdin, ";
    if(rate2 != opt_.rate_hz)
    {
        std::vector<int> bands;
        for(int32_t f : opt_.offsets)
        {
            const int b = msk144wb::bank_band(opt_.rate_hz, f) & (msk144wb::kBankBands - 1);
            if(std::find(bands.begin(), bands.end(), b) == bands.end()) bands.push_back(b);
        }
        std::cerr << "stage 1: " << msk144wb::kBankBands << "-band analysis bank, " << bands.size() << " bands occupied, sub-band rate " << rate2 << " sps, filter "
                  << msk144wb::kDefaultBankTapsPerBand << " x " << msk144wb::kBankBands << " taps; stage 2: ";
    }
    std::cerr << (rr.Q == 1 ? "decimation " + std::to_string(rr.P) : "resampling " + std::to_string(rr.P) + "/" + std::to_string(rr.Q)) << ", filter "
              << opt_.taps_per_phase << " x " << rr.P << " taps, gain " << opt_.gain << (opt_.agc ? " x 2^e (AGC, e within +-20)" : "") << ", " << nch << " channels as one GPU batch per hop:" << std::endl;
    for(int c = 0; c < nch; c++) std::cerr << "msk144hipdecoder: ch=" << c << " offset " << opt_.offsets[static_cast<size_t>(c)] << " Hz" << std::endl;

    const std::vector<double> taps = msk144wb::design_taps_rate(rate2, opt_.taps_per_phase);
    msk144_wideband_params wp{};
    wp.rate_hz = opt_.rate_hz;
    wp.format = opt_.format;
    wp.taps_per_phase = opt_.taps_per_phase;
    wp.gain = opt_.gain;
    wp.num_taps = static_cast<int32_t>(taps.size());
    wp.taps = taps.data();
    wp.offsets_hz = opt_.offsets.data();
    wp.num_offsets = nch;
    if(api_.set(h, &wp) != MSK144_OK) return set_failed(h);
    if(opt_.agc)
    {
        const msk144wb::AgcParams d;
        const msk144_wideband_agc agc{d.lo_sq, d.hi_sq, d.clip_ppm, d.hold, d.min_exp, d.max_exp};
        if(api_.set_agc(h, &agc) != MSK144_OK) return set_failed(h);
    }
    if(opt_.spectrum)
    {
        const msk144_wideband_spectrum_params sp{opt_.spectrum_bins, nullptr};
        if(api_.set_spectrum(h, &sp) != MSK144_OK) return set_failed(h);
    }
    if(opt_.ping_band)
    {
        const msk144wb::PingBandParams d = msk144wb::ping_band_design(opt_.ping_band_centre, opt_.ping_band_halfwidth);
        msk144_wideband_ping_band_params bp;
        static_assert(sizeof(bp) == sizeof(d), "msk144wb::PingBandParams is msk144_wideband_ping_band_params");
        std::memcpy(&bp, &d, sizeof(bp));
        pings_.band_shift = bp.shift;
        if(api_.set_ping_band(h, &bp) != MSK144_OK) return set_failed(h);
    }
    if(opt_.pings)
    {
        const msk144_wideband_pings_params pp{opt_.ping_params.ratio_q4, opt_.ping_params.memory, opt_.ping_params.min_ref};
        if(api_.set_pings(h, &pp) != MSK144_OK) return set_failed(h);
    }
    if(opt_.waterfall || (opt_.notch && opt_.notch_auto))  // auto reads the sums of every push; without --wideband-waterfall no file is written
    {
        const msk144_wideband_waterfall_params fp{nullptr};
        if(api_.set_waterfall(h, &fp) != MSK144_OK) return set_failed(h);
    }
    if(opt_.capture)
    {
        msk144_wideband_capture_params cp{};
        cp.pre = opt_.capture_params.pre;
        cp.post = opt_.capture_params.post;
        cp.max_units = opt_.capture_params.max_units;
        cp.num_listed = static_cast<int32_t>(opt_.capture_channels.size());
        std::copy(opt_.capture_channels.begin(), opt_.capture_channels.end(), cp.listed);
        if(api_.set_capture(h, &cp) != MSK144_OK) return set_failed(h);
    }
    if(opt_.audio)
    {
        audio_.design = msk144wb::audio_design(opt_.audio_centre, opt_.audio_halfwidth, opt_.audio_tone);
        msk144_wideband_audio_params ap;
        static_assert(sizeof(ap) == sizeof(audio_.design), "msk144wb::AudioParams is msk144_wideband_audio_params");
        std::memcpy(&ap, &audio_.design, sizeof(ap));
        if(api_.set_audio(h, &ap) != MSK144_OK) return set_failed(h);
    }
    if(opt_.notch && !opt_.notch_auto && !set_notch_table(h)) return false;
    if(opt_.gate)
    {
        const msk144_wideband_gate_params gp{opt_.gate_params.hold, opt_.gate_params.min_up, opt_.gate_params.max_channels};
        std::vector<uint8_t> always(opt_.offsets.size(), 0);
        for(int32_t c : opt_.gate_always) always[static_cast<size_t>(c)] = 1;
        if(api_.set_gate(h, &gp, always.data()) != MSK144_OK) return set_failed(h);
    }
    if(opt_.blanker)
    {
        const msk144_wideband_blanker bl{opt_.blanker_params.threshold_q4, opt_.blanker_params.pre, opt_.blanker_params.post};
        if(api_.set_blanker(h, &bl) != MSK144_OK) return set_failed(h);
    }
    return true;
}

// The one place that knows the order of the reads.  The ping records come ahead of the waterfall and the capture, which look at
// them; the events those records close are written last, with the frequency and the file this same push gave them.  A reader that
// could not write its file has said why in error_; otherwise the library's last error is the cause.
inline bool WidebandRun::read_push(msk144_handle* h)
{
    if(!pending_components_) return true;
    int64_t clipped = 0;
    bool ok = api_.clip(h, &clipped) == MSK144_OK;
    if(ok)
    {
        clipped_ += clipped;
        components_ += pending_components_;
        pending_components_ = 0;
    }
    ok = ok && (!opt_.levels || read_levels(h)) && (!opt_.spectrum || read_spectrum(h)) && (!opt_.pings || read_pings(h)) && (!opt_.waterfall || read_waterfall(h)) &&
         (!opt_.capture || read_capture(h)) && (!opt_.pings || write_ping_events()) && (!opt_.notch || read_notch(h)) && (!opt_.gate || read_gate(h));
    if(!ok && error_.empty()) error_ = msk144_last_error(h);
    return ok;
}

inline bool WidebandRun::finish()
{
    bool ok = true;
    if(opt_.spectrum && spectrum_.group_pushes) write_spectrum_line();  // the last, shorter group
    if(opt_.pings)
    {
        pings_.tracker->close(pings_.events);  // the end of the stream closes every open run
        if(waterfall_.spectra) waterfall_.spectra->close(waterfall_.freqs);
        ok = write_ping_events();
    }
    if(opt_.capture && !capture_.segments->close())  // ... and every open segment
    {
        error_ = "--wideband-capture: cannot write capture.log: " + std::string(strerror(errno));
        ok = false;
    }
    return ok;
}

// the levels of the push, summed per channel
inline bool WidebandRun::read_levels(msk144_handle* h)
{
    const size_t C = opt_.offsets.size();
    levels_.buf.resize(C);
    if(api_.levels(h, levels_.buf.data()) != MSK144_OK) return false;
    const bool fresh = levels_.run.empty();
    levels_.run.resize(C);
    for(size_t c = 0; c < C; c++)
    {
        const msk144_wideband_level& v = levels_.buf[c];
        Levels::Channel& a = levels_.run[c];
        a.samples += v.samples;
        a.sum_sq += v.sum_sq;
        a.clipped += v.clipped;
        a.gain = v.gain;
        a.min_exp = fresh ? v.exponent : std::min(a.min_exp, static_cast<int>(v.exponent));
        a.max_exp = fresh ? v.exponent : std::max(a.max_exp, static_cast<int>(v.exponent));
    }
    return true;
}

// the spectrum of the push, added to the open group and the run
inline bool WidebandRun::read_spectrum(msk144_handle* h)
{
    Spectrum& s = spectrum_;
    int64_t segments = 0;
    if(api_.spectrum(h, s.buf.data(), &segments) != MSK144_OK) return false;
    for(size_t j = 0; j < s.buf.size(); j++)
    {
        s.group[j] += s.buf[j];
        s.run[j] += s.buf[j];
    }
    s.group_segments += segments;
    s.run_segments += segments;
    s.group_pushes++;
    s.pushes++;
    if(s.group_pushes == opt_.spectrum_hops) write_spectrum_line();
    return true;
}

// hop=<index of the last push> rate=<Fs> bins=<B> segments=<sum> dbfs=<v0>,<v1>,...  in ascending frequency, two decimals,
// 0 dBFS = a full-scale tone on a bin centre (include/msk144hip.h), floored at -200
inline void WidebandRun::write_spectrum_line()
{
    Spectrum& s = spectrum_;
    fprintf(s.file, "hop=%lld rate=%lld bins=%zu segments=%lld dbfs=", s.pushes - 1, opt_.rate_hz, s.group.size(), s.group_segments);
    const double full = static_cast<double>(s.group_segments) * s.full;
    for(size_t j = 0; j < s.group.size(); j++) fprintf(s.file, j ? ",%.2f" : "%.2f", spectrum_dbfs(s.group[j], full));
    fputc('\n', s.file);
    fflush(s.file);
    std::fill(s.group.begin(), s.group.end(), 0.0);
    s.group_segments = s.group_pushes = 0;
}

// the records and block energies of the push to the event tracker
inline bool WidebandRun::read_pings(msk144_handle* h)
{
    static_assert(sizeof(msk144_wideband_ping) == sizeof(msk144wb::PingRecord), "the tracker reads msk144_wideband_ping");
    int32_t nb = 0;
    if(api_.pings(h, pings_.buf.data()) != MSK144_OK || api_.ping_blocks(h, -1, pings_.energies.data(), &nb) != MSK144_OK) return false;
    pings_.tracker->push(reinterpret_cast<const msk144wb::PingRecord*>(pings_.buf.data()), pings_.energies.data(), pings_.events);
    return true;
}

// with --wideband-waterfall event k of the tracker has frequency k of PingSpectra, which follows the same records; the two rules
// disagreeing on the events of a push is a defect of the program: it ends the run instead of writing lines without the field
inline bool WidebandRun::write_ping_events()
{
    std::vector<msk144wb::PingEvent>& events = pings_.events;
    std::vector<int32_t>& freqs = waterfall_.freqs;
    if(waterfall_.spectra && freqs.size() != events.size())
    {
        error_ = "ping events and their frequencies disagree: " + std::to_string(events.size()) + " events, " + std::to_string(freqs.size()) + " frequencies";
        return false;
    }
    for(size_t k = 0; k < events.size(); k++)
    {
        const msk144wb::PingEvent& e = events[k];
        std::string line = msk144wb::ping_event_line(e, opt_.offsets[static_cast<size_t>(e.channel)]);
        if(waterfall_.spectra) line += " freq=" + std::to_string(freqs[k]);
        if(capture_.segments) line += capture_.segments->locate(e.channel, e.start);
        fprintf(pings_.file, "%s\n", line.c_str());
    }
    if(!events.empty()) fflush(pings_.file);
    events.clear();
    freqs.clear();
    return true;
}

// The rows and sums of the push: one line per selected row (csrc/wideband.h waterfall_line) - every block of the listed channels, or
// by pings every up block of every channel.  Rows are read only for the channels that need them: the listed ones and, with the
// detector, those with an up block; more than a handful in one copy of all.
inline bool WidebandRun::read_waterfall(msk144_handle* h)
{
    Waterfall& w = waterfall_;
    constexpr size_t B = msk144wb::kWaterfallBins, R = msk144wb::kWaterfallRows;
    const size_t C = opt_.offsets.size();
    const int nb = static_cast<int>(w.pushes ? R / 2 : R);  // a first push, then hops
    std::vector<int32_t> need = opt_.waterfall_channels;
    for(size_t c = 0; w.spectra && c < C; c++)
        if(pings_.buf[c].up_mask && std::find(need.begin(), need.end(), static_cast<int32_t>(c)) == need.end()) need.push_back(static_cast<int32_t>(c));
    int32_t n = nb;
    if(need.size() > static_cast<size_t>(msk144wb::kWaterfallHandful))
    {
        if(api_.waterfall(h, -1, w.rows.data(), &n) != MSK144_OK) return false;
    }
    else
        for(int32_t c : need)
            if(api_.waterfall(h, c, w.rows.data() + static_cast<size_t>(c) * R * B, &n) != MSK144_OK) return false;
    if(n != nb || api_.waterfall_sums(h, w.sums.data()) != MSK144_OK) return false;
    for(size_t k = 0; k < w.sums.size(); k++) w.run[k] += w.sums[k];

    const auto write = [&](size_t c, int b) {
        fprintf(w.file, "%s\n", msk144wb::waterfall_line(static_cast<int32_t>(c), opt_.offsets[c], w.base + b, w.rows.data() + (c * R + static_cast<size_t>(b)) * B, w.full).c_str());
        w.written++;
    };
    const long long before = w.written;
    if(!opt_.waterfall_by_pings)
        for(int32_t c : opt_.waterfall_channels)
            for(int b = 0; b < nb; b++) write(static_cast<size_t>(c), b);
    else
        for(size_t c = 0; c < C; c++)
            for(int b = 0; b < nb; b++)
                if((pings_.buf[c].up_mask >> b) & 1) write(c, b);
    if(w.written != before) fflush(w.file);
    if(w.spectra) w.spectra->push(reinterpret_cast<const msk144wb::PingRecord*>(pings_.buf.data()), w.rows.data(), w.freqs);
    w.base += nb;
    w.pushes++;
    return true;
}

// the units of the push to their segment files (csrc/wideband.h CaptureSegments)
inline bool WidebandRun::read_capture(msk144_handle* h)
{
    static_assert(sizeof(msk144_wideband_capture_unit) == sizeof(msk144wb::CaptureUnit), "the segments read msk144_wideband_capture_unit");
    int32_t count = 0, total = 0;
    if(api_.capture(h, capture_.units.data(), capture_.data.data(), &count, &total) != MSK144_OK) return false;
    capture_.dropped += total - count;
    int32_t rows = count;
    if(opt_.audio && api_.capture_audio(h, audio_.rows.data(), audio_.clamped.data(), &rows) != MSK144_OK) return false;
    if(rows != count)
    {
        error_ = "--wideband-audio: the audio rows of a push are not its units'";
        return false;
    }
    if(capture_.segments->push(reinterpret_cast<const msk144wb::CaptureUnit*>(capture_.units.data()), capture_.data.data(), count, opt_.audio ? audio_.rows.data() : nullptr,
                               opt_.audio ? audio_.clamped.data() : nullptr))
        return true;
    error_ = "--wideband-capture: cannot write a segment: " + std::string(strerror(errno));
    return false;
}

// the whole table to the library: the default design of every notched channel; from the next push on
inline bool WidebandRun::set_notch_table(msk144_handle* h)
{
    std::vector<int32_t> channels;
    std::vector<msk144_wideband_notch_params> params;
    for(size_t c = 0; c < notch_.table.size(); c++)
    {
        const std::vector<int32_t>& f = notch_.table[c];
        if(f.empty()) continue;
        const msk144wb::NotchParams d = msk144wb::notch_design(f.data(), static_cast<int>(f.size()), opt_.notch_halfwidth);
        msk144_wideband_notch_params np;
        static_assert(sizeof(np) == sizeof(d), "msk144wb::NotchParams is msk144_wideband_notch_params");
        std::memcpy(&np, &d, sizeof(np));
        channels.push_back(static_cast<int32_t>(c));
        params.push_back(np);
    }
    if(api_.set_notch(h, channels.data(), static_cast<int32_t>(channels.size()), params.data()) != MSK144_OK) return set_failed(h);
    notch_.set = !channels.empty();
    return true;
}

// The clamped components of the push, then with auto the planner's step on the push's waterfall sums: every notch it adds is one
// line on stderr, and the new table goes to the library for the next push (a hop boundary, as an AGC step).
inline bool WidebandRun::read_notch(msk144_handle* h)
{
    Notch& n = notch_;
    const long long hop = ++n.pushes;  // the newest hop of the push: a first push carries hops 0 and 1
    if(n.set)
    {
        if(api_.notch_stats(h, n.counts.data()) != MSK144_OK) return false;
        for(const msk144_wideband_notch_count& c : n.counts) n.clamped += c.clipped;
    }
    if(!n.planner) return true;
    if(!opt_.waterfall && api_.waterfall_sums(h, n.sums.data()) != MSK144_OK) return false;
    std::vector<msk144wb::NotchAdded> added;
    n.planner->push(opt_.waterfall ? waterfall_.sums.data() : n.sums.data(), added);
    for(const msk144wb::NotchAdded& a : added)
    {
        n.table[static_cast<size_t>(a.channel)] = n.planner->notches(a.channel);
        std::cerr << msk144wb::notch_added_line(a, opt_.offsets[static_cast<size_t>(a.channel)], hop) << std::endl;
    }
    if(added.empty() || set_notch_table(h)) return true;
    error_ = msk144_last_error(h);
    return false;
}

// the gate's list of the push, counted: the decoder has mapped its records through the same list (WindowDecoder::submit_wideband)
inline bool WidebandRun::read_gate(msk144_handle* h)
{
    int32_t count = 0, total = 0;
    if(api_.gate(h, gate_.list.data(), &count, &total) != MSK144_OK) return false;
    gate_.decoded += count;
    gate_.windows += channels();
    gate_.dropped += total - count;
    gate_.busiest = std::max(gate_.busiest, static_cast<int>(count));
    return true;
}

inline void WidebandRun::print_summary(msk144_handle* h) const
{
    char buf[96];
    std::cerr << "msk144hipdecoder: wideband: " << clipped_ << " of " << components_ << " channel I/Q components clipped to int8";
    if(components_) std::cerr << " (" << 100.0 * static_cast<double>(clipped_) / static_cast<double>(components_) << " %)";
    std::cerr << (clipped_ && !opt_.agc ? "; lower --wideband-gain" : "") << std::endl;
    msk144_wideband_blanker_counts bc{};
    if(opt_.blanker && api_.blanker_stats(h, &bc) == MSK144_OK)  // MSK144_ESTATE: no push was made
        fprintf(stderr, "msk144hipdecoder: wideband blanker: threshold %g x mean power, guard %d+%d samples, %lld hits, %lld of %lld samples blanked (%.4f %%)\n",
                opt_.blanker_params.threshold_q4 / 16.0, opt_.blanker_params.pre, opt_.blanker_params.post, static_cast<long long>(bc.total_hits),
                static_cast<long long>(bc.total_blanked), static_cast<long long>(bc.total_samples),
                bc.total_samples ? 100.0 * static_cast<double>(bc.total_blanked) / static_cast<double>(bc.total_samples) : 0.0);
    if(opt_.spectrum && spectrum_.run_segments)
    {
        // over the run: the median bin (the floor) and the highest bin with its frequency from the centre
        const std::vector<double>& run = spectrum_.run;
        const double full = static_cast<double>(spectrum_.run_segments) * spectrum_.full;
        const size_t B = run.size(), top = static_cast<size_t>(std::max_element(run.begin(), run.end()) - run.begin());
        std::vector<double> sorted = run;
        std::nth_element(sorted.begin(), sorted.begin() + B / 2, sorted.end());
        const double peak_hz = (static_cast<double>(top) - static_cast<double>(B / 2)) * static_cast<double>(opt_.rate_hz) / static_cast<double>(B);
        fprintf(stderr, "msk144hipdecoder: wideband spectrum: %d bins of %.1f Hz over %lld segments, floor (median bin) %.2f dBFS, highest bin %.2f dBFS at %+.0f Hz\n",
                opt_.spectrum_bins, static_cast<double>(opt_.rate_hz) / opt_.spectrum_bins, spectrum_.run_segments, spectrum_dbfs(sorted[B / 2], full), spectrum_dbfs(run[top], full), peak_hz);
    }
    if(opt_.pings)
    {
        const msk144wb::PingTracker& tr = *pings_.tracker;
        const std::vector<int64_t>& ev = tr.channel_events();
        const std::vector<int64_t>& up = tr.channel_up_blocks();
        std::vector<int> active;
        for(int c = 0; c < static_cast<int>(ev.size()); c++)
            if(ev[static_cast<size_t>(c)]) active.push_back(c);
        const int with_events = static_cast<int>(active.size());
        std::stable_sort(active.begin(), active.end(), [&](int a, int b) {
            return ev[static_cast<size_t>(a)] != ev[static_cast<size_t>(b)] ? ev[static_cast<size_t>(a)] > ev[static_cast<size_t>(b)] : up[static_cast<size_t>(a)] > up[static_cast<size_t>(b)];
        });
        std::string line = "msk144hipdecoder: wideband pings: " + std::to_string(tr.events()) + " events on " + std::to_string(with_events) + " of " + std::to_string(ev.size()) +
                           " channels, " + std::to_string(tr.up_blocks()) + " of " + std::to_string(tr.total_blocks()) + " blocks up";
        if(opt_.ping_band)
        {
            snprintf(buf, sizeof(buf), ", band %d +-%d Hz shift %d", opt_.ping_band_centre, opt_.ping_band_halfwidth, pings_.band_shift);
            line += buf;
        }
        for(size_t i = 0; i < 3 && i < active.size(); i++)
        {
            snprintf(buf, sizeof(buf), "%s ch=%d (%lld)", i ? "" : "; most active", active[i], static_cast<long long>(ev[static_cast<size_t>(active[i])]));
            line += buf;
        }
        std::cerr << line << std::endl;
    }
    if(opt_.waterfall)
    {
        // up to three channels whose summed spectrum has a bin at least 10 dB (msk144wb::kWaterfallCarrierDb) over the channel's median
        // bin, the largest excess first
        struct Carrier
        {
            int channel;
            int32_t hz;
            double excess_db;
        };
        std::vector<Carrier> carriers;
        for(size_t c = 0; c < opt_.offsets.size(); c++)
        {
            int j = 0;
            const double excess = msk144wb::waterfall_excess_db(&waterfall_.run[c * msk144wb::kWaterfallBins], j);
            if(excess >= msk144wb::kWaterfallCarrierDb) carriers.push_back(Carrier{static_cast<int>(c), msk144wb::waterfall_hz(j), excess});
        }
        std::stable_sort(carriers.begin(), carriers.end(), [](const Carrier& a, const Carrier& b) { return a.excess_db > b.excess_db; });
        if(carriers.size() > 3) carriers.resize(3);
        std::string line = "msk144hipdecoder: wideband waterfall: " + std::to_string(waterfall_.written) + " rows written";
        line += carriers.empty() ? "; no channel has a bin 10 dB over its median bin" : "; a bin 10 dB or more over the channel's median bin:";
        for(const Carrier& c : carriers)
        {
            snprintf(buf, sizeof(buf), " ch=%d %+d Hz (+%.1f dB)", c.channel, c.hz, c.excess_db);
            line += buf;
        }
        std::cerr << line << std::endl;
    }
    if(opt_.notch)
    {
        // channels notched, notches, clamped components over the run, and up to three channels with their frequencies
        int channels = 0, notches = 0;
        std::string which;
        for(size_t c = 0; c < notch_.table.size(); c++)
        {
            const std::vector<int32_t>& f = notch_.table[c];
            if(f.empty()) continue;
            notches += static_cast<int>(f.size());
            if(++channels > 3) continue;
            which += (channels == 1 ? "; ch=" : " ch=") + std::to_string(c);
            for(size_t i = 0; i < f.size(); i++)
            {
                snprintf(buf, sizeof(buf), "%s%+d", i ? "," : " ", f[i]);
                which += buf;
            }
            which += " Hz";
        }
        std::cerr << "msk144hipdecoder: wideband notch: " << channels << " of " << notch_.table.size() << " channels notched, " << notches << " notches of +-" << opt_.notch_halfwidth
                  << " Hz, " << notch_.clamped << " components clamped" << which << std::endl;
    }
    if(opt_.capture)
    {
        const msk144wb::CaptureSegments& cs = *capture_.segments;
        fprintf(stderr, "msk144hipdecoder: wideband capture: %lld segments, %lld hops written, %lld bytes, %lld units dropped\n", static_cast<long long>(cs.segments()),
                static_cast<long long>(cs.hops()), static_cast<long long>(cs.bytes()), capture_.dropped);
        if(opt_.audio)
            fprintf(stderr, "msk144hipdecoder: wideband audio: %lld WAV files, %lld samples, %lld clamped, band %d +-%d Hz at %d Hz, shift %d\n", static_cast<long long>(cs.wav_files()),
                    static_cast<long long>(cs.wav_samples()), static_cast<long long>(cs.wav_clamped()), opt_.audio_centre, opt_.audio_halfwidth, opt_.audio_tone, audio_.design.shift);
    }
    if(opt_.gate)
        fprintf(stderr, "msk144hipdecoder: wideband gate: %lld of %lld channel windows decoded (%.1f %%), hold %d, min up %d, at most %d per push, %lld dropped, busiest push %d channels\n",
                gate_.decoded, gate_.windows, gate_.windows ? 100.0 * static_cast<double>(gate_.decoded) / static_cast<double>(gate_.windows) : 0.0, opt_.gate_params.hold,
                opt_.gate_params.min_up, msk144wb::gate_max_channels(opt_.gate_params, channels()), gate_.dropped, gate_.busiest);
    if(opt_.levels)
    {
        const std::vector<Levels::Channel>& lv = levels_.run;
        std::vector<int> by_clip, by_rms;
        for(int c = 0; c < static_cast<int>(lv.size()); c++)
        {
            const Levels::Channel& l = lv[static_cast<size_t>(c)];
            fprintf(stderr, "msk144hipdecoder: wideband level ch=%d offset=%d Hz rms=%.2f LSB clipped=%lld gain=%g exp=%d..%d\n", c, opt_.offsets[static_cast<size_t>(c)], l.rms(), l.clipped,
                    static_cast<double>(l.gain), l.min_exp, l.max_exp);
            by_clip.push_back(c);
            by_rms.push_back(c);
        }
        std::stable_sort(by_clip.begin(), by_clip.end(), [&](int a, int b) { return lv[static_cast<size_t>(a)].clipped > lv[static_cast<size_t>(b)].clipped; });
        std::stable_sort(by_rms.begin(), by_rms.end(), [&](int a, int b) { return lv[static_cast<size_t>(a)].rms() < lv[static_cast<size_t>(b)].rms(); });
        std::string line = "msk144hipdecoder: wideband levels: most clipped";
        for(size_t i = 0; i < 3 && i < by_clip.size(); i++)
        {
            snprintf(buf, sizeof(buf), " ch=%d (%lld)", by_clip[i], lv[static_cast<size_t>(by_clip[i])].clipped);
            line += buf;
        }
        line += "; quietest";
        for(size_t i = 0; i < 3 && i < by_rms.size(); i++)
        {
            snprintf(buf, sizeof(buf), " ch=%d (%.2f LSB)", by_rms[i], lv[static_cast<size_t>(by_rms[i])].rms());
            line += buf;
        }
        std::cerr << line << std::endl;
    }
}

}  // namespace msk144host
