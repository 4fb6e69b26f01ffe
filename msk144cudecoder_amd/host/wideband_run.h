// The wideband mode of msk144hipdecoder (--wideband-rate) for one library handle: the resolved entries, the parsed options, the files
// the options write and one state block per option, laid out like h->wb.{agc,spectrum,pings,...} of csrc/api_handle.h.  What one
// option needs of another - the waterfall and the capture look at the ping records, PingSpectra exists only with the detector - is
// settled here, not by the order in which a caller switches things on.
//
// Threads: no lock, by this rule.  prepare(), configure(), finish() and print_summary() run on the main thread, the first two before
// the DeviceLoop that holds this object starts its threads, the last two after it has joined them.  pushed() and read_push() run on
// the loop's ingest thread while it lives, read_push() once more on the main thread (DeviceLoop::join) after it has ended.
// With --wideband-notch=auto read_push() is also where a new notch table goes to the library, on the thread that makes the next push.
#pragma once

#include "wideband_cli.h"

#include <cstdio>
#include <memory>
#include <string>
#include <vector>

namespace msk144host
{

class WidebandRun
{
public:
    explicit WidebandRun(const WidebandOptions& options) : opt_(options) {}
    ~WidebandRun();
    WidebandRun(const WidebandRun&) = delete;
    WidebandRun& operator=(const WidebandRun&) = delete;

    const WidebandApi& api() const { return api_; }
    int channels() const { return static_cast<int>(opt_.offsets.size()); }

    // Resolves the entries of the options, then opens their files (appending; the capture directory is made and its capture.log
    // started afresh).  No library call is made.  false: the reason is on stderr, and no file was opened when an entry is missing.
    bool prepare();
    // Describes the input on stderr, then msk144_set_wideband and the `set` call of every option on `h`.  false: the library's
    // reason is on stderr.
    bool configure(msk144_handle* h);

    // a push of every channel was handed to the library: its components count once it has been read
    void pushed(bool first) { pending_components_ = 2ll * channels() * (first ? MSK144_WINDOW_SAMPLES : MSK144_HOP_SAMPLES); }
    // Reads what the last push left, if one is unread, into the state blocks and the files: the clip count (which waits for the
    // push's kernels), levels, spectrum, then the ping records with - behind them, for the events they close - the waterfall rows and
    // the capture units, then the notch counts and, with auto, the planner's step and the new table for the next push, last the gate's
    // counts.  false: error() says why.
    bool read_push(msk144_handle* h);
    // The end of the stream: the last, shorter spectrum group, the ping events still open, the open capture segments.  false: error().
    bool finish();
    const std::string& error() const { return error_; }

    // every "msk144hipdecoder: wideband ..." line of the end-of-run summary
    void print_summary(msk144_handle* h) const;

private:
    static FILE* open_to_append(const char* option, const std::string& path);
    static bool set_failed(msk144_handle* h);
    static double spectrum_dbfs(double power, double full);
    bool read_levels(msk144_handle* h);
    bool read_spectrum(msk144_handle* h);
    bool read_pings(msk144_handle* h);
    bool read_waterfall(msk144_handle* h);
    bool read_capture(msk144_handle* h);
    bool read_notch(msk144_handle* h);
    bool read_gate(msk144_handle* h);
    bool set_notch_table(msk144_handle* h);
    bool write_ping_events();
    void write_spectrum_line();

    WidebandOptions opt_;
    WidebandApi api_;
    std::string error_;
    long long clipped_ = 0, components_ = 0, pending_components_ = 0;  // over the run; of the push not yet read

    struct Levels  // --wideband-levels: every channel's statistics summed over the run, the gain of its last push, the AGC exponents it saw
    {
        struct Channel
        {
            long long samples = 0, sum_sq = 0, clipped = 0;
            float gain = 0.0f;
            int min_exp = 0, max_exp = 0;
            double rms() const;
        };
        std::vector<msk144_wideband_level> buf;
        std::vector<Channel> run;
    } levels_;
    struct Spectrum  // --wideband-spectrum: one line per spectrum_hops pushes, summed in double
    {
        FILE* file = nullptr;
        double full = 0.0;               // (sum w)^2 of the default window
        std::vector<double> buf, group, run;  // the last push, the open group, the run
        long long pushes = 0, group_pushes = 0, group_segments = 0, run_segments = 0;
    } spectrum_;
    struct Pings  // --wideband-pings: every event that closes (csrc/wideband.h PingTracker) is one line, flushed
    {
        FILE* file = nullptr;
        std::unique_ptr<msk144wb::PingTracker> tracker;
        std::vector<msk144_wideband_ping> buf;
        std::vector<int32_t> energies;
        std::vector<msk144wb::PingEvent> events;  // closed, not yet written
        int band_shift = 0;                       // of --wideband-pings-band's design
    } pings_;
    struct Waterfall  // --wideband-waterfall: one line per selected row; with the detector ` freq=<Hz>` on every event line
    {
        FILE* file = nullptr;
        std::unique_ptr<msk144wb::PingSpectra> spectra;  // with the detector only
        std::vector<int32_t> freqs;                      // of `events`, one each
        std::vector<float> rows;                         // [channels][54][96], the rows of the channels read
        std::vector<double> sums, run;                   // [channels][96]: the last push, the run
        double full = 1.0;                               // (sum w)^2 of the default window
        long long pushes = 0, base = 0, written = 0;     // pushes read, blocks of all earlier pushes, rows written
    } waterfall_;
    struct Capture  // --wideband-capture: the units go to segment files; with the detector ` file=<name> at=<sample>` on every event line
    {
        std::unique_ptr<msk144wb::CaptureSegments> segments;
        std::vector<msk144_wideband_capture_unit> units;  // [max_units]
        std::vector<int8_t> data;                         // [max_units][5184]
        long long dropped = 0;
    } capture_;
    struct Audio  // --wideband-audio: the units' audio rows go to the WAV file beside their segment
    {
        std::vector<int16_t> rows;                        // [max_units][2592]
        std::vector<int32_t> clamped;                     // [max_units]
        msk144wb::AudioParams design{};
    } audio_;
    struct Notch  // --wideband-notch: the table the library holds, a fixed one or what the planner has added so far
    {
        std::unique_ptr<msk144wb::NotchPlanner> planner;  // with auto only
        std::vector<std::vector<int32_t>> table;          // [channels] the channel's frequencies; empty: not notched
        std::vector<msk144_wideband_notch_count> counts;  // [channels] of the last push
        std::vector<double> sums;                         // [channels][96] of the last push, when --wideband-waterfall does not read them
        long long pushes = 0, clamped = 0;                // pushes read, components clamped over the run
        bool set = false;                                 // the library holds a table: the last push was made with it
    } notch_;
    struct Gate  // --wideband-gate: the channel windows the decode covered, over the run
    {
        std::vector<int32_t> list;                        // [channels] of the last push
        long long decoded = 0, windows = 0, dropped = 0;  // listed channels, channels x pushes, qualified but over the budget
        int busiest = 0;                                  // the largest list of a push
    } gate_;
};

}  // namespace msk144host

#include "wideband_run_impl.h"  // the member functions, inline: no source file is added to the program's list
