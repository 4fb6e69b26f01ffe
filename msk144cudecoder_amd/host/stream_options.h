// msk144hipdecoder's options on the audio streams - --input-rate, --stream-pings / --stream-levels, --stream-gate - as one object with
// one method per phase of the program: read the line, check it, prepare, configure every decoder, attach to it, finish.  Header-only,
// like the three headers it gathers.  The order within every phase is input rate, stats, gate.
#pragma once

#include "input_rate_cli.h"
#include "stream_gate_cli.h"
#include "stream_pings_cli.h"
#include "window_decoder.h"

#include <cstdio>
#include <ostream>
#include <string>

namespace msk144host
{

struct StreamOptions
{
    InputRate input_rate;
    StreamStats stream_stats;
    StreamGate stream_gate;

    bool any() const { return input_rate.on || stream_stats.on() || stream_gate.on; }
    bool input_rate_given() const { return input_rate.given; }  // --input-rate stood on the line, whatever its value
    // what a decoder reads through WindowDecoder::use_streams: the option, or nullptr while it is off
    InputRate* rate() { return input_rate.on ? &input_rate : nullptr; }
    StreamStats* stats() { return stream_stats.on() ? &stream_stats : nullptr; }
    StreamGate* gate() { return stream_gate.on ? &stream_gate : nullptr; }

    // ---- the getopt switch: each option keeps its first error ----
    void parse_input_rate(const char* value) { keep_first(input_rate_error_, input_rate.parse(value)); }
    void parse_stream_pings(const char* value) { keep_first(stream_stats_error_, stream_stats.parse_pings(value)); }
    void parse_stream_levels() { stream_stats.levels = true; }
    void parse_stream_gate(const char* value) { keep_first(stream_gate_error_, stream_gate.parse(value)); }
    // --taps-per-phase=K on a line with --input-rate and no wideband option: the resampler's K
    void parse_taps_per_phase(const std::string& value)
    {
        if(!parse_int_in(value, 1, msk144ir::kMaxTapsPerPhase, input_rate.taps_per_phase)) keep_first(input_rate_error_, "bad value for --taps-per-phase: '" + value + "'");
    }

    // Checked in full before anything touches the library: '' or the refusal.  --input-rate=wav reads the stream's 44-byte header
    // here (wav_header_read), and the input rate's entries and taps are made here, where a refusal of theirs has always come
    std::string check(bool wideband, int read_mode, bool have_inputs, int interleaved, bool skip_wav, bool& wav_header_read)
    {
        if(input_rate.given)
        {
            std::string why = input_rate_error_;
            if(!why.empty()) ;  // the option's own value was bad
            else if(wideband) why = "--input-rate resamples audio streams: it excludes --wideband-rate (whose rate is the I/Q stream's)";
            else if(read_mode != 1) why = "--input-rate resamples 16-bit audio: it excludes --read-mode=" + std::to_string(read_mode);
            else if(input_rate.from_wav && (have_inputs || interleaved != 0))
                why = "--input-rate=wav reads the rate of the single stdin stream: with --inputs, --inputs-file or --interleaved give the rate in Hz";
            else if(input_rate.from_wav && !skip_wav) why = "--input-rate=wav takes the rate from the stream's WAV header: it needs --skip-wav-header";
            else if(input_rate.from_wav)
            {
                unsigned char hdr[44];
                int64_t hz = 0;
                if(fread(hdr, 1, sizeof(hdr), stdin) != sizeof(hdr)) why = "--input-rate=wav: the stream ended inside its 44-byte WAV header";
                else if((why = wav_header_rate(hdr, hz)).empty()) why = input_rate.set_rate(hz);
                wav_header_read = true;
            }
            if(why.empty()) input_rate.prepare(why);
            if(!why.empty()) return why;
        }
        if(stream_stats.on())
        {
            const std::string which = stream_stats.pings ? "--stream-pings" : "--stream-levels";
            if(!stream_stats_error_.empty()) return stream_stats_error_;
            if(wideband) return which + " reads the audio streams' hops: it excludes --wideband-rate (whose channels have --wideband-pings and --wideband-levels)";
            if(read_mode != 1) return which + " reads 16-bit audio: it excludes --read-mode=" + std::to_string(read_mode);
        }
        if(stream_gate.on)
        {
            if(!stream_gate_error_.empty()) return stream_gate_error_;
            if(wideband) return "--stream-gate gates the audio streams' windows: it excludes --wideband-rate (whose channels have --wideband-gate)";
            if(read_mode != 1) return "--stream-gate reads the pings of 16-bit audio: it excludes --read-mode=" + std::to_string(read_mode);
        }
        return "";
    }

    // Once the run's number of streams is known, still before anything touches the library: the stats' entries and log; the gate's MAX
    // and ALWAYS against the streams, and its entries.  The input rate has no part here: its entries and taps were made in check(),
    // so that its refusal keeps its place ahead of the other options' checks
    bool prepare(int streams, std::string& err)
    {
        if(stream_stats.on() && !stream_stats.prepare(streams, err)) return false;
        if(!stream_gate.on) return true;
        err = stream_gate.check(streams);
        return err.empty() && stream_gate.api.resolve(err);
    }

    // a decoder's handle, which decodes streams base .. base + count - 1 of the program
    bool configure(msk144_handle* h, int base, int count, std::string& err) const
    {
        return (!input_rate.on || input_rate.configure(h, err)) && (!stream_stats.on() || stream_stats.configure(h, err)) &&
               (!stream_gate.on || stream_gate.configure(h, base, count, stream_stats.on(), err));
    }

    // behind configure() of its handle: the decoder's hops then go through the options
    void attach(WindowDecoder& dec, int base) { dec.use_streams(this, base); }

    // the end of the run: the open pings close, and the summary lines
    void finish(std::ostream& out)
    {
        if(input_rate.on) out << input_rate.summary() << std::endl;
        stream_stats.finish();
        for(const std::string& l : stream_stats.summary()) out << l << std::endl;
        if(stream_gate.on) out << stream_gate.summary() << std::endl;
    }

private:
    static void keep_first(std::string& first, const std::string& why)
    {
        if(!why.empty() && first.empty()) first = why;
    }

    std::string input_rate_error_, stream_stats_error_, stream_gate_error_;
};

}  // namespace msk144host
