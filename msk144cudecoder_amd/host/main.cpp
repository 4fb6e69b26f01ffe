// msk144hipdecoder - stdin -> stdout MSK144 stream decoder for AMD Instinct MI355X.
// Same command-line options, input framing, help text, stderr parameter block and output lines as the reference program
// (main.cu:55-426), with the GPU work behind libmsk144hip.so.  Beyond the reference: several raw
// streams (files or FIFOs) decoded as ONE GPU batch per hop, read without blocking so that a stalled stream never holds
// the others back, with per-stream hop-deadline accounting (the reference's 210 ms watchdog, per batch and per stream).  The
// multi-stream loop is pipelined over the library's two pinned staging slots (stream_loop.h): an ingest thread reads the streams and
// submits hop n+1 while the GPU decodes hop n and a second thread turns the records of hop n-1 into text.  --devices=0,1,... runs
// one such loop per GPU, each on its contiguous share of the streams (the reference binds to one device, main.cu:115).
#include "stream_loop.h"
#include "stream_options.h"
#include "wideband_run.h"

#include <getopt.h>
#include <poll.h>
#include <signal.h>
#include <sys/resource.h>
#include <unistd.h>

#include <cerrno>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

using namespace msk144host;

namespace
{

using Clock = std::chrono::steady_clock;

// The reference's help, verbatim (main.cu:58-67; its defaults differ from the code's: 100/3/2 here, 200/4/1 in effect -
// kept as printed), followed by what this program adds.
void show_help(const char* prog)
{
    // clang-format off
    std::cout << "Calling conversion: " << prog << " {[--help] | <options> }" << std::endl;
    std::cout << " Where options are: " << std::endl;
    std::cout << "                   --help                      Show this help and exit." << std::endl;
    std::cout << "                   --center-frequency=1500.0   Center frequency in Hz." << std::endl;
    std::cout << "                   --search-step=2.0           Search step in Hz. " << std::endl;
    std::cout << "                   --search-width=100.0        Window in Hz around center frequency to find msk144 signal in. The more Search Width the more GPU resources are needed." << std::endl;
    std::cout << "                   --scan-depth=[1..8]         The more depth the more averagable patterns will be tried. Default=3" << std::endl;
    std::cout << "                   --read-mode=[1|2]           1=Audio,16 bit, mono, 12000sps, 1500Hz-recommended center; 2=IQ,8 bit, 12000sps, 0Hz-center. Default mode = 1." << std::endl;
    std::cout << "                   --analytic-method=[1|2]     How to convert real signal to ananlytyc quadrature signal. 1 = FFT; 2 = Shift-left + LPF + Shift-right. Default=2." << std::endl;
    std::cout << "                   --nbadsync-threshold=[1..4] Specifies how many errors in sync pattern are acceptable to be passed to LDPC decoder. Default=2." << std::endl;
    std::cout << " Additions of msk144hipdecoder (defaults in effect, as in the reference's code: search-width 200, scan-depth 4, nbadsync-threshold 1):" << std::endl;
    std::cout << "                   --inputs=F1,F2,...          Decode several raw streams (files or FIFOs) as one GPU batch per hop instead of stdin; lines then carry ch=<index>." << std::endl;
    std::cout << "                   --inputs-file=PATH          The same, one stream path per line (for hundreds of streams)." << std::endl;
    std::cout << "                   --interleaved=N             Decode N streams that arrive on stdin as ONE interleaved stream - a block of N x 5184 samples (stream after stream), then blocks of N x 2592 per hop - as one GPU batch per hop; lines carry ch=<index>." << std::endl;
    std::cout << "                   --hop-timeout-ms=N          With --inputs: how long a batch waits for further streams once the first one has a hop ready (a batch costs what its streams cost, so small batches are cheap and keep the latency of each stream low). Default=20." << std::endl;
    std::cout << "                   --connect-timeout-ms=N      With --inputs: how long a FIFO may stay without a writer before it counts as ended. Default=10000." << std::endl;
    std::cout << "                   --skip-wav-header           Drop the first 44 bytes of every stream (the reference decodes a RIFF header as 22 samples). Default off." << std::endl;
    std::cout << "                   --strict-decode             Unpack every distinct 77-bit payload of a window on its own. Default off: like the reference, whose per-window text cache has a comparator that is always false, every decode of a window prints the text of the window's first accepted candidate (or nothing when that one does not unpack)." << std::endl;
    std::cout << "                   --reference-decode-cache    Accepted for compatibility (the reference's behaviour is the default)." << std::endl;
    std::cout << "                   --print-bits                Append the 77-bit payload to each output line." << std::endl;
    std::cout << "                   --device=N                  HIP device ordinal. Default=0." << std::endl;
    std::cout << "                   --devices=N1,N2,...|all     With --inputs/--interleaved: split the streams contiguously over these devices; each device gets its own ingest and post-processing threads, ch=<index> stays the global stream number. An ordinal may repeat (two independent loops on one GPU)." << std::endl;
    std::cout << "                   --max-results=N             Capacity of the per-hop decode list of a device (default 256 per stream + 131072). A hop that exceeds it is cut and reported; decoding goes on." << std::endl;
    std::cout << "                   --every-slot                Demodulate and decode every candidate slot on its own, as the reference does. Default off: a slot whose position folds the same frames as a lower slot of its group reports that slot's result (same output), and a candidate the nbadsync gate drops is not demodulated beyond its sync check." << std::endl;
    std::cout << "                   --timing                    With --inputs: per-hop host and device time split (ingest, H2D, GPU, D2H, post-processing) on stderr at the end." << std::endl;
    std::cout << "                   --wideband-rate=HZ          Read ONE wideband I/Q stream on stdin at HZ sps and channelise it on the GPU into one 12000 sps IQ stream per channel offset (as --read-mode=2 would read it); lines carry ch=<index>. HZ is a multiple of 125 from 24000 to 6144000: HZ = 12000 x P/Q, 2 <= P/Q <= 512; a multiple of 12000 (e.g. 1920000) decimates by the integer D = HZ/12000, any other rate (e.g. 2048000 = 12000 x 512/3, rtl_sdr's default) resamples by P/Q. Above that, HZ a multiple of 8000 up to 61440000 (e.g. 10000000, 20000000): a 64-band analysis bank takes each channel's band to HZ/32 first, then the channeliser runs at HZ/32 (--taps-per-phase then counts its taps at HZ/32)." << std::endl;
    std::cout << "                   --wideband-format=FMT       cu8 (rtl_sdr), cs8 or cs16 interleaved I,Q. Default=cu8." << std::endl;
    std::cout << "                   --channel-offsets=F1,F2,... Channel centres in integer Hz from the wideband centre, |F| <= HZ/2 - 6000." << std::endl;
    std::cout << "                   --channel-grid=F:STEP:N     The same as N offsets F, F+STEP, ..." << std::endl;
    std::cout << "                   --wideband-gain=G           Gain before each channel's int8 I/Q (the csdr gain_ff stage). Default=100." << std::endl;
    std::cout << "                   --wideband-gain=auto[:G0]   Stepped AGC per channel, on the GPU, one hop behind the levels: 6 dB down at once when more than 0.1 % of a hop's components clip or its level exceeds 32 LSB rms, 6 dB up after 4 hops below 8 LSB rms, within G0 x 2^-20 .. G0 x 2^20. G0 default=100. A step lands on a hop boundary." << std::endl;
    std::cout << "                   --wideband-levels           With --wideband-rate: at the end, on stderr, one line per channel - rms level in LSB over the run, clipped components, last gain, lowest and highest AGC step - and the three most clipped and three quietest channels." << std::endl;
    std::cout << "                   --wideband-blanker[=RATIO[:PRE[:POST]]]  With --wideband-rate: impulse-noise blanker on the input stream, on the GPU, ahead of the channel filters: a sample whose power exceeds RATIO x the mean power of its hop is zeroed together with PRE samples before and POST after it (0..4096 each). RATIO 1..4095.9, default=16; PRE default=2, POST default=8. At the end, on stderr, one line with the hits and the blanked samples." << std::endl;
    std::cout << "                   --wideband-spectrum=FILE[:BINS[:HOPS]]  With --wideband-rate: the power spectrum of the input stream at the input rate, on the GPU (of the blanked stream with --wideband-blanker): BINS-point transforms (a power of two, 256..8192, default=1024) of the hop's samples under a Hann window, summed over HOPS hops (default=5), appended to FILE as one line 'hop= rate= bins= segments= dbfs=v0,v1,...' in ascending frequency, 0 dBFS = a full-scale tone. At the end, on stderr, one line with the median bin (the floor) and the highest bin." << std::endl;
    std::cout << "                   --wideband-pings=FILE[:RATIO[:MIN_BLOCKS[:MEMORY]]]  With --wideband-rate: ping detection per channel, on the GPU, on each channel's int8 I/Q: the energy of every 8 ms block (96 samples) is compared with RATIO x the channel's quiet level (the lower quartile of a hop's blocks, the lowest of this hop and the MEMORY hops before it, 0..16; default=8). RATIO 1..4095.9, default=2. A run of at least MIN_BLOCKS (1..64, default=2) consecutive blocks above it is an event, appended to FILE when it ends as one line 'ping ch= offset= start= dur= blocks= peak= ref= peak_db='. A strong-ping detector (from about +7 dB in 2500 Hz), less sensitive than the decoder. At the end, on stderr, one line with the events and the most active channels." << std::endl;
    std::cout << "                   --wideband-pings-band[=HALFWIDTH[:CENTRE]]  With --wideband-pings: a 64-tap complex band-pass of CENTRE +- HALFWIDTH Hz, on the GPU, ahead of the detector's block energies, so that it compares the energy inside the signal's band and not that of the whole 12 kHz channel. HALFWIDTH 500..3000, default=1500; CENTRE an integer with |CENTRE| + HALFWIDTH <= 6000, default=the value of --center-frequency. The in-band energy of a block swings further on noise alone, so without a RATIO in --wideband-pings RATIO defaults to 3.25. The ping lines keep their format; peak and ref are then in-band. The detector's summary line adds 'band <CENTRE> +-<HALFWIDTH> Hz shift <s>'." << std::endl;
    std::cout << "                   --wideband-waterfall=FILE[:CHANNELS]  With --wideband-rate: a waterfall per channel, on the GPU, on each channel's int8 I/Q: one 96-point spectrum (125 Hz per bin, Hann window) per 8 ms block, the blocks of --wideband-pings. CHANNELS is a list of up to 16 channel indices c0,c1,... (every block of these is written) or 'pings' (every block above the threshold of every channel; the default with --wideband-pings, without it a list is required). After every push one line per selected row is appended to FILE: 'wf ch= offset= block= t= db=v0,...,v95' in ascending frequency from -6000 Hz, 0 dB = a tone of 1 LSB, floor -100 dB. With --wideband-pings every ping line gains ' freq=<Hz>', the strongest bin of the event's blocks. At the end, on stderr, one line with the rows written and up to three channels whose spectrum summed over the run has a bin at least 10 dB (a design parameter) over the channel's median bin: a steady carrier in the passband. A display and a frequency estimate; it does not feed the decoder." << std::endl;
    std::cout << "                   --wideband-capture=DIR[:CHANNELS[:POST[:PRE]]]  With --wideband-rate: keep each ping's channel I/Q for replay. On the GPU, after every push, the hops worth keeping are picked per channel and packed; only those bytes come to the host. CHANNELS is 'pings' (a hop is kept when the channel has a block above the threshold in it, for POST hops after that (0..16, default 1) and, with PRE = 1 (the default; 0 or 1), the one hop before it; the default with --wideband-pings, without it a list is required) or a list of up to 16 channel indices c0,c1,... that are kept whether active or not. At most min(2 x channels, 512) hops are kept per push; more are dropped and counted. Consecutive hops of a channel are appended to DIR/ch<c>_hop<k0>.cs8: int8 I/Q at 12000 samples per second, what --read-mode=2 reads. When a segment ends one line is appended to DIR/capture.log: 'capture ch= offset= hop= t= hops= file='. Every run starts capture.log afresh and overwrites segments of the same name. With --wideband-pings every ping line gains ' file=<name> at=<sample offset of the event's first block in that file>' (' file=-' when that hop was dropped). At the end, on stderr, one line with segments, hops written, bytes and dropped units." << std::endl;
    std::cout << "                   --wideband-audio[=HALFWIDTH[:CENTRE[:TONE]]]  With --wideband-capture: beside every DIR/ch<c>_hop<k0>.cs8 write DIR/ch<c>_hop<k0>.wav, the same hops as real 16-bit audio at 12000 samples per second (one channel, PCM), what WSJT-X opens in MSK144 mode and what this program reads with --skip-wav-header. On the GPU a 64-tap complex band-pass of CENTRE +- HALFWIDTH Hz runs on every channel's int8 I/Q and an integer phasor table takes CENTRE to TONE Hz. HALFWIDTH 500..3000, default=1250; CENTRE an integer with |CENTRE| + HALFWIDTH <= 6000, default=the value of --center-frequency; TONE within HALFWIDTH..6000 - HALFWIDTH with TONE - CENTRE a multiple of 125, default=1500. An int8 full scale comes out near an int16 full scale (a design parameter); louder samples are clamped and counted. The audio lags the .cs8 samples by the filter's 31.5 samples (2.6 ms). The segment's line in capture.log gains ' wav=<name>'. At the end, on stderr, one line with the WAV files, the samples and the clamped samples." << std::endl;
    std::cout << "                   --wideband-notch=SPEC[/HALFWIDTH]  With --wideband-rate: take steady carriers (a spur, a birdie, a beacon) out of single channels, on the GPU, behind the channel filter and the AGC step and ahead of everything that reads the channel's int8 I/Q: a 64-tap complex band-pass of +-HALFWIDTH Hz (50..500, default=100) around each carrier estimates it and the estimate is taken from the channel delayed by 31 samples (2.6 ms). SPEC is a fixed table 'ch:Hz[+Hz],ch:Hz,...' - one or two frequencies per channel in Hz from the channel's offset, at least 1000 Hz apart - or 'auto[:DB[:PERIOD[:PERSIST]]]': a host rule on the channels' waterfall sums (the GPU waterfall is then on even without --wideband-waterfall) that adds a notch where the highest bin of a channel lies at least DB (default=10) over its median bin in PERSIST (default=2) consecutive sums of PERIOD pushes (default=23, about 5 s), at most two per channel; notches are only added during a run, and each is reported on stderr as 'wideband notch: ch= offset= notch= excess= at hop'. DB, PERIOD and PERSIST are design parameters, not measurements. The notch costs sensitivity on a weak ping where there is no carrier: notch only the channels that have one. At the end, on stderr, one line with the channels notched, the notches and the clamped components." << std::endl;
    std::cout << "                   --wideband-gate[=HOLD[:MIN_UP[:MAX[:ALWAYS]]]]  With --wideband-pings: decode only the channels with activity, picked on the GPU from the detector's blocks. A hop of a channel is active when at least MIN_UP (1..27, default=1) of its 27 blocks are above the threshold; the channel's window is decoded in that push and for HOLD more hops (0..16, default=1; with HOLD >= 1 every window that contains an active hop is decoded). At most MAX channels are decoded per push (default and 0: all); more are dropped in ascending channel order and counted. ALWAYS is a list of channel indices c0,c1,... that are decoded on every push; with it the option needs no --wideband-pings. An empty field keeps its default. Levels, ping events, captures and snr= of every channel stay those of a run without the gate. The detector is less sensitive than the decoder: a ping it does not see is not decoded. At the end, on stderr, one line with the channel windows decoded, the dropped ones and the busiest push." << std::endl;
    std::cout << "                   --taps-per-phase=K          Channel filter length K x P taps (1..64; P = D for an integer rate). Default=16." << std::endl;
    std::cout << "                   --input-rate=HZ|wav         With --read-mode=1: every audio stream (stdin, --inputs, --inputs-file, --interleaved) arrives at HZ samples per second and is resampled to 12000 on the GPU, in exact integers, ahead of the decoder. HZ is a multiple of 125 from 24000 to 192000 (e.g. 48000; the 44.1 kHz family is not supported): HZ = 12000 x P/Q, a hop is then 2592 x P/Q samples per stream and the first one 5184 x P/Q. 12000 is the program without the option. The filter is the channel filter's design, K x P integer taps with K = --taps-per-phase; it delays the signal by 0.67 ms at K = 16. 'wav', for the single stdin stream together with --skip-wav-header, takes HZ from the 44-byte header (PCM, one channel, 16 bits). At the end, on stderr, one line with the rate, P/Q, the taps, the shift and the samples clamped." << std::endl;
    std::cout << "                   --stream-pings=FILE[:RATIO[:MIN_BLOCKS[:MEMORY[:SHIFT]]]]  With --read-mode=1 (stdin, --inputs, --inputs-file, --interleaved, --devices, --input-rate): a ping detector on every audio stream, on the GPU, on the 12 kHz samples the decoder gets. Each hop is cut into blocks of 96 samples (8 ms) with energy E = min(2^22-1, sum of squares >> SHIFT) (0..24, default=12: audio of 30 to about 13000 LSB rms stays in range); a block is up when E exceeds RATIO (1..4095.9, default=3.5) x the stream's quiet level, the lowest lower-quartile E of this hop and the MEMORY (0..16, default=8) before it. A run of at least MIN_BLOCKS (1..64, default=2) up blocks is an event; when it closes one line is appended to FILE: ping ch=<stream> start=<s> dur=<s> blocks=<n> peak=<E> ref=<R> peak_db=<dB>, start counted from the stream's first sample. An empty field keeps its default. At the end, on stderr, one line with the events, the streams that had any, the blocks up and the three most active streams. A strong-ping detector, less sensitive than the decoder; the default RATIO comes from a CPU simulation on noise. Stdout is unchanged." << std::endl;
    std::cout << "                   --stream-levels             With --read-mode=1: at the end, on stderr, one line per stream - rms in LSB over the run, peak, full-scale samples, hops and all-zero hops, of the 12 kHz samples the decoder gets (behind the resampler with --input-rate) - and one line with the three streams with the most full-scale samples, the three quietest and every stream whose hops were all zero. Stdout is unchanged." << std::endl;
    std::cout << "                   --stream-gate[=HOLD[:MIN_UP[:MAX[:RATIO[:ALWAYS]]]]]  With --read-mode=1 (stdin, --inputs, --inputs-file, --interleaved, --devices, --input-rate): decode only the streams with activity, picked on the GPU from the blocks of the --stream-pings detector (without --stream-pings the detector runs with its defaults and writes no log). A hop of a stream is active when at least MIN_UP (1..27, default=1) of its 27 blocks are up; the stream's window is decoded in that hop and for HOLD more hops (0..16, default=1; with HOLD >= 1 every window that contains an active hop is decoded). At most MAX stream windows are decoded per hop and device (default and 0: all); more are dropped in ascending stream order and counted. RATIO (1..4095.9; empty or 0: the detector's own blocks) gives the gate a threshold of its own on the detector's energies and quiet level, so that the log keeps a strict ratio while the gate triggers on a looser one. In a CPU simulation against the reference decoder's model (three-frame pings in 300..2700 Hz noise; nothing run on the air) the default lost no decode from +2 dB up, a quarter at 0 dB and nearly all below, and listed no noise window; RATIO 2.5 kept 98.7 % of the decodes and listed 4.6 % of the noise windows; 2.0 and below kept all and listed most noise windows. ALWAYS is a list of stream numbers s0,s1,... that are decoded on every hop. An empty field keeps its default. snr= of every stream stays that of a run without the gate; stdout carries the lines of the decoded windows. The detector is less sensitive than the decoder: a ping it does not see is not decoded. At the end, on stderr, one line with the stream windows decoded of those pushed, the dropped ones and the busiest hop." << std::endl;
    // clang-format on
}

const char* mode_name(int mode)
{
    if(mode == 1) return "Audio. 16 bits signed.";
    if(mode == 2) return "IQ. 8+8 bits.";
    return "unknown";
}

void split_list(const std::string& list, std::vector<std::string>& out)
{
    for(const std::string& item : split_fields(list, ','))
        if(!item.empty()) out.push_back(item);
}

void warn_if_late(long long ms)
{
    const int soft_limit_ms = 210;  // of the 216 ms a hop lasts (main.cu:398-403)
    if(ms > soft_limit_ms)
    {
        std::cerr << "Warning: Working loop takes too much time: " << ms << " ms"
                  << " of " << soft_limit_ms << " ms max." << std::endl;
    }
}

// SIGINT / SIGTERM in the multi-stream modes: ask the loops to finish what is in flight and leave in order.  The handler only sets the
// flag; every place that can sleep - the --inputs poll, the --interleaved reader below and DeviceLoop::feed()'s back-pressure wait - looks at
// it at least every 50 ms, so the stop does not depend on where the signal lands.  The single-stream loop returns before the handlers
// are installed and keeps the reference's behaviour (default action).
void on_stop_signal(int)
{
    g_stop_requested.store(true, std::memory_order_relaxed);
}

// --interleaved reader: up to n bytes of stdin, waiting in slices of 50 ms so that a stop request is seen whether stdin is a slow pipe
// (poll times out) or a source that never blocks (checked before every read).  Short count = end of input or stop.
size_t read_stdin(unsigned char* dst, size_t n)
{
    size_t got = 0;
    while(got < n && !g_stop_requested.load(std::memory_order_relaxed))
    {
        pollfd p{0, POLLIN, 0};
        const int pr = poll(&p, 1, 50);
        if(pr < 0 && errno != EINTR) break;
        if(pr <= 0) continue;
        const ssize_t r = read(0, dst + got, n - got);
        if(r > 0) got += static_cast<size_t>(r);
        else if(r == 0 || (errno != EINTR && errno != EAGAIN)) break;
    }
    return got;
}

// one share of the input streams: the loop of `device` decodes global streams [first, first + count)
struct Share
{
    int device = 0, first = 0, count = 0;
};

}  // namespace

int main(int argc, char* const argv[])
{
    DecoderOptions opt;
    bool center_set = false;
    bool skip_wav = false;
    int hop_timeout_ms = 20;
    int connect_timeout_ms = 10000;
    int interleaved = 0;
    bool timing = false;
    std::vector<std::string> input_paths;
    std::vector<std::string> device_list;
    bool read_mode_set = false;
    WidebandOptions wbo;
    StreamOptions so;  // --input-rate, --stream-pings, --stream-levels, --stream-gate
    std::string taps_per_phase_arg;
    int wideband_options = 0, taps_per_phase_options = 0;  // how many options went to take_wideband_option, and how many of them were --taps-per-phase

    static struct option long_options[] = {{"help", no_argument, 0, 0},
                                           {"center-frequency", required_argument, 0, 0},
                                           {"search-step", required_argument, 0, 0},
                                           {"search-width", required_argument, 0, 0},
                                           {"scan-depth", required_argument, 0, 0},
                                           {"read-mode", required_argument, 0, 0},
                                           {"analytic-method", required_argument, 0, 0},
                                           {"nbadsync-threshold", required_argument, 0, 0},
                                           {"strict-decode", no_argument, 0, 0},
                                           {"print-bits", no_argument, 0, 0},
                                           {"device", required_argument, 0, 0},
                                           {"inputs", required_argument, 0, 0},
                                           {"reference-decode-cache", no_argument, 0, 0},
                                           {"skip-wav-header", no_argument, 0, 0},
                                           {"hop-timeout-ms", required_argument, 0, 0},
                                           {"inputs-file", required_argument, 0, 0},
                                           {"timing", no_argument, 0, 0},
                                           {"connect-timeout-ms", required_argument, 0, 0},
                                           {"interleaved", required_argument, 0, 0},
                                           {"devices", required_argument, 0, 0},
                                           {"max-results", required_argument, 0, 0},
                                           {"every-slot", no_argument, 0, 0},
                                           {"wideband-rate", required_argument, 0, 0},
                                           {"wideband-format", required_argument, 0, 0},
                                           {"channel-offsets", required_argument, 0, 0},
                                           {"channel-grid", required_argument, 0, 0},
                                           {"wideband-gain", required_argument, 0, 0},
                                           {"taps-per-phase", required_argument, 0, 0},
                                           {"wideband-levels", no_argument, 0, 0},
                                           {"wideband-blanker", optional_argument, 0, 0},
                                           {"wideband-spectrum", required_argument, 0, 0},
                                           {"wideband-pings", required_argument, 0, 0},
                                           {"wideband-waterfall", required_argument, 0, 0},
                                           {"wideband-capture", required_argument, 0, 0},
                                           {"wideband-pings-band", optional_argument, 0, 0},
                                           {"wideband-notch", required_argument, 0, 0},
                                           {"wideband-audio", optional_argument, 0, 0},
                                           {"wideband-gate", optional_argument, 0, 0},
                                           {"input-rate", required_argument, 0, 0},
                                           {"stream-pings", required_argument, 0, 0},
                                           {"stream-levels", no_argument, 0, 0},
                                           {"stream-gate", optional_argument, 0, 0},
                                           {0, 0, 0, 0}};
    while(true)
    {
        int idx = 0;
        const int c = getopt_long(argc, argv, "", long_options, &idx);
        if(c == -1) break;
        if(c != 0) continue;  // unknown option: getopt has printed its own message, carry on like the reference
        if(!strcmp(long_options[idx].name, "input-rate"))
        {
            so.parse_input_rate(optarg);
            continue;
        }
        if(!strcmp(long_options[idx].name, "stream-pings"))
        {
            so.parse_stream_pings(optarg);
            continue;
        }
        if(!strcmp(long_options[idx].name, "stream-levels"))
        {
            so.parse_stream_levels();
            continue;
        }
        if(!strcmp(long_options[idx].name, "stream-gate"))
        {
            so.parse_stream_gate(optarg);
            continue;
        }
        if(!strcmp(long_options[idx].name, "taps-per-phase"))
        {
            // the wideband channeliser's, as ever; with --input-rate and no wideband option it is the resampler's (below)
            taps_per_phase_arg = optarg;
            taps_per_phase_options++;
        }
        if(take_wideband_option(long_options[idx].name, optarg, wbo))
        {
            wideband_options++;
            continue;
        }
        switch(idx)
        {
        case 0: show_help(argv[0]); return 0;
        case 1: opt.center_hz = static_cast<float>(atof(optarg)); center_set = true; break;
        case 2: opt.step_hz = static_cast<float>(atof(optarg)); break;
        case 3: opt.width_hz = static_cast<float>(atof(optarg)); break;
        case 4: opt.scan_depth = atoi(optarg); break;
        case 5: opt.read_mode = atoi(optarg); read_mode_set = true; break;
        case 6: opt.analytic_method = atoi(optarg); break;
        case 7: opt.nbadsync_threshold = atoi(optarg); break;
        case 8: opt.reference_cache_quirk = false; break;
        case 9: opt.print_bits = true; break;
        case 10: opt.device = atoi(optarg); break;
        case 11: split_list(optarg, input_paths); break;
        case 12: opt.reference_cache_quirk = true; break;
        case 13: skip_wav = true; break;
        case 14: hop_timeout_ms = atoi(optarg); break;
        case 15:
        {
            std::ifstream f(optarg);
            if(!f)
            {
                std::cerr << "Cannot open input list " << optarg << std::endl;
                return 2;
            }
            for(std::string line; std::getline(f, line);)
                if(!line.empty()) input_paths.push_back(line);
            break;
        }
        case 16: timing = true; break;
        case 17: connect_timeout_ms = atoi(optarg); break;
        case 18: interleaved = atoi(optarg); break;
        case 19: split_list(optarg, device_list); break;
        case 20: opt.max_results = atoi(optarg); break;
        case 21: opt.every_slot = true; break;
        default: show_help(argv[0]); return 0;
        }
    }

    // --taps-per-phase with --input-rate and nothing else of the wideband options: the resampler's K, and no wideband run
    if(so.input_rate_given() && taps_per_phase_options > 0 && wideband_options == taps_per_phase_options)
    {
        so.parse_taps_per_phase(taps_per_phase_arg);
        wbo = WidebandOptions();
    }

    // --wideband-pings-band: its CENTRE defaults to --center-frequency, wherever on the line that stood
    if(wbo.ping_band && !parse_wideband_ping_band(wbo.ping_band_arg, center_set ? static_cast<int>(std::lrint(opt.center_hz)) : 0, wbo) && wbo.parse_error.empty())
        wbo.parse_error = "bad value for --wideband-pings-band: '" + wbo.ping_band_arg + "'";

    // --wideband-audio likewise; a value the design refuses is reported with the design's own text
    if(std::string why; wbo.audio && !parse_wideband_audio(wbo.audio_arg, center_set ? static_cast<int>(std::lrint(opt.center_hz)) : 0, wbo, why) && wbo.parse_error.empty())
        wbo.parse_error = why.empty() ? "bad value for --wideband-audio: '" + wbo.audio_arg + "'" : "--wideband-audio: " + why;

    // --wideband-rate: checked in full before anything touches the library
    const bool wideband = wbo.any_option;
    if(wideband)
    {
        std::string why;
        if(!input_paths.empty() || interleaved != 0 || !device_list.empty())
            why = "--wideband-rate decodes the channels of one stdin stream on one device: it excludes --inputs, --inputs-file, --interleaved and --devices";
        else if(read_mode_set && opt.read_mode != 2)
            why = "--wideband-rate produces IQ channels: it excludes --read-mode=" + std::to_string(opt.read_mode);
        else
            why = check_wideband_options(wbo);
        if(!why.empty())
        {
            std::cerr << why << std::endl;
            return 2;
        }
        opt.read_mode = 2;
    }

    // the options on the audio streams: checked in full, and the header of --input-rate=wav read, before anything touches the library
    bool wav_header_read = false;
    if(const std::string why = so.check(wideband, opt.read_mode, !input_paths.empty(), interleaved, skip_wav, wav_header_read); !why.empty())
    {
        std::cerr << why << std::endl;
        return 2;
    }

    if(!center_set)
    {
        if(opt.read_mode == 1) opt.center_hz = 1500.0f;
        else if(opt.read_mode == 2) opt.center_hz = 0.0f;
        else
        {
            std::cerr << "Wrong read mode " << opt.read_mode << std::endl;
            return 2;
        }
    }
    if(opt.read_mode != 1 && opt.read_mode != 2)
    {
        // reached only with an explicit centre frequency: the reference enters its loop, reports the mode and stops
        std::cerr << "Unsupported mode. Exit." << std::endl;
        std::cout << "Done" << std::endl;
        return 0;
    }

    if(interleaved < 0 || (interleaved > 0 && !input_paths.empty()))
    {
        std::cerr << "--interleaved=N takes N >= 1 streams from stdin and excludes --inputs" << std::endl;
        return 2;
    }
    // --wideband-rate: the entries resolved and the files opened before anything touches the library (wideband_run.h)
    WidebandRun wideband_run(wbo);
    if(wideband && !wideband_run.prepare()) return 2;
    const bool batched = interleaved > 0 || !input_paths.empty() || wideband;
    const int nch = wideband ? static_cast<int>(wbo.offsets.size()) : interleaved > 0 ? interleaved : (input_paths.empty() ? 1 : static_cast<int>(input_paths.size()));
    opt.profile = timing && batched;
    // the options on the audio streams: the entries resolved and the log opened before anything touches the library
    if(std::string why; !so.prepare(nch, why))
    {
        std::cerr << why << std::endl;
        return 2;
    }
    {
        // one descriptor per stream plus what the runtime opens: lift the soft limit when the hard limit allows
        rlimit lim{};
        const rlim_t want = static_cast<rlim_t>(nch) + 256;
        if(getrlimit(RLIMIT_NOFILE, &lim) == 0 && lim.rlim_cur < want)
        {
            lim.rlim_cur = (lim.rlim_max == RLIM_INFINITY || lim.rlim_max > want) ? want : lim.rlim_max;
            setrlimit(RLIMIT_NOFILE, &lim);
        }
    }

    // which device decodes which streams: contiguous shares, sizes differing by at most one
    std::vector<int> devices;
    if(device_list.size() == 1 && device_list[0] == "all")
    {
        int32_t n = 0;
        if(msk144_device_count(&n) != MSK144_OK)
        {
            std::cerr << "msk144hip: " << msk144_last_error(nullptr) << std::endl;
            return 2;
        }
        for(int d = 0; d < n; d++) devices.push_back(d);
    }
    else
        for(const std::string& d : device_list)
        {
            if(d.empty() || d.find_first_not_of("0123456789") != std::string::npos)
            {
                std::cerr << "--devices takes HIP device ordinals (0,1,...) or 'all', not '" << d << "'" << std::endl;
                return 2;
            }
            devices.push_back(atoi(d.c_str()));
        }
    if(devices.empty()) devices.push_back(opt.device);
    if(devices.size() > 1 && !batched)
    {
        std::cerr << "--devices splits the streams of --inputs / --inputs-file / --interleaved; a single stdin stream runs on one device (--device=N)" << std::endl;
        return 2;
    }
    std::vector<Share> shares(std::min<size_t>(devices.size(), static_cast<size_t>(nch)));  // a device without a stream gets no loop
    for(size_t i = 0; i < shares.size(); i++)
    {
        shares[i].device = devices[i];
        split_streams(nch, static_cast<int>(shares.size()), static_cast<int>(i), shares[i].first, shares[i].count);
    }
    opt.device = shares[0].device;
    opt.channels = shares[0].count;

    LinePrinter printer;
    LoopOptions lo;
    lo.hop_timeout_ms = hop_timeout_ms;
    lo.connect_timeout_ms = connect_timeout_ms;
    lo.skip_wav = skip_wav;
    lo.tag_channels = nch > 1;
    std::unique_ptr<WindowDecoder> single;
    std::unique_ptr<DeviceLoop> first_loop;
    if(batched) first_loop = std::make_unique<DeviceLoop>(opt, 0, lo, printer);
    else single = std::make_unique<WindowDecoder>(opt);
    WindowDecoder& dec = batched ? first_loop->decoder() : *single;
    if(!dec.ok())
    {
        std::cerr << "msk144hip: " << dec.error() << std::endl;
        return 2;
    }

    // The reference's parameter block (main.cu:233-252), line for line.  Its four launch-geometry lines are kept with the
    // values the reference would print for these options (F blocks x 256 threads; F*(depth*8) blocks x 160 threads); the
    // geometry actually used here follows under its own names.
    const int F = dec.num_freqs(), D = dec.scan_depth();
    std::cerr << "Actual parameters:" << std::endl
              << "Center Frequency: " << opt.center_hz << "Hz" << std::endl
              << "Search Step: " << opt.step_hz << "Hz" << std::endl
              << "Search Width: " << opt.width_hz << "Hz" << std::endl
              << "Scan Depth: " << D << std::endl
              << "Left Boundary: " << dec.left_bound() << "Hz" << std::endl
              << "Right Boundary: " << dec.right_bound() << "Hz" << std::endl
              << "Read Mode: (" << mode_name(opt.read_mode) << ")" << std::endl;
    if(opt.read_mode == 1) std::cerr << "Analytic Method: " << opt.analytic_method << std::endl;
    std::cerr << "Badsync Threshold: " << opt.nbadsync_threshold << std::endl
              << "Scan-kernel CUDA blocks: " << F << std::endl
              << "Scan-kernel CUDA threads: " << 256 << std::endl
              << "Softbit-kernel CUDA blocks: " << F << "*" << D * 8 << "=" << (F * D * 8) << std::endl
              << "Softbit-kernel CUDA threads: " << 160 << std::endl
              << std::endl;
    std::cerr << "msk144hipdecoder: " << F << " frequency hypotheses x " << D << " patterns x 8 = " << F * D * 8 << " candidates per window; HIP workgroups per window: scan "
              << F << " x 512, softbits " << F << " x 512, LDPC one wave per gated candidate" << std::endl;
    if(batched && !wideband) std::cerr << "msk144hipdecoder: " << nch << " input streams per GPU batch" << (interleaved > 0 ? " (interleaved on stdin)" : "") << ", hop timeout " << hop_timeout_ms << " ms" << std::endl;
    if(wideband && !wideband_run.configure(dec.handle())) return 2;
    if(so.any())
    {
        std::string why;
        if(!so.configure(dec.handle(), shares[0].first, shares[0].count, why))
        {
            std::cerr << "msk144hip: " << why << std::endl;
            return 2;
        }
        so.attach(dec, shares[0].first);
    }
    if(shares.size() > 1)
        for(const Share& sh : shares) std::cerr << "msk144hipdecoder: device " << sh.device << " decodes streams " << sh.first << ".." << sh.first + sh.count - 1 << std::endl;

    const size_t half = dec.hop_bytes();  // with --input-rate a hop is 2592 x P/Q samples
    const size_t win_bytes = 2 * half;
    const size_t unit = (opt.read_mode == 1) ? sizeof(int16_t) : sizeof(int8_t);  // the reference counts items of this size

    if(!batched)
    {
        // ---- the reference's loop: one stream on stdin, blocking reads (main.cu:261-422) ----
        if(skip_wav && !wav_header_read)
        {
            unsigned char hdr[44];
            if(fread(hdr, 1, sizeof(hdr), stdin) != sizeof(hdr)) std::cerr << "Incomplete read error. rc=0" << std::endl;
        }
        if(so.any())
        {
            // the same loop over the library's hop ring (msk144_push_rate_hops at the input rate, msk144_push_hops for the levels and
            // pings of a 12 kHz stream, which a whole-window submit does not produce): a hop carries its new samples only
            WindowDecoder::HopStage hs;
            std::vector<std::vector<FilteredResult>> all;
            bool first = true;
            while(true)
            {
                if(!dec.hop_stage(0, hs))
                {
                    std::cerr << "msk144hip: " << dec.error() << std::endl;
                    return 2;
                }
                const size_t want = (first ? win_bytes : half) / unit;
                size_t rc = 0;
                if(first)
                {
                    rc = fread(hs.first_halves, unit, half / unit, stdin);
                    if(rc == half / unit) rc += fread(hs.hops, unit, half / unit, stdin);
                }
                else rc = fread(hs.hops, unit, want, stdin);
                if(rc != want)
                {
                    std::cerr << "Incomplete read error. rc=" << rc << std::endl;
                    break;
                }
                hs.streams[0] = 0;
                hs.is_first[0] = first ? 1 : 0;
                first = false;
                const auto t0 = Clock::now();
                if(!dec.submit_hops(0, 1) || !dec.collect(0, all))
                {
                    std::cerr << "msk144hip: " << dec.error() << std::endl;
                    return 2;
                }
                if(dec.last_hop_overflowed()) std::cerr << "msk144hipdecoder: the window held more decodes than the result list (raise --max-results): the list was cut, decoding goes on" << std::endl;
                warn_if_late(std::chrono::duration_cast<std::chrono::milliseconds>(Clock::now() - t0).count());
                for(const FilteredResult& l : all[0]) std::cout << l.format_line() << std::endl;
            }
            so.finish(std::cerr);
            std::cout << "Done" << std::endl;
            return 0;
        }
        std::vector<unsigned char> ring(win_bytes, 0);
        bool first = true;
        std::vector<FilteredResult> lines;
        while(true)
        {
            unsigned char* w = ring.data();
            size_t want, rc;
            if(first)
            {
                want = win_bytes / unit;
                rc = fread(w, unit, want, stdin);
            }
            else
            {
                memcpy(w, w + half, half);
                want = half / unit;
                rc = fread(w + half, unit, want, stdin);
            }
            first = false;
            if(rc != want)
            {
                std::cerr << "Incomplete read error. rc=" << rc << std::endl;
                break;
            }
            const auto t0 = Clock::now();
            if(!dec.process(ring.data(), lines))
            {
                std::cerr << "msk144hip: " << dec.error() << std::endl;
                return 2;
            }
            if(dec.last_hop_overflowed()) std::cerr << "msk144hipdecoder: the window held more decodes than the result list (raise --max-results): the list was cut, decoding goes on" << std::endl;
            warn_if_late(std::chrono::duration_cast<std::chrono::milliseconds>(Clock::now() - t0).count());
            for(const FilteredResult& l : lines) std::cout << l.format_line() << std::endl;
        }
        std::cout << "Done" << std::endl;
        return 0;
    }

    // ---- several streams: one DeviceLoop per listed device (stream_loop.h), each with its contiguous share of the streams ----
    std::vector<std::unique_ptr<DeviceLoop>> loops;
    loops.push_back(std::move(first_loop));
    for(size_t i = 1; i < shares.size(); i++)
    {
        DecoderOptions o = opt;
        o.device = shares[i].device;
        o.channels = shares[i].count;
        loops.push_back(std::make_unique<DeviceLoop>(o, shares[i].first, lo, printer));
        if(!loops.back()->ok())
        {
            std::cerr << "msk144hip: device " << o.device << ": " << loops.back()->error() << std::endl;
            return 2;
        }
    }
    for(size_t i = 0; i < loops.size(); i++)
    {
        if(i > 0 && so.any())
        {
            std::string why;
            if(!so.configure(loops[i]->decoder().handle(), shares[i].first, shares[i].count, why))
            {
                std::cerr << "msk144hip: device " << shares[i].device << ": " << why << std::endl;
                return 2;
            }
            so.attach(loops[i]->decoder(), shares[i].first);
        }
        if(wideband) loops[i]->use_wideband(&wideband_run);
        else if(interleaved > 0) loops[i]->use_feed();
        else if(!loops[i]->open_inputs(std::vector<std::string>(input_paths.begin() + shares[i].first, input_paths.begin() + shares[i].first + shares[i].count)))
        {
            std::cerr << loops[i]->error() << std::endl;
            return 2;
        }
    }
    {
        struct sigaction sa{};
        sa.sa_handler = on_stop_signal;
        sigemptyset(&sa.sa_mask);
        sigaction(SIGINT, &sa, nullptr);
        sigaction(SIGTERM, &sa, nullptr);
    }
    const auto run_since = Clock::now();
    for(auto& l : loops) l->start();

    if(wideband)
    {
        // one push per hop on stdin: 5184 x P/Q wideband samples, then 2592 x P/Q (Q divides 2592)
        const size_t wb_sample = static_cast<size_t>(msk144wb::sample_bytes(wbo.format));
        const msk144wb::RateRatio rr = msk144wb::rate_ratio(wbo.rate_hz);
        std::vector<unsigned char> block;
        bool first_block = true;
        while(!g_stop_requested.load(std::memory_order_relaxed))
        {
            block.resize((first_block ? MSK144_WINDOW_SAMPLES : MSK144_HOP_SAMPLES) / static_cast<size_t>(rr.Q) * static_cast<size_t>(rr.P) * wb_sample);
            const size_t got = read_stdin(block.data(), block.size());
            if(g_stop_requested.load(std::memory_order_relaxed)) break;
            if(got != block.size())
            {
                printer.log("Incomplete read error. rc=" + std::to_string(got / wb_sample));
                break;
            }
            if(!loops[0]->feed_raw(block.data(), block.size())) break;
            first_block = false;
        }
        loops[0]->feed_end();
    }
    else if(interleaved > 0)
    {
        // one block per hop on stdin: the hop of stream 0, then of stream 1, ... (the reference's fread, but interruptible); every
        // loop receives the slice of its own streams.  A stop request ends the reader at the next block boundary at the latest: the
        // blocks already handed over are decoded and printed.
        if(skip_wav)
        {
            unsigned char hdr[44];
            if(read_stdin(hdr, sizeof(hdr)) != sizeof(hdr) && !g_stop_requested.load()) printer.log("Incomplete read error. rc=0");
        }
        std::vector<unsigned char> block;
        bool first_block = true;
        while(!g_stop_requested.load(std::memory_order_relaxed))
        {
            const size_t need = first_block ? win_bytes : half;
            block.resize(need * nch);
            const size_t got = read_stdin(block.data(), block.size());
            if(g_stop_requested.load(std::memory_order_relaxed)) break;  // a partial block is dropped, like a partial hop of --inputs
            if(got != block.size())
            {
                printer.log("Incomplete read error. rc=" + std::to_string(got / unit));
                break;
            }
            bool alive = true;
            for(size_t i = 0; i < loops.size() && alive; i++) alive = loops[i]->feed(block.data() + need * shares[i].first, need);
            if(!alive) break;
            first_block = false;
        }
        for(auto& l : loops) l->feed_end();
    }

    int rc = 0;
    for(auto& l : loops) rc = std::max(rc, l->join());
    if(rc != 0) return rc;

    if(g_stop_requested.load()) std::cerr << "msk144hipdecoder: stopped by signal; hops in flight were finished" << std::endl;
    long total_hops = 0, total_late = 0, batches = 0, overflowed = 0;
    long long worst = 0;
    for(size_t i = 0; i < loops.size(); i++)
    {
        const LoopStats& ls = loops[i]->stats();
        total_hops += ls.hops;
        total_late += ls.late;
        batches += ls.batches;
        overflowed += ls.overflowed_hops;
        worst = std::max(worst, ls.worst_ms);
        for(int c = 0; c < loops[i]->streams(); c++)
        {
            const DeviceLoop::StreamReport r = loops[i]->stream_report(c);
            if(r.late) std::cerr << "ch=" << shares[i].first + c << ": " << r.late << " of " << r.hops << " hops answered later than 210 ms (worst " << r.worst_ms << " ms)" << std::endl;
        }
        if(loops.size() > 1)
            std::cerr << "msk144hipdecoder: device " << shares[i].device << " (streams " << shares[i].first << ".." << shares[i].first + shares[i].count - 1 << "): " << ls.batches << " batches, "
                      << ls.hops << " stream hops, " << ls.late << " late, worst latency " << ls.worst_ms << " ms" << std::endl;
    }
    std::cerr << "msk144hipdecoder: " << batches << " batches, " << total_hops << " stream hops, " << total_late << " late, worst latency " << worst << " ms" << std::endl;
    if(wideband) wideband_run.print_summary(loops[0]->decoder().handle());
    so.finish(std::cerr);
    if(overflowed) std::cerr << "msk144hipdecoder: " << overflowed << " hops overflowed the result list (lists cut, see above)" << std::endl;
    if(timing)
    {
        const double wall_s = std::chrono::duration<double>(Clock::now() - run_since).count();
        auto row = [](const char* name, const Accumulator& a) { fprintf(stderr, "msk144hipdecoder timing: %-34s mean %9.3f ms  max %9.3f ms\n", name, a.mean(), a.worst); };
        for(size_t i = 0; i < loops.size(); i++)
        {
            const LoopStats& ls = loops[i]->stats();
            if(loops.size() > 1) fprintf(stderr, "msk144hipdecoder timing: ---- device %d: %d streams (%d..%d), own ingest and post-processing threads ----\n", shares[i].device, shares[i].count, shares[i].first, shares[i].first + shares[i].count - 1);
            fprintf(stderr, "msk144hipdecoder timing: %d streams, %ld batches in %.2f s wall; per batch (host wall time):\n", shares[i].count, ls.batches, loops.size() > 1 ? ls.wall_s : wall_s);
            row("ingest (read syscalls, all streams)", ls.ingest);
            row("copy new hops into pinned slot", ls.assemble);
            row("submit (3 asynchronous calls)", ls.submit);
            row("wait for GPU + D2H (post thread)", ls.wait);
            row("post-processing (text, SNR, filter)", ls.post);
            row("print", ls.print);
            row("batch released -> lines printed", ls.latency);
            fprintf(stderr, "msk144hipdecoder timing: records per batch mean %.0f max %.0f\n", ls.records.mean(), ls.records.worst);
            const float* dev = ls.device_ms;
            if(ls.have_device_ms)
                fprintf(stderr, "msk144hipdecoder timing: device per batch (HIP events): H2D %.3f  front end %.3f  scan %.3f  softbits %.3f  index %.3f  LDPC %.3f  collect %.3f  D2H %.3f ms\n",
                        dev[MSK144_T_H2D], dev[MSK144_T_FRONTEND], dev[MSK144_T_SCAN], dev[MSK144_T_SOFTBITS], dev[MSK144_T_INDEX], dev[MSK144_T_LDPC], dev[MSK144_T_COLLECT], dev[MSK144_T_D2H]);
        }
    }
    std::cout << "Done" << std::endl;
    return 0;
}
