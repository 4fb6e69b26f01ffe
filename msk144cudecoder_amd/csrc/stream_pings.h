// Per-stream levels and ping detection on the audio hops of the stream path (msk144_set_stream_pings, include/msk144hip.h "Stream
// levels and pings").  Plain C++: the kernel (stream_pings.hip), the library's host code, the program and libmsk144host.so all take
// the arithmetic from here, and the ping rule itself from wideband.h (ping_rank, ping_history_min, ping_reference, ping_up,
// ping_history_put) - it is not restated.
//
// Per listed position j of a push, for stream s = streams[j], over the new 12 kHz int16 samples x of that push as the hop ring's
// staging holds them (behind the resampler when an input rate is set): 2592 samples = 27 blocks of 96 for a later hop, 5184 = 54
// blocks for a first hop (the first-half row, then the hop row).
//
//   E[b]   = min(2^22 - 1, (sum over n < 96 of x[96b + n]^2) >> shift), the sum exact: it reaches 96 x 2^30 and needs 64 bits (two
//            squares fit an unsigned dword, a block does not);
//   rule   the wideband detector's on E with the scale fixed at 1.0f, one PingHistory per stream;
//   restart  on the stream's is_first hop and on its first listed hop after msk144_set_stream_pings; unlisted streams keep their state;
//   levels exact integer sums over the same samples (Level).
//
// The shift.  E is capped at 2^22 - 1 so that the 22-step select and the peak key of the wideband kernel serve unchanged.  Audio of
// rms r LSB gives a block sum near 96 r^2, so shift 12 maps r to E = 96 r^2 / 4096: r = 30 LSB still leaves a quiet level of about
// 17 (96 x 900 / 4096 = 21 at the mean, its lower quartile a little under), and the cap is reached at r^2 = 2^34 / 96, r = 13 377 LSB.
// Shift 12 is therefore a design parameter derived from the cap: 30 to about 13 000 LSB rms lie inside the range.  Louder audio
// saturates, and the saturated blocks are counted (Level::saturated_blocks).
//
// The default ratio was found as MSK144_PING_BAND_RATIO_Q4 was: the smallest multiple of 0.25 at which no block of noise alone is up.
// tools/stream_pings_sim.py, the Python model (stream_pings.StreamPings) on Gaussian noise band-limited to 300..2700 Hz, shift 12,
// memory 8, min_ref 1 (the default floor of 96 would hide the quiet stream), 3000 hops = 81 027 blocks per level, seed 1:
//
//   rms LSB   quiet level (median)   worst E/R   up at 2.0    up at 3.0   up at 3.25   up at 3.5
//        30                     17      3.400     2.101 %     0.001 %      0.001 %           0
//       100                    196      2.994     2.192 %           0            0           0
//      1000                  19598      3.113     2.068 %     0.002 %            0           0
//
// One block of the quiet stream, where E and R are small integers, reached 3.40 x the reference; seeds 2 and 3 of the same run gave
// worst ratios of 3.214 and 3.113 and would have allowed 3.25, the ping band's value.  The default is the smallest multiple of 0.25
// at which no block of any of the three runs (243 081 blocks per level) is up: 3.5 x the reference, ratio_q4 = 56.  A whole-channel
// energy on SSB audio is already close to an in-band one, which is why it lands next to the ping band's 52.  It rests on these numpy
// runs alone; nothing was measured on the air.
#pragma once

#include "wideband.h"

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace msk144sp
{

constexpr int kBlock = msk144wb::kPingBlock;           // 96 samples, 8 ms
constexpr int kHopBlocks = msk144wb::kHopBlocks;       // 27
constexpr int kMaxBlocks = msk144wb::kPingMaxBlocks;   // 54
constexpr int kHopSamples = kHopBlocks * kBlock;       // 2592
constexpr int32_t kEnergyCap = (1 << msk144wb::kPingEnergyBits) - 1;
constexpr int kMaxShift = 24;
constexpr int kDefaultShift = 12;
constexpr int kDefaultRatioQ4 = 56;                    // 3.5 x the reference: the table above

// msk144_stream_pings_params, field for field
struct Params
{
    int32_t ratio_q4 = kDefaultRatioQ4;
    int32_t memory = 8;
    int32_t min_ref = 96;
    int32_t shift = kDefaultShift;
};

// msk144_stream_level, field for field: the levels of one position's samples.  With an input rate set they are the levels of the
// resampled stream: clipping of the input at Fs is smeared by the filter, and the resampler's clamp count is a separate figure.
struct Level
{
    int64_t sum;               // sum of x
    int64_t sum_sq;            // sum of x^2
    int32_t peak;              // max |x|, 0..32768
    int32_t full_scale;        // samples equal to 32767 or -32768
    int32_t samples;           // 2592 or 5184
    int32_t saturated_blocks;  // blocks whose E is the cap
};
static_assert(sizeof(Level) == 32, "msk144_stream_level is 32 bytes");

inline msk144wb::PingParams rule(const Params& p) { return msk144wb::PingParams{p.ratio_q4, p.memory, p.min_ref}; }

// The rules of msk144_set_stream_pings that need no handle.  Empty string = valid.
inline std::string check_params(const Params& p)
{
    const std::string why = msk144wb::check_pings(rule(p));
    if(!why.empty()) return why;
    if(p.shift < 0 || p.shift > kMaxShift) return "stream ping shift must lie within 0..24";
    return std::string();
}

// E of a block from its exact sum of squares
MSK144WB_HD inline int32_t block_energy(uint64_t sum_sq, int shift)
{
    const uint64_t e = sum_sq >> shift;
    return e > static_cast<uint64_t>(kEnergyCap) ? kEnergyCap : static_cast<int32_t>(e);
}

// One position on the host: x[96 nb] the samples of the push, nb = 27 or 54.  Writes E[nb] and returns the levels.
inline Level levels_and_energies(const int16_t* x, int nb, int shift, int32_t* E)
{
    Level l{};
    l.samples = nb * kBlock;
    for(int b = 0; b < nb; b++)
    {
        uint64_t sq = 0;
        for(int n = b * kBlock; n < (b + 1) * kBlock; n++)
        {
            const int32_t v = x[n];
            const int32_t a = v < 0 ? -v : v;
            l.sum += v;
            sq += static_cast<uint64_t>(static_cast<int64_t>(v) * v);
            if(a > l.peak) l.peak = a;
            if(v == 32767 || v == -32768) l.full_scale++;
        }
        l.sum_sq += static_cast<int64_t>(sq);
        E[b] = block_energy(sq, shift);
        if(E[b] == kEnergyCap) l.saturated_blocks++;
    }
    return l;
}

// The detector of a handle on the host: one history and one seen-bit per stream.  What libmsk144host.so holds the Python model to.
class Model
{
public:
    Model(int streams, const Params& p) : p_(p), state_(static_cast<size_t>(streams)), seen_(static_cast<size_t>(streams), 0) {}

    int streams() const { return static_cast<int>(state_.size()); }

    // one listed position: stream s, its samples (5184 when first, else 2592); energies[54], zero behind nb
    msk144wb::PingRecord push(int s, bool first, const int16_t* x, Level& level, int32_t* energies)
    {
        const int nb = first ? kMaxBlocks : kHopBlocks;
        for(int b = nb; b < kMaxBlocks; b++) energies[b] = 0;
        level = levels_and_energies(x, nb, p_.shift, energies);
        const bool restart = first || !seen_[static_cast<size_t>(s)];
        seen_[static_cast<size_t>(s)] = 1;
        return msk144wb::ping_record(rule(p_), state_[static_cast<size_t>(s)], restart, 1.0f, energies, nb);
    }

private:
    Params p_;
    std::vector<msk144wb::PingHistory> state_;
    std::vector<uint8_t> seen_;
};

// The event rule per stream: PingTracker's, one tracker per stream, so that `start` counts the blocks of that stream alone from its
// first sample.  Events come out by push, then by position (ascending stream), then by start.  Host only: the program's log.
class Tracker
{
public:
    Tracker(int streams, int min_blocks)
    {
        for(int s = 0; s < streams; s++) per_.emplace_back(1, min_blocks);
    }

    // position j of a push: the record and energies[54] of stream s
    void push(int s, const msk144wb::PingRecord& r, const int32_t* energies, std::vector<msk144wb::PingEvent>& out)
    {
        const size_t at = out.size();
        per_[static_cast<size_t>(s)].push(&r, energies, out);
        for(size_t i = at; i < out.size(); i++) out[i].channel = s;
    }

    // the end of every stream, ascending
    void close(std::vector<msk144wb::PingEvent>& out)
    {
        for(size_t s = 0; s < per_.size(); s++)
        {
            const size_t at = out.size();
            per_[s].close(out);
            for(size_t i = at; i < out.size(); i++) out[i].channel = static_cast<int32_t>(s);
        }
    }

    int streams() const { return static_cast<int>(per_.size()); }
    int64_t events(int s) const { return per_[static_cast<size_t>(s)].events(); }
    int64_t up_blocks(int s) const { return per_[static_cast<size_t>(s)].up_blocks(); }
    int64_t total_blocks(int s) const { return per_[static_cast<size_t>(s)].total_blocks(); }

private:
    std::vector<msk144wb::PingTracker> per_;
};

// One line of the event log (--stream-pings=FILE): the wideband line without the offset
inline std::string event_line(const msk144wb::PingEvent& e)
{
    char buf[256];
    const long long s = static_cast<long long>(e.start) * 8, d = static_cast<long long>(e.blocks) * 8;
    snprintf(buf, sizeof(buf), "ping ch=%d start=%lld.%03lld dur=%lld.%03lld blocks=%lld peak=%d ref=%d peak_db=%.1f", e.channel, s / 1000, s % 1000, d / 1000, d % 1000,
             static_cast<long long>(e.blocks), e.peak, e.reference, 10.0 * std::log10(static_cast<double>(e.peak) / static_cast<double>(e.reference)));
    return buf;
}

}  // namespace msk144sp
