// The stream gate: only the streams with activity are decoded (msk144_set_stream_gate, include/msk144hip.h "Stream gate").  Plain
// C++: the kernels (stream_gate.hip), the library's host code, the program and libmsk144host.so all take the rule from here, and
// the rule itself is wideband.h's - gate_step, since_next, ping_up - applied per listed position; it is not restated.
//
// Per listed position j of a push, for stream s = streams[j]:
//
//   mask   ratio_q4 == 0: records[j].up_mask of the push's stream-ping record; else bit b < records[j].blocks is
//          ping_up(E[j][b], records[j].reference, ratio_q4) on the energies and reference the detector left; 0 while the detector is off;
//   step   in = gate_step(since[s], is_first[j], is_first[j] || restart[j], mask, always[s], hold, min_up), restart[j] the stream's
//          first listed hop since the `set`; `since` is by stream, and a stream a push does not list keeps it;
//   list   the positions with `in`, ascending; the first max_streams are listed, the rest only counted.
//
// The gate's own ratio.  The detector's default ratio (3.5 x, stream_pings.h) is set so that the ping log stays empty on noise; a
// gate may trade noise windows for weaker pings, which is what ratio_q4 != 0 is for.  tools/stream_gate_sim.py: synth.synth_audio
// streams - noise of 1000 LSB with one ping of three frames (216 ms) at 1500 Hz every eight hops, 40 pings per level, behind a
// 300..2700 Hz audio filter - through stream_pings.StreamPings at its defaults and one stream_pings.StreamGate per RATIO (hold 1,
// min_up 1), against the oracle decoder (width 20 Hz, step 2 Hz, depth 4) on the 120 windows per level that overlap a ping; seed 1.
// Of the windows the oracle decodes, those the gate lists, and of 3000 windows of noise alone, those it lists:
//
//   ping dB   oracle decodes   at 3.5 (the detector's)   at 2.5       at 2.0   at 1.75   at 1.5
//        -4               44            1    2.3 %      36  81.8 %     all      all       all
//        -2               63            4    6.3 %      62  98.4 %     all      all       all
//         0               90           67   74.4 %      all            all      all       all
//    +2..+10    95 .. 102 each          all              all            all      all       all
//       all              689          564   81.9 %     680  98.7 %     689      689       689
//   noise-only windows listed    0 of 3000             4.63 %         67.1 %   97.6 %    100 %
//
// At its default the gate loses what the detector does not see: a quarter of the decodes at 0 dB and nearly all below; from +2 dB
// up it lost none.  RATIO 2.5 kept 98.7 % of all decodes and listed 4.6 % of the noise windows; at 2.0 and below the gate keeps
// every decode and saves little or nothing, as most noise windows have one block that high.  The default stays 0, the detector's
// mask: a run that must not lose weak pings sets 2.5.  This is a CPU simulation of the models and the oracle decoder; nothing was run
// on the air.
#pragma once

#include "wideband.h"

#include <cstdint>
#include <string>
#include <vector>

namespace msk144sg
{

constexpr int kMaxBlocks = msk144wb::kPingMaxBlocks;   // 54: a row of the detector's energies

// msk144_stream_gate_params, field for field.  hold and min_up are the wideband gate's design parameters; ratio_q4 0 adds no number.
struct Params
{
    int32_t hold = 1, min_up = 1, max_streams = 0, ratio_q4 = 0;   // max_streams 0: every stream; ratio_q4 0: the detector's own up mask
};

// max_streams as the rule uses it: 0 stands for every stream
inline int32_t cap(const Params& p, int channels) { return p.max_streams ? p.max_streams : channels; }

// The rules of msk144_set_stream_gate that need no handle.  Empty string = valid.
inline std::string check_params(const Params& p, int channels)
{
    const std::string why = msk144wb::check_gate(msk144wb::GateParams{p.hold, p.min_up, 0}, channels);
    if(!why.empty()) return "stream " + why;
    if(p.max_streams < 0 || p.max_streams > channels) return "stream gate max_streams must lie within 1.." + std::to_string(channels) + ", or be 0 for all";
    if(p.ratio_q4 != 0 && (p.ratio_q4 < 16 || p.ratio_q4 > 65535)) return "stream gate ratio_q4 must be 0 (the detector's mask) or lie within 16..65535";
    return std::string();
}

// The gate's own mask of one position: E[54] and the record as the detector left them
MSK144WB_HD inline uint64_t ratio_mask(const msk144wb::PingRecord& r, const int32_t* E, int32_t ratio_q4)
{
    uint64_t m = 0;
    for(int b = 0; b < r.blocks && b < kMaxBlocks; b++)
        if(msk144wb::ping_up(E[b], r.reference, ratio_q4)) m |= 1ull << b;
    return m;
}

// The gate of a handle on the host: `since` and one seen-bit per stream.  What the plan kernel computes, and through
// libmsk144host.so the yardstick of stream_pings.StreamGate.
class Model
{
public:
    Model(int streams, const Params& p, const uint8_t* always)
        : p_(p), since_(static_cast<size_t>(streams), msk144wb::kSinceQuiet), always_(static_cast<size_t>(streams), 0), seen_(static_cast<size_t>(streams), 0)
    {
        for(int s = 0; always && s < streams; s++) always_[static_cast<size_t>(s)] = always[s] != 0;
    }

    int streams() const { return static_cast<int>(since_.size()); }
    int32_t since(int s) const { return since_[static_cast<size_t>(s)]; }

    // One push of n listed positions: streams[n] ascending, is_first[n], records[n] and energies[n][54] of the detector, or both
    // nullptr: the detector is off.  Appends the listed positions and returns the total.
    int32_t push(int n, const int32_t* streams, const uint8_t* is_first, const msk144wb::PingRecord* records, const int32_t* energies, std::vector<int32_t>& out)
    {
        const int32_t most = cap(p_, this->streams());
        int32_t total = 0;
        for(int j = 0; j < n; j++)
        {
            const size_t s = static_cast<size_t>(streams[j]);
            const bool first = is_first[j] != 0;
            const uint64_t mask = !records ? 0ull : p_.ratio_q4 == 0 ? records[j].up_mask : ratio_mask(records[j], energies + static_cast<size_t>(j) * kMaxBlocks, p_.ratio_q4);
            const bool clear = first || !seen_[s];
            seen_[s] = 1;
            if(msk144wb::gate_step(since_[s], first, clear, mask, always_[s] != 0, p_.hold, p_.min_up) && total++ < most) out.push_back(j);
        }
        return total;
    }

private:
    Params p_;
    std::vector<int32_t> since_;
    std::vector<uint8_t> always_, seen_;
};

}  // namespace msk144sg
