// msk144hipdecoder --stream-pings and --stream-levels: the options, the library entries of the per-stream levels and pings
// (include/msk144hip.h "Stream levels and pings"), the event log and the end-of-run lines.  Header-only: the entries are resolved
// with dlsym when an option is given, so a program built against a library without them still links and runs in every other mode.
// The event rule and the arithmetic are csrc/stream_pings.h's; nothing here touches the GPU or waits for it.
#pragma once

#include "../../include/msk144hip.h"
#include "../csrc/stream_pings.h"
#include "wideband_cli.h"

#include <cerrno>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace msk144host
{

struct StreamPingsApi
{
    int (*set)(msk144_handle*, const msk144_stream_pings_params*) = nullptr;
    int (*slot)(msk144_handle*, int32_t, const msk144_wideband_ping**, const msk144_stream_level**, const int32_t**, int32_t*) = nullptr;

    bool resolve(std::string& err)
    {
        const ApiEntry entries[] = {{"msk144_set_stream_pings", &set}, {"msk144_stream_pings_slot", &slot}};
        return resolve_entries(entries, 2, "stream pings", ": --stream-pings and --stream-levels need a library built from these sources", err);
    }
};

// What the run has seen of one stream, from the levels of its hops
struct StreamLevelSum
{
    unsigned __int128 sum_sq = 0;
    long long samples = 0, full_scale = 0, hops = 0, zero_hops = 0;
    int32_t peak = 0;

    void add(const msk144sp::Level& l)
    {
        sum_sq += static_cast<unsigned __int128>(static_cast<uint64_t>(l.sum_sq));
        samples += l.samples;
        full_scale += l.full_scale;
        hops++;
        zero_hops += l.peak == 0 ? 1 : 0;
        peak = l.peak > peak ? l.peak : peak;
    }
    double rms() const { return samples ? std::sqrt(static_cast<double>(sum_sq) / static_cast<double>(samples)) : 0.0; }
};

// "FILE[:RATIO[:MIN_BLOCKS[:MEMORY[:SHIFT]]]]": an empty field keeps its default
inline bool parse_stream_pings(const std::string& s, std::string& file, msk144sp::Params& p, int& min_blocks)
{
    p = msk144sp::Params();
    min_blocks = msk144wb::kPingDefaultMinBlocks;
    const std::vector<std::string> f = split_fields(s, ':');
    file = f[0];
    if(f[0].empty() || f.size() > 5) return false;
    if(f.size() > 1 && !f[1].empty() && !parse_ratio_q4(f[1], p.ratio_q4)) return false;
    if(f.size() > 2 && !f[2].empty() && !parse_int_in(f[2], 1, msk144wb::kPingMaxMinBlocks, min_blocks)) return false;
    if(f.size() > 3 && !f[3].empty() && !parse_int_in(f[3], INT32_MIN, INT32_MAX, p.memory)) return false;
    if(f.size() > 4 && !f[4].empty() && !parse_int_in(f[4], INT32_MIN, INT32_MAX, p.shift)) return false;
    return msk144sp::check_params(p).empty();
}

// The three streams with the largest (or, `smallest`, the smallest) key among those `take` admits, ties to the lower stream
template<typename Key, typename Take>
inline std::vector<int> three_streams(int streams, bool smallest, Key key, Take take)
{
    std::vector<int> order;
    for(int s = 0; s < streams; s++)
        if(take(s)) order.push_back(s);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return smallest ? key(a) < key(b) : key(a) > key(b); });
    if(order.size() > 3) order.resize(3);
    return order;
}

// Both options of a run.  One object serves every device loop: a loop's collect() hands it the slot's records under the mutex, with
// `base` the number of the loop's first stream, so the trackers and sums are indexed by the program's stream numbers.
struct StreamStats
{
    bool pings = false, levels = false;
    std::string file;
    msk144sp::Params params;
    int min_blocks = msk144wb::kPingDefaultMinBlocks;
    StreamPingsApi api;

    bool on() const { return pings || levels; }

    // '' or the refusal
    std::string parse_pings(const std::string& value)
    {
        pings = true;
        return parse_stream_pings(value, file, params, min_blocks) ? "" : "bad value for --stream-pings: '" + value + "' (FILE[:RATIO[:MIN_BLOCKS[:MEMORY[:SHIFT]]]])";
    }

    // after the options are read and before anything touches the library: the entries and the log
    bool prepare(int streams, std::string& err)
    {
        if(!api.resolve(err)) return false;
        if(pings && !(log_ = fopen(file.c_str(), "a")))
        {
            err = "--stream-pings: cannot open '" + file + "': " + strerror(errno);
            return false;
        }
        tracker_.reset(new msk144sp::Tracker(streams, min_blocks));
        sums_.assign(static_cast<size_t>(streams), StreamLevelSum());
        return true;
    }

    bool configure(msk144_handle* h, std::string& err) const
    {
        const msk144_stream_pings_params p{params.ratio_q4, params.memory, params.min_ref, params.shift};
        if(api.set(h, &p) == MSK144_OK) return true;
        err = msk144_last_error(h);
        return false;
    }

    // One position of a hop, in the order the library lists them: the tracker, the log, the sums
    void take_position(int stream, const msk144wb::PingRecord& r, const msk144sp::Level& l, const int32_t* energies)
    {
        events_.clear();
        tracker_->push(stream, r, energies, events_);
        write_events();
        sums_[static_cast<size_t>(stream)].add(l);
    }

    // behind msk144_fetch_wait of the slot's hop (msk144_stream_pings_slot: no wait of its own); streams: the hop's, by position
    bool take(msk144_handle* h, int slot, int base, const std::vector<int>& streams, std::string& err)
    {
        static_assert(sizeof(msk144_wideband_ping) == sizeof(msk144wb::PingRecord) && sizeof(msk144_stream_level) == sizeof(msk144sp::Level), "the tracker reads the library's records");
        const msk144_wideband_ping* records = nullptr;
        const msk144_stream_level* lev = nullptr;
        const int32_t* energies = nullptr;
        int32_t n = 0;
        if(api.slot(h, slot, &records, &lev, &energies, &n) != MSK144_OK)
        {
            err = msk144_last_error(h);
            return false;
        }
        if(static_cast<size_t>(n) != streams.size())
        {
            err = "stream pings: the slot holds " + std::to_string(n) + " positions, the hop listed " + std::to_string(streams.size());
            return false;
        }
        std::lock_guard<std::mutex> lock(mutex_);
        for(int32_t j = 0; j < n; j++)
        {
            msk144wb::PingRecord r;
            msk144sp::Level l;
            std::memcpy(&r, &records[j], sizeof(r));
            std::memcpy(&l, &lev[j], sizeof(l));
            take_position(base + streams[static_cast<size_t>(j)], r, l, energies + static_cast<size_t>(j) * msk144sp::kMaxBlocks);
        }
        return true;
    }

    // the end of every stream: the open runs close, the log is closed
    void finish()
    {
        if(!tracker_) return;
        events_.clear();
        tracker_->close(events_);
        write_events();
        if(log_) fclose(log_);
        log_ = nullptr;
    }

    // the end-of-run lines, for stderr
    std::vector<std::string> summary() const
    {
        std::vector<std::string> out;
        char buf[256];
        const int S = tracker_ ? tracker_->streams() : 0;
        if(pings)
        {
            long long events = 0, up = 0, total = 0;
            int with_events = 0;
            for(int s = 0; s < S; s++)
            {
                events += tracker_->events(s);
                up += tracker_->up_blocks(s);
                total += tracker_->total_blocks(s);
                with_events += tracker_->events(s) > 0 ? 1 : 0;
            }
            snprintf(buf, sizeof(buf), "msk144hipdecoder: stream pings: %lld events on %d of %d streams, %lld of %lld blocks up (ratio %g, min blocks %d, memory %d, shift %d)", events,
                     with_events, S, up, total, params.ratio_q4 / 16.0, min_blocks, params.memory, params.shift);
            std::string line = buf;
            const std::vector<int> top = three_streams(S, false, [&](int s) { return tracker_->events(s); }, [&](int s) { return tracker_->events(s) > 0; });
            for(size_t i = 0; i < top.size(); i++)
            {
                snprintf(buf, sizeof(buf), "%s ch=%d (%lld events, %lld blocks up)", i ? "," : "; most active", top[i], static_cast<long long>(tracker_->events(top[i])),
                         static_cast<long long>(tracker_->up_blocks(top[i])));
                line += buf;
            }
            out.push_back(line);
        }
        if(levels)
        {
            for(int s = 0; s < S; s++)
            {
                const StreamLevelSum& v = sums_[static_cast<size_t>(s)];
                snprintf(buf, sizeof(buf), "msk144hipdecoder: stream levels: ch=%d rms=%.1f peak=%d full_scale=%lld hops=%lld zero_hops=%lld", s, v.rms(), v.peak, v.full_scale, v.hops, v.zero_hops);
                out.push_back(buf);
            }
            auto seen = [&](int s) { return sums_[static_cast<size_t>(s)].hops > 0; };
            std::string line = "msk144hipdecoder: stream levels: most full-scale";
            const std::vector<int> full = three_streams(S, false, [&](int s) { return sums_[static_cast<size_t>(s)].full_scale; }, [&](int s) { return sums_[static_cast<size_t>(s)].full_scale > 0; });
            for(int s : full) line += " ch=" + std::to_string(s) + " (" + std::to_string(sums_[static_cast<size_t>(s)].full_scale) + ")";
            if(full.empty()) line += " none";
            line += "; quietest";
            for(int s : three_streams(S, true, [&](int s) { return sums_[static_cast<size_t>(s)].rms(); }, seen))
            {
                snprintf(buf, sizeof(buf), " ch=%d (%.1f)", s, sums_[static_cast<size_t>(s)].rms());
                line += buf;
            }
            line += "; all hops zero";
            bool any = false;
            for(int s = 0; s < S; s++)
                if(seen(s) && sums_[static_cast<size_t>(s)].zero_hops == sums_[static_cast<size_t>(s)].hops)
                {
                    line += " ch=" + std::to_string(s);
                    any = true;
                }
            if(!any) line += " none";
            out.push_back(line);
        }
        return out;
    }

private:
    void write_events()
    {
        if(!log_) return;
        for(const msk144wb::PingEvent& e : events_) fprintf(log_, "%s\n", msk144sp::event_line(e).c_str());
        if(!events_.empty()) fflush(log_);
    }

    FILE* log_ = nullptr;
    std::mutex mutex_;
    std::unique_ptr<msk144sp::Tracker> tracker_;
    std::vector<StreamLevelSum> sums_;
    std::vector<msk144wb::PingEvent> events_;
};

}  // namespace msk144host
