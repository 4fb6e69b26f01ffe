// Input-rate entries for the stand-in library (compiled together with msk144hip_stub.cpp).  No resampler: a slot holds rows of
// 2592 P/Q int16 per stream, and a push hands every listed stream a 12 kHz hop through the stub's own hop ring whose first two samples
// are the first two samples of the stream's input row (of both rows on a first hop) and whose rest is zero.  A stream marked like
// those of tests/test_host_loop.py at the input rate - input row k starts with (0x7777, tag + k) - therefore shows in the records
// which input row reached which window, i.e. that the program cut every stream into hops of the right size.  Every push is reported
// on stderr with its row length, and every position counts 3 clamped samples.
#include "../../include/msk144hip.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <vector>

namespace
{

struct Rate
{
    long long rate = 0;
    int row = 0, channels = 0, last_n = 0;
    std::vector<int32_t> slot_counts[MSK144_SLOTS];
    std::vector<uint8_t> started;
    std::vector<int16_t> hops[MSK144_SLOTS], first_halves[MSK144_SLOTS];
};
std::map<const msk144_handle*, Rate> g_rate;

}  // namespace

extern "C" {

int msk144_set_input_rate(msk144_handle* h, const msk144_input_rate_params* p)
{
    if(!h) return MSK144_EINVAL;
    if(!p)
    {
        g_rate.erase(h);
        return MSK144_OK;
    }
    if(p->rate_hz % 125 != 0 || p->rate_hz < 24000 || p->rate_hz > 192000 || !p->taps) return MSK144_EINVAL;
    const long long g = std::gcd(static_cast<long long>(p->rate_hz), 12000LL);
    const int P = static_cast<int>(p->rate_hz / g), Q = static_cast<int>(12000 / g);
    if(p->num_taps % P != 0) return MSK144_EINVAL;
    int32_t nch = 0;
    if(msk144_llr_block_channels(h, &nch) != MSK144_OK) return MSK144_EINVAL;  // the stub reports the handle's channels there
    Rate& r = g_rate[h];
    r = Rate{};
    r.rate = p->rate_hz;
    r.row = MSK144_HOP_SAMPLES / Q * P;
    r.channels = nch;
    r.started.assign(static_cast<size_t>(nch), 0);
    long long sum = 0;
    for(int k = 0; k < p->num_taps; k++) sum += p->taps[k];
    fprintf(stderr, "stub: msk144_set_input_rate(rate %lld, shift %d, %d taps summing to %lld, row %d)\n", static_cast<long long>(p->rate_hz), p->shift, p->num_taps, sum, r.row);
    return MSK144_OK;
}

int msk144_rate_hop_slot(msk144_handle* h, int32_t s, void** hops, void** first_halves, int32_t** streams, uint8_t** is_first, int32_t* row)
{
    auto it = g_rate.find(h);
    if(it == g_rate.end() || s < 0 || s >= MSK144_SLOTS) return MSK144_ESTATE;
    Rate& r = it->second;
    void *h12 = nullptr, *f12 = nullptr;
    int rc = msk144_hop_slot(h, s, &h12, &f12, streams, is_first);
    if(rc != MSK144_OK) return rc;
    const size_t n = static_cast<size_t>(r.channels) * r.row;
    if(r.hops[s].size() != n)
    {
        r.hops[s].assign(n, 0);
        r.first_halves[s].assign(n, 0);
    }
    *hops = r.hops[s].data();
    *first_halves = r.first_halves[s].data();
    *row = r.row;
    return MSK144_OK;
}

int msk144_push_rate_hops(msk144_handle* h, int32_t s, int32_t n)
{
    auto it = g_rate.find(h);
    if(it == g_rate.end() || s < 0 || s >= MSK144_SLOTS) return MSK144_ESTATE;
    Rate& r = it->second;
    if(n < 1 || n > r.channels || r.hops[s].empty()) return MSK144_EINVAL;
    void *h12 = nullptr, *f12 = nullptr;
    int32_t* streams = nullptr;
    uint8_t* is_first = nullptr;
    int rc = msk144_hop_slot(h, s, &h12, &f12, &streams, &is_first);
    if(rc != MSK144_OK) return rc;
    int firsts = 0;
    for(int j = 0; j < n; j++)
    {
        const int c = streams[j];
        if(c < 0 || c >= r.channels) return MSK144_EINVAL;
        if(!is_first[j] && !r.started[static_cast<size_t>(c)]) return MSK144_ESTATE;
        r.started[static_cast<size_t>(c)] = 1;
        firsts += is_first[j] ? 1 : 0;
        int16_t* hp = static_cast<int16_t*>(h12) + static_cast<size_t>(MSK144_HOP_SAMPLES) * j;
        int16_t* fp = static_cast<int16_t*>(f12) + static_cast<size_t>(MSK144_HOP_SAMPLES) * j;
        memset(hp, 0, MSK144_HOP_SAMPLES * sizeof(int16_t));
        memcpy(hp, r.hops[s].data() + static_cast<size_t>(r.row) * j, 2 * sizeof(int16_t));
        if(is_first[j])
        {
            memset(fp, 0, MSK144_HOP_SAMPLES * sizeof(int16_t));
            memcpy(fp, r.first_halves[s].data() + static_cast<size_t>(r.row) * j, 2 * sizeof(int16_t));
        }
    }
    r.last_n = n;
    r.slot_counts[s].assign(static_cast<size_t>(n), 3);
    fprintf(stderr, "stub: msk144_push_rate_hops(slot %d, n %d, firsts %d, row %d)\n", s, n, firsts, r.row);
    return msk144_push_hops(h, s, n);
}

int msk144_input_rate_clamped(msk144_handle* h, int32_t* clamped)
{
    auto it = g_rate.find(h);
    if(it == g_rate.end() || !clamped || it->second.last_n == 0) return MSK144_ESTATE;
    for(int j = 0; j < it->second.last_n; j++) clamped[j] = 3;
    return MSK144_OK;
}

int msk144_input_rate_slot_clamped(msk144_handle* h, int32_t s, const int32_t** clamped, int32_t* n)
{
    auto it = g_rate.find(h);
    if(it == g_rate.end() || s < 0 || s >= MSK144_SLOTS || !clamped || !n || it->second.slot_counts[s].empty()) return MSK144_ESTATE;
    *clamped = it->second.slot_counts[s].data();
    *n = static_cast<int32_t>(it->second.slot_counts[s].size());
    return MSK144_OK;
}

int msk144_dump_rate_hop(msk144_handle*, int32_t, int16_t*, int32_t*) { return MSK144_ESTATE; }

}  // extern "C"
