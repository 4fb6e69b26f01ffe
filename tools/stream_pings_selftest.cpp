// Stand-alone check of the host code behind --stream-pings and --stream-levels (host/stream_pings_cli.h, csrc/stream_pings.h), meant
// to be built with the sanitizers; no GPU, no library:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -rdynamic tools/stream_pings_selftest.cpp -ldl -o stream_pings_selftest
//   ./stream_pings_selftest
//
// It stands in for the two library entries itself (found through dlsym, hence -rdynamic), drives StreamStats through hops with partial
// lists, a run that stays open across hops, a stream that ends early, full-scale and all-zero rows and the extremes of every
// parameter, and checks the log and the summaries against values worked out by hand.  Exit status 0 and "ok" when everything holds.
#include "../msk144cudecoder_amd/host/stream_pings_cli.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <unistd.h>

using namespace msk144host;

namespace
{

// the stand-in library: one model, the slot's results worked out from rows the test lays down
struct Fake
{
    std::unique_ptr<msk144sp::Model> model;
    std::vector<msk144wb::PingRecord> records;
    std::vector<msk144sp::Level> levels;
    std::vector<int32_t> energies;
} g_fake;

int g_failed = 0;
#define CHECK(cond)                                                          \
    do                                                                       \
    {                                                                        \
        if(!(cond))                                                          \
        {                                                                    \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            g_failed++;                                                      \
        }                                                                    \
    } while(0)

// a row whose block b is the constant v[b] with alternating sign: E[b] = 96 v^2 >> shift
std::vector<int16_t> row(const std::vector<int>& v)
{
    std::vector<int16_t> x(v.size() * 96);
    for(size_t i = 0; i < x.size(); i++) x[i] = static_cast<int16_t>((i & 1) ? -v[i / 96] : v[i / 96]);
    return x;
}

void lay(const std::vector<int>& streams, const std::vector<bool>& first, const std::vector<std::vector<int16_t>>& rows)
{
    const size_t n = streams.size();
    g_fake.records.resize(n);
    g_fake.levels.resize(n);
    g_fake.energies.assign(n * msk144sp::kMaxBlocks, 0);
    for(size_t j = 0; j < n; j++) g_fake.records[j] = g_fake.model->push(streams[j], first[j], rows[j].data(), g_fake.levels[j], g_fake.energies.data() + j * msk144sp::kMaxBlocks);
}

}  // namespace

extern "C" {
const char* msk144_last_error(const msk144_handle*) { return "fake"; }
int msk144_set_stream_pings(msk144_handle*, const msk144_stream_pings_params* p)
{
    g_fake.model.reset(new msk144sp::Model(4, msk144sp::Params{p->ratio_q4, p->memory, p->min_ref, p->shift}));
    return MSK144_OK;
}
int msk144_stream_pings_slot(msk144_handle*, int32_t, const msk144_wideband_ping** records, const msk144_stream_level** levels, const int32_t** energies, int32_t* n)
{
    *records = reinterpret_cast<const msk144_wideband_ping*>(g_fake.records.data());
    *levels = reinterpret_cast<const msk144_stream_level*>(g_fake.levels.data());
    *energies = g_fake.energies.data();
    *n = static_cast<int32_t>(g_fake.records.size());
    return MSK144_OK;
}
}

int main()
{
    char path[] = "/tmp/stream_pings_selftest_XXXXXX";
    const int fd = mkstemp(path);
    if(fd < 0) return 2;
    close(fd);

    // the option's fields, every edge
    {
        std::string file;
        msk144sp::Params p;
        int mb = 0;
        CHECK(parse_stream_pings("f", file, p, mb) && p.ratio_q4 == msk144sp::kDefaultRatioQ4 && mb == 2 && p.memory == 8 && p.shift == 12 && file == "f");
        CHECK(parse_stream_pings("f:4095.9:64:16:24", file, p, mb) && p.ratio_q4 == 65534 && mb == 64 && p.memory == 16 && p.shift == 24);
        CHECK(parse_stream_pings("f:1:1:0:0", file, p, mb) && p.ratio_q4 == 16 && p.memory == 0 && p.shift == 0);
        CHECK(parse_stream_pings("f::::", file, p, mb) && p.shift == 12);
        for(const char* bad : {"", ":1", "f:0.5", "f:1e9", "f:2:0", "f:2:65", "f:2:2:17", "f:2:2:-1", "f:2:2:2:25", "f:2:2:2:-1", "f:2:2:2:2:2", "f:99999999999999999999"})
            CHECK(!parse_stream_pings(bad, file, p, mb));
    }

    StreamStats st;
    std::string err;
    CHECK(st.parse_pings(std::string(path) + ":2:2:8:0").empty());
    st.levels = true;
    CHECK(st.prepare(4, err));
    CHECK(st.configure(nullptr, err));

    const int q = 10, loud = 100;
    // hop 0: streams 0, 1, 3 start; stream 0 ends its first hop inside a run, stream 3 is at full scale
    std::vector<int> a(54, q);
    a[52] = a[53] = loud;
    lay({0, 1, 3}, {true, true, true}, {row(a), row(std::vector<int>(54, 0)), std::vector<int16_t>(5184, -32768)});
    CHECK(st.take(nullptr, 0, 0, {0, 1, 3}, err));
    // hop 1: stream 0 alone, the run goes on for three blocks; a second handle's stream 0 is the program's stream 2 (base 2)
    std::vector<int> b(27, q);
    b[0] = b[1] = b[2] = loud;
    lay({0}, {false}, {row(b)});
    CHECK(st.take(nullptr, 1, 0, {0}, err));
    std::vector<int> c(27, q);
    c[26] = loud;
    c[25] = loud;
    lay({2}, {true}, {row(std::vector<int>(54, q))});
    CHECK(st.take(nullptr, 0, 0, {2}, err));
    lay({2}, {false}, {row(c)});
    CHECK(st.take(nullptr, 1, 0, {2}, err));
    // a slot whose n disagrees with the hop's list is an error, not a read past the end
    CHECK(!st.take(nullptr, 1, 0, {2, 3}, err) && !err.empty());
    st.finish();
    st.finish();  // twice is harmless

    std::ifstream in(path);
    std::vector<std::string> lines;
    for(std::string l; std::getline(in, l);) lines.push_back(l);
    CHECK(lines.size() == 2);
    if(lines.size() == 2)
    {
        CHECK(lines[0] == "ping ch=0 start=0.416 dur=0.040 blocks=5 peak=960000 ref=9600 peak_db=20.0");
        CHECK(lines[1] == "ping ch=2 start=0.632 dur=0.016 blocks=2 peak=960000 ref=9600 peak_db=20.0");  // closed by the end of the stream
    }
    const std::vector<std::string> sum = st.summary();
    CHECK(sum.size() == 6);
    if(sum.size() == 6)
    {
        // stream 3: 54 blocks at the cap, each 4194303 x 16 > 4194303 x 32? no: E = R, nothing up
        CHECK(sum[0] == "msk144hipdecoder: stream pings: 2 events on 2 of 4 streams, 7 of 270 blocks up (ratio 2, min blocks 2, memory 8, shift 0); most active ch=0 (1 events, 5 blocks up), ch=2 (1 events, 2 blocks up)");
        CHECK(sum[2] == "msk144hipdecoder: stream levels: ch=1 rms=0.0 peak=0 full_scale=0 hops=1 zero_hops=1");
        CHECK(sum[4] == "msk144hipdecoder: stream levels: ch=3 rms=32768.0 peak=32768 full_scale=5184 hops=1 zero_hops=0");
        CHECK(sum[5].find("most full-scale ch=3 (5184); quietest ch=1 (0.0)") != std::string::npos && sum[5].find("all hops zero ch=1") != std::string::npos);
        for(const std::string& l : sum) std::cout << l << std::endl;
    }
    // the sums of a long run at full scale stay exact: 2^40 samples' worth would overflow 64 bits, 128 do not
    StreamLevelSum big;
    msk144sp::Level full{};
    full.sum_sq = static_cast<int64_t>(5184) << 30;
    full.samples = 5184;
    full.peak = 32768;
    for(int i = 0; i < 100000; i++) big.add(full);
    CHECK(big.rms() == 32768.0 && big.hops == 100000);

    unlink(path);
    if(g_failed) return 1;
    std::cout << "ok" << std::endl;
    return 0;
}
