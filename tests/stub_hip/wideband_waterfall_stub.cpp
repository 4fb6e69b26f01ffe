// The waterfall entries for the stand-in library (compiled together with msk144hip_stub.cpp and wideband_stub.cpp): what
// msk144hipdecoder resolves for --wideband-waterfall.  Every call is reported on stderr.  The program reads the sums once per push,
// behind that push's rows, so read i (0 the first: 54 blocks, then 27) ends with the sums call.  In read i block b of channel c holds
// the integer samples
//     x[n] = 40 e^{j 2 pi q n / 8} rounded as in kTone, plus (7 n + 3 c + b) mod 5 - 2 on both components,   q = (c + b + i) mod 7 - 3,
// a tone 1500 q Hz from the channel's offset (slot j = 48 + 12 q) over a small pattern, and a row is its direct transform in double,
//     re += w[i] (xr cos + xi sin),  im += w[i] (xi cos - xr sin)   with cos and sin of 2 pi ((i k) mod 96) / 96 from a table, i ascending,
// re^2 + im^2 rounded to f32.  tests/test_wideband_waterfall_cli.py holds the same rule, operation for operation.
#include "../../include/msk144hip.h"

#include <cmath>
#include <cstdio>
#include <map>
#include <vector>

namespace
{

constexpr int B = MSK144_WATERFALL_BINS, R = MSK144_PING_MAX_BLOCKS;
const int kTone[8][2] = {{40, 0}, {28, 28}, {0, 40}, {-28, 28}, {-40, 0}, {-28, -28}, {0, -40}, {28, -28}};

struct Waterfall
{
    bool on = false;
    int channels = 0;
    int reads = 0;  // sums calls so far: the index of the push whose rows are being read
    std::vector<double> window;
};
std::map<const msk144_handle*, Waterfall> g_wf;

bool ready(msk144_handle* h, Waterfall& g)
{
    if(!g.on) return false;
    if(!g.channels)
    {
        int32_t n = 0;
        if(msk144_llr_block_channels(h, &n) != MSK144_OK || n < 1) return false;  // the stand-in reports the handle's channels
        g.channels = n;
    }
    return true;
}

void row_of(const Waterfall& g, int i, int c, int b, float* out)
{
    static double cs[B], sn[B];  // cos and sin of 2 pi m / 96
    if(cs[0] == 0.0)
        for(int m = 0; m < B; m++) cs[m] = std::cos(2.0 * M_PI * m / B), sn[m] = std::sin(2.0 * M_PI * m / B);
    const int q = (c + b + i) % 7 - 3;
    double xr[B], xi[B];
    for(int n = 0; n < B; n++)
    {
        const int m = ((q * n) % 8 + 8) % 8, e = (7 * n + 3 * c + b) % 5 - 2;
        xr[n] = kTone[m][0] + e;
        xi[n] = kTone[m][1] + e;
    }
    for(int j = 0; j < B; j++)
    {
        const int k = (j + B / 2) % B;
        double re = 0.0, im = 0.0;
        for(int n = 0; n < B; n++)
        {
            const int m = (n * k) % B;
            re += g.window[n] * (xr[n] * cs[m] + xi[n] * sn[m]);
            im += g.window[n] * (xi[n] * cs[m] - xr[n] * sn[m]);
        }
        out[j] = static_cast<float>(re * re + im * im);
    }
}

}  // namespace

extern "C" {

int msk144_set_wideband_waterfall(msk144_handle* h, const msk144_wideband_waterfall_params* p)
{
    if(!h) return MSK144_EINVAL;
    fprintf(stderr, "stub: msk144_set_wideband_waterfall(%s)\n", !p ? "off" : p->window ? "window given" : "window default");
    Waterfall& g = g_wf[h];
    g.on = p != nullptr;
    g.window.assign(B, 0.0);
    for(int i = 0; p && i < B; i++) g.window[i] = static_cast<double>(static_cast<float>(p->window ? p->window[i] : 0.5 - 0.5 * std::cos(2.0 * M_PI * i / B)));
    return MSK144_OK;
}

int msk144_wideband_waterfall(msk144_handle* h, int32_t channel, float* rows, int32_t* n)
{
    if(!h || !rows || !n) return MSK144_EINVAL;
    Waterfall& g = g_wf[h];
    if(!ready(h, g)) return MSK144_ESTATE;
    if(channel < -1 || channel >= g.channels) return MSK144_EINVAL;
    fprintf(stderr, "stub: msk144_wideband_waterfall(channel %d) read %d\n", channel, g.reads);
    const int nb = g.reads == 0 ? R : R / 2;
    const int c0 = channel < 0 ? 0 : channel, c1 = channel < 0 ? g.channels : channel + 1;
    for(int c = c0; c < c1; c++)
        for(int b = 0; b < R; b++)
        {
            float* row = rows + (static_cast<size_t>(c - c0) * R + b) * B;
            if(b < nb) row_of(g, g.reads, c, b, row);
            else
                for(int j = 0; j < B; j++) row[j] = 0.0f;
        }
    *n = nb;
    return MSK144_OK;
}

int msk144_wideband_waterfall_sums(msk144_handle* h, double* sums)
{
    if(!h || !sums) return MSK144_EINVAL;
    Waterfall& g = g_wf[h];
    if(!ready(h, g)) return MSK144_ESTATE;
    fprintf(stderr, "stub: msk144_wideband_waterfall_sums read %d\n", g.reads);
    const int nb = g.reads == 0 ? R : R / 2;
    float row[B];
    for(int c = 0; c < g.channels; c++)
    {
        double* s = sums + static_cast<size_t>(c) * B;
        for(int j = 0; j < B; j++) s[j] = 0.0;
        for(int b = 0; b < nb; b++)
        {
            row_of(g, g.reads, c, b, row);
            for(int j = 0; j < B; j++) s[j] += static_cast<double>(row[j]);
        }
    }
    g.reads++;
    return MSK144_OK;
}

}  // extern "C"
