// The per-channel level and AGC entries for the stand-in library (compiled together with msk144hip_stub.cpp and wideband_stub.cpp):
// only the three entries that msk144hipdecoder resolves for --wideband-gain=auto and --wideband-levels.  Every call is reported on
// stderr; the levels are a fixed function of the channel and of how often they were read, so that a test can add the table up:
// read i (0 the first: 5184 samples, then 2592) gives channel c sum_sq = 2 samples (c + 1)^2 - an rms of c + 1 LSB -, clipped = c (3 c
// on the first read), exponent = (c % 3) - 1 - (i % 2) and gain = 100 x 2^exponent.
#include "../../include/msk144hip.h"

#include <cmath>
#include <cstdio>
#include <map>

namespace
{

struct Levels
{
    int channels = 0;
    int reads = 0;
};
std::map<const msk144_handle*, Levels> g_levels;

}  // namespace

extern "C" {

int msk144_set_wideband_agc(msk144_handle* h, const msk144_wideband_agc* p)
{
    if(!h) return MSK144_EINVAL;
    if(!p) fprintf(stderr, "stub: msk144_set_wideband_agc(off)\n");
    else
        fprintf(stderr, "stub: msk144_set_wideband_agc(lo_sq %d, hi_sq %d, clip_ppm %d, hold %d, min_exp %d, max_exp %d)\n", p->lo_sq, p->hi_sq, p->clip_ppm, p->hold,
                p->min_exp, p->max_exp);
    return MSK144_OK;
}

int msk144_set_wideband_gains(msk144_handle* h, const float* gains)
{
    if(!h) return MSK144_EINVAL;
    fprintf(stderr, "stub: msk144_set_wideband_gains(%s)\n", gains ? "array" : "reset");
    return MSK144_OK;
}

int msk144_wideband_levels(msk144_handle* h, msk144_wideband_level* out)
{
    if(!h || !out) return MSK144_EINVAL;
    Levels& l = g_levels[h];
    if(!l.channels)
    {
        int32_t n = 0;
        if(msk144_llr_block_channels(h, &n) != MSK144_OK || n < 1) return MSK144_ESTATE;  // the stand-in reports the handle's channels
        l.channels = n;
    }
    const int i = l.reads++;
    for(int c = 0; c < l.channels; c++)
    {
        out[c].samples = i == 0 ? MSK144_WINDOW_SAMPLES : MSK144_HOP_SAMPLES;
        out[c].sum_sq = 2 * out[c].samples * (c + 1) * (c + 1);
        out[c].clipped = i == 0 ? 3 * c : c;
        out[c].exponent = (c % 3) - 1 - (i % 2);
        out[c].gain = std::ldexp(100.0f, out[c].exponent);
    }
    if(i == 0) fprintf(stderr, "stub: msk144_wideband_levels(%d channels)\n", l.channels);
    return MSK144_OK;
}

}  // extern "C"
