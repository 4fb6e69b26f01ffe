// The input-spectrum entries for the stand-in library (compiled together with msk144hip_stub.cpp and wideband_stub.cpp): what
// msk144hipdecoder resolves for --wideband-spectrum.  Every call is reported on stderr.  Read n (0, 1, ...) returns 100 + n segments
// and power[j] = segments x (B/2)^2 x 10^(-(j mod 64) / 10): with the periodic Hann window (sum w = B/2) slot j reads -(j mod 64).00
// dBFS over any group of pushes, the highest bin is slot 0 at -Fs/2 and the median bin reads -31.00.
#include "../../include/msk144hip.h"

#include <cmath>
#include <cstdio>

namespace
{
int g_bins = 0;
int g_reads = 0;
}  // namespace

extern "C" {

int msk144_set_wideband_spectrum(msk144_handle* h, const msk144_wideband_spectrum_params* p)
{
    if(!h) return MSK144_EINVAL;
    if(!p) fprintf(stderr, "stub: msk144_set_wideband_spectrum(off)\n");
    else fprintf(stderr, "stub: msk144_set_wideband_spectrum(bins %d, window %s)\n", p->bins, p->window ? "given" : "default");
    g_bins = p ? p->bins : 0;
    return MSK144_OK;
}

int msk144_wideband_spectrum(msk144_handle* h, double* power, int64_t* segments)
{
    if(!h || !power || !segments) return MSK144_EINVAL;
    if(!g_bins) return MSK144_ESTATE;
    fprintf(stderr, "stub: msk144_wideband_spectrum read %d\n", g_reads);
    *segments = 100 + g_reads++;
    for(int j = 0; j < g_bins; j++) power[j] = static_cast<double>(*segments) * (g_bins / 2.0) * (g_bins / 2.0) * std::pow(10.0, -(j % 64) / 10.0);
    return MSK144_OK;
}

}  // extern "C"
