// The impulse-noise blanker entries for the stand-in library (compiled together with msk144hip_stub.cpp and wideband_stub.cpp): what
// msk144hipdecoder resolves for --wideband-blanker.  Every call is reported on stderr; the statistics are fixed totals, so that a
// test can find them in the program's summary line: 1234 hits and 56789 of 98765432 samples blanked.
#include "../../include/msk144hip.h"

#include <cstdio>

extern "C" {

int msk144_set_wideband_blanker(msk144_handle* h, const msk144_wideband_blanker* p)
{
    if(!h) return MSK144_EINVAL;
    if(!p) fprintf(stderr, "stub: msk144_set_wideband_blanker(off)\n");
    else fprintf(stderr, "stub: msk144_set_wideband_blanker(threshold_q4 %d, pre %d, post %d)\n", p->threshold_q4, p->pre, p->post);
    return MSK144_OK;
}

int msk144_wideband_blanker_stats(msk144_handle* h, msk144_wideband_blanker_counts* out)
{
    if(!h || !out) return MSK144_EINVAL;
    fprintf(stderr, "stub: msk144_wideband_blanker_stats\n");
    *out = msk144_wideband_blanker_counts{};
    out->total_hits = 1234;
    out->total_blanked = 56789;
    out->total_samples = 98765432;
    return MSK144_OK;
}

int msk144_dump_wideband_blanked(msk144_handle*, int16_t*) { return MSK144_ESTATE; }

}  // extern "C"
