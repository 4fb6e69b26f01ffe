// The ping-band entry for the stand-in library (compiled together with msk144hip_stub.cpp, wideband_stub.cpp and
// wideband_pings_stub.cpp): what msk144hipdecoder resolves for --wideband-pings-band.  The call is reported on stderr with its shift
// and its 128 tap bytes in hexadecimal, (br, bi) of b[0] first.  The stand-in's ping records do not depend on it.
#include "../../include/msk144hip.h"

#include <cstdio>

extern "C" {

int msk144_set_wideband_ping_band(msk144_handle* h, const msk144_wideband_ping_band_params* p)
{
    if(!h) return MSK144_EINVAL;
    if(!p)
    {
        fprintf(stderr, "stub: msk144_set_wideband_ping_band(off)\n");
        return MSK144_OK;
    }
    fprintf(stderr, "stub: msk144_set_wideband_ping_band(shift %d, taps ", p->shift);
    for(int k = 0; k < 64; k++) fprintf(stderr, "%02x%02x", static_cast<unsigned>(static_cast<uint8_t>(p->taps[k][0])), static_cast<unsigned>(static_cast<uint8_t>(p->taps[k][1])));
    fprintf(stderr, ")\n");
    return MSK144_OK;
}

}  // extern "C"
