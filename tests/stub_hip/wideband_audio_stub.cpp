// The audio entries for the stand-in library (compiled together with msk144hip_stub.cpp, wideband_stub.cpp and
// wideband_pings_stub.cpp; it takes wideband_capture_stub.cpp in as it is, under another name for the read entry it has to stand in
// front of): what msk144hipdecoder resolves for --wideband-audio.  Every call is reported on stderr.
//
//   msk144_wideband_capture        the capture stand-in's units and bytes; the units are remembered.
//   msk144_set_wideband_audio      reported with the shift, tap 31 and phasors 1 and 95.
//   msk144_wideband_capture_audio  one row per remembered unit: sample j of the row of (c, k) is 3 ((17 c + 5 k + j) mod 2001 - 1000),
//                                  its clamp count c + k.  MSK144_ESTATE while the audio is off or no unit has been read.
//                                  tests/test_wideband_audio_cli.py holds the same rule.
#include "../../include/msk144hip.h"

#define msk144_wideband_capture msk144stub_wideband_capture_base
#include "wideband_capture_stub.cpp"
#undef msk144_wideband_capture

namespace
{

struct Audio
{
    bool on = false, read = false;
    int reads = 0;
    std::vector<msk144_wideband_capture_unit> units;  // of the last msk144_wideband_capture
};
std::map<const msk144_handle*, Audio> g_audio;

}  // namespace

extern "C" {

int msk144_wideband_capture(msk144_handle* h, msk144_wideband_capture_unit* units, int8_t* data, int32_t* count, int32_t* total)
{
    const int rc = msk144stub_wideband_capture_base(h, units, data, count, total);
    if(rc != MSK144_OK) return rc;
    Audio& a = g_audio[h];
    a.units.assign(units, units + *count);
    a.read = true;
    return rc;
}

int msk144_set_wideband_audio(msk144_handle* h, const msk144_wideband_audio_params* p)
{
    if(!h) return MSK144_EINVAL;
    if(!p) fprintf(stderr, "stub: msk144_set_wideband_audio(off)\n");
    else
        fprintf(stderr, "stub: msk144_set_wideband_audio(shift %d, tap31 %d %d, phasor1 %d %d, phasor95 %d %d)\n", p->shift, p->taps[31][0], p->taps[31][1], p->phasor[1][0],
                p->phasor[1][1], p->phasor[95][0], p->phasor[95][1]);
    g_audio[h].on = p != nullptr;
    return MSK144_OK;
}

int msk144_wideband_capture_audio(msk144_handle* h, int16_t* audio, int32_t* clamped, int32_t* count)
{
    if(!h || !audio || !clamped || !count) return MSK144_EINVAL;
    Audio& a = g_audio[h];
    if(!a.on || !a.read) return MSK144_ESTATE;
    fprintf(stderr, "stub: msk144_wideband_capture_audio read %d: %d rows\n", a.reads++, static_cast<int>(a.units.size()));
    for(size_t n = 0; n < a.units.size(); n++)
    {
        const int c = a.units[n].channel, k = static_cast<int>(a.units[n].hop);
        for(int j = 0; j < MSK144_HOP_SAMPLES; j++) audio[n * MSK144_HOP_SAMPLES + j] = static_cast<int16_t>(3 * ((17 * c + 5 * k + j) % 2001 - 1000));
        clamped[n] = c + k;
    }
    *count = static_cast<int32_t>(a.units.size());
    return MSK144_OK;
}

}  // extern "C"
