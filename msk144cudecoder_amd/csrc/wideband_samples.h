// Wideband input samples as the device reads them (channelise.hip, bank.hip): the raw formats of msk144_wideband_params.format and
// the complex-f32 sub-band streams of the two-stage bank.
#pragma once

#include <hip/hip_runtime.h>

namespace msk144
{

// FMT 0 cu8 (u - 127.5) / 128, 1 cs8 s / 128, 2 cs16 s / 32768, 3 complex f32 (a sub-band stream of the bank, as stored)
template<int FMT>
__device__ inline float2 load_sample(const void* __restrict__ raw, int i)
{
    if(FMT == 0)
    {
        const uchar2 v = static_cast<const uchar2*>(raw)[i];
        return make_float2((static_cast<float>(v.x) - 127.5f) * (1.0f / 128.0f), (static_cast<float>(v.y) - 127.5f) * (1.0f / 128.0f));
    }
    else if(FMT == 1)
    {
        const char2 v = static_cast<const char2*>(raw)[i];
        return make_float2(static_cast<float>(v.x) * (1.0f / 128.0f), static_cast<float>(v.y) * (1.0f / 128.0f));
    }
    else if(FMT == 2)
    {
        const short2 v = static_cast<const short2*>(raw)[i];
        return make_float2(static_cast<float>(v.x) * (1.0f / 32768.0f), static_cast<float>(v.y) * (1.0f / 32768.0f));
    }
    else
        return static_cast<const float2*>(raw)[i];
}

}  // namespace msk144
