// blend_channels.h — what the kernels that composite many caller-supplied channels per walk share (blend_channels.hip, blend_slab.hip):
// where a walk finds its rows and its pixels, and the 16-byte load of a row's words.
#pragma once
#include "gsr_internal.h"

namespace gsr {

struct ChannelArgs {
    const float *features;  // channel c0 of gaussian 0: row i at features + i * stride
    int64_t stride;         // floats between rows
    int channels;           // of the whole map: a pixel's values lie channels floats apart
    int c0, nch;            // this walk composites channels c0 .. c0 + nch - 1, 1 <= nch <= CH
    int vec_in, vec_out;    // 16-byte loads of the rows / stores of the pixels are aligned (decided on the host)
};

// Four consecutive floats of a row in one 16-byte global load (the address is 16-byte aligned: ChannelArgs.vec_in).
__device__ __forceinline__ float4 ldg4(const float *p, int q)
{
    typedef float V4 __attribute__((ext_vector_type(4)));
    const V4 v = ((const __attribute__((address_space(1))) V4 *)p)[q];
    return make_float4(v.x, v.y, v.z, v.w);
}

}  // namespace gsr
