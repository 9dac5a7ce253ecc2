// The uint16 launches of image_codec.hip's stitch_hwc_kernel and blend_finish_hwc_kernel, for image_u16.hip's exports:
// the kernels are instantiated in image_codec.hip alone.  mis follows from the output's address.
#pragma once
#include "tile_grid.h"
#include "u16_scale.h"

namespace dsic {

void launch_stitch_u16(bool res, dim3 grid, hipStream_t st, const float* tiles, const float* q, int step, uint16_t* out,
                       const Grid& g, int C, const int* ids, const Clip& clip, const Scale& sc);
void launch_blend_finish_u16(hipStream_t st, const float* canvas, uint16_t* out, int C, int64_t hw, const Scale& sc);

}  // namespace dsic
