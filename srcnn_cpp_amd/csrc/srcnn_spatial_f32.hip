// srcnn_spatial_f32.hip -- the float image path's kernels (srcnn_forward_f32*), for gfx950: spatial_l1_kernel<C, ZERO, Scale, float>
// (layer 1 reading float planes; f32 and split-f16 map) and spatial_l3_kernel<C, false, ZERO, float> (layer 3 writing float
// planes), C = 1, 3, replicate and zero padding, behind launch_spatial_l1f / launch_spatial_l3f.  The templates are the ones of
// srcnn_spatial_kernels.hip, included here with its own launchers switched off: a translation unit of its own, so that unit
// keeps exactly the kernels it had.
#define SRCNN_SPATIAL_F32_UNIT 1
#include "srcnn_spatial_kernels.hip"
