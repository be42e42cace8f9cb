// srcnn_image.h -- images as they are stored (include/srcnn_amd.h, srcnn_image): what the kernels of srcnn_pipeline.hip take for
// one side of an image call, and their launchers.  Host layer: srcnn_image.cpp.
#pragma once
#include "srcnn_kernels.h"

namespace srcnn {

enum { ELEM_F32 = 0, ELEM_F16 = 1, ELEM_BF16 = 2, ELEM_U8 = 3 };      // SRCNN_ELEM_*

// Element (f, c, y, x) at data + f frame_pitch + c ch_pitch + y stride + x px_step, all in elements of `elem`; scale: U8 only
struct ImageRef {
    void *data;
    int elem;
    float scale;
    long px_step, stride, ch_pitch, frame_pitch;
};
inline bool image_is_planar_f32(const ImageRef &im) { return im.elem == ELEM_F32 && im.px_step == 1; }

// The accessor forms of the float resize (launch_resize_cubic_f32, launch_luma_resize_f32, launch_resize_merge_f32): the same
// tables, the same tile, the same variant choice and summation order; only the element access of the tile's fill and of the
// vertical pass's store goes through the load and the store of an ImageRef.  yup / ysr stay packed float32 planes (the
// context's workspace).
hipError_t launch_resize_cubic_image(const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels,
                                     int n_frames, const int *xfirst, const float *xcoef, const int *yfirst, const float *ycoef,
                                     hipStream_t st);
hipError_t launch_luma_resize_image(const ImageRef &src, int sw, int sh, float *yup, long ystride, long yframe_pitch, int dw, int dh,
                                    int n_frames, const float luma[4], const int *xfirst, const float *xcoef, const int *yfirst,
                                    const float *ycoef, hipStream_t st);
hipError_t launch_resize_merge_image(const ImageRef &src, int sw, int sh, const float *ysr, long ysr_stride, long ysr_frame_pitch,
                                     const float *yup, long yup_stride, long yup_frame_pitch, const ImageRef &dst, int dw, int dh,
                                     int n_frames, float g, const float *clamp, const int *xfirst, const float *xcoef,
                                     const int *yfirst, const float *ycoef, hipStream_t st);
// dst = store(load(src)): `channels` (1 or 3) planes x n_frames frames of width x height
hipError_t launch_convert_image(const ImageRef &src, const ImageRef &dst, int width, int height, int channels, int n_frames,
                                hipStream_t st);

}  // namespace srcnn
