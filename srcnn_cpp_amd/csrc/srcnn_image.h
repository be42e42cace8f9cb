// srcnn_image.h -- images as they are stored (include/srcnn_amd.h, srcnn_image): what the kernels of srcnn_pipeline.hip take for
// one side of an image call, and their launchers.  Host layer: srcnn_image.cpp.
#pragma once
#include "srcnn_kernels.h"

struct srcnn_ctx;

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

// ---- the antialiased cubic resize (srcnn_resize_cubic_aa_*; include/srcnn_amd.h has the arithmetic) -------------------------
// Two forms, the same bits.  tiled: one launch; a workgroup of 256 threads produces AA_TR output rows x AA_TC columns, the
// horizontal results of the source rows the tile spans stay in LDS (hbuf[AA_RMAX][AA_TC] floats = 20,480 bytes).  general:
// two launches, the horizontal pass into a float32 workspace of sh x dw per plane, the vertical pass out of it -- any ratio and
// any tap count.  Both read the source through an ImageRef's load and write through its store.
constexpr int AA_TR = 16;         // output rows per workgroup (tiled form)
constexpr int AA_TC = 64;         // output columns per workgroup: one per lane of a wave
constexpr int AA_RATIO = 4;       // the tiled form takes source sizes up to AA_RATIO x the destination's, per axis
constexpr int AA_KMAX = 17;       // ... and tables of at most this many taps per output sample (ratio 4: 4 * 4 + 1)
constexpr int AA_RMAX = AA_RATIO * (AA_TR - 1) + 1 + AA_KMAX + 2;      // source rows a tile may span: 80
enum { RESAMPLE_AA_GENERAL = 0, RESAMPLE_AA_TILED = 1 };
// Which form resizes (sw x sh) -> (dw x dh) with tables of at most kx / ky taps: the ONE place that keeps a tile inside hbuf.
// The rows of a tile are first[dy0] .. first[dy1 - 1] + count[dy1 - 1] - 1 with first[d] = max(0, trunc(rho (d + 0.5) - support
// + 0.5)): over AA_TR outputs `first` advances by at most ceil(rho (AA_TR - 1)) (+ 1 for the float64 rounding of the two
// products), and the last output adds its ky taps.  Columns need no array: the horizontal pass reads the source itself.
inline int resample_aa_variant(int sw, int sh, int dw, int dh, int kx, int ky)
{
    if ((long)sw > (long)AA_RATIO * dw || (long)sh > (long)AA_RATIO * dh || kx > AA_KMAX || ky > AA_KMAX) return RESAMPLE_AA_GENERAL;
    const long span = ((long)(AA_TR - 1) * sh + dh - 1) / dh + 1 + ky;
    return span <= AA_RMAX ? RESAMPLE_AA_TILED : RESAMPLE_AA_GENERAL;
}
// The tables of one geometry on the device (srcnn_cubic_aa_f32_taps per axis).  xcoef is TAP-major, [kx][dw]: lanes that hold
// neighbouring output columns load neighbouring floats; ycoef is [dh][ky]: the row is the same for a whole wave.
struct ResampleAaTables {
    const int *xfirst, *xcount, *yfirst, *ycount;
    const float *xcoef, *ycoef;
    int kx, ky;
};
// `channels` planes x n_frames frames; variant: resample_aa_variant() of the geometry and the tables, or RESAMPLE_AA_GENERAL
// for any geometry; work: sh * dw floats per plane (general form only).  hipErrorInvalidValue for RESAMPLE_AA_TILED on a
// geometry resample_aa_variant() does not send there.
hipError_t launch_resample_aa(const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels, int n_frames,
                              const ResampleAaTables &t, int variant, float *work, hipStream_t st);

namespace host {
// The launch behind every antialiased resize (srcnn_resize_f32.cpp): checked arguments, device memory, the context's stream;
// tables cached per geometry, the form chosen by resample_aa_variant(), the general form's workspace grown on demand.
int resample_aa_dev(srcnn_ctx *c, const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels, int n_frames);
}  // namespace host

}  // namespace srcnn
