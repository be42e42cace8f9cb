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

#ifdef __HIPCC__
// The ONE load rule of a stored image (include/srcnn_amd.h, "Load"): every kernel that reads an ImageRef -- the accessor forms and
// the antialiased resize of srcnn_pipeline.hip, the metric kernels of srcnn_metrics.hip -- reads it through this.  The element
// kind is uniform over a launch: the switch is a scalar branch beside a global load.
__device__ __forceinline__ float image_load(const ImageRef &im, long at)
{
    switch (im.elem) {
    case ELEM_F32: return static_cast<const float *>(im.data)[at];
    case ELEM_F16: return (float)static_cast<const _Float16 *>(im.data)[at];                           // exact
    case ELEM_BF16: return __uint_as_float((unsigned)static_cast<const uint16_t *>(im.data)[at] << 16);  // exact
    default: return __fmul_rn((float)static_cast<const uint8_t *>(im.data)[at], im.scale);
    }
}
#endif

// The launchers of the float cubic resize, for float32 planes and for every other stored format: two families of kernels in
// srcnn_pipeline.hip, the float32 ones and their accessor forms, nine in all.  A call launches the float32 kernel (resize_cubic_f32_*, luma_resize_f32,
// resize_merge_f32: pointers and strides of the two descriptors) when BOTH sides are planar float32 (image_is_planar_f32; for
// the luma front the destination always is), the image kernel (element access through the ImageRef's load and store)
// otherwise: the same tables, tile, variant choice and summation order, and the same bits.
// `channels` planes x n_frames frames in one launch.  xfirst / yfirst: first[d] = floor(r), unclamped (the taps are first - 1 ..
// first + 2, each clamped to the plane by the kernels); xcoef / ycoef: four float32 coefficients per output column / row
// (srcnn_cubic_f32_taps).  The two launches around the banded path of a 3-channel image through a 1-channel model are the
// tiled form (hipErrorInvalidValue for a geometry resize_f32_variant() does not send there: the call never shrinks, and every
// up-scale fits the tile).  Front: Yup = the resize of Y = ((w0 x0 + w1 x1) + w2 x2) + off, luma = {w0, w1, w2, off}, the
// pixel's three channels ch_pitch apart.  Back: dst_c = resize(x_c) + (Ysr - Yup) g for c = 0, 1, 2, clamped to [clamp[0],
// clamp[1]] unless clamp is null; every product and sum rounded on its own.  yup / ysr are packed float32 planes (the
// context's workspace), strides and pitches in floats.
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

// ---- Pillow's resize of uint8 images (srcnn_resize_pil_image_dev; include/srcnn_amd.h has the arithmetic) -------------------
// The antialiased resize's two forms on integers, the same bytes from both.  tiled: one launch; a workgroup of 256 threads
// produces PIL_TR output rows x PIL_TC columns, the ROUNDED horizontal results of the source rows the tile spans stay in LDS as
// bytes (hbuf[PIL_RMAX][PIL_TC] = 5,120 bytes).  general: two launches of PIL_HC threads per workgroup, the horizontal pass
// into a uint8 workspace of sh x dw per plane, the vertical pass out of it -- any ratio and any tap count.
constexpr int PIL_TR = 16;        // output rows per workgroup (tiled form)
constexpr int PIL_TC = 64;        // output columns per workgroup (tiled form): one per lane of a wave
constexpr int PIL_HC = 256;       // output columns per workgroup (general form, both launches)
constexpr int PIL_RATIO = 4;      // the tiled form takes source sizes up to PIL_RATIO x the destination's, per axis
constexpr int PIL_KMAX = 17;      // ... and tables of at most this many taps per output sample
constexpr int PIL_RMAX = PIL_RATIO * (PIL_TR - 1) + 1 + PIL_KMAX + 2;      // source rows a tile may span: 80
constexpr int PIL_BITS = 22;      // fractional bits of a coefficient
constexpr long PIL_COEF_SUM_MAX = (1L << 23) - 1;      // sum |c_j| of one output sample: 24-bit products, an int32 sum
enum { RESAMPLE_PIL_GENERAL = 0, RESAMPLE_PIL_TILED = 1 };
// The tables of one geometry and filter on the device (srcnn_pil_taps per axis; the identity for an axis that keeps its length).
// xcoef is TAP-major, [kx][dw]; ycoef is [dh][ky].  tile_span: the most source rows a tile of PIL_TR output rows reads, walked
// over yfirst / ycount on the host when the tables were made (INT_MAX where yfirst is not ascending).
struct ResamplePilTables {
    const int *xfirst, *xcount, *yfirst, *ycount;
    const int *xcoef, *ycoef;
    int kx, ky, tile_span;
};
// Which form runs a geometry with these tables: the tiled one inside the antialiased tiled form's range, and only where the
// TABLES keep every tile inside hbuf
inline int resample_pil_variant(int sw, int sh, int dw, int dh, const ResamplePilTables &t)
{
    if ((long)sw > (long)PIL_RATIO * dw || (long)sh > (long)PIL_RATIO * dh || t.kx > PIL_KMAX || t.ky > PIL_KMAX) return RESAMPLE_PIL_GENERAL;
    return t.tile_span > 0 && t.tile_span <= PIL_RMAX ? RESAMPLE_PIL_TILED : RESAMPLE_PIL_GENERAL;
}
// Both descriptors ELEM_U8 (their scale is not read).  variant: resample_pil_variant(), or RESAMPLE_PIL_GENERAL for any
// geometry; work: sh * dw bytes per plane (general form only).  hipErrorInvalidValue for RESAMPLE_PIL_TILED with tables whose
// tile_span does not fit hbuf.
hipError_t launch_resample_pil(const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels, int n_frames,
                               const ResamplePilTables &t, int variant, uint8_t *work, hipStream_t st);

// ---- full-reference metrics (srcnn_metrics_image_dev; include/srcnn_amd.h has the semantics): srcnn_metrics.hip -------------
// Everything after the load is float64.  Three kernels, no floating-point atomic: metric_sse_kernel and metric_ssim_kernel write
// one partial sum per workgroup into a workspace, metric_finish_kernel adds the partials of a plane in a fixed order and writes
// {sse, n_px, ssim_sum, n_win}.  Tiles, partial counts and both reduction orders depend on the region's size only, so a plane's
// four doubles do not depend on the batch it is measured in.
//   SSE:  a workgroup of 256 threads takes METRIC_SSE_ROWS rows of the region, thread t the columns 4 t .. 4 t + 3, + 1024, ...
//   SSIM: a workgroup is ONE wave.  It owns METRIC_T window columns (64 source columns, one per lane) and a band of METRIC_B window
//         rows, walks down the band's METRIC_B + 10 source rows with a register ring of 11 rows of (a, b) per lane, forms the five
//         vertical 11-tap sums per row, writes them to LDS (5 x 64 doubles = 2,560 bytes), and lanes 0 .. METRIC_T - 1 form the five
//         horizontal sums and the window's SSIM.  Source rows re-read: 10 / METRIC_B; source columns re-read: 10 / METRIC_T.
constexpr int METRIC_WIN = 11;                       // the Gaussian window's taps
constexpr int METRIC_T = 64 - (METRIC_WIN - 1);      // window columns per workgroup: 54
constexpr int METRIC_B = 64;                         // window rows per workgroup
constexpr int METRIC_SSE_ROWS = 4;                   // region rows per workgroup of the SSE kernel
constexpr int METRIC_LDS_BYTES = 5 * 64 * 8;
enum { METRIC_FLAG_SSE = 1, METRIC_FLAG_SSIM = 2 };  // SRCNN_METRIC_*
inline long metric_sse_partials(int rh) { return ((long)rh + METRIC_SSE_ROWS - 1) / METRIC_SSE_ROWS; }
inline long metric_ssim_partials(int rw, int rh)     // 0 where the region holds no window
{
    if (rw < METRIC_WIN || rh < METRIC_WIN) return 0;
    return (((long)rw - METRIC_WIN + 1 + METRIC_T - 1) / METRIC_T) * (((long)rh - METRIC_WIN + 1 + METRIC_B - 1) / METRIC_B);
}
// a, b: the REGION (border already shaved off) of rw x rh, n_frames frames of `channels` channels; luma: null, or the four
// weights (channels == 3: one result per frame); gauss: the 11 normalised window weights; work: n_frames * P *
// (metric_sse_partials + metric_ssim_partials) doubles; out: n_frames * P * 4 doubles
hipError_t launch_metrics(const ImageRef &a, const ImageRef &b, int rw, int rh, int channels, int n_frames, const float *luma,
                          const double gauss[METRIC_WIN], double c1, double c2, int flags, double *work, double *out, hipStream_t st);

// ---- MS-SSIM (srcnn_msssim_image_dev; include/srcnn_amd.h has the semantics): srcnn_msssim.hip ------------------------------
// Scale 0 is the region of the stored pictures; scale j + 1 is scale j reduced by 2 x 2 means, a packed float64 plane of
// ceil(w_j / 2) x ceil(h_j / 2) in a workspace.  Three kernels, no floating-point atomic: msssim_pyramid_kernel makes the next
// scale of both pictures (256 threads: MSSSIM_PYR_ROWS rows x 64 columns), msssim_window_kernel is metric_ssim_kernel's shape
// (one wave, MSSSIM_T window columns x a band of window rows, 5 x 64 doubles of LDS) and writes one partial of the cs sum and one
// of the SSIM sum per workgroup, msssim_finish_kernel adds a scale's partials in a fixed order and writes {cs_sum, ssim_sum,
// n_win} per scale.  Every size below follows from (rw, rh, n_scales) alone.
constexpr int MSSSIM_MAX_SCALES = 5;
constexpr int MSSSIM_T = 64 - (METRIC_WIN - 1);      // window columns per workgroup: 54
// window rows per workgroup: a wave walks its band's rows one after the other, so the band sets how long the launch of a small
// scale lasts; scale 0 takes metric_ssim_kernel's band (10 / 64 of its rows read again), the scales >= 1 a short one
constexpr int MSSSIM_B0 = 64;
constexpr int MSSSIM_B1 = 16;
inline int msssim_band(int s) { return s ? MSSSIM_B1 : MSSSIM_B0; }
constexpr int MSSSIM_PYR_ROWS = 4;                   // rows of the next scale per workgroup of the pyramid kernel
constexpr int MSSSIM_LDS_BYTES = 5 * 64 * 8;
// the smallest region side n_scales scales fit in: 11 at the last scale, 10 * 2^(S - 1) + 1
inline int msssim_min_side(int n_scales) { return 10 * (1 << (n_scales - 1)) + 1; }
struct MsssimPlan {
    int w[MSSSIM_MAX_SCALES], h[MSSSIM_MAX_SCALES];            // the size of scale s
    long n_ct[MSSSIM_MAX_SCALES], n_bt[MSSSIM_MAX_SCALES];     // its column tiles and row bands
    long plane_off[MSSSIM_MAX_SCALES];      // scale s >= 1 of one picture of one result begins here, in doubles
    long plane_doubles;                     // ... and the scales 1 .. S - 1 of one picture of one result take this many
    long part_off[MSSSIM_MAX_SCALES];       // the partials of scale s of one result begin here: n_ct n_bt of cs, then as many of ssim
    long part_doubles;                      // ... and one result takes this many
};
inline bool msssim_plan(int rw, int rh, int n_scales, MsssimPlan *plan)      // false where a scale holds no window
{
    if (n_scales < 1 || n_scales > MSSSIM_MAX_SCALES || rw < msssim_min_side(n_scales) || rh < msssim_min_side(n_scales)) return false;
    MsssimPlan p{};
    for (int s = 0; s < n_scales; ++s) {
        p.w[s] = s ? (p.w[s - 1] + 1) / 2 : rw;
        p.h[s] = s ? (p.h[s - 1] + 1) / 2 : rh;
        p.n_ct[s] = ((long)p.w[s] - METRIC_WIN + 1 + MSSSIM_T - 1) / MSSSIM_T;
        p.n_bt[s] = ((long)p.h[s] - METRIC_WIN + 1 + msssim_band(s) - 1) / msssim_band(s);
        p.plane_off[s] = p.plane_doubles;
        if (s) p.plane_doubles += (long)p.w[s] * p.h[s];
        p.part_off[s] = p.part_doubles;
        p.part_doubles += 2 * p.n_ct[s] * p.n_bt[s];
    }
    *plan = p;
    return true;
}
// a, b: the REGION of rw x rh, as launch_metrics takes it; planes: 2 * n_frames * P * plan.plane_doubles doubles (may be null
// for one scale); parts: n_frames * P * plan.part_doubles doubles; out: n_frames * P * n_scales * 3 doubles.
// srcnn_image.cpp names no symbol of srcnn_msssim.hip: that unit hands its launcher over from a constructor that runs when
// the library is loaded, as the wide units do (srcnn_kernels.h), and where no unit has, the call is refused.
typedef hipError_t (*MsssimLauncher)(const ImageRef &a, const ImageRef &b, int rw, int rh, int channels, int n_frames,
                                     const float *luma, const double gauss[METRIC_WIN], double c1, double c2, int n_scales,
                                     double *planes, double *parts, double *out, hipStream_t st);
void set_msssim_launcher(MsssimLauncher l);
MsssimLauncher msssim_launcher();               // null until a unit has called set_msssim_launcher

namespace host {
// What the _f32 entry points (srcnn_resize_f32.cpp) and the _image_dev ones (srcnn_image.cpp, where these live) share.  All take
// checked arguments and device memory and run on the context's stream.
// planar float32 planes as a descriptor (strides and pitches in floats)
ImageRef f32_image(const float *p, size_t stride, size_t ch_pitch, size_t frame_pitch);
// the cubic resize: tables cached per geometry, one launch
int resize_cubic_dev(srcnn_ctx *c, const ImageRef &src, int src_w, int src_h, const ImageRef &dst, int dst_w, int dst_h, int channels,
                     int n_frames);
// resize + model, frame after frame through the context's one-frame workspace (claim_workspace / release_workspace)
int process_frames_dev(srcnn_ctx *c, const ImageRef &src, int src_w, int src_h, const ImageRef &dst, int dst_w, int dst_h, int n_frames);
// a 3-channel image through the 1-channel model: the rules behind the descriptors' own (SRCNN_OK and the gain, or the code and the
// reason; runs_colour ends the sentence that names the call for a colour model), and luma front, model, merge back per frame
int process_rgb_refusal(srcnn_ctx *c, const char *what, const char *runs_colour, int src_w, int src_h, int dst_w, int dst_h,
                        const float *luma, const float *clamp, float *g);
int process_rgb_frames_dev(srcnn_ctx *c, const ImageRef &src, int src_w, int src_h, const ImageRef &dst, int dst_w, int dst_h,
                           const float *luma, float g, const float *clamp, int n_frames);
// The launch behind every antialiased resize (srcnn_resize_f32.cpp): checked arguments, device memory, the context's stream;
// tables cached per geometry, the form chosen by resample_aa_variant(), the general form's workspace grown on demand.
int resample_aa_dev(srcnn_ctx *c, const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels, int n_frames);
// The launch behind every Pillow resize (srcnn_resize_f32.cpp): checked arguments, two ELEM_U8 descriptors in device memory, a
// known filter, the context's stream; tables cached per geometry and filter, the form chosen by resample_pil_variant(), the
// general form's byte workspace grown on demand.
int resample_pil_dev(srcnn_ctx *c, const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels, int n_frames,
                     int filter);
// The context's planar uint8 image of `channels` x n_frames planes of width x height (srcnn_process_pil_image_dev and
// srcnn_process_rgb_pil_image_dev resize into it), grown on demand
int pil_workspace_image(srcnn_ctx *c, int width, int height, int channels, int n_frames, void **data);
}  // namespace host

}  // namespace srcnn
