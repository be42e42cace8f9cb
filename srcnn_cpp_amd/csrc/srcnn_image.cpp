// srcnn_image.cpp -- images as they are stored: the descriptor check (srcnn_image_check) and the four device calls of the float
// image path on interleaved or planar pixels of float32, float16, bfloat16 or uint8 (srcnn_forward_image_dev,
// srcnn_resize_cubic_image_dev, srcnn_process_image_dev, srcnn_process_rgb_image_dev), and the antialiased resize on them
// (srcnn_resize_cubic_aa_image_dev; its launch is resample_aa_dev of srcnn_resize_f32.cpp).
// Each call equals store(its _f32_dev counterpart(load(x))) bit for bit.  With both descriptors planar float32 (and inside that
// counterpart's own gate) a call IS that counterpart; otherwise it runs the same per-frame routines, which live here and take
// two ImageRefs (the _f32 entry points of srcnn_resize_f32.cpp call them with float32 descriptors): the resize, the luma front
// and the merge back in the accessor forms of their kernels (srcnn_pipeline.hip), and the model itself on float32 planes
// in the context's workspace, converted in and out by convert_image_kernel where the stored format is not planar float32 already.
#include "srcnn_ctx.h"
#include "srcnn_image.h"

using namespace srcnn;
using namespace srcnn::host;

namespace {

size_t elem_size(int elem) { return elem == SRCNN_ELEM_F32 ? 4 : elem == SRCNN_ELEM_U8 ? 1 : 2; }

struct Dim {
    uint64_t n, step;
};
// the dimensions of an image that are used (count above 1): x, y, channel, frame
int used_dims(const srcnn_image *im, int width, int height, int channels, int n_frames, Dim out[4])
{
    const Dim all[4] = {{(uint64_t)width, im->px_step}, {(uint64_t)height, im->stride}, {(uint64_t)channels, im->ch_pitch},
                        {(uint64_t)n_frames, im->frame_pitch}};
    int k = 0;
    for (const Dim &d : all)
        if (d.n > 1) out[k++] = d;
    return k;
}

// offset of the last element, in elements; false when it (times the element size) does not fit in 63 bits
bool last_offset(const Dim *dims, int k, size_t es, uint64_t *last)
{
    unsigned __int128 sum = 0;
    for (int i = 0; i < k; ++i) sum += (unsigned __int128)(dims[i].n - 1) * dims[i].step;
    if ((sum + 1) * es > (unsigned __int128)INT64_MAX) return false;
    *last = (uint64_t)sum;
    return true;
}

int image_check(const srcnn_image *im, int width, int height, int channels, int n_frames, int is_dst)
{
    if (!im || !im->data || width <= 0 || height <= 0 || channels <= 0 || n_frames <= 0) return SRCNN_ERR_INVALID;
    if (im->elem < SRCNN_ELEM_F32 || im->elem > SRCNN_ELEM_U8) return SRCNN_ERR_INVALID;
    if (im->elem == SRCNN_ELEM_U8 && !(std::isfinite(im->scale) && im->scale > 0.f)) return SRCNN_ERR_INVALID;
    const size_t es = elem_size(im->elem);
    if (reinterpret_cast<uintptr_t>(im->data) % es) return SRCNN_ERR_INVALID;
    Dim d[4];
    const int k = used_dims(im, width, height, channels, n_frames, d);
    for (int i = 0; i < k; ++i)
        if (d[i].step == 0) return SRCNN_ERR_INVALID;
    uint64_t last;
    if (!last_offset(d, k, es, &last)) return SRCNN_ERR_INVALID;
    if (is_dst) {
        // injective where, sorted by step, every step exceeds the largest offset the smaller ones reach (sufficient)
        std::sort(d, d + k, [](const Dim &a, const Dim &b) { return a.step < b.step; });
        unsigned __int128 reach = 0;
        for (int i = 0; i < k; ++i) {
            if (!((unsigned __int128)d[i].step > reach)) return SRCNN_ERR_INVALID;
            reach += (unsigned __int128)(d[i].n - 1) * d[i].step;
        }
    }
    return SRCNN_OK;
}

size_t image_bytes(const srcnn_image *im, int width, int height, int channels, int n_frames)
{
    Dim d[4];
    const int k = used_dims(im, width, height, channels, n_frames, d);
    uint64_t last = 0;
    (void)last_offset(d, k, elem_size(im->elem), &last);      // (checked before)
    return (size_t)(last + 1) * elem_size(im->elem);
}

// a pitch whose count is 1 is ignored: the kernels multiply it by 0 only, but keep every field they see small and defined
ImageRef image_ref(const srcnn_image *im, int width, int height, int channels, int n_frames)
{
    return ImageRef{im->data, im->elem, im->elem == SRCNN_ELEM_U8 ? im->scale : 0.f, width > 1 ? (long)im->px_step : 1,
                    height > 1 ? (long)im->stride : 0, channels > 1 ? (long)im->ch_pitch : 0, n_frames > 1 ? (long)im->frame_pitch : 0};
}
// frame f of an image, as an image of one frame
ImageRef frame_of(const ImageRef &im, int f)
{
    ImageRef r = im;
    r.data = static_cast<char *>(im.data) + (size_t)f * (size_t)im.frame_pitch * elem_size(im.elem);
    r.frame_pitch = 0;
    return r;
}
// a packed float32 image of `channels` planes in the workspace
ImageRef packed_f32(float *p, int width, int height)
{
    return ImageRef{p, ELEM_F32, 0.f, 1, (long)width, (long)width * height, 0};
}

// planar float32 whose rows do not overlap: what the existing calls take, and (f32_row) the row stride they expect
bool planar_f32(const ImageRef &im, int width) { return image_is_planar_f32(im) && (im.stride == 0 || im.stride >= width); }
size_t f32_row(const ImageRef &im, int width) { return im.stride ? (size_t)im.stride : (size_t)width; }
// ... as a DESTINATION of the existing calls and of the banded path: their own gate on top (planes apart from each other, pitches
// in range).  A planar float32 destination that srcnn_image_check accepts and this refuses -- a channel pitch inside the row
// stride, say -- is written through the workspace and the converting kernel like any other layout, whatever the source is.
bool f32_direct_dst(const ImageRef &im, int C, int width, int height, int n_frames)
{
    constexpr long kMaxPitch = 1L << 40;
    return planar_f32(im, width) && im.ch_pitch < kMaxPitch && im.frame_pitch < kMaxPitch &&
           f32_planes_disjoint(C, f32_row(im, width), (size_t)im.ch_pitch, (size_t)im.frame_pitch, width, height, n_frames);
}
bool f32_direct_src(const ImageRef &im, int width) { return planar_f32(im, width) && im.ch_pitch < (1L << 40) && im.frame_pitch < (1L << 40); }

// the descriptors of a call: both checked, and the destination's bytes apart from the source's
int images_refusal(srcnn_ctx *c, const char *what, const srcnn_image *src, int src_w, int src_h, const srcnn_image *dst, int dst_w,
                   int dst_h, int channels, int n_frames)
{
    if (image_check(src, src_w, src_h, channels, n_frames, 0))
        return fail(c, SRCNN_ERR_INVALID, "%s: bad source image (srcnn_image_check)", what);
    if (image_check(dst, dst_w, dst_h, channels, n_frames, 1))
        return fail(c, SRCNN_ERR_INVALID, "%s: bad destination image: a descriptor srcnn_image_check refuses, or an address map "
                                          "it cannot show injective", what);
    if ((long)channels * n_frames > 0x7fffffffL) return fail(c, SRCNN_ERR_INVALID, "%s: bad arguments", what);
    if (ranges_overlap(src->data, image_bytes(src, src_w, src_h, channels, n_frames), dst->data,
                       image_bytes(dst, dst_w, dst_h, channels, n_frames)))
        return fail(c, SRCNN_ERR_INVALID, "%s: src and dst overlap (the call cannot run in place)", what);
    return SRCNN_OK;
}

// the workspace (and the band maps) were last used on another stream: wait for that work before this call overwrites it
int claim_workspace(srcnn_ctx *c, size_t floats, float **work)
{
    int rc;
    if (c->sp_done && c->sp_stream && c->sp_stream != c->stream) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->sp_done, 0));
    if ((rc = reserve(c, c->f32_work, floats * sizeof(float)))) return rc;      // (growing waits for the device)
    *work = static_cast<float *>(c->f32_work.p);
    return SRCNN_OK;
}
int release_workspace(srcnn_ctx *c)      // the last kernel read the workspace behind forward_banded's event
{
    HIP_TRY(c, hipEventRecord(c->sp_done, c->stream));
    c->sp_stream = c->stream;
    return SRCNN_OK;
}

// The model on one frame: `in` (packed float32 planes) -> frame `dst`; direct: dst is planar float32 the banded path can write
// itself, else through `out` (a second set of packed planes in the workspace) and a converting pass
int model_frame(srcnn_ctx *c, const float *in, float *out, const ImageRef &dst, bool direct, int width, int height)
{
    const int C = c->channels;
    const size_t plane = (size_t)width * height;
    int rc;
    BandedPlanes io;
    io.f32 = true;
    io.src = in;
    io.src_stride = (size_t)width;
    io.ch_step = C == 1 ? 0 : plane;
    io.dst = direct ? dst.data : out;
    io.dst_stride = direct ? (height > 1 ? (size_t)dst.stride : (size_t)width) : (size_t)width;
    io.dst_ch_pitch = C == 1 ? 0 : direct ? (size_t)dst.ch_pitch : plane;
    if ((rc = forward_banded(c, io, width, height, 1))) return rc;
    if (!direct) HIP_TRY(c, launch_convert_image(packed_f32(out, width, height), dst, width, height, C, 1, c->stream));
    return SRCNN_OK;
}

}  // namespace

// ---- what the _f32 entry points (srcnn_resize_f32.cpp) and the _image_dev ones below share: checked arguments, device memory,
// the context's stream ----
namespace srcnn {
namespace host {

ImageRef f32_image(const float *p, size_t stride, size_t ch_pitch, size_t frame_pitch)
{
    return ImageRef{const_cast<float *>(p), ELEM_F32, 0.f, 1, (long)stride, (long)ch_pitch, (long)frame_pitch};
}

int resize_cubic_dev(srcnn_ctx *c, const ImageRef &src, int src_w, int src_h, const ImageRef &dst, int dst_w, int dst_h, int channels,
                     int n_frames)
{
    ResizeTablesF32 t;
    int rc;
    if ((rc = ensure_tables_f32(c, src_w, src_h, dst_w, dst_h, &t))) return rc;
    HIP_TRY(c, launch_resize_cubic_image(src, src_w, src_h, dst, dst_w, dst_h, channels, n_frames, t.xfirst, t.xcoef, t.yfirst, t.ycoef,
                                         c->stream));
    return SRCNN_OK;
}

// Resize + model: every channel of a frame into the context's one-frame workspace (packed float32 planes), then the model on that
// frame exactly as srcnn_forward_f32_dev runs it -- into the destination itself where the banded path can write it
// (f32_direct_dst), else through a second set of planes and a converting pass; frame after frame on the context's stream.
int process_frames_dev(srcnn_ctx *c, const ImageRef &src, int src_w, int src_h, const ImageRef &dst, int dst_w, int dst_h, int n_frames)
{
    const int C = c->channels;
    const bool direct = f32_direct_dst(dst, C, dst_w, dst_h, n_frames);
    const size_t plane = (size_t)dst_w * dst_h;
    int rc;
    float *work = nullptr;
    if ((rc = claim_workspace(c, (direct ? 1 : 2) * C * plane, &work))) return rc;      // the resized frame, and the model's output
    for (int f = 0; f < n_frames; ++f) {
        if ((rc = resize_cubic_dev(c, frame_of(src, f), src_w, src_h, packed_f32(work, dst_w, dst_h), dst_w, dst_h, C, 1))) return rc;
        if ((rc = model_frame(c, work, work + C * plane, frame_of(dst, f), direct, dst_w, dst_h))) return rc;
    }
    return release_workspace(c);
}

// What a 3-channel image through a 1-channel model asks beyond its descriptors, in this order: the luma row (and its gain), the
// clamp, no shrinking (which implies that the geometry fits the resize's tile, what the two kernels rest on), a 1-channel model
// (`runs_colour`: the call that runs a colour model, and on what), the gate of srcnn_forward_f32.
int process_rgb_refusal(srcnn_ctx *c, const char *what, const char *runs_colour, int src_w, int src_h, int dst_w, int dst_h,
                        const float *luma, const float *clamp, float *g)
{
    if (!luma || srcnn_luma_gain(luma, g) != SRCNN_OK)
        return fail(c, SRCNN_ERR_INVALID, "%s: luma must be four finite floats {w0, w1, w2, offset} with w0 + w1 + w2 > 0", what);
    if (clamp && !(clamp[0] <= clamp[1]))
        return fail(c, SRCNN_ERR_INVALID, "%s: clamp {%g, %g}: expected lo <= hi, neither a NaN", what, (double)clamp[0], (double)clamp[1]);
    if (dst_w < src_w || dst_h < src_h)
        return fail(c, SRCNN_ERR_INVALID, "%s: %d x %d -> %d x %d shrinks the image (a super-resolution call resizes up or not at all)",
                    what, src_w, src_h, dst_w, dst_h);
    if (resize_f32_variant(src_w, src_h, dst_w, dst_h) != RESIZE_F32_TILED)
        return fail(c, SRCNN_ERR_INVALID, "%s: %d x %d -> %d x %d does not fit the resize's tile", what, src_w, src_h, dst_w, dst_h);
    if (c->channels != 1)
        return fail(c, SRCNN_ERR_STATE, "%s runs a 1-channel model on the luma of the image: the context holds a colour model (3 "
                                        "channels, 9-%d-5), which %s themselves", what, c->f2, runs_colour);
    return forward_f32_refusal(c);
}

// Per frame: Yup = resize(luma of the three channels) into the first plane of the workspace, Ysr = the model on Yup -- exactly as
// srcnn_forward_f32_dev runs it -- into the second, then every output channel = resize of its source channel + (Ysr - Yup) g.
int process_rgb_frames_dev(srcnn_ctx *c, const ImageRef &src, int src_w, int src_h, const ImageRef &dst, int dst_w, int dst_h,
                           const float *luma, float g, const float *clamp, int n_frames)
{
    const size_t plane = (size_t)dst_w * dst_h;
    int rc;
    float *yup = nullptr;
    if ((rc = claim_workspace(c, 2 * plane, &yup))) return rc;
    float *ysr = yup + plane;
    ResizeTablesF32 t;
    if ((rc = ensure_tables_f32(c, src_w, src_h, dst_w, dst_h, &t))) return rc;
    for (int f = 0; f < n_frames; ++f) {
        const ImageRef sf = frame_of(src, f);
        HIP_TRY(c, launch_luma_resize_image(sf, src_w, src_h, yup, dst_w, 0, dst_w, dst_h, 1, luma, t.xfirst, t.xcoef, t.yfirst,
                                            t.ycoef, c->stream));
        BandedPlanes io;
        io.f32 = true;
        io.src = yup;
        io.src_stride = (size_t)dst_w;
        io.dst = ysr;
        io.dst_stride = (size_t)dst_w;
        if ((rc = forward_banded(c, io, dst_w, dst_h, 1))) return rc;
        HIP_TRY(c, launch_resize_merge_image(sf, src_w, src_h, ysr, dst_w, 0, yup, dst_w, 0, frame_of(dst, f), dst_w, dst_h, 1, g, clamp,
                                             t.xfirst, t.xcoef, t.yfirst, t.ycoef, c->stream));
    }
    return release_workspace(c);      // (the merge read the workspace behind forward_banded's event)
}

}  // namespace host

static MsssimLauncher g_msssim_launcher = nullptr;
void set_msssim_launcher(MsssimLauncher l) { g_msssim_launcher = l; }
MsssimLauncher msssim_launcher() { return g_msssim_launcher; }
}  // namespace srcnn

namespace {

// what srcnn_metrics_image_dev and srcnn_msssim_image_dev refuse alike, up to the region the border leaves: rw x rh
int metric_args_refusal(srcnn_ctx *c, const char *what, const srcnn_image *a, const srcnn_image *b, int width, int height, int channels,
                        int n_frames, int border, const float *luma, double data_range, long *rw_out, long *rh_out)
{
    if (image_check(a, width, height, channels, n_frames, 0)) return fail(c, SRCNN_ERR_INVALID, "%s: bad image a (srcnn_image_check)", what);
    if (image_check(b, width, height, channels, n_frames, 0)) return fail(c, SRCNN_ERR_INVALID, "%s: bad image b (srcnn_image_check)", what);
    if (channels != 1 && channels != 3) return fail(c, SRCNN_ERR_INVALID, "%s: %d channels: expected 1 or 3", what, channels);
    if (luma && channels != 3)
        return fail(c, SRCNN_ERR_INVALID, "%s: a luma needs 3 channels, the images have %d (pass NULL to measure the plane itself)", what, channels);
    if (luma && !(std::isfinite(luma[0]) && std::isfinite(luma[1]) && std::isfinite(luma[2]) && std::isfinite(luma[3])))
        return fail(c, SRCNN_ERR_INVALID, "%s: luma must be four finite floats {w0, w1, w2, offset}", what);
    if (!(std::isfinite(data_range) && data_range > 0.0))
        return fail(c, SRCNN_ERR_INVALID, "%s: data_range %g: expected a finite number > 0", what, data_range);
    if (border < 0) return fail(c, SRCNN_ERR_INVALID, "%s: border %d: expected >= 0", what, border);
    const long rw = (long)width - 2L * border, rh = (long)height - 2L * border;
    if (rw < 1 || rh < 1)
        return fail(c, SRCNN_ERR_INVALID, "%s: a border of %d leaves nothing of a %d x %d image", what, border, width, height);
    *rw_out = rw;
    *rh_out = rh;
    return SRCNN_OK;
}

// the region: the first pixel inside the border becomes element (0, 0)
ImageRef metric_region(const srcnn_image *im, int width, int height, int channels, int n_frames, int border)
{
    ImageRef r = image_ref(im, width, height, channels, n_frames);
    r.data = static_cast<char *>(r.data) + ((size_t)border * (size_t)r.stride + (size_t)border * (size_t)r.px_step) * elem_size(r.elem);
    return r;
}

// the window in float64: exp(-(i - 5)^2 / 4.5), divided by the sum taken in ascending order; and C1, C2 of a data range
void metric_constants(double data_range, double g[METRIC_WIN], double *c1, double *c2)
{
    double total = 0.0;
    for (int k = 0; k < METRIC_WIN; ++k) {
        g[k] = std::exp(-(double)((k - 5) * (k - 5)) / 4.5);
        total += g[k];
    }
    for (int k = 0; k < METRIC_WIN; ++k) g[k] /= total;
    *c1 = (0.01 * data_range) * (0.01 * data_range);
    *c2 = (0.03 * data_range) * (0.03 * data_range);
}

}  // namespace

extern "C" {

int srcnn_image_check(const srcnn_image *im, int width, int height, int channels, int n_frames, int is_dst)
{
    return image_check(im, width, height, channels, n_frames, is_dst);
}

int srcnn_forward_image_dev(srcnn_ctx *c, const srcnn_image *src, const srcnn_image *dst, int width, int height, int n_frames)
{
    BIND(c);
    int rc;
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    const int C = c->channels;
    if ((rc = images_refusal(c, "forward_image_dev", src, width, height, dst, width, height, C, n_frames))) return rc;
    const ImageRef s = image_ref(src, width, height, C, n_frames), d = image_ref(dst, width, height, C, n_frames);
    const bool direct = f32_direct_dst(d, C, width, height, n_frames);
    if (f32_direct_src(s, width) && direct)
        return srcnn_forward_f32_dev(c, static_cast<const float *>(s.data), f32_row(s, width), s.ch_pitch, s.frame_pitch,
                                     static_cast<float *>(d.data), f32_row(d, width), d.ch_pitch, d.frame_pitch, width, height,
                                     n_frames);
    if ((rc = forward_f32_refusal(c))) return rc;      // the gate of srcnn_forward_f32, before anything is launched
    const size_t plane = (size_t)width * height;
    // the workspace holds what the call needs: C planes for a source that is not packed float32 already, C for a destination the
    // banded path cannot write itself
    const bool packed = image_is_planar_f32(s) && (height == 1 || (size_t)s.stride == (size_t)width) && (C == 1 || (size_t)s.ch_pitch == plane);
    float *work = nullptr;
    if ((rc = claim_workspace(c, ((packed ? 0 : 1) + (direct ? 0 : 1)) * C * plane, &work))) return rc;
    float *out = work + (packed ? 0 : C * plane);
    for (int f = 0; f < n_frames; ++f) {
        const float *in = work;
        if (packed)
            in = static_cast<const float *>(frame_of(s, f).data);
        else
            HIP_TRY(c, launch_convert_image(frame_of(s, f), packed_f32(work, width, height), width, height, C, 1, c->stream));
        if ((rc = model_frame(c, in, out, frame_of(d, f), direct, width, height))) return rc;
    }
    return release_workspace(c);
}

int srcnn_resize_cubic_image_dev(srcnn_ctx *c, const srcnn_image *src, int src_w, int src_h, const srcnn_image *dst, int dst_w,
                                 int dst_h, int channels, int n_frames)
{
    BIND(c);
    int rc;
    if ((rc = images_refusal(c, "resize_cubic_image_dev", src, src_w, src_h, dst, dst_w, dst_h, channels, n_frames))) return rc;
    const ImageRef s = image_ref(src, src_w, src_h, channels, n_frames), d = image_ref(dst, dst_w, dst_h, channels, n_frames);
    if (f32_direct_src(s, src_w) && f32_direct_dst(d, channels, dst_w, dst_h, n_frames))
        return srcnn_resize_cubic_f32_dev(c, static_cast<const float *>(s.data), f32_row(s, src_w), s.ch_pitch, s.frame_pitch, src_w,
                                          src_h, static_cast<float *>(d.data), f32_row(d, dst_w), d.ch_pitch, d.frame_pitch, dst_w,
                                          dst_h, channels, n_frames);
    return resize_cubic_dev(c, s, src_w, src_h, d, dst_w, dst_h, channels, n_frames);
}

int srcnn_resize_cubic_aa_image_dev(srcnn_ctx *c, const srcnn_image *src, int src_w, int src_h, const srcnn_image *dst, int dst_w,
                                    int dst_h, int channels, int n_frames)
{
    BIND(c);
    int rc;
    if ((rc = images_refusal(c, "resize_cubic_aa_image_dev", src, src_w, src_h, dst, dst_w, dst_h, channels, n_frames))) return rc;
    // (one set of kernels for every format: planar float32 is an element kind like the others)
    return resample_aa_dev(c, image_ref(src, src_w, src_h, channels, n_frames), src_w, src_h,
                           image_ref(dst, dst_w, dst_h, channels, n_frames), dst_w, dst_h, channels, n_frames);
}

int srcnn_process_image_dev(srcnn_ctx *c, const srcnn_image *src, int src_w, int src_h, const srcnn_image *dst, int dst_w, int dst_h,
                            int n_frames)
{
    BIND(c);
    int rc;
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    const int C = c->channels;
    if ((rc = images_refusal(c, "process_image_dev", src, src_w, src_h, dst, dst_w, dst_h, C, n_frames))) return rc;
    const ImageRef s = image_ref(src, src_w, src_h, C, n_frames), d = image_ref(dst, dst_w, dst_h, C, n_frames);
    if (f32_direct_src(s, src_w) && f32_direct_dst(d, C, dst_w, dst_h, n_frames))
        return srcnn_process_f32_dev(c, static_cast<const float *>(s.data), f32_row(s, src_w), s.ch_pitch, s.frame_pitch, src_w, src_h,
                                     static_cast<float *>(d.data), f32_row(d, dst_w), d.ch_pitch, d.frame_pitch, dst_w, dst_h,
                                     n_frames);
    if ((rc = forward_f32_refusal(c))) return rc;
    return process_frames_dev(c, s, src_w, src_h, d, dst_w, dst_h, n_frames);
}

int srcnn_process_rgb_image_dev(srcnn_ctx *c, const srcnn_image *src, int src_w, int src_h, const srcnn_image *dst, int dst_w,
                                int dst_h, const float *luma, const float *clamp, int n_frames)
{
    BIND(c);
    int rc;
    const char *what = "process_rgb_image_dev";
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    if ((rc = images_refusal(c, what, src, src_w, src_h, dst, dst_w, dst_h, 3, n_frames))) return rc;
    const ImageRef s = image_ref(src, src_w, src_h, 3, n_frames), d = image_ref(dst, dst_w, dst_h, 3, n_frames);
    if (f32_direct_src(s, src_w) && f32_direct_dst(d, 3, dst_w, dst_h, n_frames))
        return srcnn_process_rgb_f32_dev(c, static_cast<const float *>(s.data), f32_row(s, src_w), s.ch_pitch, s.frame_pitch, src_w,
                                         src_h, static_cast<float *>(d.data), f32_row(d, dst_w), d.ch_pitch, d.frame_pitch, dst_w,
                                         dst_h, luma, clamp, n_frames);
    float g = 0.f;
    if ((rc = process_rgb_refusal(c, what, "srcnn_process_image_dev runs on the three channels", src_w, src_h, dst_w, dst_h, luma, clamp,
                                  &g)))
        return rc;
    return process_rgb_frames_dev(c, s, src_w, src_h, d, dst_w, dst_h, luma, g, clamp, n_frames);
}

/* ---- Pillow's resize of uint8 images (tables and launch: resample_pil_dev of srcnn_resize_f32.cpp) ---- */
static bool pil_filter_known(int filter) { return filter == SRCNN_PIL_BILINEAR || filter == SRCNN_PIL_BICUBIC; }
static const char *const kPilBytes = "Pillow's resize works on the bytes of SRCNN_ELEM_U8 images";
static const char *const kPilFilter = "expected SRCNN_PIL_BILINEAR (2) or SRCNN_PIL_BICUBIC (3)";

int srcnn_resize_pil_image_dev(srcnn_ctx *c, const srcnn_image *src, int src_w, int src_h, const srcnn_image *dst, int dst_w, int dst_h,
                               int channels, int n_frames, int filter)
{
    BIND(c);
    int rc;
    const char *what = "resize_pil_image_dev";
    // the scale of a descriptor is not read: the check sees a valid one in its place
    srcnn_image s8{}, d8{};
    if (src) { s8 = *src; s8.scale = 1.f; }
    if (dst) { d8 = *dst; d8.scale = 1.f; }
    if ((rc = images_refusal(c, what, src ? &s8 : nullptr, src_w, src_h, dst ? &d8 : nullptr, dst_w, dst_h, channels, n_frames))) return rc;
    if (s8.elem != SRCNN_ELEM_U8 || d8.elem != SRCNN_ELEM_U8)
        return fail(c, SRCNN_ERR_INVALID, "%s: elem %d -> %d: %s", what, s8.elem, d8.elem, kPilBytes);
    if (!pil_filter_known(filter)) return fail(c, SRCNN_ERR_INVALID, "%s: filter %d: %s", what, filter, kPilFilter);
    return resample_pil_dev(c, image_ref(&s8, src_w, src_h, channels, n_frames), src_w, src_h,
                            image_ref(&d8, dst_w, dst_h, channels, n_frames), dst_w, dst_h, channels, n_frames, filter);
}

// what the two process calls ask of the source beyond their counterparts' gates; then the resize into the context's planar
// uint8 image, which carries the source's scale: *mid describes it
static int pil_front_refusal(srcnn_ctx *c, const char *what, const srcnn_image *src, int src_w, int src_h, int dst_w, int dst_h, int filter)
{
    if (src->elem != SRCNN_ELEM_U8) return fail(c, SRCNN_ERR_INVALID, "%s: source elem %d: %s", what, src->elem, kPilBytes);
    if (!pil_filter_known(filter)) return fail(c, SRCNN_ERR_INVALID, "%s: filter %d: %s", what, filter, kPilFilter);
    if (dst_w < src_w || dst_h < src_h)
        return fail(c, SRCNN_ERR_INVALID, "%s: %d x %d -> %d x %d shrinks the image (a super-resolution call resizes up or not at all)",
                    what, src_w, src_h, dst_w, dst_h);
    return SRCNN_OK;
}
static int pil_front_dev(srcnn_ctx *c, const srcnn_image *src, int src_w, int src_h, int dst_w, int dst_h, int channels, int n_frames,
                         int filter, srcnn_image *mid)
{
    int rc;
    void *p = nullptr;
    if ((rc = pil_workspace_image(c, dst_w, dst_h, channels, n_frames, &p))) return rc;
    const size_t plane = (size_t)dst_w * dst_h;
    *mid = srcnn_image{p, SRCNN_ELEM_U8, src->scale, 1, (size_t)dst_w, plane, (size_t)channels * plane};
    return resample_pil_dev(c, image_ref(src, src_w, src_h, channels, n_frames), src_w, src_h,
                            image_ref(mid, dst_w, dst_h, channels, n_frames), dst_w, dst_h, channels, n_frames, filter);
}

int srcnn_process_pil_image_dev(srcnn_ctx *c, const srcnn_image *src, int src_w, int src_h, const srcnn_image *dst, int dst_w, int dst_h,
                                int n_frames, int filter)
{
    BIND(c);
    int rc;
    const char *what = "process_pil_image_dev";
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    const int C = c->channels;
    if ((rc = images_refusal(c, what, src, src_w, src_h, dst, dst_w, dst_h, C, n_frames))) return rc;
    if ((rc = pil_front_refusal(c, what, src, src_w, src_h, dst_w, dst_h, filter))) return rc;
    if ((rc = forward_f32_refusal(c))) return rc;      // the gate of srcnn_forward_f32, before anything is launched
    srcnn_image mid;
    if ((rc = pil_front_dev(c, src, src_w, src_h, dst_w, dst_h, C, n_frames, filter, &mid))) return rc;
    return srcnn_forward_image_dev(c, &mid, dst, dst_w, dst_h, n_frames);
}

int srcnn_process_rgb_pil_image_dev(srcnn_ctx *c, const srcnn_image *src, int src_w, int src_h, const srcnn_image *dst, int dst_w,
                                    int dst_h, const float *luma, const float *clamp, int n_frames, int filter)
{
    BIND(c);
    int rc;
    const char *what = "process_rgb_pil_image_dev";
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    if ((rc = images_refusal(c, what, src, src_w, src_h, dst, dst_w, dst_h, 3, n_frames))) return rc;
    float g = 0.f;
    if ((rc = process_rgb_refusal(c, what, "srcnn_process_pil_image_dev runs on the three channels", src_w, src_h, dst_w, dst_h, luma,
                                  clamp, &g)))
        return rc;
    if ((rc = pil_front_refusal(c, what, src, src_w, src_h, dst_w, dst_h, filter))) return rc;
    srcnn_image mid;
    if ((rc = pil_front_dev(c, src, src_w, src_h, dst_w, dst_h, 3, n_frames, filter, &mid))) return rc;
    return srcnn_process_rgb_image_dev(c, &mid, dst_w, dst_h, dst, dst_w, dst_h, luma, clamp, n_frames);
}

/* ---- full-reference metrics: {sse, n_px, ssim_sum, n_win} per (frame, result), float64 after the load (srcnn_metrics.hip) ---- */
int srcnn_metrics_image_dev(srcnn_ctx *c, const srcnn_image *a, const srcnn_image *b, int width, int height, int channels,
                            int n_frames, int border, const float *luma, double data_range, int flags, double *d_out)
{
    BIND(c);
    int rc;
    const char *what = "metrics_image_dev";
    long rw, rh;
    if ((rc = metric_args_refusal(c, what, a, b, width, height, channels, n_frames, border, luma, data_range, &rw, &rh))) return rc;
    if (!flags || (flags & ~(SRCNN_METRIC_SSE | SRCNN_METRIC_SSIM)))
        return fail(c, SRCNN_ERR_INVALID, "%s: flags %#x: expected SRCNN_METRIC_SSE, SRCNN_METRIC_SSIM or both", what, (unsigned)flags);
    if ((flags & SRCNN_METRIC_SSIM) && (rw < METRIC_WIN || rh < METRIC_WIN))
        return fail(c, SRCNN_ERR_INVALID, "%s: SSIM needs a region of at least 11 x 11, this one is %ld x %ld", what, rw, rh);
    if (!d_out) return fail(c, SRCNN_ERR_INVALID, "%s: null output", what);
    const int per_frame = luma ? 1 : channels;
    if ((long)per_frame * n_frames > 0x7fffffffL) return fail(c, SRCNN_ERR_INVALID, "%s: bad arguments", what);
    auto region = [&](const srcnn_image *im) { return metric_region(im, width, height, channels, n_frames, border); };
    double g[METRIC_WIN], c1, c2;
    metric_constants(data_range, g, &c1, &c2);
    const unsigned __int128 doubles = (unsigned __int128)per_frame * n_frames *
                                      (size_t)(metric_sse_partials((int)rh) + metric_ssim_partials((int)rw, (int)rh));
    if (doubles > ((unsigned __int128)1 << 40)) return fail(c, SRCNN_ERR_NOMEM, "%s: the workspace of the partial sums is too large", what);
    // the partials were last written on another stream: that work ends before this call overwrites them
    if (c->metric_stream && c->metric_stream != c->stream) HIP_TRY(c, hipStreamSynchronize(c->metric_stream));
    if ((rc = reserve(c, c->metric_work, (size_t)doubles * sizeof(double)))) return rc;      // (growing waits for the device)
    c->metric_stream = c->stream;
    HIP_TRY(c, launch_metrics(region(a), region(b), (int)rw, (int)rh, channels, n_frames, luma, g, c1, c2, flags,
                              static_cast<double *>(c->metric_work.p), d_out, c->stream));
    return SRCNN_OK;
}

double srcnn_metric_psnr(double sse, double n_px, double data_range)
{
    if (!(sse >= 0.0) || !(n_px > 0.0) || !(data_range > 0.0)) return std::nan("");
    if (sse == 0.0) return HUGE_VAL;
    return 10.0 * std::log10(data_range * data_range * n_px / sse);
}

/* ---- MS-SSIM: {cs_sum, ssim_sum, n_win} per (frame, result, scale), float64 after the load (srcnn_msssim.hip) ---- */
int srcnn_msssim_image_dev(srcnn_ctx *c, const srcnn_image *a, const srcnn_image *b, int width, int height, int channels,
                           int n_frames, int border, const float *luma, double data_range, int n_scales, double *d_out)
{
    BIND(c);
    int rc;
    const char *what = "msssim_image_dev";
    long rw, rh;
    if ((rc = metric_args_refusal(c, what, a, b, width, height, channels, n_frames, border, luma, data_range, &rw, &rh))) return rc;
    if (n_scales < 1 || n_scales > MSSSIM_MAX_SCALES)
        return fail(c, SRCNN_ERR_INVALID, "%s: n_scales %d: expected 1 .. %d", what, n_scales, (int)MSSSIM_MAX_SCALES);
    if (rw < msssim_min_side(n_scales) || rh < msssim_min_side(n_scales))
        return fail(c, SRCNN_ERR_INVALID, "%s: %d scales need a region of at least %d x %d (11 x 11 at the last scale), this one is %ld x %ld",
                    what, n_scales, msssim_min_side(n_scales), msssim_min_side(n_scales), rw, rh);
    if (!d_out) return fail(c, SRCNN_ERR_INVALID, "%s: null output", what);
    const int per_frame = luma ? 1 : channels;
    if ((long)per_frame * n_frames > 0x7fffffffL) return fail(c, SRCNN_ERR_INVALID, "%s: bad arguments", what);
    if (!msssim_launcher())
        return fail(c, SRCNN_ERR_STATE, "%s: this library was linked without srcnn_msssim.hip, the unit that holds the MS-SSIM kernels", what);
    MsssimPlan plan;
    if (!msssim_plan((int)rw, (int)rh, n_scales, &plan)) return fail(c, SRCNN_ERR_INVALID, "%s: bad arguments", what);
    double g[METRIC_WIN], c1, c2;
    metric_constants(data_range, g, &c1, &c2);
    // both pictures' planes of the scales >= 1, then the partials
    const unsigned __int128 results = (unsigned __int128)per_frame * n_frames;
    const unsigned __int128 plane_doubles = 2 * results * (unsigned __int128)plan.plane_doubles;
    const unsigned __int128 doubles = plane_doubles + results * (unsigned __int128)plan.part_doubles;
    if (doubles > ((unsigned __int128)1 << 40)) return fail(c, SRCNN_ERR_NOMEM, "%s: the workspace of the scales is too large", what);
    // the workspace was last written on another stream: that work ends before this call overwrites it
    if (c->msssim_stream && c->msssim_stream != c->stream) HIP_TRY(c, hipStreamSynchronize(c->msssim_stream));
    if ((rc = reserve(c, c->msssim_work, (size_t)doubles * sizeof(double)))) return rc;      // (growing waits for the device)
    c->msssim_stream = c->stream;
    double *work = static_cast<double *>(c->msssim_work.p);
    HIP_TRY(c, msssim_launcher()(metric_region(a, width, height, channels, n_frames, border),
                                 metric_region(b, width, height, channels, n_frames, border), (int)rw, (int)rh, channels, n_frames, luma,
                                 g, c1, c2, n_scales, work, work + (size_t)plane_doubles, d_out, c->stream));
    return SRCNN_OK;
}

double srcnn_metric_msssim(const double *sums, int n_scales, const double *weights)
{
    static const double kWang[MSSSIM_MAX_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    if (!sums || n_scales < 1 || n_scales > MSSSIM_MAX_SCALES || (!weights && n_scales != MSSSIM_MAX_SCALES)) return std::nan("");
    const double *w = weights ? weights : kWang;
    double product = 1.0;
    for (int s = 0; s < n_scales; ++s) {
        const double cs = sums[3 * s], ssim = sums[3 * s + 1], n_win = sums[3 * s + 2];
        if (std::isnan(cs) || std::isnan(ssim) || std::isnan(w[s]) || !(n_win > 0.0)) return std::nan("");
        const double mean = (s == n_scales - 1 ? ssim : cs) / n_win;
        product *= mean > 0.0 ? std::pow(mean, w[s]) : 0.0;      // never a power of a negative number
    }
    return product;
}

#ifdef SRCNN_TUNING_BUILD
/* Undocumented test hook (tuning build only, not part of the ABI): MSSSIM_T (window columns of one workgroup of the MS-SSIM
 * window kernel), MSSSIM_B0 and MSSSIM_B1 (its window rows at scale 0 and at the scales >= 1), MSSSIM_PYR_ROWS, and the LDS
 * bytes of the window kernel. */
int srcnn_debug_msssim_limits(int *out5)
{
    if (!out5) return SRCNN_ERR_INVALID;
    const int v[5] = {MSSSIM_T, MSSSIM_B0, MSSSIM_B1, MSSSIM_PYR_ROWS, MSSSIM_LDS_BYTES};
    for (int k = 0; k < 5; ++k) out5[k] = v[k];
    return SRCNN_OK;
}

/* Undocumented test hook (tuning build only, not part of the ABI): METRIC_T, METRIC_B (window columns and rows of one SSIM
 * workgroup), METRIC_SSE_ROWS, and the LDS bytes of the SSIM kernel. */
int srcnn_debug_metric_limits(int *out4)
{
    if (!out4) return SRCNN_ERR_INVALID;
    const int v[4] = {METRIC_T, METRIC_B, METRIC_SSE_ROWS, METRIC_LDS_BYTES};
    for (int k = 0; k < 4; ++k) out4[k] = v[k];
    return SRCNN_OK;
}
#endif

}  // extern "C"
