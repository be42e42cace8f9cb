// srcnn_color.cpp -- the colour models (srcnn_set_model_color: 3 input and 3 output channels, 9-f2-5): their weight table, the
// banded path colour layer 1 -> spatial layer 2 -> colour layer 3 (srcnn_color_kernels.hip, srcnn_spatial_kernels.hip) behind
// srcnn_forward_color_dev, the host-buffer form, and srcnn_process_bgr(_dev) with a colour model loaded.
#include "srcnn_ctx.h"

using namespace srcnn;
using namespace srcnn::host;

namespace srcnn {
namespace host {

// The fragment table of srcnn_kernels.h (color_table_floats()).  w1 [64][3][9][9], w2 [32][64][f2][f2], w3 [3][32][5][5].
static void pack_color(int f2, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, float *out)
{
    for (int ch = 0; ch < 3; ++ch)
        for (int l = 0; l < 64; ++l) {
            const int i = l & 31, kk = l >> 5;
            for (int t = 0; t < 2; ++t)
                for (int s = 0; s < 41; ++s) {
                    const int tap = 2 * s + kk, k = 32 * t + i;
                    out[((ch * 2 + t) * 41 + s) * 64 + l] = tap < 81 ? w1[(k * 3 + ch) * 81 + tap] : (ch == 2 ? b1[k] : 0.f);
                }
        }
    pack_spatial_l2(f2, w2, b2, out + color_l2_offset());
    for (int o = 0; o < 3; ++o) pack_l3z(w3 + o * 800, out + color_l3_offset(f2) + (size_t)o * SPATIAL_NFRAG_L3Z * 64);
}

// SRCNN_ERR_STATE unless a colour model is loaded and the mode has its arithmetic
static int refuse_color(srcnn_ctx *c)
{
    if (c->channels != 3)
        return fail(c, SRCNN_ERR_STATE, "srcnn_forward_color runs a colour model only: the context holds a 1-channel 9-%d-5 "
                                        "model (srcnn_set_model_color loads one)", c->f2);
    if (c->mode != SRCNN_MODE_MFMA)
        return fail(c, SRCNN_ERR_STATE, "a colour model runs in SRCNN_MODE_MFMA only (mode %d has no arithmetic for it)", c->mode);
    return SRCNN_OK;
}

// The bands of forward_spatial_impl (srcnn_spatial.cpp): rows [b0, b1) need layer-2 rows [b0 - 2, b1 + 2) and layer-1 rows
// [b0 - 2 - r2, b1 + 2 + r2), clamped to the image; the two maps of a band stay within kSpatialWorkBytes.  The input is read at
// src[y * src_stride + x * px_step + c * ch_step] (interleaved pixels, or three planes); dst (and pre) hold interleaved pixels.
static int forward_color_impl(srcnn_ctx *c, const uint8_t *src, size_t src_stride, int px_step, size_t ch_step,
                              size_t src_frame_pitch, uint8_t *dst, size_t dst_stride, size_t dst_frame_pitch, int width, int height,
                              int n_frames, float *pre)
{
    int rc;
    if ((rc = refuse_color(c))) return rc;
    const bool zero = c->padding == SRCNN_PAD_ZERO;
    const int r2 = (c->f2 - 1) / 2;
    const long row_bytes = 4L * width;
    const long cap = (long)(kSpatialWorkBytes / (size_t)row_bytes) - 64L * (4 + 2 * r2) - 32L * 4;
    const int band_max = (int)std::max(16L, cap / 96);
    const int n_bands = (height + band_max - 1) / band_max;
    const int band = (height + n_bands - 1) / n_bands;
    const long mrows = std::min<long>(height, band + 4 + 2 * r2), orows = std::min<long>(height, band + 4);
    const long mpitch = mrows * width, opitch = orows * width;
    if (bad_pitch((size_t)mpitch) || bad_pitch((size_t)opitch))
        return fail(c, SRCNN_ERR_INVALID, "forward_color_dev: plane too large for a colour 9-%d-5 model", c->f2);
    if ((rc = reserve(c, c->sp_map64, (size_t)64 * mpitch * sizeof(float)))) return rc;
    if ((rc = reserve(c, c->sp_map32, (size_t)32 * opitch * sizeof(float)))) return rc;
    if (!c->sp_done) HIP_TRY(c, hipEventCreateWithFlags(&c->sp_done, hipEventDisableTiming));
    // the maps were last used on another stream: wait for that work
    if (c->sp_stream && c->sp_stream != c->stream) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->sp_done, 0));
    const float *frag = static_cast<const float *>(c->col_frag.p);
    const float *frag2 = frag + color_l2_offset(), *bias2 = frag2 + (size_t)c->f2 * c->f2 * 2048, *frag3 = frag + color_l3_offset(c->f2);
    float *map64 = static_cast<float *>(c->sp_map64.p), *map32 = static_cast<float *>(c->sp_map32.p);
    for (int f = 0; f < n_frames; ++f) {
        const uint8_t *sf = src + (size_t)f * src_frame_pitch;
        for (int b0 = 0; b0 < height; b0 += band) {
            const int b1 = std::min(height, b0 + band);
            const int o0 = std::max(0, b0 - 2), o1 = std::min(height, b1 + 2);
            const int m0 = std::max(0, o0 - r2), m1 = std::min(height, o1 + r2);
            HIP_TRY(c, launch_color_l1(zero, sf, (long)src_stride, px_step, (long)ch_step, width, height, m0, m1, frag, map64, mpitch,
                                       c->stream));
            HIP_TRY(c, launch_spatial_l2(c->f2, zero, map64, mpitch, m0, m1, width, height, o0, o1, frag2, bias2, map32, opitch,
                                         c->stream));
            HIP_TRY(c, launch_color_l3(zero, map32, opitch, o0, o1, width, height, b0, b1, frag3, c->col_b3,
                                       dst + (size_t)f * dst_frame_pitch, (long)dst_stride,
                                       pre ? pre + (size_t)f * dst_frame_pitch : nullptr, c->stream));
        }
    }
    HIP_TRY(c, hipEventRecord(c->sp_done, c->stream));
    c->sp_stream = c->stream;
    return SRCNN_OK;
}

// srcnn_process_bgr(_dev) with a colour model: the three channels split into planes, each resized with the bicubic arithmetic
// of the 1-channel pipeline (resize_planes_dev), then the model on the three resized planes, written as interleaved pixels.
static int process_bgr_color_impl(srcnn_ctx *c, const uint8_t *d_bgr, size_t stride, int w, int h, int ow, int oh, uint8_t *d_out,
                                  size_t out_stride)
{
    const size_t lo = (size_t)w * h, hi = (size_t)ow * oh;
    int rc;
    if ((rc = reserve(c, c->ycc_lo, 3 * lo))) return rc;
    if ((rc = reserve(c, c->ycc_hi, 3 * hi))) return rc;
    uint8_t *planes_lo = static_cast<uint8_t *>(c->ycc_lo.p), *planes_hi = static_cast<uint8_t *>(c->ycc_hi.p);
    HIP_TRY(c, launch_split3(d_bgr, (long)stride, w, h, planes_lo, (long)lo, c->stream));
    if ((rc = resize_planes_dev(c, planes_lo, w, (long)lo, w, h, planes_hi, ow, (long)hi, ow, oh, 3))) return rc;
    return forward_color_impl(c, planes_hi, (size_t)ow, 1, hi, 0, d_out, out_stride, 0, ow, oh, 1, nullptr);
}

static const bool color_registered = (process_bgr_color = &process_bgr_color_impl, true);

}  // namespace host
}  // namespace srcnn

extern "C" {

int srcnn_set_model_color(srcnn_ctx *c, int f2, const float *k1, const float *b1, const float *k2, const float *b2,
                          const float *k3, const float *b3)
{
    BIND(c);
    int rc;
    if (!k1 || !b1 || !k2 || !b2 || !k3 || !b3) return fail(c, SRCNN_ERR_INVALID, "null weight table");
    if (f2 != 1 && f2 != 3 && f2 != 5) return fail(c, SRCNN_ERR_INVALID, "srcnn_set_model_color: f2 = %d (1, 3 or 5)", f2);
    std::vector<float> table(color_table_floats(f2));
    pack_color(f2, k1, b1, k2, b2, k3, table.data());
    // the 9-1-5 tables hold a zero model (and the has-model state): no gate lets them run while the colour model is loaded
    static const std::vector<float> zeros(5184, 0.f);
    c->f2 = 1;
    c->channels = 1;
    if ((rc = upload_weights(c, zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data(), 0.f))) return rc;
    c->has_l12 = c->has_l3 = true;
    if ((rc = reserve(c, c->col_frag, table.size() * sizeof(float)))) return rc;
    HIP_TRY(c, hipDeviceSynchronize());        // launches on any stream may still read the old table
    HIP_TRY(c, hipMemcpy(c->col_frag.p, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    std::memcpy(c->col_b3, b3, sizeof(c->col_b3));
    c->f2 = f2;
    c->channels = 3;
    c->whole_model = true;
    return SRCNN_OK;
}

int srcnn_get_model_channels(const srcnn_ctx *c) { return c ? c->channels : SRCNN_ERR_INVALID; }

int srcnn_forward_color_dev(srcnn_ctx *c, const uint8_t *d_src, size_t src_stride, size_t src_frame_pitch, uint8_t *d_dst,
                            size_t dst_stride, size_t dst_frame_pitch, int width, int height, int n_frames, float *d_preclamp)
{
    BIND(c);
    if (width <= 0 || height <= 0 || width > (1 << 28) || bad_plane(d_src, src_stride, 3 * width, height) ||
        bad_plane(d_dst, dst_stride, 3 * width, height) || n_frames <= 0)
        return fail(c, SRCNN_ERR_INVALID, "forward_color_dev: bad arguments");
    // every output pixel reads a window of input pixels that other workgroups may already have overwritten
    if (ranges_overlap(d_src, span_elems(src_stride, src_frame_pitch, 3 * width, height, n_frames), d_dst,
                       span_elems(dst_stride, dst_frame_pitch, 3 * width, height, n_frames)))
        return fail(c, SRCNN_ERR_INVALID, "forward_color_dev: src and dst overlap (the path cannot run in place)");
    return forward_color_impl(c, d_src, src_stride, 3, 1, src_frame_pitch, d_dst, dst_stride, dst_frame_pitch, width, height, n_frames,
                              d_preclamp);
}

int srcnn_forward_color(srcnn_ctx *c, const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int width, int height,
                        float *preclamp, size_t preclamp_stride)
{
    BIND(c);
    int rc;
    if (width <= 0 || height <= 0 || width > (1 << 28) || bad_plane(src, src_stride, 3 * width, height) ||
        bad_plane(dst, dst_stride, 3 * width, height) || (preclamp && preclamp_stride < 3 * (size_t)width))
        return fail(c, SRCNN_ERR_INVALID, "forward_color: bad arguments");
    if ((rc = refuse_color(c))) return rc;
    const size_t row = 3 * (size_t)width, n = row * height;
    if ((rc = reserve(c, c->in_u8, n))) return rc;
    if ((rc = reserve(c, c->out_u8, n))) return rc;
    if (preclamp && (rc = reserve(c, c->pre_f32, n * sizeof(float)))) return rc;
    uint8_t *d_in = static_cast<uint8_t *>(c->in_u8.p), *d_out = static_cast<uint8_t *>(c->out_u8.p);
    float *d_pre = preclamp ? static_cast<float *>(c->pre_f32.p) : nullptr;
    HIP_TRY(c, hipMemcpy2DAsync(d_in, row, src, src_stride, row, height, hipMemcpyHostToDevice, c->stream));
    if ((rc = forward_color_impl(c, d_in, row, 3, 1, n, d_out, row, n, width, height, 1, d_pre))) return rc;
    HIP_TRY(c, hipMemcpy2DAsync(dst, dst_stride, d_out, row, row, height, hipMemcpyDeviceToHost, c->stream));
    if (preclamp)
        HIP_TRY(c, hipMemcpy2DAsync(preclamp, preclamp_stride * sizeof(float), d_pre, row * sizeof(float), row * sizeof(float), height,
                                    hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SRCNN_OK;
}

}  // extern "C"
