// srcnn_spatial.cpp -- the banded path, layer 1 -> spatial layer 2 -> layer 3 per row band (srcnn_spatial_kernels.hip): the
// 9-3-5 / 9-5-5 models (srcnn_set_model, f2 = 3 or 5) behind srcnn_forward_y_dev, every model under zero padding
// (srcnn_set_padding), f2 = 1 included, and the colour models (srcnn_set_model_color: 3 input and 3 output channels, 9-f2-5)
// behind srcnn_forward_color(_dev) and srcnn_process_bgr(_dev); and the float image path, srcnn_forward_f32(_dev): every whole
// model on float32 planes, the value before truncation out.  One weight table per model, one gate, one band loop.
// Models of other widths (srcnn_set_model_shape: up to 128 / 64 filters, padded with zero channels to 64 or 128 and 32 or 64)
// load here too: one that fits 64 / 32 as an ordinary model, a wider one into the same table and band loop, where the launchers
// of layers 2 and 3 pick the forms for its widths.
#include "srcnn_ctx.h"

using namespace srcnn;
using namespace srcnn::host;

namespace srcnn {
namespace host {

// The fragment table of srcnn_kernels.h of a C-channel model of padded widths n1p (64 or 128) and n2p (32 or 64),
// spatial_table_floats(C, f2, n1p, n2p) floats: n1p / 64 layer-1 groups, n1p / 8 layer-2 chunks x n2p / 32 groups, n2p / 2
// layer-3 k-steps.  w1 [n1p][C][9][9], w2 [n2p][n1p][f2][f2], w3 [C][n2p][5][5] (PyTorch's conv weights, padded with zeros).
static void pack_spatial(int C, int f2, int n1p, int n2p, const float *w1, const float *b1, const float *w2, const float *b2,
                         const float *w3, float *out)
{
    for (int g = 0; g < n1p / 64; ++g)
        for (int ch = 0; ch < C; ++ch)
            for (int l = 0; l < 64; ++l) {
                const int i = l & 31, kk = l >> 5;
                for (int t = 0; t < 2; ++t)
                    for (int s = 0; s < 41; ++s) {
                        const int tap = 2 * s + kk, k = 64 * g + 32 * t + i;
                        out[(size_t)g * C * SPATIAL_NFRAG_L1 * 64 + ((ch * 2 + t) * 41 + s) * 64 + l] =
                            tap < 81 ? w1[((size_t)k * C + ch) * 81 + tap] : (ch == C - 1 ? b1[k] : 0.f);
                    }
            }
    const int taps = f2 * f2, chunks = n1p / 8;
    float *o2 = out + spatial_l2_offset(C, n1p);
    for (int g = 0; g < n2p / 32; ++g)
        for (int chunk = 0; chunk < chunks; ++chunk)
            for (int tap = 0; tap < taps; ++tap)
                for (int pp = 0; pp < 4; ++pp)
                    for (int l = 0; l < 64; ++l) {
                        const int k = 32 * g + (l & 31), ci = 8 * chunk + 2 * pp + (l >> 5);
                        o2[((((size_t)g * chunks + chunk) * taps + tap) * 4 + pp) * 64 + l] = w2[((size_t)k * n1p + ci) * taps + tap];
                    }
    std::memcpy(o2 + spatial_l2_floats(f2, n1p, n2p), b2, n2p * sizeof(float));
    float *o3 = out + spatial_l3_offset(C, f2, n1p, n2p);
    const int ksteps = n2p / 2;
    for (int o = 0; o < C; ++o)
        for (int s = 0; s < ksteps; ++s)
            for (int l = 0; l < 64; ++l) {
                const int tap = l3_row_tap(l & 31);
                o3[((size_t)o * ksteps + s) * 64 + l] = tap < 0 ? 0.f : w3[((size_t)o * n2p + 2 * s + (l >> 5)) * 25 + tap];
            }
}
// (the geometry of a 64 / 32 model, spelled out: the table the kernels with compile-time counts have always read)
static_assert(spatial_l2_offset(3) == 3 * 82 * 64 && spatial_l3_offset(3, 5) == spatial_l2_offset(3) + 25 * 2048 + 32 &&
              spatial_table_floats(3, 5) == spatial_l3_offset(3, 5) + 3 * 16 * 64 && spatial_table_floats(1, 1) == 82 * 64 + 2048 + 32 + 16 * 64,
              "a 64 / 32 model keeps its table");

// ---- SRCNN_MODE_BANDED16: exact power-of-two scales and the split W2 table (srcnn_spatial_kernels.hip, spatial_l2h_kernel) ----
// sum |w1[k]| and |b1[k]| of the n1p layer-1 channels (doubles), what the bound below is made from; false when one is not finite
static bool l1_magnitudes(int C, int n1p, const float *w1, const float *b1, double *sum, double *absb)
{
    bool finite = true;
    for (int k = 0; k < n1p; ++k) {
        sum[k] = 0.0;
        for (int i = 0; i < C * 81; ++i) sum[k] += std::fabs((double)w1[(size_t)k * C * 81 + i]);
        absb[k] = std::fabs((double)b1[k]);
        finite = finite && std::isfinite(sum[k]) && std::isfinite(absb[k]);
    }
    return finite;
}

// The largest value layer 1 can give for inputs of magnitude <= range: max over the n1p channels of range sum |w1[k]| + |b1[k]|
static double l1_bound(int n1p, const double *sum, const double *absb, double range)
{
    double bound = 0.0;
    for (int k = 0; k < n1p; ++k) bound = std::max(bound, range * sum[k] + absb[k]);
    return bound;
}

// ... for 8-bit input (range 255, what the byte entry points use), or the range of a float call (srcnn_set_input_range)
double banded16_l1_bound(int C, const float *w1, const float *b1, double range, int n1p)
{
    double sum[128], absb[128];
    if (n1p < 1 || n1p > 128 || !l1_magnitudes(C, n1p, w1, b1, sum, absb)) return HUGE_VAL;
    return l1_bound(n1p, sum, absb, range);
}

// e with bound * 2^e in [2^14, 2^15) (0 for a bound of 0); false when the bound is not finite
bool banded16_exponent(double bound, int *e)
{
    *e = 0;
    if (!std::isfinite(bound)) return false;
    if (bound > 0.0) {
        int x;
        (void)std::frexp(bound, &x);           // bound = m 2^x, m in [0.5, 1)
        *e = 15 - x;
    }
    return true;
}

// W2 [n2p][n1p][f2][f2] times 2^e2 (max |W2| 2^e2 in [2^14, 2^15)) as f16 (hi, lo) pairs, round to nearest, in the A-operand
// order of spatial_l2h_kernel (srcnn_kernels.h: n2p / 32 groups x n1p / 16 K steps; 64 / 32 is the one group of 4 steps of
// SRCNN_MODE_BANDED16); false when a weight is not finite or the scaled weights leave float32's range
bool banded16_pack_w2(int f2, const float *w2, uint16_t *table, int *e2, int n1p, int n2p)
{
    const int taps = f2 * f2, steps = n1p / 16;
    double wmax = 0.0;
    for (size_t i = 0; i < (size_t)n2p * n1p * taps; ++i) {
        if (!std::isfinite(w2[i])) return false;
        wmax = std::max(wmax, std::fabs((double)w2[i]));
    }
    if (!banded16_exponent(wmax, e2) || std::abs(*e2) > 120) return false;
    const float scale = std::ldexp(1.f, *e2);
    for (int g = 0; g < n2p / 32; ++g)
        for (int s = 0; s < steps; ++s)
            for (int tap = 0; tap < taps; ++tap)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 8; ++e) {
                        const int k = 32 * g + (l & 31), ci = 64 * (s >> 2) + spatial_l2h_channel(s & 3, l >> 5, e);
                        uint16_t *hi = table + (((((size_t)g * steps + s) * taps + tap) * 2) * 64 + l) * 8 + e;
                        split16(w2[((size_t)k * n1p + ci) * taps + tap], scale, hi, hi + 64 * 8);
                    }
    return true;
}

// The table and b3 of a C-channel 9-f2-5 model into sp_table / sp_b3 (pack_spatial's arguments).  A wide model (n1p = 128 or
// n2p = 64) keeps what the split needs too, for srcnn_set_wide_split16 (SRCNN_MODE_BANDED16 refuses it).
static int upload_table(srcnn_ctx *c, int C, int f2, const float *w1, const float *b1, const float *w2, const float *b2,
                        const float *w3, const float *b3, int n1p = 64, int n2p = 32)
{
    std::vector<float> table(spatial_table_floats(C, f2, n1p, n2p));
    pack_spatial(C, f2, n1p, n2p, w1, b1, w2, b2, w3, table.data());
    int rc;
    if ((rc = reserve(c, c->sp_table, table.size() * sizeof(float)))) return rc;
    HIP_TRY(c, hipDeviceSynchronize());        // launches on any stream may still read the old table
    HIP_TRY(c, hipMemcpy(c->sp_table.p, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    std::memcpy(c->sp_b3, b3, C * sizeof(float));
    c->sp_f2 = f2;
    // what SRCNN_MODE_BANDED16 (a wide model: srcnn_set_wide_split16) makes its table and scales from, when a call first runs the
    // model that way
    c->sp_w2.assign(w2, w2 + (size_t)n2p * n1p * f2 * f2);
    c->sp_l1_bound = l1_magnitudes(C, n1p, w1, b1, c->sp_l1_sum, c->sp_l1_absb) ? l1_bound(n1p, c->sp_l1_sum, c->sp_l1_absb, 255.0) : HUGE_VAL;
    c->sp16_f2 = 0;
    return SRCNN_OK;
}

// What refuses a model the split cannot scale: the mode, or for a wide model the option
static const char *split_name(const srcnn_ctx *c) { return wide_model(c) ? "srcnn_set_wide_split16" : "SRCNN_MODE_BANDED16"; }
static const char *split_way_out(const srcnn_ctx *c) { return wide_model(c) ? "switch the option off" : "use SRCNN_MODE_MFMA"; }

// The split W2 table and the scales of SRCNN_MODE_BANDED16 (a wide model: of srcnn_set_wide_split16, for its n1p / n2p) for the
// model in sp_table, made once per loaded model
static int upload_table16(srcnn_ctx *c)
{
    if (c->sp16_f2 == c->sp_f2) return SRCNN_OK;
    const char *const refuse = "%s cannot scale this model into f16 (a weight or bias of layers 1-2 is not finite, "
                               "or their magnitudes are beyond float32's exponent range); %s";
    if (c->sp16_f2 < 0) return fail(c, SRCNN_ERR_STATE, refuse, split_name(c), split_way_out(c));
    const int f2 = c->sp_f2, n1p = c->n1p, n2p = c->n2p;
    int e1 = 0, e2 = 0;
    std::vector<uint16_t> table(spatial_l2h_table_bytes(f2, n1p, n2p) / sizeof(uint16_t));
    if (c->sp_w2.size() != (size_t)n2p * n1p * f2 * f2 || !banded16_exponent(c->sp_l1_bound, &e1) ||
        !banded16_pack_w2(f2, c->sp_w2.data(), table.data(), &e2, n1p, n2p) || std::abs(e1 + e2) > 120) {
        c->sp16_f2 = -1;
        return fail(c, SRCNN_ERR_STATE, refuse, split_name(c), split_way_out(c));
    }
    int rc;
    if ((rc = reserve(c, c->sp16_table, table.size() * sizeof(uint16_t)))) return rc;
    HIP_TRY(c, hipDeviceSynchronize());        // launches on any stream may still read the old table
    HIP_TRY(c, hipMemcpy(c->sp16_table.p, table.data(), table.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    c->sp16_scale1 = std::ldexp(1.f, e1);
    c->sp16_unscale = std::ldexp(1.f, -(e1 + e2));
    c->sp16_e2 = e2;
    c->sp16_f2 = f2;
    return SRCNN_OK;
}

// The one gate of the banded path: SRCNN_OK when it may run the loaded model in the current mode and padding, else
// SRCNN_ERR_STATE with a message that names what blocks the call.  f32: a call of the float image path (srcnn_forward_f32*),
// which runs every whole model in SRCNN_MODE_MFMA and SRCNN_MODE_BANDED16 and nothing else.  rows: a call of the stripe entry
// points (srcnn_model_rows*_dev, srcnn_model_striped* and their colour and float forms), which run the whole models
static int banded_refusal(srcnn_ctx *c, bool f32 = false, bool rows = false)
{
    const bool zero = c->padding == SRCNN_PAD_ZERO;
    if (wide_model(c) && (c->mode != SRCNN_MODE_MFMA || rows))      // before the other gates: the message names the widths
        return fail(c, SRCNN_ERR_STATE, "a model of %d / %d filters (srcnn_set_model_shape; padded to %d / %d) runs whole images in "
                                        "SRCNN_MODE_MFMA only: %s", c->n1, c->n2, c->n1p, c->n2p,
                    rows ? "row stripes and several GPUs are not built for it" : "this mode has no arithmetic for it");
    if (f32) {
        if (c->mode != SRCNN_MODE_MFMA && c->mode != SRCNN_MODE_BANDED16)
            return fail(c, SRCNN_ERR_STATE, "srcnn_forward_f32 runs in SRCNN_MODE_MFMA and SRCNN_MODE_BANDED16 only (mode %d has no "
                                            "float image path)", c->mode);
        if (!c->whole_model)
            return fail(c, SRCNN_ERR_STATE, "srcnn_forward_f32 needs a model loaded by srcnn_set_weights / srcnn_set_model(_color): "
                                            "the loaded layers came from per-filter calls");
    }
    if (c->mode == SRCNN_MODE_BANDED16) {      // every whole model, in either padding
        if (!c->whole_model)
            return fail(c, SRCNN_ERR_STATE, "SRCNN_MODE_BANDED16 needs a model loaded by srcnn_set_weights / srcnn_set_model(_color): "
                                            "the loaded layers came from per-filter calls");
        return SRCNN_OK;
    }
    if (c->mode != SRCNN_MODE_MFMA && c->channels != 1)
        return fail(c, SRCNN_ERR_STATE, "a colour model runs in SRCNN_MODE_MFMA only (mode %d has no arithmetic for it)", c->mode);
    if (c->mode != SRCNN_MODE_MFMA && zero)
        return fail(c, SRCNN_ERR_STATE, "SRCNN_PAD_ZERO (srcnn_set_padding) runs in SRCNN_MODE_MFMA only (mode %d has replicate "
                                        "padding only)", c->mode);
    if (c->mode != SRCNN_MODE_MFMA)
        return fail(c, SRCNN_ERR_STATE, "a 9-%d-5 model runs in SRCNN_MODE_MFMA only (mode %d has no arithmetic for a spatial "
                                        "layer 2)", c->f2, c->mode);
    if (zero && !c->whole_model)
        return fail(c, SRCNN_ERR_STATE, "SRCNN_PAD_ZERO needs a model loaded by srcnn_set_weights / srcnn_set_model: the loaded "
                                        "layers came from per-filter calls");
    return SRCNN_OK;
}

// The stripe entry points (srcnn_model_rows*_dev, srcnn_model_striped*) run the whole 1-channel models: on the banded path behind
// banded_refusal(), or, where the strip path runs the model, through that path's stripe calls, which gate themselves
int model_rows_refusal(srcnn_ctx *c, StripeKind kind)
{
    // float planes: every whole model, as srcnn_forward_f32 (whose gate names the mode or the per-filter layers)
    if (kind == STRIPE_F32) return banded_refusal(c, true, true);
    if (kind == STRIPE_COLOR) {
        if (c->channels != 3)
            return fail(c, SRCNN_ERR_STATE, "srcnn_model_color_rows / srcnn_model_color_striped run a colour model only: the context "
                                            "holds a 1-channel 9-%d-5 model (srcnn_set_model_color loads one)", c->f2);
        return banded_refusal(c, false, true);
    }
    if (c->channels != 1)
        return fail(c, SRCNN_ERR_STATE, "srcnn_model_rows / srcnn_model_striped: the context holds a colour model (3 channels, "
                                        "9-%d-5); row stripes run the 1-channel models only", c->f2);
    if (!c->whole_model)
        return fail(c, SRCNN_ERR_STATE, "srcnn_model_rows / srcnn_model_striped need a model loaded by srcnn_set_weights / "
                                        "srcnn_set_model: the loaded layers came from per-filter calls");
    return luma_path_ok(c) ? SRCNN_OK : banded_refusal(c, false, true);
}

// the colour entry points run a colour model only
static int refuse_luma_model(srcnn_ctx *c)
{
    if (c->channels == 3) return SRCNN_OK;
    return fail(c, SRCNN_ERR_STATE, "srcnn_forward_color runs a colour model only: the context holds a 1-channel 9-%d-5 model "
                                    "(srcnn_set_model_color loads one)", c->f2);
}

// Rows [b0, b1) of a plane need layer-2 rows [b0 - 2, b1 + 2) and layer-1 rows [b0 - 2 - r2, b1 + 2 + r2), clamped to the
// image: a band recomputes the 2 + r2 layer-1 rows and 2 layer-2 rows either side it shares with its neighbours.  Bands are
// as tall as kSpatialWorkBytes allows for the two maps (256 + 128 B per pixel of a row).
// A stripe call (io.rows) runs the same loop inside [row_begin, row_end): o0 / o1 / m0 / m1 are clamped to the IMAGE, so the
// first and last band of a stripe compute the map rows beyond it that a whole-image call's neighbouring band would, from input
// rows the caller provides (layer 1 reads [m0 - 4, m1 + 4), i.e. no further than R = 6 + r2 rows from the stripe).
int forward_banded(srcnn_ctx *c, const uint8_t *src, size_t src_stride, int px_step, size_t ch_step, size_t src_frame_pitch,
                   uint8_t *dst, size_t dst_stride, size_t dst_frame_pitch, int width, int height, int n_frames, float *pre)
{
    BandedPlanes io;
    io.src = src;
    io.src_stride = src_stride;
    io.px_step = px_step;
    io.ch_step = ch_step;
    io.src_frame_pitch = src_frame_pitch;
    io.dst = dst;
    io.dst_stride = dst_stride;
    io.dst_frame_pitch = dst_frame_pitch;
    io.pre = pre;
    return forward_banded(c, io, width, height, n_frames);
}

int forward_banded(srcnn_ctx *c, const BandedPlanes &io, int width, int height, int n_frames)
{
    int rc;
    if ((rc = banded_refusal(c, io.f32, io.rows))) return rc;
    // (only a 9-1-5 model gets here unpacked: the others pack when they load)
    if (c->sp_f2 != c->f2 && !wide_model(c)) {
        const float *hr = c->host_raw.data();
        if ((rc = upload_table(c, 1, 1, hr + 64, hr, hr + 5280, hr + 5248, hr + 7329, hr + 7328))) return rc;
    }
    // (n1p / n2p = 64 / 32 but for a model of srcnn_set_model_shape: 4 (n1p + n2p) bytes per pixel of a row)
    const int n1p = c->n1p, n2p = c->n2p;
    const bool wide = wide_model(c);
    // layer 2 in split f16: the mode, or for a wide model (which the gate lets run in SRCNN_MODE_MFMA only) the option
    const bool split = wide ? c->wide_split16 != 0 : c->mode == SRCNN_MODE_BANDED16;
    if (split && (rc = upload_table16(c))) return rc;
    // a float call scales the layer-1 map by the bound for inputs up to input_range, not 255: the same W2 table, other scales
    float scale1 = c->sp16_scale1, unscale = c->sp16_unscale;
    if (split && io.f32) {
        int e1 = 0;
        if (!banded16_exponent(l1_bound(n1p, c->sp_l1_sum, c->sp_l1_absb, (double)c->input_range), &e1) || std::abs(e1 + c->sp16_e2) > 120)
            return fail(c, SRCNN_ERR_STATE, "%s cannot scale this model into f16 for inputs up to %g "
                                            "(srcnn_set_input_range); %s", split_name(c), (double)c->input_range, split_way_out(c));
        scale1 = std::ldexp(1.f, e1);
        unscale = std::ldexp(1.f, -(e1 + c->sp16_e2));
    }
    const int C = c->channels, r2 = (c->f2 - 1) / 2;
    const bool zero = c->padding == SRCNN_PAD_ZERO;
    const long row_bytes = 4L * width;
    const long cap = (long)(kSpatialWorkBytes / (size_t)row_bytes) - (long)n1p * (4 + 2 * r2) - (long)n2p * 4;
    const int band_max = (int)std::max(16L, cap / (n1p + n2p));
    const int row_begin = io.rows ? io.row_begin : 0, row_end = io.rows ? io.row_end : height;
    const int n_bands = (row_end - row_begin + band_max - 1) / band_max;
    const int band = (row_end - row_begin + n_bands - 1) / n_bands;
    const long mrows = std::min<long>(height, band + 4 + 2 * r2), orows = std::min<long>(height, band + 4);
    const long mpitch = mrows * width, opitch = orows * width;
    if (bad_pitch((size_t)mpitch) || bad_pitch((size_t)opitch))
        return fail(c, SRCNN_ERR_INVALID, "%s: plane too large for a %s9-%d-5 model",
                    io.rows ? (io.f32 ? "model_rows_f32_dev" : C == 1 ? "model_rows_dev" : "model_color_rows_dev")
                            : io.f32 ? "forward_f32_dev" : C == 1 ? "forward_y_dev" : "forward_color_dev",
                    C == 1 ? "" : "colour ", c->f2);
    if ((rc = reserve(c, c->sp_map64, (size_t)n1p * mpitch * sizeof(float)))) return rc;
    if ((rc = reserve(c, c->sp_map32, (size_t)n2p * opitch * sizeof(float)))) return rc;
    if (!c->sp_done) HIP_TRY(c, hipEventCreateWithFlags(&c->sp_done, hipEventDisableTiming));
    // the maps were last used on another stream (the two lanes of srcnn_forward_y_frames): wait for that work
    if (c->sp_stream && c->sp_stream != c->stream) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->sp_done, 0));
    const float *frag = static_cast<const float *>(c->sp_table.p);
    const float *frag2 = frag + spatial_l2_offset(C, n1p), *bias2 = frag2 + spatial_l2_floats(c->f2, n1p, n2p);
    const float *frag3 = frag + spatial_l3_offset(C, c->f2, n1p, n2p);
    float *map64 = static_cast<float *>(c->sp_map64.p), *map32 = static_cast<float *>(c->sp_map32.p);
    const size_t dst_stride = io.dst_stride;
    // where layer 1 reads the image (a stripe: the image's rows in src and the halo buffers) and what layer 3 writes (a stripe:
    // dst / pre addressed by image row from dst_row0); src, dst and pre are set per frame
    L1Input in{nullptr, io.f32, C, (long)io.src_stride, io.px_step, (long)io.ch_step, io.rows, io.halo_top, io.halo_bot,
               (long)io.halo_stride, (long)io.halo_ch_pitch, io.src_row0, io.src_row0 + io.src_rows, kHaloRows + r2};
    L3Output out{nullptr, io.f32, (long)dst_stride, (long)io.dst_ch_pitch, nullptr};
    const long dst_off = io.rows ? (long)io.dst_row0 * (long)dst_stride : 0;
    const size_t es = io.f32 ? sizeof(float) : 1;      // bytes per element of the call's planes
    for (int f = 0; f < n_frames; ++f) {
        // frame f of the call's planes: bytes, or floats (the float image path, which has no pre)
        in.src = static_cast<const uint8_t *>(io.src) + es * f * io.src_frame_pitch;
        uint8_t *df = static_cast<uint8_t *>(io.dst) + es * f * io.dst_frame_pitch;
        float *pf = io.pre && !io.f32 ? io.pre + (size_t)f * io.dst_frame_pitch : nullptr;
        out.dst = df - (long)es * dst_off;
        out.pre = pf ? pf - dst_off : nullptr;
        for (int b0 = row_begin; b0 < row_end; b0 += band) {
            const int b1 = std::min(row_end, b0 + band);
            const int o0 = std::max(0, b0 - 2), o1 = std::min(height, b1 + 2);
            const int m0 = std::max(0, o0 - r2), m1 = std::min(height, o1 + r2);
            // layer 1 group by group (64 output channels each: its own table, its own planes of the map; one group but for a
            // wide model); split: each group's 64 planes, the same bytes, as 8 planes of f16 (hi, lo) pixels, all with the model's
            // one scale, and layer 2 on the f16 MFMA
            for (int g = 0; g < n1p / 64; ++g)
                HIP_TRY(c, launch_spatial_l1(in, zero, split, scale1, width, height, m0, m1, frag + (size_t)g * C * SPATIAL_NFRAG_L1 * 64,
                                             map64 + (size_t)g * 64 * mpitch, mpitch, c->stream));
            HIP_TRY(c, launch_spatial_l2(c->f2, zero, split, map64, mpitch, m0, m1, width, height, o0, o1,
                                         split ? c->sp16_table.p : (const void *)frag2, bias2, unscale, map32, opitch, n1p, n2p, c->stream));
            // float planes out, the 1-channel replicate model included (MODE_L3 has no float form), and every form from 64 maps
            // (MODE_L3 reads 32)
            if (io.f32 || C > 1 || zero || n2p > 32) {
                HIP_TRY(c, launch_spatial_l3(C, zero, map32, opitch, o0, o1, width, height, b0, b1, frag3, c->sp_b3, out, n2p, c->stream));
                continue;
            }
            StripParams q{};
            q.planes_in = map32 - (long)o0 * width;          // MODE_L3 addresses image rows; the band map starts at row o0
            q.pl_stride = width;
            q.pl_pitch = opitch;
            q.dst = df;
            q.pre = pf;
            q.dst_stride = (long)dst_stride;
            q.dst_row0 = io.rows ? io.dst_row0 : 0;
            q.width = width;
            q.height = height;
            q.row_begin = b0;
            q.row_end = b1;
            if ((rc = run_strip(c, MODE_L3, q, 1))) return rc;
        }
    }
    HIP_TRY(c, hipEventRecord(c->sp_done, c->stream));
    c->sp_stream = c->stream;
    return SRCNN_OK;
}

// the float planes of a call: elements spanned from the first, and whether the planes the call WRITES are disjoint (frames of
// channels, or channels of frames)
size_t f32_span(int C, size_t stride, size_t ch_pitch, size_t frame_pitch, int width, int height, int n_frames)
{
    return (size_t)(n_frames - 1) * frame_pitch + (size_t)(C - 1) * ch_pitch + (size_t)(height - 1) * stride + (size_t)width;
}
bool f32_planes_disjoint(int C, size_t stride, size_t ch_pitch, size_t frame_pitch, int width, int height, int n_frames)
{
    const size_t plane = (size_t)(height - 1) * stride + (size_t)width;
    if (C == 1) return n_frames == 1 || frame_pitch >= plane;
    if (n_frames == 1) return ch_pitch >= plane;
    return (ch_pitch >= plane && frame_pitch >= (size_t)(C - 1) * ch_pitch + plane) ||
           (frame_pitch >= plane && ch_pitch >= (size_t)(n_frames - 1) * frame_pitch + plane);
}

// the gate of the float image path for the callers outside this file (srcnn_process_f32*)
int forward_f32_refusal(srcnn_ctx *c) { return banded_refusal(c, true); }

}  // namespace host
}  // namespace srcnn

extern "C" {

int srcnn_set_model(srcnn_ctx *c, int f2, const float *k99, const float *b99, const float *k2, const float *b2, const float *k55,
                    float b55)
{
    if (f2 == 1) return srcnn_set_weights(c, k99, b99, k2, b2, k55, b55);      // the 9-1-5 path, bit for bit
    BIND(c);
    int rc;
    if (!k99 || !b99 || !k2 || !b2 || !k55) return fail(c, SRCNN_ERR_INVALID, "null weight table");
    if (f2 != 3 && f2 != 5) return fail(c, SRCNN_ERR_INVALID, "srcnn_set_model: f2 = %d (1, 3 or 5)", f2);
    // layer 3 (and the has-model state) through the 9-1-5 tables, with a zero 1x1 layer 2 that nothing of this model reads
    static const std::vector<float> zero_w2(2048, 0.f);
    c->f2 = 1;
    c->channels = 1;
    if ((rc = upload_weights(c, k99, b99, zero_w2.data(), b2, k55, b55))) return rc;
    c->has_l12 = c->has_l3 = true;
    if ((rc = upload_table(c, 1, f2, k99, b99, k2, b2, k55, &b55))) return rc;
    c->f2 = f2;
    c->whole_model = true;
    return SRCNN_OK;
}

int srcnn_set_model_color(srcnn_ctx *c, int f2, const float *k1, const float *b1, const float *k2, const float *b2,
                          const float *k3, const float *b3)
{
    BIND(c);
    int rc;
    if (!k1 || !b1 || !k2 || !b2 || !k3 || !b3) return fail(c, SRCNN_ERR_INVALID, "null weight table");
    if (f2 != 1 && f2 != 3 && f2 != 5) return fail(c, SRCNN_ERR_INVALID, "srcnn_set_model_color: f2 = %d (1, 3 or 5)", f2);
    // the 9-1-5 tables hold a zero model (and the has-model state): no gate lets them run while the colour model is loaded
    static const std::vector<float> zeros(5184, 0.f);
    c->f2 = 1;
    c->channels = 1;
    if ((rc = upload_weights(c, zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data(), 0.f))) return rc;
    c->has_l12 = c->has_l3 = true;
    if ((rc = upload_table(c, 3, f2, k1, b1, k2, b2, k3, b3))) return rc;
    c->f2 = f2;
    c->channels = 3;
    c->whole_model = true;
    return SRCNN_OK;
}

int srcnn_set_model_shape(srcnn_ctx *c, int channels, int n1, int f2, int n2, const float *k1, const float *b1, const float *k2,
                          const float *b2, const float *k3, const float *b3)
{
    BIND(c);
    int rc;
    if (!k1 || !b1 || !k2 || !b2 || !k3 || !b3) return fail(c, SRCNN_ERR_INVALID, "null weight table");
    if ((channels != 1 && channels != 3) || (f2 != 1 && f2 != 3 && f2 != 5) || n1 < 1 || n1 > 128 || n2 < 1 || n2 > 64)
        return fail(c, SRCNN_ERR_INVALID, "srcnn_set_model_shape: %d channel(s), n1 = %d, f2 = %d, n2 = %d (channels 1 or 3, "
                                          "1 <= n1 <= 128, f2 = 1, 3 or 5, 1 <= n2 <= 64)", channels, n1, f2, n2);
    const int C = channels, taps = f2 * f2, n1p = 64 * ((n1 + 63) / 64), n2p = 32 * ((n2 + 31) / 32);
    // the padded tensors: zero weights and zero biases for the channels beyond n1 / n2
    std::vector<float> w1((size_t)n1p * C * 81, 0.f), pb1((size_t)n1p, 0.f), w2((size_t)n2p * n1p * taps, 0.f), pb2((size_t)n2p, 0.f),
        w3((size_t)C * n2p * 25, 0.f);
    std::memcpy(w1.data(), k1, (size_t)n1 * C * 81 * sizeof(float));
    std::memcpy(pb1.data(), b1, (size_t)n1 * sizeof(float));
    for (int k = 0; k < n2; ++k)
        std::memcpy(w2.data() + (size_t)k * n1p * taps, k2 + (size_t)k * n1 * taps, (size_t)n1 * taps * sizeof(float));
    std::memcpy(pb2.data(), b2, (size_t)n2 * sizeof(float));
    for (int o = 0; o < C; ++o) std::memcpy(w3.data() + (size_t)o * n2p * 25, k3 + (size_t)o * n2 * 25, (size_t)n2 * 25 * sizeof(float));
    if (n1p == 64 && n2p == 32) {      // a narrow model is an ordinary model: every mode and entry point that runs one runs it
        rc = C == 3 ? srcnn_set_model_color(c, f2, w1.data(), pb1.data(), w2.data(), pb2.data(), w3.data(), b3)
                    : srcnn_set_model(c, f2, w1.data(), pb1.data(), w2.data(), pb2.data(), w3.data(), b3[0]);
        if (rc) return rc;
        c->n1 = n1;
        c->n2 = n2;
        return SRCNN_OK;
    }
    // A wide model lives in sp_table.  The 9-1-5 tables hold a zero model (and the has-model state) that no gate lets run -- but
    // for layer 3 of a 1-channel model with n2p = 32, which MODE_L3 runs from them under replicate padding (as srcnn_set_model).
    static const std::vector<float> zeros(5184, 0.f);
    const bool l3_strip = C == 1 && n2p == 32;
    c->f2 = 1;
    c->channels = 1;
    if ((rc = upload_weights(c, zeros.data(), zeros.data(), zeros.data(), zeros.data(), l3_strip ? w3.data() : zeros.data(),
                             l3_strip ? b3[0] : 0.f)))
        return rc;
    c->has_l12 = c->has_l3 = true;
    if ((rc = upload_table(c, C, f2, w1.data(), pb1.data(), w2.data(), pb2.data(), w3.data(), b3, n1p, n2p))) return rc;
    c->f2 = f2;
    c->channels = C;
    c->whole_model = true;
    c->n1 = n1;
    c->n2 = n2;
    c->n1p = n1p;
    c->n2p = n2p;
    return SRCNN_OK;
}

int srcnn_get_model_shape(const srcnn_ctx *c, int *channels, int *n1, int *f2, int *n2)
{
    if (!c) return SRCNN_ERR_INVALID;
    if (channels) *channels = c->channels;
    if (n1) *n1 = c->n1;
    if (f2) *f2 = c->f2;
    if (n2) *n2 = c->n2;
    return SRCNN_OK;
}

int srcnn_set_wide_split16(srcnn_ctx *c, int on)
{
    if (!c) return SRCNN_ERR_INVALID;
    if (on != 0 && on != 1) return fail(c, SRCNN_ERR_INVALID, "srcnn_set_wide_split16: %d (0: layer 2 of a wide model in float32, 1: in split f16)", on);
    c->wide_split16 = on;      // read when a call launches, like the padding; a model that cannot be scaled is refused there
    return SRCNN_OK;
}

int srcnn_get_wide_split16(const srcnn_ctx *c) { return c ? c->wide_split16 : SRCNN_ERR_INVALID; }

#ifdef SRCNN_TUNING_BUILD
/* Undocumented test hook (not part of the ABI, needs no device): the host side of srcnn_set_wide_split16 for a model of `channels`
 * channels padded to n1p (64 or 128) / n2p (32 or 64) filters: w1 [n1p][channels][9][9], b1 [n1p], w2 [n2p][n1p][f2][f2], `range`
 * the largest |input| (255 for the byte entry points).  table: spatial_l2h_table_bytes(f2, n1p, n2p) bytes or null; exps: {e1, e2}.
 * Returns the table's size in bytes, or SRCNN_ERR_STATE for a model the option refuses. */
int srcnn_debug_wide16_tables(int channels, int n1p, int n2p, int f2, const float *w1, const float *b1, const float *w2, float range,
                              uint16_t *table, int *exps)
{
    if ((channels != 1 && channels != 3) || (n1p != 64 && n1p != 128) || (n2p != 32 && n2p != 64) || (f2 != 1 && f2 != 3 && f2 != 5) ||
        !w1 || !b1 || !w2 || !exps || !std::isfinite(range) || !(range > 0.f))
        return SRCNN_ERR_INVALID;
    std::vector<uint16_t> own;
    if (!table) {
        own.resize(spatial_l2h_table_bytes(f2, n1p, n2p) / sizeof(uint16_t));
        table = own.data();
    }
    if (!banded16_exponent(banded16_l1_bound(channels, w1, b1, (double)range, n1p), &exps[0]) ||
        !banded16_pack_w2(f2, w2, table, &exps[1], n1p, n2p) || std::abs(exps[0] + exps[1]) > 120)
        return SRCNN_ERR_STATE;
    return (int)spatial_l2h_table_bytes(f2, n1p, n2p);
}

/* ... and the dynamic LDS the launcher of spatial_l2h_kernel asks for (spatial_l2h_lds_bytes; the kernel asserts it is its layout's). */
int srcnn_debug_wide16_lds_bytes(int f2) { return (f2 != 1 && f2 != 3 && f2 != 5) ? SRCNN_ERR_INVALID : (int)spatial_l2h_lds_bytes(f2); }

/* Undocumented test hooks (not part of the ABI, need no device): the host side of SRCNN_MODE_BANDED16 for a model of `channels`
 * channels, the 64 / 32 case of srcnn_debug_wide16_tables.  table: spatial_l2h_table_bytes(f2) bytes or null; exps: {e1, e2}, the
 * exponents of the layer-1 map's and W2's scales.  Returns the table's size in bytes, or SRCNN_ERR_STATE for a model the mode
 * refuses.  _range: for a float call with srcnn_set_input_range(range): e1 follows the range, the table and e2 do not. */
int srcnn_debug_banded16_tables_range(int channels, int f2, const float *w1, const float *b1, const float *w2, float range,
                                      uint16_t *table, int *exps)
{
    return srcnn_debug_wide16_tables(channels, 64, 32, f2, w1, b1, w2, range, table, exps);
}
int srcnn_debug_banded16_tables(int channels, int f2, const float *w1, const float *b1, const float *w2, uint16_t *table, int *exps)
{
    return srcnn_debug_banded16_tables_range(channels, f2, w1, b1, w2, 255.f, table, exps);
}

/* srcnn_set_input_range on a context that is bound to no device (the call touches none): its return code, and in *after the
 * setting the context then holds. */
int srcnn_debug_set_input_range(float r, float *after)
{
    srcnn_ctx ctx;
    const int rc = srcnn_set_input_range(&ctx, r);
    if (after) *after = srcnn_get_input_range(&ctx);
    return rc;
}
#endif

int srcnn_get_model_f2(const srcnn_ctx *c) { return c ? c->f2 : SRCNN_ERR_INVALID; }

int srcnn_get_model_channels(const srcnn_ctx *c) { return c ? c->channels : SRCNN_ERR_INVALID; }

int srcnn_set_padding(srcnn_ctx *c, int padding)
{
    if (!c) return SRCNN_ERR_INVALID;
    if (padding != SRCNN_PAD_REPLICATE && padding != SRCNN_PAD_ZERO)
        return fail(c, SRCNN_ERR_INVALID, "srcnn_set_padding: %d (SRCNN_PAD_REPLICATE = 0 or SRCNN_PAD_ZERO = 1)", padding);
    c->padding = padding;      // read when a call launches: work already queued keeps the padding it was queued with
    return SRCNN_OK;
}

int srcnn_get_padding(const srcnn_ctx *c) { return c ? c->padding : SRCNN_ERR_INVALID; }

int srcnn_forward_color_dev(srcnn_ctx *c, const uint8_t *d_src, size_t src_stride, size_t src_frame_pitch, uint8_t *d_dst,
                            size_t dst_stride, size_t dst_frame_pitch, int width, int height, int n_frames, float *d_preclamp)
{
    BIND(c);
    int rc;
    if (width <= 0 || height <= 0 || width > (1 << 28) || bad_plane(d_src, src_stride, 3 * width, height) ||
        bad_plane(d_dst, dst_stride, 3 * width, height) || n_frames <= 0)
        return fail(c, SRCNN_ERR_INVALID, "forward_color_dev: bad arguments");
    // every output pixel reads a window of input pixels that other workgroups may already have overwritten
    if (ranges_overlap(d_src, span_elems(src_stride, src_frame_pitch, 3 * width, height, n_frames), d_dst,
                       span_elems(dst_stride, dst_frame_pitch, 3 * width, height, n_frames)))
        return fail(c, SRCNN_ERR_INVALID, "forward_color_dev: src and dst overlap (the path cannot run in place)");
    if ((rc = refuse_luma_model(c))) return rc;
    return forward_banded(c, d_src, src_stride, 3, 1, src_frame_pitch, d_dst, dst_stride, dst_frame_pitch, width, height, n_frames,
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
    if ((rc = refuse_luma_model(c)) || (rc = banded_refusal(c))) return rc;     // before anything is staged
    const size_t row = 3 * (size_t)width, n = row * height;
    if ((rc = reserve(c, c->in_u8, n))) return rc;
    if ((rc = reserve(c, c->out_u8, n))) return rc;
    if (preclamp && (rc = reserve(c, c->pre_f32, n * sizeof(float)))) return rc;
    uint8_t *d_in = static_cast<uint8_t *>(c->in_u8.p), *d_out = static_cast<uint8_t *>(c->out_u8.p);
    float *d_pre = preclamp ? static_cast<float *>(c->pre_f32.p) : nullptr;
    HIP_TRY(c, hipMemcpy2DAsync(d_in, row, src, src_stride, row, height, hipMemcpyHostToDevice, c->stream));
    if ((rc = forward_banded(c, d_in, row, 3, 1, n, d_out, row, n, width, height, 1, d_pre))) return rc;
    HIP_TRY(c, hipMemcpy2DAsync(dst, dst_stride, d_out, row, row, height, hipMemcpyDeviceToHost, c->stream));
    if (preclamp)
        HIP_TRY(c, hipMemcpy2DAsync(preclamp, preclamp_stride * sizeof(float), d_pre, row * sizeof(float), row * sizeof(float), height,
                                    hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SRCNN_OK;
}

/* ---- row stripes of every whole model (include/srcnn_amd.h) ---- */

int srcnn_model_halo_rows(const srcnn_ctx *c) { return c ? kHaloRows + (c->f2 - 1) / 2 : SRCNN_ERR_INVALID; }

// Every stripe call.  kind: what the planes are -- one byte channel, interleaved 3-byte pixels, or float planes of the loaded
// model's channel count; strides and pitches in elements (bytes, or floats).  src_rows < 0: the plain form, src holds every row
// the range needs
struct RowsCall {
    const char *what;
    StripeKind kind;
    const void *src;
    size_t src_stride, src_ch_pitch;
    int src_row0, src_rows;
    const void *halo_top, *halo_bot;
    size_t halo_stride, halo_ch_pitch;
    void *dst;
    size_t dst_stride, dst_ch_pitch;
    int dst_row0, width, height, row_begin, row_end;
    float *pre;
};

static int model_rows(srcnn_ctx *c, const RowsCall &a)
{
    BIND_KEEP(c);
    int rc;
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    const char *what = a.what;
    const bool halo = a.src_rows >= 0, f32 = a.kind == STRIPE_F32;
    const int width = a.width, height = a.height, row_begin = a.row_begin, row_end = a.row_end, src_row0 = a.src_row0;
    const int planes = f32 ? c->channels : 1;                     // channel planes (the bytes of a colour pixel share a row)
    const size_t es = f32 ? sizeof(float) : 1;                    // bytes per element
    const int roww = a.kind == STRIPE_COLOR ? 3 * std::min(width, 1 << 28) : width;      // elements of a row
    const size_t src_ch_pitch = planes > 1 ? a.src_ch_pitch : 0, dst_ch_pitch = planes > 1 ? a.dst_ch_pitch : 0;
    const size_t halo_ch_pitch = planes > 1 ? a.halo_ch_pitch : 0;
    constexpr size_t kMaxPitch = (size_t)1 << 40;      // (elements: every offset the kernels form stays far inside 63 bits)
    if (bad_plane(a.src, a.src_stride, roww, height) || bad_plane(a.dst, a.dst_stride, roww, height) || width > (1 << 28) ||
        row_begin < 0 || row_end > height || row_begin >= row_end || src_row0 < 0 || a.dst_row0 < 0 || a.dst_row0 > row_begin ||
        src_ch_pitch >= kMaxPitch || dst_ch_pitch >= kMaxPitch || halo_ch_pitch >= kMaxPitch ||
        (halo && (a.src_rows == 0 || a.src_rows > height - src_row0 ||
                  ((a.halo_top || a.halo_bot) && a.halo_stride < (size_t)roww) || a.halo_stride >= ((size_t)1 << 30))))
        return fail(c, SRCNN_ERR_INVALID, "%s: bad arguments", what);
    // a model of the wrong channel count, layers from per-filter calls, the banded path's gate
    if ((rc = model_rows_refusal(c, a.kind))) return rc;
    // the receptive field of rows [row_begin, row_end) must lie in src (halo form: in top | src | bot)
    const int R = srcnn_model_halo_rows(c);
    const int need0 = std::max(0, row_begin - R), need1 = std::min(height, row_end + R);
    const int src_row1 = halo ? src_row0 + a.src_rows : height;
    if (!halo && src_row0 > need0)
        return fail(c, SRCNN_ERR_INVALID, "%s: rows [%d,%d) need input rows [%d,%d) (a halo of %d rows); src starts at row %d", what,
                    row_begin, row_end, need0, need1, R, src_row0);
    if (halo && ((need0 < src_row0 && (!a.halo_top || src_row0 < R || need0 < src_row0 - R)) ||
                 (need1 > src_row1 && (!a.halo_bot || need1 > src_row1 + R))))
        return fail(c, SRCNN_ERR_INVALID, "%s: rows [%d,%d) need input rows [%d,%d); src holds [%d,%d) and the halo buffers %d rows "
                                          "either side", what, row_begin, row_end, need0, need1, src_row0, src_row1, R);
    // a side the call reads nothing from keeps a null pointer: with both null this is the plain form
    const void *top = halo && need0 < src_row0 ? a.halo_top : nullptr, *bot = halo && need1 > src_row1 ? a.halo_bot : nullptr;
    if (a.kind == STRIPE_Y && luma_path_ok(c)) {      // the strip path runs this model: the stripe calls of that path, R = 6, the same bytes
        const uint8_t *d_src = static_cast<const uint8_t *>(a.src);
        uint8_t *d_dst = static_cast<uint8_t *>(a.dst);
        if (a.pre)
            return fail(c, SRCNN_ERR_STATE, "%s: the replicate-padded 9-1-5 model runs its stripes on the strip path, which has no "
                                            "pre-clamp output (srcnn_forward_y_dev has one)", what);
        if (!halo)
            return srcnn_forward_y_rows_dev(c, d_src, a.src_stride, src_row0, d_dst, a.dst_stride, a.dst_row0, width, height, row_begin,
                                            row_end);
        return srcnn_forward_y_rows_halo_dev(c, d_src, a.src_stride, src_row0, a.src_rows, static_cast<const uint8_t *>(a.halo_top),
                                             static_cast<const uint8_t *>(a.halo_bot), a.halo_stride, d_dst, a.dst_stride, a.dst_row0,
                                             width, height, row_begin, row_end);
    }
    if (planes > 1 && !f32_planes_disjoint(planes, a.dst_stride, dst_ch_pitch, 0, width, row_end - row_begin, 1))
        return fail(c, SRCNN_ERR_INVALID, "%s: the output planes overlap each other (channel pitch %zu floats for %d rows of stride "
                                          "%zu)", what, dst_ch_pitch, row_end - row_begin, a.dst_stride);
    {   // like the whole-image calls: the path cannot run in place -- the rows written must overlap none of the rows read
        // (float planes: the span from the first channel's first row to the last channel's last)
        const size_t row_elems = (size_t)roww;
        const uint8_t *out0 = static_cast<const uint8_t *>(a.dst) + es * (size_t)(row_begin - a.dst_row0) * a.dst_stride;
        const size_t out_bytes = es * ((size_t)(planes - 1) * dst_ch_pitch + (size_t)(row_end - row_begin - 1) * a.dst_stride + row_elems);
        const int s0 = top ? src_row0 : need0, s1 = bot ? src_row1 : need1;         // the rows read from src
        const size_t halo_bytes = es * ((size_t)(planes - 1) * halo_ch_pitch + (size_t)(R - 1) * a.halo_stride + row_elems);
        if ((s1 > s0 && ranges_overlap(out0, out_bytes, static_cast<const uint8_t *>(a.src) + es * (size_t)(s0 - src_row0) * a.src_stride,
                                       es * ((size_t)(planes - 1) * src_ch_pitch + (size_t)(s1 - s0 - 1) * a.src_stride + row_elems))) ||
            (top && ranges_overlap(out0, out_bytes, top, halo_bytes)) || (bot && ranges_overlap(out0, out_bytes, bot, halo_bytes)))
            return fail(c, SRCNN_ERR_INVALID, "%s: the output rows overlap the input (src or a halo buffer)", what);
    }
    if ((rc = flush_seams(c))) return rc;
    BandedPlanes io;
    io.f32 = f32;
    io.src = a.src;
    io.src_stride = a.src_stride;
    io.px_step = a.kind == STRIPE_COLOR ? 3 : 1;
    io.ch_step = a.kind == STRIPE_COLOR ? 1 : src_ch_pitch;
    io.dst = a.dst;
    io.dst_stride = a.dst_stride;
    io.dst_ch_pitch = dst_ch_pitch;
    io.pre = a.pre;
    io.rows = true;
    io.row_begin = row_begin;
    io.row_end = row_end;
    io.src_row0 = src_row0;
    io.src_rows = src_row1 - src_row0;
    io.dst_row0 = a.dst_row0;
    io.halo_top = top;
    io.halo_bot = bot;
    io.halo_stride = a.halo_stride;
    io.halo_ch_pitch = halo_ch_pitch;
    return forward_banded(c, io, width, height, 1);
}

int srcnn_model_rows_dev(srcnn_ctx *c, const uint8_t *d_src, size_t src_stride, int src_row0, uint8_t *d_dst, size_t dst_stride,
                         int dst_row0, int width, int height, int row_begin, int row_end, float *d_preclamp)
{
    return model_rows(c, RowsCall{"model_rows_dev", STRIPE_Y, d_src, src_stride, 0, src_row0, -1, nullptr, nullptr, 0, 0, d_dst,
                                  dst_stride, 0, dst_row0, width, height, row_begin, row_end, d_preclamp});
}

int srcnn_model_rows_halo_dev(srcnn_ctx *c, const uint8_t *d_src, size_t src_stride, int src_row0, int src_rows,
                              const uint8_t *d_halo_top, const uint8_t *d_halo_bot, size_t halo_stride, uint8_t *d_dst,
                              size_t dst_stride, int dst_row0, int width, int height, int row_begin, int row_end, float *d_preclamp)
{
    if (c && src_rows < 0) return fail(c, SRCNN_ERR_INVALID, "model_rows_halo_dev: bad arguments");
    return model_rows(c, RowsCall{"model_rows_halo_dev", STRIPE_Y, d_src, src_stride, 0, src_row0, src_rows, d_halo_top, d_halo_bot,
                                  halo_stride, 0, d_dst, dst_stride, 0, dst_row0, width, height, row_begin, row_end, d_preclamp});
}

/* ---- row stripes of a colour model and of float planes (include/srcnn_amd.h) ---- */

int srcnn_model_color_rows_dev(srcnn_ctx *c, const uint8_t *d_src, size_t src_stride, int src_row0, uint8_t *d_dst, size_t dst_stride,
                               int dst_row0, int width, int height, int row_begin, int row_end, float *d_preclamp)
{
    return model_rows(c, RowsCall{"model_color_rows_dev", STRIPE_COLOR, d_src, src_stride, 0, src_row0, -1, nullptr, nullptr, 0, 0,
                                  d_dst, dst_stride, 0, dst_row0, width, height, row_begin, row_end, d_preclamp});
}

int srcnn_model_color_rows_halo_dev(srcnn_ctx *c, const uint8_t *d_src, size_t src_stride, int src_row0, int src_rows,
                                    const uint8_t *d_halo_top, const uint8_t *d_halo_bot, size_t halo_stride, uint8_t *d_dst,
                                    size_t dst_stride, int dst_row0, int width, int height, int row_begin, int row_end,
                                    float *d_preclamp)
{
    if (c && src_rows < 0) return fail(c, SRCNN_ERR_INVALID, "model_color_rows_halo_dev: bad arguments");
    return model_rows(c, RowsCall{"model_color_rows_halo_dev", STRIPE_COLOR, d_src, src_stride, 0, src_row0, src_rows, d_halo_top,
                                  d_halo_bot, halo_stride, 0, d_dst, dst_stride, 0, dst_row0, width, height, row_begin, row_end,
                                  d_preclamp});
}

int srcnn_model_rows_f32_dev(srcnn_ctx *c, const float *d_src, size_t src_stride, size_t src_ch_pitch, int src_row0, float *d_dst,
                             size_t dst_stride, size_t dst_ch_pitch, int dst_row0, int width, int height, int row_begin, int row_end)
{
    return model_rows(c, RowsCall{"model_rows_f32_dev", STRIPE_F32, d_src, src_stride, src_ch_pitch, src_row0, -1, nullptr, nullptr, 0,
                                  0, d_dst, dst_stride, dst_ch_pitch, dst_row0, width, height, row_begin, row_end, nullptr});
}

int srcnn_model_rows_halo_f32_dev(srcnn_ctx *c, const float *d_src, size_t src_stride, size_t src_ch_pitch, int src_row0, int src_rows,
                                  const float *d_halo_top, const float *d_halo_bot, size_t halo_stride, size_t halo_ch_pitch,
                                  float *d_dst, size_t dst_stride, size_t dst_ch_pitch, int dst_row0, int width, int height,
                                  int row_begin, int row_end)
{
    if (c && src_rows < 0) return fail(c, SRCNN_ERR_INVALID, "model_rows_halo_f32_dev: bad arguments");
    return model_rows(c, RowsCall{"model_rows_halo_f32_dev", STRIPE_F32, d_src, src_stride, src_ch_pitch, src_row0, src_rows,
                                  d_halo_top, d_halo_bot, halo_stride, halo_ch_pitch, d_dst, dst_stride, dst_ch_pitch, dst_row0, width,
                                  height, row_begin, row_end, nullptr});
}

int srcnn_set_input_range(srcnn_ctx *c, float r)
{
    if (!c) return SRCNN_ERR_INVALID;
    if (!std::isfinite(r) || !(r > 0.f))
        return fail(c, SRCNN_ERR_INVALID, "srcnn_set_input_range: %g (a finite range > 0: the largest |input| of a float call)", (double)r);
    c->input_range = r;        // read when a float call launches, like the padding
    return SRCNN_OK;
}

float srcnn_get_input_range(const srcnn_ctx *c) { return c ? c->input_range : (float)SRCNN_ERR_INVALID; }

int srcnn_forward_f32_dev(srcnn_ctx *c, const float *d_src, size_t src_stride, size_t src_ch_pitch, size_t src_frame_pitch,
                          float *d_dst, size_t dst_stride, size_t dst_ch_pitch, size_t dst_frame_pitch, int width, int height,
                          int n_frames)
{
    BIND(c);
    int rc;
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    const int C = c->channels;
    constexpr size_t kMaxPitch = (size_t)1 << 40;      // (elements: every offset the kernels form stays far inside 63 bits)
    if (bad_plane(d_src, src_stride, width, height) || bad_plane(d_dst, dst_stride, width, height) || n_frames <= 0 ||
        src_ch_pitch >= kMaxPitch || dst_ch_pitch >= kMaxPitch || src_frame_pitch >= kMaxPitch || dst_frame_pitch >= kMaxPitch)
        return fail(c, SRCNN_ERR_INVALID, "forward_f32_dev: bad arguments");
    if (!f32_planes_disjoint(C, dst_stride, dst_ch_pitch, dst_frame_pitch, width, height, n_frames))
        return fail(c, SRCNN_ERR_INVALID, "forward_f32_dev: the output planes overlap each other (channel pitch %zu, frame pitch %zu "
                                          "floats for %d channel(s) and %d frame(s))", dst_ch_pitch, dst_frame_pitch, C, n_frames);
    // every output pixel reads a window of input pixels that other workgroups may already have overwritten
    if (ranges_overlap(d_src, sizeof(float) * f32_span(C, src_stride, src_ch_pitch, src_frame_pitch, width, height, n_frames), d_dst,
                       sizeof(float) * f32_span(C, dst_stride, dst_ch_pitch, dst_frame_pitch, width, height, n_frames)))
        return fail(c, SRCNN_ERR_INVALID, "forward_f32_dev: src and dst overlap (the path cannot run in place)");
    BandedPlanes io;
    io.f32 = true;
    io.src = d_src;
    io.src_stride = src_stride;
    io.ch_step = C == 1 ? 0 : src_ch_pitch;
    io.src_frame_pitch = src_frame_pitch;
    io.dst = d_dst;
    io.dst_stride = dst_stride;
    io.dst_ch_pitch = C == 1 ? 0 : dst_ch_pitch;
    io.dst_frame_pitch = dst_frame_pitch;
    if ((rc = forward_banded(c, io, width, height, n_frames))) return rc;
    return SRCNN_OK;
}

int srcnn_forward_f32(srcnn_ctx *c, const float *src, size_t src_stride, size_t src_ch_pitch, float *dst, size_t dst_stride,
                      size_t dst_ch_pitch, int width, int height)
{
    BIND(c);
    int rc;
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    const int C = c->channels;
    if (bad_plane(src, src_stride, width, height) || bad_plane(dst, dst_stride, width, height) ||
        !f32_planes_disjoint(C, dst_stride, dst_ch_pitch, 0, width, height, 1))
        return fail(c, SRCNN_ERR_INVALID, "forward_f32: bad arguments");
    if ((rc = banded_refusal(c, true))) return rc;      // before anything is staged
    const size_t row = (size_t)width * sizeof(float), plane = (size_t)width * height;
    if ((rc = reserve(c, c->in_u8, C * plane * sizeof(float)))) return rc;
    if ((rc = reserve(c, c->pre_f32, C * plane * sizeof(float)))) return rc;
    float *d_in = static_cast<float *>(c->in_u8.p), *d_out = static_cast<float *>(c->pre_f32.p);
    for (int ch = 0; ch < C; ++ch)
        HIP_TRY(c, hipMemcpy2DAsync(d_in + ch * plane, row, src + ch * src_ch_pitch, src_stride * sizeof(float), row, height,
                                    hipMemcpyHostToDevice, c->stream));
    BandedPlanes io;
    io.f32 = true;
    io.src = d_in;
    io.src_stride = width;
    io.ch_step = plane;
    io.dst = d_out;
    io.dst_stride = width;
    io.dst_ch_pitch = plane;
    if ((rc = forward_banded(c, io, width, height, 1))) return rc;
    for (int ch = 0; ch < C; ++ch)
        HIP_TRY(c, hipMemcpy2DAsync(dst + ch * dst_ch_pitch, dst_stride * sizeof(float), d_out + ch * plane, row, row, height,
                                    hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SRCNN_OK;
}

}  // extern "C"
