// srcnn_model.cpp -- the weight tables of the C-ABI layer: rigorous bounds of the layer maps and the exact power-of-two scales
// derived from them, the per-lane MFMA A-operand fragments (float32 and split-f16), the ranges the split-f16 mode needs, the
// flag threshold of SRCNN_MODE_REFBYTES, and the upload (srcnn_set_weights; the per-call tables of the reference surface,
// src/srcnn.cpp:609,627).
#include "srcnn_ctx.h"

using namespace srcnn;
using namespace srcnn::host;

namespace srcnn {
namespace host {

// Smallest e with  bound * (1 + 2^-16) <= 2^e  (0 for a zero / non-finite bound).
int scale_exponent(double bound)
{
    if (!(bound > 0.0) || !std::isfinite(bound)) return 0;
    int e = 0;
    (void)std::frexp(bound * (1.0 + 1.0 / 65536.0), &e);      // bound' = m * 2^e, m in [0.5, 1)  ->  bound' < 2^e
    return e;
}

// Power-of-two scales of layers 1 and 2 (srcnn_kernels.h): rigorous bounds of the two maps for ANY 8-bit input --
// layer-1 channel c is at most 255 * sum(max(w1, 0)) + b1, layer-2 channel k at most sum(max(w2, 0) * bound1) + b2.
// SRCNN_MODE_REFBYTES flags a pixel for exact recomputation when the MFMA path's pre-truncation value v lies within delta of
// an integer.  delta has to exceed |v_mfma - v_ref|, the difference of two float32 evaluations of the same sums in different
// orders with different roundings -- rounding NOISE: a rigorous worst-case bound (every rounding error at its maximum, all of
// one sign) is ~10 grey levels and useless, the measured maximum over 54 MPix of varied content is 4.4e-4 with a tail that
// falls by a factor of 100 per 0.9e-4 (profiles/r03/fixup_margin.txt).  The noise scales with the magnitudes the model can
// produce, so delta is tied to the model, not to a constant: E0 = 2^-24 * ||W3||_2 * B2 (one half-ulp rounding error of a
// layer-2 activation at its rigorous bound B2, carried through the 800 layer-3 weights as independent errors) is 3.3e-4 for the
// shipped model -- the scale of the measured maximum -- and delta = 6 * E0 = 2.0e-3: 4.5 x the largest difference ever seen,
// 0.4 % of the pixels flagged.  fix_apply_kernel records the largest |v_mfma - v_ref| it meets (srcnn_fixup_stats), so the margin
// of a deployment can be watched; tests/test_gpu_refbytes.py asserts it stays below delta / 2.
// A second, absolute term covers what does NOT scale with the weights: the roundings AT the output's own magnitude -- the kernels
// add b3 last (one rounding), the reference rounds its double sum to float and adds b3 (two): at most 3 half-ulps of a value
// below 256 = 2.3e-5, rigorous.  A model with small weights and a large b3 (tests/checks/soak_models.py found one: 6 * E0 =
// 3.6e-5, deviation met 3.1e-5) lives on that term alone; delta = 6 * E0 + 4 * 2^-24 * 256 (+ 6.1e-5: 2.03e-3 for the shipped model).
float fixup_delta(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, double margin)
{
    double a1[64], m2 = 0.0, s3 = 0.0;
    for (int c = 0; c < 64; ++c) {
        double s = 0.0;
        for (int t = 0; t < 81; ++t) s += std::max(w1[c * 81 + t], 0.f);
        a1[c] = std::max(0.0, 255.0 * s + b1[c]);
    }
    for (int k = 0; k < 32; ++k) {
        double s = b2[k];
        for (int i = 0; i < 64; ++i) s += (double)std::max(w2[k * 64 + i], 0.f) * a1[i];
        m2 = std::max(m2, s);
    }
    for (int i = 0; i < 800; ++i) s3 += (double)w3[i] * w3[i];
    const double d = margin * std::ldexp(1.0, -24) * std::sqrt(s3) * m2 + 4.0 * std::ldexp(1.0, -24) * 256.0;
    if (!std::isfinite(d)) return 0.25f;
    return (float)std::min(0.25, std::max(d, 1e-6));
}

void layer_scales(const float *w1, const float *b1, const float *w2, const float *b2, int *e1, int *e2)
{
    double a1[64], m1 = 0.0, m2 = 0.0;
    for (int c = 0; c < 64; ++c) {
        double s = 0.0;
        for (int t = 0; t < 81; ++t) s += std::max(w1[c * 81 + t], 0.f);
        a1[c] = std::max(0.0, 255.0 * s + b1[c]);
        m1 = std::max(m1, a1[c]);
    }
    for (int k = 0; k < 32; ++k) {
        double s = b2[k];
        for (int i = 0; i < 64; ++i) s += (double)std::max(w2[k * 64 + i], 0.f) * a1[i];
        m2 = std::max(m2, s);
    }
    *e1 = scale_exponent(m1);
    *e2 = scale_exponent(m2);
}

// Pack the reference-layout weights into per-lane MFMA A-operand fragments.
// Fragment q, lane l: i = l & 31 is the accumulator row the lane's weight
// feeds, kk = l >> 5 the k-slot (see srcnn_mfma.hip header).
void pack_fragments(const float *w1 /*[64][81]*/, const float *b1, const float *w2 /*[32][64]*/,
                    const float *b2, const float *w3 /*[32][25]*/, float *out /*[NFRAG][64]*/)
{
    int e1, e2;
    layer_scales(w1, b1, w2, b2, &e1, &e2);
    for (int l = 0; l < 64; ++l) {
        const int i = l & 31, kk = l >> 5;
        const int ch = row_chan(i);
        for (int t = 0; t < 2; ++t)
            for (int s = 0; s < 41; ++s) {
                const int tap = 2 * s + kk, c = 32 * t + ch;
                out[(t * 41 + s) * 64 + l] = std::ldexp(tap < 81 ? w1[c * 81 + tap] : b1[c], -e1);
            }
        for (int t = 0; t < 2; ++t)
            for (int r = 0; r < 16; ++r) {
                const float w = w2[ch * 64 + 32 * t + 2 * r + kk];
                out[(FRAG_L2 + t * 16 + r) * 64 + l] = std::ldexp(w, e1 - e2);
                out[(FRAG_L2U + t * 16 + r) * 64 + l] = std::ldexp(w, e1);
            }
        for (int r = 0; r < 16; ++r) {
            const int tap = l3_row_tap(i);
            const float w = tap >= 0 ? w3[(2 * r + kk) * 25 + tap] : 0.f;
            // the local-scale rows of the fused kernel (l3_row_is_scale()): a_c = max over the taps of |W3[c][tap]|
            float a = 0.f;
            if (l3_row_is_scale(i))
                for (int t = 0; t < 25; ++t) a = std::max(a, std::fabs(w3[(2 * r + kk) * 25 + t]));
            out[(FRAG_L3 + r) * 64 + l] = std::ldexp(tap >= 0 ? w : a, e2);
            out[(FRAG_L3U + r) * 64 + l] = w;
        }
        for (int r = 0; r < 16; ++r) {
            out[(FRAG_B2 + r) * 64 + l] = std::ldexp(b2[2 * r + kk], -e2);
            out[(FRAG_B2U + r) * 64 + l] = b2[2 * r + kk];
        }
    }
}

// Split-f16 A-operand fragments (srcnn_split16.hip).  A float w becomes the f16 pair
// hi = f16(w * scale), lo = f16(w * scale - hi), both round-to-nearest; the power-of-two scales are
// listed in the kernel's header comment.
void split16(float w, float scale, uint16_t *hi, uint16_t *lo)
{
    const float ws = w * scale;
    const _Float16 h = (_Float16)ws;
    const _Float16 l = (_Float16)(ws - (float)h);
    std::memcpy(hi, &h, 2);
    std::memcpy(lo, &l, 2);
}

void pack_fragments16(const float *w1 /*[64][81]*/, const float *b1, const float *w2 /*[32][64]*/,
                      const float *b2, const float *w3 /*[32][25]*/, uint8_t *out /*S16_TABLE_BYTES*/)
{
    constexpr float SCALE = 16384.f, SCALE1 = 2048.f;     // see the scale table in srcnn_split16.hip
    uint16_t *tab = reinterpret_cast<uint16_t *>(out);
    auto slot = [&](int frag, int l, int e) -> uint16_t * { return tab + ((size_t)frag * 64 + l) * 8 + e; };
    for (int l = 0; l < 64; ++l) {
        const int m = l & 31, h = l >> 5;
        for (int e = 0; e < 8; ++e) {
            for (int t = 0; t < 2; ++t)
                for (int b = 0; b < 6; ++b) {
                    const int tap = l1s_tap(b, h, e), c = 32 * t + m;
                    const float w = tap < 0 ? 0.f : (tap == 81 ? b1[c] : w1[c * 81 + tap]);
                    split16(w, tap == 81 ? 0.125f : SCALE1, slot((2 * t) * 6 + b, l, e), slot((2 * t + 1) * 6 + b, l, e));
                }
            // layer 2, k-block b: slot 8h+e is register 8(b&1)+e of layer-1 tile b>>1 on lane-half h,
            // i.e. layer-1 channel 32(b>>1) + acc_row(8(b&1)+e, h); row m = layer-2 channel m
            for (int b = 0; b < 4; ++b) {
                const int c1 = 32 * (b >> 1) + acc_row(8 * (b & 1) + e, h);
                split16(w2[m * 64 + c1], SCALE, slot(S16_FRAG_L2 + b, l, e), slot(S16_FRAG_L2 + 4 + b, l, e));
            }
            // layer 3, k-block b: slot 8h+e is layer-2 channel acc_row(8b+e, h); row m = tap l3_row_tap(m)
            for (int b = 0; b < 2; ++b) {
                const int c2 = acc_row(8 * b + e, h), tap = l3_row_tap(m);
                float a = 0.f;          // the local-scale rows (l3_row_is_scale()): a_c = max over the taps of |W3[c][tap]|, <= the f16 range the taps fit
                if (l3_row_is_scale(m))
                    for (int t = 0; t < 25; ++t) a = std::max(a, std::fabs(w3[c2 * 25 + t]));
                split16(tap >= 0 ? w3[c2 * 25 + tap] : a, SCALE, slot(S16_FRAG_L3 + b, l, e),
                        slot(S16_FRAG_L3 + 2 + b, l, e));
            }
        }
    }
    float *b2t = reinterpret_cast<float *>(out + (size_t)S16_NFRAG * 64 * 16);
    for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 16; ++r) b2t[h * 16 + r] = b2[acc_row(r, h)] * 0.0625f;
}

// SRCNN_MODE_SPLIT16 keeps its scaled activations below 1024 and its scaled weights inside f16
// (srcnn_split16.hip).  Rigorous bounds for ANY 8-bit input: layer-1 channel c is at most
// 255 * sum(max(w1,0)) + b1, layer-2 channel k at most sum(max(w2,0) * bound1) + b2.
bool split16_range_ok(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3)
{
    float a1[64], wmax1 = 0.f, wmax23 = 0.f, a1max = 0.f, a2max = 0.f;
    for (int c = 0; c < 64; ++c) {
        double s = 0;
        for (int t = 0; t < 81; ++t) {
            s += std::max(w1[c * 81 + t], 0.f);
            wmax1 = std::max(wmax1, std::fabs(w1[c * 81 + t]));
        }
        a1[c] = std::max(0.f, (float)(255.0 * s + b1[c]));
        a1max = std::max(a1max, a1[c]);
        wmax1 = std::max(wmax1, std::fabs(b1[c]) / 256.f);      // b1/8 must fit f16 as well
    }
    for (int k = 0; k < 32; ++k) {
        double s = b2[k];
        for (int i = 0; i < 64; ++i) {
            s += (double)std::max(w2[k * 64 + i], 0.f) * a1[i];
            wmax23 = std::max(wmax23, std::fabs(w2[k * 64 + i]));
        }
        a2max = std::max(a2max, (float)s);
    }
    for (int i = 0; i < 800; ++i) wmax23 = std::max(wmax23, std::fabs(w3[i]));
    return std::isfinite(a1max) && std::isfinite(a2max) && a1max < 8.f * 1024.f && a2max < 16.f * 1024.f &&
           wmax1 < 30.f && wmax23 < 3.9f;
}

int upload_weights(srcnn_ctx *c, const float *k99, const float *b99, const float *k11, const float *b11,
                   const float *k55, float b55)
{
    static const float zeros64[64] = {0};
    static std::vector<float> zero_w(64 * 81, 0.f);
    const float *w1 = k99 ? k99 : zero_w.data();
    const float *b1 = b99 ? b99 : zeros64;
    const float *w2 = k11 ? k11 : zero_w.data();
    const float *b2 = b11 ? b11 : zeros64;
    const float *w3 = k55 ? k55 : zero_w.data();
    std::vector<float> frag((size_t)NFRAG * 64);
    pack_fragments(w1, b1, w2, b2, w3, frag.data());
    // + W2 transposed [64][32] for the exact layer-1/2 kernel, + W1 transposed [81][64] (fix-up), + one tap of zeros: the fix-up
    // fetches a tap's weights one tap ahead, the last fetch lands here
    std::vector<float> raw(8129 + 2048 + 5184 + 64, 0.f);
    std::memcpy(raw.data(), b1, 64 * 4);
    std::memcpy(raw.data() + 64, w1, 5184 * 4);
    std::memcpy(raw.data() + 5248, b2, 32 * 4);
    std::memcpy(raw.data() + 5280, w2, 2048 * 4);
    raw[7328] = b55;
    std::memcpy(raw.data() + 7329, w3, 800 * 4);
    for (int k = 0; k < 32; ++k)
        for (int i = 0; i < 64; ++i) raw[8129 + i * 32 + k] = w2[k * 64 + i];
    for (int ch = 0; ch < 64; ++ch)
        for (int t = 0; t < 81; ++t) raw[10177 + t * 64 + ch] = w1[ch * 81 + t];
    std::vector<uint8_t> frag16(S16_TABLE_BYTES);
    pack_fragments16(w1, b1, w2, b2, w3, frag16.data());
    c->sp_f2 = c->sp16_f2 = 0;   // the banded path's tables no longer hold the model (srcnn_spatial.cpp)
    c->n1 = c->n1p = 64;         // ... and every model loaded through here has the plain widths (srcnn_set_model_shape sets
    c->n2 = c->n2p = 32;         // its own afterwards)
    int rc;
    if ((rc = reserve(c, c->wfrag, frag.size() * 4))) return rc;
    if ((rc = reserve(c, c->wfrag16, frag16.size()))) return rc;
    if ((rc = reserve(c, c->sink, 1 << 20))) return rc;   // scratch words (+ diagnostics in debug builds)
    if ((rc = reserve(c, c->wraw, raw.size() * 4))) return rc;
    // synchronous copies: the host vectors die at return; launches on any stream may still read the old tables
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(c->wfrag.p, frag.data(), frag.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->wraw.p, raw.data(), raw.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->wfrag16.p, frag16.data(), frag16.size(), hipMemcpyHostToDevice));
    c->b3 = b55;
    c->fix_delta = fixup_delta(w1, b1, w2, b2, w3, c->fix_margin);
    c->split16_ok = split16_range_ok(w1, b1, w2, b2, w3);
    std::memcpy(c->host_raw.data(), raw.data(), 8129 * sizeof(float));
    return SRCNN_OK;
}

// The whole-path entry points need all three layers.  srcnn_conv99x11 / srcnn_conv55 (the reference surface) load only the
// layers they are given -- the others stay zero -- and must not make a later srcnn_forward_y run on half a model.
const char *const kNoModel = "the model is not loaded: srcnn_set_weights not called (srcnn_conv99x11 / srcnn_conv55 load only their own layers)";

// The per-call tables of the reference surface (src/srcnn.cpp:609, :627: the same const arrays on every call).
// Layers 1-2 of the model are replaced, layer 3 of any loaded model is kept (and the other way round for layer 3);
// tables equal to the uploaded ones are not packed or uploaded again.
int refuse_spatial(srcnn_ctx *c, const char *what, bool banded_entry)
{
    if (wide_model(c))
        return fail(c, SRCNN_ERR_STATE, "%s does not run a model of %d / %d filters (srcnn_set_model_shape; padded to %d / %d): "
                                        "such a model runs in SRCNN_MODE_MFMA through srcnn_forward_y(_dev) / srcnn_forward_y_frames / "
                                        "srcnn_forward_color(_dev) / srcnn_process_bgr(_dev) / srcnn_forward_f32* / srcnn_process_f32* / "
                                        "srcnn_process_rgb_f32* / the srcnn_*_image_dev calls",
                    what, c->n1, c->n2, c->n1p, c->n2p);
    if (c->mode == SRCNN_MODE_BANDED16 && !banded_entry)
        return fail(c, SRCNN_ERR_STATE, "%s does not run in SRCNN_MODE_BANDED16 (that mode runs whole models on the banded path: "
                                        "srcnn_forward_y / srcnn_forward_y_dev / srcnn_forward_y_frames / srcnn_forward_color* / "
                                        "srcnn_process_bgr*); use SRCNN_MODE_MFMA",
                    what);
    if (c->channels != 1)
        return fail(c, SRCNN_ERR_STATE, "%s runs a 1-channel model only: the context holds a colour 9-%d-5 model "
                                        "(srcnn_set_model_color); use srcnn_forward_color / srcnn_forward_color_dev / "
                                        "srcnn_process_bgr* in SRCNN_MODE_MFMA or SRCNN_MODE_BANDED16, or load a 1-channel model",
                    what, c->f2);
    if (c->padding == SRCNN_PAD_ZERO)
        return fail(c, SRCNN_ERR_STATE, "%s has replicate padding only: the context is set to SRCNN_PAD_ZERO (srcnn_set_padding); "
                                        "use srcnn_forward_y_dev / srcnn_forward_y / srcnn_forward_y_frames / srcnn_process_bgr* "
                                        "in SRCNN_MODE_MFMA, or srcnn_set_padding(SRCNN_PAD_REPLICATE)",
                    what);
    return fail(c, SRCNN_ERR_STATE, "%s runs the 9-1-5 model only: the context holds a 9-%d-5 model (srcnn_set_model); "
                                    "use srcnn_forward_y_dev / srcnn_forward_y / srcnn_forward_y_frames / srcnn_process_bgr*",
                what, c->f2);
}

// A per-filter call that loads weights under a 9-3-5 / 9-5-5 or a colour model ends that model (include/srcnn_amd.h,
// srcnn_set_model, srcnn_set_model_color): the context goes back to the 9-1-5 tables holding only the layers loaded from then
// on, so a whole-path call returns SRCNN_ERR_STATE until srcnn_set_model / srcnn_set_weights (or the per-filter calls have
// loaded all three layers).
void drop_spatial_model(srcnn_ctx *c)
{
    if (c->f2 == 1 && c->channels == 1 && !wide_model(c)) {
        c->n1 = 64;      // (a narrow model of srcnn_set_model_shape lives on as the 9-1-5 tables it is)
        c->n2 = 32;
        return;
    }
    c->f2 = 1;
    c->channels = 1;
    c->n1 = c->n1p = 64;
    c->n2 = c->n2p = 32;
    c->has_l12 = c->has_l3 = false;
    std::fill(c->host_raw.begin(), c->host_raw.end(), 0.f);
}

int use_layers12(srcnn_ctx *c, const float *kernel99, const float *bias99, const float *kernel11, const float *bias11)
{
    if (c->padding == SRCNN_PAD_ZERO) return refuse_spatial(c, "a per-filter call", true);
    drop_spatial_model(c);
    const float *hr = c->host_raw.data();
    const bool same = c->has_l12 && !std::memcmp(hr, bias99, 64 * 4) && !std::memcmp(hr + 64, kernel99, 5184 * 4) &&
                      !std::memcmp(hr + 5248, bias11, 32 * 4) && !std::memcmp(hr + 5280, kernel11, 2048 * 4);
    if (same) return SRCNN_OK;
    const std::vector<float> w3(hr + 7329, hr + 8129);      // upload_weights rewrites host_raw
    const int rc = upload_weights(c, kernel99, bias99, kernel11, bias11, w3.data(), c->b3);
    c->whole_model = false;
    if (rc == SRCNN_OK) c->has_l12 = true;
    return rc;
}
int use_layer3(srcnn_ctx *c, const float *kernel, float bias)
{
    if (c->padding == SRCNN_PAD_ZERO) return refuse_spatial(c, "a per-filter call", true);
    drop_spatial_model(c);
    const float *hr = c->host_raw.data();
    if (c->has_l3 && hr[7328] == bias && !std::memcmp(hr + 7329, kernel, 800 * 4)) return SRCNN_OK;
    const std::vector<float> raw(c->host_raw);               // upload_weights rewrites host_raw
    const int rc = upload_weights(c, raw.data() + 64, raw.data(), raw.data() + 5280, raw.data() + 5248, kernel, bias);
    c->whole_model = false;
    if (rc == SRCNN_OK) c->has_l3 = true;
    return rc;
}

}  // namespace host
}  // namespace srcnn

extern "C" {

int srcnn_set_weights(srcnn_ctx *c, const float *k99, const float *b99, const float *k11, const float *b11,
                      const float *k55, float b55)
{
    BIND(c);
    int rc = SRCNN_OK;
    (void)rc;
    if (!k99 || !b99 || !k11 || !b11 || !k55) return fail(c, SRCNN_ERR_INVALID, "null weight table");
    c->f2 = 1;                  // back on the 9-1-5 path (srcnn_set_model)
    // the end of a colour model or of a wide one: its zero 9-1-5 tables are replaced whatever the caller passes
    if (c->channels != 1 || wide_model(c)) {
        c->channels = 1;
        c->has_l12 = c->has_l3 = false;
    }
    c->n1 = c->n1p = 64;
    c->n2 = c->n2p = 32;
    // a caller that passes its const tables on every call (the reference does, src/srcnn.cpp:609,627) packs and uploads once
    const float *hr = c->host_raw.data();
    if (c->has_l12 && c->has_l3 && hr[7328] == b55 && !std::memcmp(hr, b99, 64 * 4) && !std::memcmp(hr + 64, k99, 5184 * 4) &&
        !std::memcmp(hr + 5248, b11, 32 * 4) && !std::memcmp(hr + 5280, k11, 2048 * 4) && !std::memcmp(hr + 7329, k55, 800 * 4)) {
        c->whole_model = true;
        return SRCNN_OK;
    }
    if ((rc = upload_weights(c, k99, b99, k11, b11, k55, b55))) return rc;
    c->has_l12 = c->has_l3 = true;
    c->whole_model = true;
    return SRCNN_OK;
}

}  // extern "C"
