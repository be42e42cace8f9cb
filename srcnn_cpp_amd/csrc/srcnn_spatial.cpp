// srcnn_spatial.cpp -- the 9-3-5 / 9-5-5 models (srcnn_set_model, f2 = 3 or 5): their weight table and the banded path
// layer 1 -> spatial layer 2 (srcnn_spatial_kernels.hip) -> MODE_L3 strip kernel (srcnn_mfma.hip) behind srcnn_forward_y_dev;
// and zero padding (srcnn_set_padding): every model, f2 = 1 included, on the same bands with the kernels' zero-padding forms
// and the zero-padding layer 3 (spatial_l3z_kernel).
#include "srcnn_ctx.h"

using namespace srcnn;
using namespace srcnn::host;

namespace srcnn {
namespace host {

// Layer 2 of the fragment table (srcnn_kernels.h): [8 chunks][f2 * f2 taps][4 pairs][64], then b2 [32].  w2 is [32][64][f2][f2]
// (PyTorch's conv2.weight).  Also the layer 2 of a colour model (srcnn_color.cpp).
void pack_spatial_l2(int f2, const float *w2, const float *b2, float *o2)
{
    const int taps = f2 * f2;
    for (int chunk = 0; chunk < 8; ++chunk)
        for (int tap = 0; tap < taps; ++tap)
            for (int pp = 0; pp < 4; ++pp)
                for (int l = 0; l < 64; ++l) {
                    const int k = l & 31, ci = 8 * chunk + 2 * pp + (l >> 5);
                    o2[(((size_t)chunk * taps + tap) * 4 + pp) * 64 + l] = w2[((size_t)k * 64 + ci) * taps + tap];
                }
    std::memcpy(o2 + (size_t)taps * 2048, b2, 32 * sizeof(float));
}

// The fragment table of srcnn_kernels.h (spatial_table_floats()).
static void pack_spatial(int f2, const float *w1, const float *b1, const float *w2, const float *b2, float *out)
{
    for (int l = 0; l < 64; ++l) {
        const int i = l & 31, kk = l >> 5;
        for (int t = 0; t < 2; ++t)
            for (int s = 0; s < 41; ++s) {
                const int tap = 2 * s + kk, c = 32 * t + i;
                out[(t * 41 + s) * 64 + l] = tap < 81 ? w1[c * 81 + tap] : b1[c];
            }
    }
    pack_spatial_l2(f2, w2, b2, out + (size_t)SPATIAL_NFRAG_L1 * 64);
}

// The A fragments of spatial_l3z_kernel (srcnn_kernels.h, SPATIAL_NFRAG_L3Z) from W3 [32][5][5]; a colour model packs one
// such set per output channel.
void pack_l3z(const float *w3, float *out)
{
    for (int s = 0; s < SPATIAL_NFRAG_L3Z; ++s)
        for (int l = 0; l < 64; ++l) {
            const int tap = l3_row_tap(l & 31);
            out[s * 64 + l] = tap < 0 ? 0.f : w3[(2 * s + (l >> 5)) * 25 + tap];
        }
}

// The zero-padding tables of the loaded model, packed from host_raw the first time a zero-padded call needs them after a load:
// the layer-3 fragments, and for f2 = 1 the layer-1/2 table that srcnn_set_model builds for f2 = 3, 5.
static int ensure_zero_tables(srcnn_ctx *c)
{
    if (c->zp_f2 == c->f2) return SRCNN_OK;
    const float *hr = c->host_raw.data();
    std::vector<float> l3((size_t)SPATIAL_NFRAG_L3Z * 64), table;
    pack_l3z(hr + 7329, l3.data());
    if (c->f2 == 1) {
        table.resize(spatial_table_floats(1));
        pack_spatial(1, hr + 64, hr, hr + 5280, hr + 5248, table.data());
    }
    int rc;
    if ((rc = reserve(c, c->zp_frag, l3.size() * sizeof(float)))) return rc;
    if (!table.empty() && (rc = reserve(c, c->sp_frag, table.size() * sizeof(float)))) return rc;
    HIP_TRY(c, hipDeviceSynchronize());        // launches on any stream may still read the old tables
    HIP_TRY(c, hipMemcpy(c->zp_frag.p, l3.data(), l3.size() * sizeof(float), hipMemcpyHostToDevice));
    if (!table.empty()) HIP_TRY(c, hipMemcpy(c->sp_frag.p, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    c->zp_f2 = c->f2;
    return SRCNN_OK;
}

// Rows [b0, b1) of a plane need layer-2 rows [b0 - 2, b1 + 2) and layer-1 rows [b0 - 2 - r2, b1 + 2 + r2), clamped to the
// image: a band recomputes the 2 + r2 layer-1 rows and 2 layer-2 rows either side it shares with its neighbours.  Bands are
// as tall as kSpatialWorkBytes allows for the two maps (256 + 128 B per pixel of a row).
static int forward_spatial_impl(srcnn_ctx *c, const uint8_t *src, size_t src_stride, size_t src_frame_pitch, uint8_t *dst,
                                size_t dst_stride, size_t dst_frame_pitch, int width, int height, int n_frames, float *pre)
{
    int rc;
    const bool zero = c->padding == SRCNN_PAD_ZERO;
    if (zero && c->mode != SRCNN_MODE_MFMA)
        return fail(c, SRCNN_ERR_STATE, "SRCNN_PAD_ZERO (srcnn_set_padding) runs in SRCNN_MODE_MFMA only (mode %d has replicate "
                                        "padding only)", c->mode);
    if (c->mode != SRCNN_MODE_MFMA)
        return fail(c, SRCNN_ERR_STATE, "a 9-%d-5 model runs in SRCNN_MODE_MFMA only (mode %d has no arithmetic for a spatial "
                                        "layer 2)", c->f2, c->mode);
    if (zero && !c->whole_model)
        return fail(c, SRCNN_ERR_STATE, "SRCNN_PAD_ZERO needs a model loaded by srcnn_set_weights / srcnn_set_model: the loaded "
                                        "layers came from per-filter calls");
    if (zero && (rc = ensure_zero_tables(c))) return rc;
    const int r2 = (c->f2 - 1) / 2;
    const long row_bytes = 4L * width;
    const long cap = (long)(kSpatialWorkBytes / (size_t)row_bytes) - 64L * (4 + 2 * r2) - 32L * 4;
    const int band_max = (int)std::max(16L, cap / 96);
    const int n_bands = (height + band_max - 1) / band_max;
    const int band = (height + n_bands - 1) / n_bands;
    const long mrows = std::min<long>(height, band + 4 + 2 * r2), orows = std::min<long>(height, band + 4);
    const long mpitch = mrows * width, opitch = orows * width;
    if (bad_pitch((size_t)mpitch) || bad_pitch((size_t)opitch))
        return fail(c, SRCNN_ERR_INVALID, "forward_y_dev: plane too large for a 9-%d-5 model", c->f2);
    if ((rc = reserve(c, c->sp_map64, (size_t)64 * mpitch * sizeof(float)))) return rc;
    if ((rc = reserve(c, c->sp_map32, (size_t)32 * opitch * sizeof(float)))) return rc;
    if (!c->sp_done) HIP_TRY(c, hipEventCreateWithFlags(&c->sp_done, hipEventDisableTiming));
    // the maps were last used on another stream (the two lanes of srcnn_forward_y_frames): wait for that work
    if (c->sp_stream && c->sp_stream != c->stream) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->sp_done, 0));
    const float *frag = static_cast<const float *>(c->sp_frag.p);
    const float *frag2 = frag + (size_t)SPATIAL_NFRAG_L1 * 64, *bias2 = frag2 + (size_t)c->f2 * c->f2 * 2048;
    float *map64 = static_cast<float *>(c->sp_map64.p), *map32 = static_cast<float *>(c->sp_map32.p);
    for (int f = 0; f < n_frames; ++f) {
        const uint8_t *sf = src + (size_t)f * src_frame_pitch;
        for (int b0 = 0; b0 < height; b0 += band) {
            const int b1 = std::min(height, b0 + band);
            const int o0 = std::max(0, b0 - 2), o1 = std::min(height, b1 + 2);
            const int m0 = std::max(0, o0 - r2), m1 = std::min(height, o1 + r2);
            HIP_TRY(c, launch_spatial_l1(zero, sf, (long)src_stride, width, height, m0, m1, frag, map64, mpitch, c->stream));
            HIP_TRY(c, launch_spatial_l2(c->f2, zero, map64, mpitch, m0, m1, width, height, o0, o1, frag2, bias2, map32, opitch,
                                         c->stream));
            if (zero) {
                HIP_TRY(c, launch_spatial_l3z(map32, opitch, o0, o1, width, height, b0, b1,
                                              static_cast<const float *>(c->zp_frag.p), c->b3, dst + (size_t)f * dst_frame_pitch,
                                              (long)dst_stride, pre ? pre + (size_t)f * dst_frame_pitch : nullptr, c->stream));
                continue;
            }
            StripParams q{};
            q.planes_in = map32 - (long)o0 * width;          // MODE_L3 addresses image rows; the band map starts at row o0
            q.pl_stride = width;
            q.pl_pitch = opitch;
            q.dst = dst + (size_t)f * dst_frame_pitch;
            q.pre = pre ? pre + (size_t)f * dst_frame_pitch : nullptr;
            q.dst_stride = (long)dst_stride;
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

static const bool forward_spatial_registered = (forward_spatial = &forward_spatial_impl, true);

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
    std::vector<float> table(spatial_table_floats(f2));
    pack_spatial(f2, k99, b99, k2, b2, table.data());
    // layer 3 (and the has-model state) through the 9-1-5 tables, with a zero 1x1 layer 2 that nothing of this model reads
    static const std::vector<float> zero_w2(2048, 0.f);
    c->f2 = 1;
    c->channels = 1;
    if ((rc = upload_weights(c, k99, b99, zero_w2.data(), b2, k55, b55))) return rc;
    c->has_l12 = c->has_l3 = true;
    if ((rc = reserve(c, c->sp_frag, table.size() * sizeof(float)))) return rc;
    HIP_TRY(c, hipDeviceSynchronize());        // launches on any stream may still read the old table
    HIP_TRY(c, hipMemcpy(c->sp_frag.p, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    c->f2 = f2;
    c->whole_model = true;
    return SRCNN_OK;
}

int srcnn_get_model_f2(const srcnn_ctx *c) { return c ? c->f2 : SRCNN_ERR_INVALID; }

int srcnn_set_padding(srcnn_ctx *c, int padding)
{
    if (!c) return SRCNN_ERR_INVALID;
    if (padding != SRCNN_PAD_REPLICATE && padding != SRCNN_PAD_ZERO)
        return fail(c, SRCNN_ERR_INVALID, "srcnn_set_padding: %d (SRCNN_PAD_REPLICATE = 0 or SRCNN_PAD_ZERO = 1)", padding);
    c->padding = padding;      // read when a call launches: work already queued keeps the padding it was queued with
    return SRCNN_OK;
}

int srcnn_get_padding(const srcnn_ctx *c) { return c ? c->padding : SRCNN_ERR_INVALID; }

}  // extern "C"
