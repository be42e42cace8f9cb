// srcnn_resize_f32.cpp -- the step in front of the float image path: the cubic resize of float32 planes as torch's bicubic
// interpolation defines it (srcnn_cubic_f32_taps, srcnn_resize_cubic_f32*), resize + model in one call (srcnn_process_f32*), and a
// 3-plane image through a 1-channel model (srcnn_luma_gain, srcnn_process_rgb_f32*).
// The tap tables are built here, on the host in float64.  The planes of a call become descriptors (f32_image), and the device
// steps -- the resize, the per-frame loops of resize + model and of luma front, model, merge back -- are the ones the
// srcnn_*_image_dev calls run (srcnn_image.cpp; launchers and kernels: srcnn_image.h, srcnn_pipeline.hip).
// The antialiased down-scaling resize lives here too (srcnn_cubic_aa_f32_taps, srcnn_resize_cubic_aa_f32*, and resample_aa_dev,
// the launch srcnn_resize_cubic_aa_image_dev shares): its tables have a tap count per output sample; kernels resample_aa_*.
// And Pillow's resize of uint8 images (srcnn_pil_taps, and resample_pil_dev, the launch behind srcnn_resize_pil_image_dev and
// the two process calls of srcnn_image.cpp): the same tables with int32 coefficients of 22 fractional bits; kernels resample_pil_*.
#include "srcnn_ctx.h"
#include "srcnn_image.h"

#include <climits>

using namespace srcnn;
using namespace srcnn::host;

namespace srcnn {
namespace host {

// Keys cubic (A = -0.75) taps of one axis as torch.nn.functional.interpolate(mode="bicubic", align_corners=False) defines
// them, for float32 planes: r = (n_src / n_dst) * (d + 0.5) - 0.5, first[d] = floor(r) (unclamped: the taps are first - 1 ..
// first + 2, the kernels clamp each index), t = r - first[d], coef[d] = c2(t + 1), c1(t), c1(1 - t), c2(2 - t) with
// c1(x) = ((A + 2) x - (A + 3)) x^2 + 1 and c2(x) = ((A x - 5 A) x + 8 A) x - 4 A.  All of it in float64, the coefficients
// rounded once to float32 (torch does the coordinates in float32 and drifts from this at non-dyadic ratios).
void cubic_f32_taps(int n_src, int n_dst, int *first, float *coef)
{
    const double scale = (double)n_src / (double)n_dst, A = -0.75;
    auto c1 = [A](double x) { return ((A + 2) * x - (A + 3)) * x * x + 1; };
    auto c2 = [A](double x) { return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A; };
    for (int d = 0; d < n_dst; ++d) {
        const double r = scale * (d + 0.5) - 0.5;
        const double i = std::floor(r), t = r - i;
        first[d] = (int)i;
        coef[4 * (size_t)d + 0] = (float)c2(t + 1);
        coef[4 * (size_t)d + 1] = (float)c1(t);
        coef[4 * (size_t)d + 2] = (float)c1(1 - t);
        coef[4 * (size_t)d + 3] = (float)c2(2 - t);
    }
}

// The float tables of a (sw x sh) -> (dw x dh) resize on the device, cached like the 8-bit ones above.  Layout: float
// xcoef[4 dw], ycoef[4 dh] (16-byte aligned: the kernels load a row of four at once), then int xfirst[dw], yfirst[dh].
int ensure_tables_f32(srcnn_ctx *c, int sw, int sh, int dw, int dh, ResizeTablesF32 *t)
{
    const size_t n = (size_t)dw + dh;
    if (!(c->f32_tables.p && c->ftab_sw == sw && c->ftab_sh == sh && c->ftab_dw == dw && c->ftab_dh == dh)) {
        std::vector<float> coef(4 * n);
        std::vector<int> first(n);
        cubic_f32_taps(sw, dw, first.data(), coef.data());
        cubic_f32_taps(sh, dh, first.data() + dw, coef.data() + 4 * (size_t)dw);
        // an earlier launch may still read the old tables, on this stream or on the one the context had then
        if (c->ftab_stream && c->ftab_stream != c->stream) HIP_TRY(c, hipStreamSynchronize(c->ftab_stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->ftab_sw = 0;
        int rc;
        if ((rc = reserve(c, c->f32_tables, n * 20))) return rc;
        HIP_TRY(c, hipMemcpy(c->f32_tables.p, coef.data(), n * 16, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(static_cast<char *>(c->f32_tables.p) + n * 16, first.data(), n * 4, hipMemcpyHostToDevice));
        c->ftab_sw = sw; c->ftab_sh = sh; c->ftab_dw = dw; c->ftab_dh = dh;
    }
    c->ftab_stream = c->stream;
    t->xcoef = static_cast<const float *>(c->f32_tables.p);
    t->ycoef = t->xcoef + 4 * (size_t)dw;
    t->xfirst = reinterpret_cast<const int *>(t->xcoef + 4 * n);
    t->yfirst = t->xfirst + dw;
    return SRCNN_OK;
}

// ---- sited tables: the chroma planes of a video frame (srcnn_chroma_taps; include/srcnn_amd.h has the arithmetic; host only) ----
static bool chroma_axis_ok(int sub, double d)
{
    return (sub == 1 || sub == 2) && std::isfinite(d) && std::fabs(d) <= 0.5 && (sub == 2 || d == 0.0);
}

// One axis.  Lengths are LUMA lengths; sample j of a grid lies at j + 0.5 + d in its own samples, `sub` luma samples wide.
// Output d at (d + 0.5) + dst_d maps to r = rho ((d + 0.5) + dst_d) - (0.5 + src_d) with rho = (src_len dst_sub) / (dst_len
// src_sub); first and the four coefficients from r as cubic_f32_taps forms them.  Float64 in this order, rounded once.
static int chroma_taps(int src_len, int dst_len, int src_sub, int dst_sub, double src_d, double dst_d, int *first, float *coef)
{
    if (src_len <= 0 || dst_len <= 0 || !first || !coef || !chroma_axis_ok(src_sub, src_d) || !chroma_axis_ok(dst_sub, dst_d))
        return SRCNN_ERR_INVALID;
    const double rho = ((double)src_len * (double)dst_sub) / ((double)dst_len * (double)src_sub), A = -0.75;
    auto c1 = [A](double x) { return ((A + 2) * x - (A + 3)) * x * x + 1; };
    auto c2 = [A](double x) { return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A; };
    const int n = (dst_len + dst_sub - 1) / dst_sub;
    for (int d = 0; d < n; ++d) {
        const double r = rho * ((d + 0.5) + dst_d) - (0.5 + src_d);
        const double i = std::floor(r), t = r - i;
        first[d] = (int)i;
        coef[4 * (size_t)d + 0] = (float)c2(t + 1);
        coef[4 * (size_t)d + 1] = (float)c1(t);
        coef[4 * (size_t)d + 2] = (float)c1(1 - t);
        coef[4 * (size_t)d + 3] = (float)c2(2 - t);
    }
    return SRCNN_OK;
}

// Keys cubic with A = -0.5 (the antialiased resize; the 4-tap resize above has -0.75)
static double keys_aa(double x)
{
    const double A = -0.5;
    x = std::fabs(x);
    if (x < 1.0) return ((A + 2) * x - (A + 3)) * x * x + 1;
    if (x < 2.0) return A * (((x - 5) * x + 8) * x - 4);
    return 0.0;
}

// first and count of output d: xmin = max(0, trunc(c - support + 0.5)), xend = min(s, trunc(c + support + 0.5))
static void aa_span(double c, double support, int s, int *xmin, int *count)
{
    const long long lo = std::max(0LL, (long long)(c - support + 0.5)), hi = std::min((long long)s, (long long)(c + support + 0.5));
    *xmin = (int)lo;
    *count = (int)(hi - lo);
}

// One axis of torch.nn.functional.interpolate(mode="bicubic", align_corners=False, antialias=True), in float64 and in the
// operation order include/srcnn_amd.h writes out; each coefficient rounded once to float32.
int cubic_aa_f32_taps(int n_src, int n_dst, int *first, int *count, float *coef, int max_taps)
{
    const double rho = (double)n_src / (double)n_dst, m = rho > 1.0 ? rho : 1.0, support = 2.0 * m;
    int kmax = 0;
    for (int d = 0; d < n_dst; ++d) {
        int xmin, cnt;
        aa_span(rho * (d + 0.5), support, n_src, &xmin, &cnt);
        kmax = std::max(kmax, cnt);
    }
    if (!coef) return kmax;
    if (max_taps < kmax) return SRCNN_ERR_INVALID;
    std::vector<double> w((size_t)kmax);
    for (int d = 0; d < n_dst; ++d) {
        const double c = rho * (d + 0.5);
        int xmin, cnt;
        aa_span(c, support, n_src, &xmin, &cnt);
        double total = 0.0;
        for (int j = 0; j < cnt; ++j) {
            w[(size_t)j] = keys_aa(((double)(j + xmin) - c + 0.5) / m);
            total += w[(size_t)j];
        }
        float *row = coef + (size_t)d * (size_t)max_taps;
        for (int j = 0; j < max_taps; ++j) row[j] = j < cnt ? (float)(total != 0.0 ? w[(size_t)j] / total : w[(size_t)j]) : 0.f;
        first[d] = xmin;
        count[d] = cnt;
    }
    return kmax;
}

// The antialiased tables of a (sw x sh) -> (dw x dh) resize on the device, cached like the float ones above.  Layout: float
// xcoef[kx][dw] (tap-major), ycoef[dh][ky], then int xfirst[dw], xcount[dw], yfirst[dh], ycount[dh].
static int ensure_tables_aa(srcnn_ctx *c, int sw, int sh, int dw, int dh, ResampleAaTables *t)
{
    if (!(c->aa_tables.p && c->atab_sw == sw && c->atab_sh == sh && c->atab_dw == dw && c->atab_dh == dh)) {
        const int kx = cubic_aa_f32_taps(sw, dw, nullptr, nullptr, nullptr, 0), ky = cubic_aa_f32_taps(sh, dh, nullptr, nullptr, nullptr, 0);
        const size_t nx = (size_t)kx * dw, ny = (size_t)ky * dh, n = (size_t)dw + dh;
        std::vector<float> coef(nx + ny), rows(nx);
        std::vector<int> ints(2 * n);
        cubic_aa_f32_taps(sw, dw, ints.data(), ints.data() + dw, rows.data(), kx);
        for (int d = 0; d < dw; ++d)
            for (int j = 0; j < kx; ++j) coef[(size_t)j * dw + d] = rows[(size_t)d * kx + j];
        cubic_aa_f32_taps(sh, dh, ints.data() + 2 * (size_t)dw, ints.data() + 2 * (size_t)dw + dh, coef.data() + nx, ky);
        // an earlier launch on this stream may still read the old tables (one on another stream: resample_aa_dev has waited)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->atab_sw = 0;
        int rc;
        if ((rc = reserve(c, c->aa_tables, (nx + ny + 2 * n) * 4))) return rc;
        HIP_TRY(c, hipMemcpy(c->aa_tables.p, coef.data(), (nx + ny) * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(static_cast<float *>(c->aa_tables.p) + nx + ny, ints.data(), 2 * n * 4, hipMemcpyHostToDevice));
        c->atab_sw = sw; c->atab_sh = sh; c->atab_dw = dw; c->atab_dh = dh; c->atab_kx = kx; c->atab_ky = ky;
    }
    const size_t nx = (size_t)c->atab_kx * dw, ny = (size_t)c->atab_ky * dh;
    t->xcoef = static_cast<const float *>(c->aa_tables.p);
    t->ycoef = t->xcoef + nx;
    t->xfirst = reinterpret_cast<const int *>(t->ycoef + ny);
    t->xcount = t->xfirst + dw;
    t->yfirst = t->xcount + dw;
    t->ycount = t->yfirst + dh;
    t->kx = c->atab_kx;
    t->ky = c->atab_ky;
    return SRCNN_OK;
}

#ifdef SRCNN_TUNING_BUILD
static int g_aa_force_general = 0, g_aa_last_form = -1;      // srcnn_debug_resample_aa_form / _last_form
#endif

int resample_aa_dev(srcnn_ctx *c, const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels, int n_frames)
{
    ResampleAaTables t;
    int rc;
    // tables and workspace were last used on another stream: that work ends before this call replaces or overwrites them
    if (c->aa_stream && c->aa_stream != c->stream) HIP_TRY(c, hipStreamSynchronize(c->aa_stream));
    if ((rc = ensure_tables_aa(c, sw, sh, dw, dh, &t))) return rc;
    int variant = resample_aa_variant(sw, sh, dw, dh, t.kx, t.ky);
#ifdef SRCNN_TUNING_BUILD
    if (g_aa_force_general) variant = RESAMPLE_AA_GENERAL;
    g_aa_last_form = variant;
#endif
    float *work = nullptr;
    if (variant == RESAMPLE_AA_GENERAL) {
        const unsigned __int128 bytes = (unsigned __int128)channels * n_frames * (size_t)sh * (size_t)dw * sizeof(float);
        if (bytes > ((unsigned __int128)1 << 46))
            return fail(c, SRCNN_ERR_NOMEM, "antialiased resize: the workspace of the two-launch form (%d planes of %d x %d floats) is too large",
                        channels * n_frames, dw, sh);
        if ((rc = reserve(c, c->aa_work, (size_t)bytes))) return rc;      // (growing waits for the device)
        work = static_cast<float *>(c->aa_work.p);
    }
    c->aa_stream = c->stream;
    HIP_TRY(c, launch_resample_aa(src, sw, sh, dst, dw, dh, channels, n_frames, t, variant, work, c->stream));
    return SRCNN_OK;
}

// ---- Pillow's resize of uint8 images (srcnn_pil_taps, resample_pil_dev; include/srcnn_amd.h has the arithmetic) ----
// the filter of Pillow's Resample.c: bilinear (support 1) or bicubic with a = -0.5 (support 2), the operations as written there
static double pil_filter(int filter, double x)
{
    x = std::fabs(x);
    if (filter == SRCNN_PIL_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// One axis of Image.resize on a uint8 picture (precompute_coeffs and normalize_coeffs_8bpc), float64 in the header's order, each
// coefficient an int32 with PIL_BITS fractional bits.  The conventions of cubic_aa_f32_taps.
int pil_taps(int n_src, int n_dst, int filter, int *first, int *count, int32_t *coef, int max_taps)
{
    const double scale = (double)n_src / (double)n_dst, fs = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == SRCNN_PIL_BILINEAR ? 1.0 : 2.0) * fs, ss = 1.0 / fs;
    int kmax = 0;
    for (int d = 0; d < n_dst; ++d) {
        int xmin, cnt;
        aa_span((d + 0.5) * scale, support, n_src, &xmin, &cnt);
        kmax = std::max(kmax, cnt);
    }
    if (!coef) return kmax;
    if (max_taps < kmax) return SRCNN_ERR_INVALID;
    std::vector<double> w((size_t)kmax);
    for (int d = 0; d < n_dst; ++d) {
        const double center = (d + 0.5) * scale;
        int xmin, cnt;
        aa_span(center, support, n_src, &xmin, &cnt);
        double ww = 0.0;
        for (int j = 0; j < cnt; ++j) {
            w[(size_t)j] = pil_filter(filter, ((double)(j + xmin) - center + 0.5) * ss);
            ww += w[(size_t)j];
        }
        int32_t *row = coef + (size_t)d * (size_t)max_taps;
        for (int j = 0; j < max_taps; ++j) {
            if (j >= cnt) { row[j] = 0; continue; }
            const double v = ww != 0.0 ? w[(size_t)j] / ww : w[(size_t)j];
            row[j] = v < 0.0 ? (int32_t)(-0.5 + v * (double)(1 << PIL_BITS)) : (int32_t)(0.5 + v * (double)(1 << PIL_BITS));
        }
        first[d] = xmin;
        count[d] = cnt;
    }
    return kmax;
}

// The table of one axis as the kernels take it: the identity (one tap of 1 << PIL_BITS, which returns the byte untouched) where
// the axis keeps its length -- Pillow skips that pass -- and pil_taps otherwise.  False where an output sample's sum |c_j|
// exceeds PIL_COEF_SUM_MAX (no geometry found does: DESIGN.md 4.22), which the kernels' 24-bit products and int32 sums rest on.
static bool pil_axis(int n_src, int n_dst, int filter, std::vector<int> *first, std::vector<int> *count, std::vector<int32_t> *coef,
                     int *k)
{
    first->assign((size_t)n_dst, 0);
    count->assign((size_t)n_dst, 1);
    if (n_src == n_dst) {
        *k = 1;
        coef->assign((size_t)n_dst, 1 << PIL_BITS);
        for (int d = 0; d < n_dst; ++d) (*first)[(size_t)d] = d;
        return true;
    }
    *k = pil_taps(n_src, n_dst, filter, nullptr, nullptr, nullptr, 0);
    coef->assign((size_t)*k * n_dst, 0);
    pil_taps(n_src, n_dst, filter, first->data(), count->data(), coef->data(), *k);
    for (int d = 0; d < n_dst; ++d) {
        long sum = 0;
        for (int j = 0; j < *k; ++j) sum += std::labs((long)(*coef)[(size_t)d * *k + j]);
        if (sum > PIL_COEF_SUM_MAX) return false;
    }
    return true;
}

// The most source rows a tile of PIL_TR output rows reads, from the tables themselves: rows yfirst[dy0] .. max(yfirst + ycount) - 1
static int pil_tile_span(const std::vector<int> &yfirst, const std::vector<int> &ycount)
{
    const int dh = (int)yfirst.size();
    long span = 0;
    for (int dy0 = 0; dy0 < dh; dy0 += PIL_TR) {
        const int dy1 = std::min(dy0 + PIL_TR, dh);
        long end = 0;
        for (int dy = dy0; dy < dy1; ++dy) {
            if (yfirst[(size_t)dy] < yfirst[(size_t)dy0] || ycount[(size_t)dy] <= 0) return INT_MAX;
            end = std::max(end, (long)yfirst[(size_t)dy] + ycount[(size_t)dy]);
        }
        // (the kernel takes the tile's end from its last row: the two must agree)
        if (end != (long)yfirst[(size_t)dy1 - 1] + ycount[(size_t)dy1 - 1]) return INT_MAX;
        span = std::max(span, end - yfirst[(size_t)dy0]);
    }
    return span > INT_MAX ? INT_MAX : (int)span;
}

// The Pillow tables of a (sw x sh) -> (dw x dh) resize with `filter` on the device, a cache slot of their own.  Layout, all
// int32: xcoef[kx][dw] (tap-major), ycoef[dh][ky], xfirst[dw], xcount[dw], yfirst[dh], ycount[dh].
static int ensure_tables_pil(srcnn_ctx *c, int sw, int sh, int dw, int dh, int filter, ResamplePilTables *t)
{
    if (!(c->pil_tables.p && c->ptab_sw == sw && c->ptab_sh == sh && c->ptab_dw == dw && c->ptab_dh == dh && c->ptab_filter == filter)) {
        std::vector<int> xfirst, xcount, yfirst, ycount;
        std::vector<int32_t> xrows, ycoef;
        int kx = 0, ky = 0;
        if (!pil_axis(sw, dw, filter, &xfirst, &xcount, &xrows, &kx) || !pil_axis(sh, dh, filter, &yfirst, &ycount, &ycoef, &ky))
            return fail(c, SRCNN_ERR_INVALID, "Pillow resize %d x %d -> %d x %d: a coefficient sum leaves the int32 accumulator's range",
                        sw, sh, dw, dh);
        const size_t nx = (size_t)kx * dw, ny = (size_t)ky * dh;
        std::vector<int32_t> all(nx + ny + 2 * ((size_t)dw + dh));
        for (int d = 0; d < dw; ++d)
            for (int j = 0; j < kx; ++j) all[(size_t)j * dw + d] = xrows[(size_t)d * kx + j];
        std::copy(ycoef.begin(), ycoef.end(), all.begin() + nx);
        int32_t *ints = all.data() + nx + ny;
        std::copy(xfirst.begin(), xfirst.end(), ints);
        std::copy(xcount.begin(), xcount.end(), ints + dw);
        std::copy(yfirst.begin(), yfirst.end(), ints + 2 * (size_t)dw);
        std::copy(ycount.begin(), ycount.end(), ints + 2 * (size_t)dw + dh);
        // an earlier launch on this stream may still read the old tables (one on another stream: resample_pil_dev has waited)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->ptab_sw = 0;
        int rc;
        if ((rc = reserve(c, c->pil_tables, all.size() * 4))) return rc;
        HIP_TRY(c, hipMemcpy(c->pil_tables.p, all.data(), all.size() * 4, hipMemcpyHostToDevice));
        c->ptab_sw = sw; c->ptab_sh = sh; c->ptab_dw = dw; c->ptab_dh = dh; c->ptab_filter = filter;
        c->ptab_kx = kx; c->ptab_ky = ky; c->ptab_span = pil_tile_span(yfirst, ycount);
    }
    const size_t nx = (size_t)c->ptab_kx * dw, ny = (size_t)c->ptab_ky * dh;
    t->xcoef = static_cast<const int *>(c->pil_tables.p);
    t->ycoef = t->xcoef + nx;
    t->xfirst = t->ycoef + ny;
    t->xcount = t->xfirst + dw;
    t->yfirst = t->xcount + dw;
    t->ycount = t->yfirst + dh;
    t->kx = c->ptab_kx;
    t->ky = c->ptab_ky;
    t->tile_span = c->ptab_span;
    return SRCNN_OK;
}

#ifdef SRCNN_TUNING_BUILD
static int g_pil_force_general = 0, g_pil_last_form = -1;      // srcnn_debug_resample_pil_form / _last_form
#endif

int resample_pil_dev(srcnn_ctx *c, const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels, int n_frames,
                     int filter)
{
    ResamplePilTables t;
    int rc;
    // tables and workspace were last used on another stream: that work ends before this call replaces or overwrites them
    if (c->pil_stream && c->pil_stream != c->stream) HIP_TRY(c, hipStreamSynchronize(c->pil_stream));
    if ((rc = ensure_tables_pil(c, sw, sh, dw, dh, filter, &t))) return rc;
    int variant = resample_pil_variant(sw, sh, dw, dh, t);
#ifdef SRCNN_TUNING_BUILD
    if (g_pil_force_general) variant = RESAMPLE_PIL_GENERAL;
    g_pil_last_form = variant;
#endif
    uint8_t *work = nullptr;
    if (variant == RESAMPLE_PIL_GENERAL) {
        const unsigned __int128 bytes = (unsigned __int128)channels * n_frames * (size_t)sh * (size_t)dw;
        if (bytes > ((unsigned __int128)1 << 46))
            return fail(c, SRCNN_ERR_NOMEM, "Pillow resize: the workspace of the two-launch form (%d planes of %d x %d bytes) is too large",
                        channels * n_frames, dw, sh);
        if ((rc = reserve(c, c->pil_work, (size_t)bytes))) return rc;      // (growing waits for the device)
        work = static_cast<uint8_t *>(c->pil_work.p);
    }
    c->pil_stream = c->stream;
    HIP_TRY(c, launch_resample_pil(src, sw, sh, dst, dw, dh, channels, n_frames, t, variant, work, c->stream));
    return SRCNN_OK;
}

int pil_workspace_image(srcnn_ctx *c, int width, int height, int channels, int n_frames, void **data)
{
    const unsigned __int128 bytes = (unsigned __int128)channels * n_frames * (size_t)width * (size_t)height;
    if (bytes > ((unsigned __int128)1 << 46))
        return fail(c, SRCNN_ERR_NOMEM, "Pillow resize: the resized image (%d planes of %d x %d bytes) is too large", channels * n_frames,
                    width, height);
    // the image was last read on another stream: that work ends before this call overwrites it
    if (c->pil_stream && c->pil_stream != c->stream) HIP_TRY(c, hipStreamSynchronize(c->pil_stream));
    int rc;
    if ((rc = reserve(c, c->pil_image, (size_t)bytes))) return rc;      // (growing waits for the device)
    *data = c->pil_image.p;
    return SRCNN_OK;
}

}  // namespace host
}  // namespace srcnn

// SRCNN_OK, or SRCNN_ERR_INVALID and the reason: the planes of a float resize (C channels x n_frames frames each side)
static int resize_f32_refusal(srcnn_ctx *c, const char *what, const float *src, size_t src_stride, size_t src_ch_pitch,
                              size_t src_frame_pitch, int src_w, int src_h, const float *dst, size_t dst_stride, size_t dst_ch_pitch,
                              size_t dst_frame_pitch, int dst_w, int dst_h, int C, int n_frames)
{
    constexpr size_t kMaxPitch = (size_t)1 << 40;      // (elements: every offset the kernels form stays far inside 63 bits)
    if (bad_plane(src, src_stride, src_w, src_h) || bad_plane(dst, dst_stride, dst_w, dst_h) || C <= 0 || n_frames <= 0 ||
        (long)C * n_frames > 0x7fffffffL || src_ch_pitch >= kMaxPitch || dst_ch_pitch >= kMaxPitch || src_frame_pitch >= kMaxPitch ||
        dst_frame_pitch >= kMaxPitch)
        return fail(c, SRCNN_ERR_INVALID, "%s: bad arguments", what);
    if (!f32_planes_disjoint(C, dst_stride, dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, n_frames))
        return fail(c, SRCNN_ERR_INVALID, "%s: the output planes overlap each other (channel pitch %zu, frame pitch %zu floats for %d "
                                          "channel(s) and %d frame(s))", what, dst_ch_pitch, dst_frame_pitch, C, n_frames);
    if (ranges_overlap(src, sizeof(float) * f32_span(C, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, n_frames), dst,
                       sizeof(float) * f32_span(C, dst_stride, dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, n_frames)))
        return fail(c, SRCNN_ERR_INVALID, "%s: src and dst overlap (the resize cannot run in place)", what);
    return SRCNN_OK;
}

// g = 1 / (w0 + w1 + w2) of a luma row {w0, w1, w2, off}: the sum in float64, rounded once.  False for a non-finite entry or a
// sum that is not positive.
static bool luma_gain(const float *luma, float *g)
{
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(luma[k])) return false;
    const double sum = (double)luma[0] + (double)luma[1] + (double)luma[2];
    if (!(sum > 0.0)) return false;
    *g = (float)(1.0 / sum);
    return std::isfinite(*g) && *g > 0.f;
}

// The gate of srcnn_process_rgb_f32*, before anything is staged or launched: SRCNN_OK and the gain, or the code and the reason
static int rgb_f32_refusal(srcnn_ctx *c, const char *what, const float *src, size_t src_stride, size_t src_ch_pitch,
                           size_t src_frame_pitch, int src_w, int src_h, const float *dst, size_t dst_stride, size_t dst_ch_pitch,
                           size_t dst_frame_pitch, int dst_w, int dst_h, const float *luma, const float *clamp, int n_frames, float *g)
{
    int rc;
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    if ((rc = resize_f32_refusal(c, what, src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, dst, dst_stride, dst_ch_pitch,
                                 dst_frame_pitch, dst_w, dst_h, 3, n_frames)))
        return rc;
    return process_rgb_refusal(c, what, "srcnn_process_f32 runs on the three planes", src_w, src_h, dst_w, dst_h, luma, clamp, g);
}

// The host-memory form of a call on one image of `C` planes: the planes into the packed device buffer lo (src_w x src_h), the
// device step on lo -> hi (dst_w x dst_h, packed), hi back into dst; returns when dst is written.
template <class Step>
static int f32_staged(srcnn_ctx *c, const float *src, size_t src_stride, size_t src_ch_pitch, int src_w, int src_h, float *dst,
                      size_t dst_stride, size_t dst_ch_pitch, int dst_w, int dst_h, int C, Step step)
{
    const size_t lo = (size_t)src_w * src_h, hi = (size_t)dst_w * dst_h;
    const size_t lo_row = (size_t)src_w * sizeof(float), hi_row = (size_t)dst_w * sizeof(float);
    int rc;
    if ((rc = reserve(c, c->f32_hi, C * hi * sizeof(float)))) return rc;
    if ((rc = reserve(c, c->f32_lo, C * lo * sizeof(float)))) return rc;
    float *d_lo = static_cast<float *>(c->f32_lo.p), *d_hi = static_cast<float *>(c->f32_hi.p);
    for (int ch = 0; ch < C; ++ch)
        HIP_TRY(c, hipMemcpy2DAsync(d_lo + ch * lo, lo_row, src + ch * src_ch_pitch, src_stride * sizeof(float), lo_row, src_h,
                                    hipMemcpyHostToDevice, c->stream));
    if ((rc = step(f32_image(d_lo, (size_t)src_w, lo, 0), f32_image(d_hi, (size_t)dst_w, hi, 0)))) return rc;
    for (int ch = 0; ch < C; ++ch)
        HIP_TRY(c, hipMemcpy2DAsync(dst + ch * dst_ch_pitch, dst_stride * sizeof(float), d_hi + ch * hi, hi_row, hi_row, dst_h,
                                    hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SRCNN_OK;
}

extern "C" {

int srcnn_cubic_f32_taps(int src_n, int dst_n, int *first, float *coef)
{
    if (src_n <= 0 || dst_n <= 0 || !first || !coef) return SRCNN_ERR_INVALID;
    cubic_f32_taps(src_n, dst_n, first, coef);
    return SRCNN_OK;
}

int srcnn_chroma_taps(int src_len, int dst_len, int src_sub, int dst_sub, double src_d, double dst_d, int *first, float *coef)
{
    return chroma_taps(src_len, dst_len, src_sub, dst_sub, src_d, dst_d, first, coef);
}

int srcnn_resize_cubic_f32_dev(srcnn_ctx *c, const float *d_src, size_t src_stride, size_t src_ch_pitch, size_t src_frame_pitch,
                               int src_w, int src_h, float *d_dst, size_t dst_stride, size_t dst_ch_pitch, size_t dst_frame_pitch,
                               int dst_w, int dst_h, int channels, int n_frames)
{
    BIND(c);
    int rc;
    if ((rc = resize_f32_refusal(c, "resize_cubic_f32_dev", d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, d_dst,
                                 dst_stride, dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, channels, n_frames)))
        return rc;
    return resize_cubic_dev(c, f32_image(d_src, src_stride, src_ch_pitch, src_frame_pitch), src_w, src_h,
                            f32_image(d_dst, dst_stride, dst_ch_pitch, dst_frame_pitch), dst_w, dst_h, channels, n_frames);
}

int srcnn_resize_cubic_f32(srcnn_ctx *c, const float *src, size_t src_stride, size_t src_ch_pitch, int src_w, int src_h, float *dst,
                           size_t dst_stride, size_t dst_ch_pitch, int dst_w, int dst_h, int channels)
{
    BIND(c);
    int rc;
    if ((rc = resize_f32_refusal(c, "resize_cubic_f32", src, src_stride, src_ch_pitch, 0, src_w, src_h, dst, dst_stride, dst_ch_pitch,
                                 0, dst_w, dst_h, channels, 1)))
        return rc;
    return f32_staged(c, src, src_stride, src_ch_pitch, src_w, src_h, dst, dst_stride, dst_ch_pitch, dst_w, dst_h, channels,
                      [&](const ImageRef &lo, const ImageRef &hi) {
                          return resize_cubic_dev(c, lo, src_w, src_h, hi, dst_w, dst_h, channels, 1);
                      });
}

int srcnn_cubic_aa_f32_taps(int src_n, int dst_n, int *first, int *count, float *coef, int max_taps)
{
    if (src_n <= 0 || dst_n <= 0) return SRCNN_ERR_INVALID;
    if (!coef) return cubic_aa_f32_taps(src_n, dst_n, nullptr, nullptr, nullptr, 0);
    if (!first || !count) return SRCNN_ERR_INVALID;
    return cubic_aa_f32_taps(src_n, dst_n, first, count, coef, max_taps);
}

int srcnn_pil_taps(int src_n, int dst_n, int filter, int *first, int *count, int32_t *coef, int max_taps)
{
    if (src_n <= 0 || dst_n <= 0 || (filter != SRCNN_PIL_BILINEAR && filter != SRCNN_PIL_BICUBIC)) return SRCNN_ERR_INVALID;
    if (!coef) return pil_taps(src_n, dst_n, filter, nullptr, nullptr, nullptr, 0);
    if (!first || !count) return SRCNN_ERR_INVALID;
    return pil_taps(src_n, dst_n, filter, first, count, coef, max_taps);
}

int srcnn_resize_cubic_aa_f32_dev(srcnn_ctx *c, const float *d_src, size_t src_stride, size_t src_ch_pitch, size_t src_frame_pitch,
                                  int src_w, int src_h, float *d_dst, size_t dst_stride, size_t dst_ch_pitch, size_t dst_frame_pitch,
                                  int dst_w, int dst_h, int channels, int n_frames)
{
    BIND(c);
    int rc;
    if ((rc = resize_f32_refusal(c, "resize_cubic_aa_f32_dev", d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, d_dst,
                                 dst_stride, dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, channels, n_frames)))
        return rc;
    return resample_aa_dev(c, f32_image(d_src, src_stride, src_ch_pitch, src_frame_pitch), src_w, src_h,
                           f32_image(d_dst, dst_stride, dst_ch_pitch, dst_frame_pitch), dst_w, dst_h, channels, n_frames);
}

int srcnn_resize_cubic_aa_f32(srcnn_ctx *c, const float *src, size_t src_stride, size_t src_ch_pitch, int src_w, int src_h, float *dst,
                              size_t dst_stride, size_t dst_ch_pitch, int dst_w, int dst_h, int channels)
{
    BIND(c);
    int rc;
    if ((rc = resize_f32_refusal(c, "resize_cubic_aa_f32", src, src_stride, src_ch_pitch, 0, src_w, src_h, dst, dst_stride, dst_ch_pitch,
                                 0, dst_w, dst_h, channels, 1)))
        return rc;
    return f32_staged(c, src, src_stride, src_ch_pitch, src_w, src_h, dst, dst_stride, dst_ch_pitch, dst_w, dst_h, channels,
                      [&](const ImageRef &lo, const ImageRef &hi) {
                          return resample_aa_dev(c, lo, src_w, src_h, hi, dst_w, dst_h, channels, 1);
                      });
}

int srcnn_process_f32_dev(srcnn_ctx *c, const float *d_src, size_t src_stride, size_t src_ch_pitch, size_t src_frame_pitch, int src_w,
                          int src_h, float *d_dst, size_t dst_stride, size_t dst_ch_pitch, size_t dst_frame_pitch, int dst_w, int dst_h,
                          int n_frames)
{
    BIND(c);
    int rc;
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    if ((rc = resize_f32_refusal(c, "process_f32_dev", d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, d_dst,
                                 dst_stride, dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, c->channels, n_frames)))
        return rc;
    if ((rc = forward_f32_refusal(c))) return rc;      // the gate of srcnn_forward_f32, before anything is launched
    return process_frames_dev(c, f32_image(d_src, src_stride, src_ch_pitch, src_frame_pitch), src_w, src_h,
                              f32_image(d_dst, dst_stride, dst_ch_pitch, dst_frame_pitch), dst_w, dst_h, n_frames);
}

int srcnn_process_f32(srcnn_ctx *c, const float *src, size_t src_stride, size_t src_ch_pitch, int src_w, int src_h, float *dst,
                      size_t dst_stride, size_t dst_ch_pitch, int dst_w, int dst_h)
{
    BIND(c);
    int rc;
    if (!has_model(c)) return fail(c, SRCNN_ERR_STATE, "%s", kNoModel);
    const int C = c->channels;
    if ((rc = resize_f32_refusal(c, "process_f32", src, src_stride, src_ch_pitch, 0, src_w, src_h, dst, dst_stride, dst_ch_pitch, 0,
                                 dst_w, dst_h, C, 1)))
        return rc;
    if ((rc = forward_f32_refusal(c))) return rc;      // before anything is staged
    return f32_staged(c, src, src_stride, src_ch_pitch, src_w, src_h, dst, dst_stride, dst_ch_pitch, dst_w, dst_h, C,
                      [&](const ImageRef &lo, const ImageRef &hi) { return process_frames_dev(c, lo, src_w, src_h, hi, dst_w, dst_h, 1); });
}

int srcnn_luma_gain(const float *luma, float *g)
{
    float v;
    if (!luma || !g || !luma_gain(luma, &v)) return SRCNN_ERR_INVALID;
    *g = v;
    return SRCNN_OK;
}

int srcnn_process_rgb_f32_dev(srcnn_ctx *c, const float *d_src, size_t src_stride, size_t src_ch_pitch, size_t src_frame_pitch,
                              int src_w, int src_h, float *d_dst, size_t dst_stride, size_t dst_ch_pitch, size_t dst_frame_pitch,
                              int dst_w, int dst_h, const float *luma, const float *clamp, int n_frames)
{
    BIND(c);
    int rc;
    float g = 0.f;
    if ((rc = rgb_f32_refusal(c, "process_rgb_f32_dev", d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, d_dst,
                              dst_stride, dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, luma, clamp, n_frames, &g)))
        return rc;
    return process_rgb_frames_dev(c, f32_image(d_src, src_stride, src_ch_pitch, src_frame_pitch), src_w, src_h,
                                  f32_image(d_dst, dst_stride, dst_ch_pitch, dst_frame_pitch), dst_w, dst_h, luma, g, clamp, n_frames);
}

int srcnn_process_rgb_f32(srcnn_ctx *c, const float *src, size_t src_stride, size_t src_ch_pitch, int src_w, int src_h, float *dst,
                          size_t dst_stride, size_t dst_ch_pitch, int dst_w, int dst_h, const float *luma, const float *clamp)
{
    BIND(c);
    int rc;
    float g = 0.f;
    if ((rc = rgb_f32_refusal(c, "process_rgb_f32", src, src_stride, src_ch_pitch, 0, src_w, src_h, dst, dst_stride, dst_ch_pitch, 0,
                              dst_w, dst_h, luma, clamp, 1, &g)))
        return rc;
    return f32_staged(c, src, src_stride, src_ch_pitch, src_w, src_h, dst, dst_stride, dst_ch_pitch, dst_w, dst_h, 3,
                      [&](const ImageRef &lo, const ImageRef &hi) {
                          return process_rgb_frames_dev(c, lo, src_w, src_h, hi, dst_w, dst_h, luma, g, clamp, 1);
                      });
}

#ifdef SRCNN_TUNING_BUILD
/* Undocumented test hooks (tuning build only, not part of the ABI) of the antialiased resize.  _form: 0 sends every later call of
 * this library to the general (two-launch) form, anything else gives the choice back to resample_aa_variant(); _last_form: the
 * form the last call ran (1 tiled, 0 general, -1 none yet); _variant: what resample_aa_variant() says for a geometry with its own
 * tables' tap counts (host only); _limits: AA_TR, AA_TC, AA_RATIO, AA_KMAX, AA_RMAX. */
int srcnn_debug_resample_aa_form(int form)
{
    g_aa_force_general = form == 0;
    return SRCNN_OK;
}

int srcnn_debug_resample_aa_last_form(void) { return g_aa_last_form; }

int srcnn_debug_resample_aa_variant(int sw, int sh, int dw, int dh)
{
    if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0) return SRCNN_ERR_INVALID;
    return resample_aa_variant(sw, sh, dw, dh, cubic_aa_f32_taps(sw, dw, nullptr, nullptr, nullptr, 0),
                               cubic_aa_f32_taps(sh, dh, nullptr, nullptr, nullptr, 0));
}

int srcnn_debug_resample_aa_limits(int *out5)
{
    if (!out5) return SRCNN_ERR_INVALID;
    const int v[5] = {AA_TR, AA_TC, AA_RATIO, AA_KMAX, AA_RMAX};
    for (int k = 0; k < 5; ++k) out5[k] = v[k];
    return SRCNN_OK;
}

/* ... and of Pillow's resize, the same three: _form (0: the general form for every later call, else the library's choice),
 * _last_form (1 tiled, 0 general, -1 none yet), _limits: PIL_TR, PIL_TC, PIL_HC, PIL_RATIO, PIL_KMAX, PIL_RMAX. */
int srcnn_debug_resample_pil_form(int form)
{
    g_pil_force_general = form == 0;
    return SRCNN_OK;
}

int srcnn_debug_resample_pil_last_form(void) { return g_pil_last_form; }

int srcnn_debug_resample_pil_limits(int *out6)
{
    if (!out6) return SRCNN_ERR_INVALID;
    const int v[6] = {PIL_TR, PIL_TC, PIL_HC, PIL_RATIO, PIL_KMAX, PIL_RMAX};
    for (int k = 0; k < 6; ++k) out6[k] = v[k];
    return SRCNN_OK;
}
#endif  /* SRCNN_TUNING_BUILD */

}  // extern "C"
