// srcnn_metrics.hip -- full-reference quality metrics on two stored images (srcnn_metrics_image_dev): the sum of squared errors
// and the Gaussian-window SSIM of Wang et al. 2004, on the channel planes or on a luma, with a border shaved off.
// Semantics: include/srcnn_amd.h.  Tile geometry, partial counts and the launcher: srcnn_image.h.  Host layer: srcnn_image.cpp.
//
// Both pictures are read where they lie through image_load (srcnn_image.h), each value is widened to float64 at once, and
// everything after that is float64.  This unit is built without FMA contraction: the luma and the SSIM formula are the products
// and sums of the header, each rounded on its own, which is what makes identical pictures give exactly 1.0 per window and what
// makes the result symmetric in a and b.  The 11-tap window sums are written with explicit fused multiply-adds
// (acc = g_0 v_0, then acc = fma(g_j, v_j, acc) for j ascending): one rounding per tap, and the same sequence for every one of
// the five quantities, so E[a^2], E[b^2] and E[ab] of identical pictures are the same bits.
// A translation unit of its own because float64 division compiles to v_fma_f64, which srcnn_pipeline.hip must not contain.
//
// No floating-point atomic anywhere: a workgroup adds its threads' sums by a fixed tree in LDS and writes ONE partial, and
// metric_finish_kernel adds a plane's partials by a fixed stride-256 pass and the same tree.
#include "srcnn_image.h"

namespace srcnn {
namespace {

struct MetricArgs {
    ImageRef a, b;                 // the region: element (0, 0) is the first pixel inside the border
    int rw, rh;                    // its size
    int per_frame, n_planes;       // results per frame (1 with a luma, else the channel count), and per call
    float lw[4];                   // the luma row (LUMA kernels only)
    double g[METRIC_WIN];          // the window, normalised
    double c1, c2;
    int n_ct, n_bt;                // SSIM column tiles and row bands of one plane
    long n_sse, n_ssim;            // partials per plane
    double *sse_part, *ssim_part;  // [n_planes][n_sse], [n_planes][n_ssim]
    int flags;
    double *out;                   // [n_planes][4]
};

// the measured value of one pixel: the loaded element, or ((w0 c0 + w1 c1) + w2 c2) + offset in float64
template <bool LUMA>
__device__ __forceinline__ double metric_value(const ImageRef &im, long at, const MetricArgs &p)
{
    if (!LUMA) return (double)image_load(im, at);
    const double c0 = (double)image_load(im, at), c1 = (double)image_load(im, at + im.ch_pitch);
    const double c2 = (double)image_load(im, at + 2 * im.ch_pitch);
    return (((double)p.lw[0] * c0 + (double)p.lw[1] * c1) + (double)p.lw[2] * c2) + (double)p.lw[3];
}

// red[0] = ((red[0] + red[N/2]) + ...): the fixed tree every reduction of this unit uses; all N threads call it
template <int N>
__device__ __forceinline__ double tree_sum(double *red, double mine)
{
    const int t = threadIdx.x;
    red[t] = mine;
    __syncthreads();
#pragma unroll
    for (int o = N / 2; o > 0; o >>= 1) {
        if (t < o) red[t] = red[t] + red[t + o];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();          // the next use of `red` overwrites it
    return total;
}

__device__ __forceinline__ void plane_offsets(const MetricArgs &p, int z, bool luma, long *sa, long *sb)
{
    const int frame = z / p.per_frame, ch = luma ? 0 : z - frame * p.per_frame;
    *sa = frame * p.a.frame_pitch + ch * p.a.ch_pitch;
    *sb = frame * p.b.frame_pitch + ch * p.b.ch_pitch;
}

// ---- SSE: workgroup k of a plane takes rows [k METRIC_SSE_ROWS, ...), thread t the columns 4 t .. 4 t + 3, + 1024, ... --------
// Every thread adds its pixels in one order -- column group ascending, row ascending within it, column ascending within the row --
// whatever the stored format is.  VEC (both images planar float32, no luma) reads a thread's four columns of a row in one
// 16-byte load (global loads need the alignment of a float only); the other formats read them one by one: the same values in
// the same order, so the sum does not depend on how a picture is stored.  All loads of a column group are issued before the
// first is used: rows and columns beyond the region are clamped to its last ones and their terms replaced by +0.0, which
// leaves a non-negative sum as it is.
struct __attribute__((packed, aligned(4))) F32x4U {
    float v[4];
};

template <bool LUMA, bool VEC>
__device__ __forceinline__ void sse_rows(const MetricArgs &p, double *red)
{
    const int t = threadIdx.x;
    const long k = blockIdx.x;
    const int y0 = (int)(k * METRIC_SSE_ROWS);
    for (int z = blockIdx.z; z < p.n_planes; z += gridDim.z) {
        long sa, sb;
        plane_offsets(p, z, LUMA, &sa, &sb);
        double acc = 0.0;
        for (int x = 4 * t; x < p.rw; x += 4 * 256) {
            double va[METRIC_SSE_ROWS][4], vb[METRIC_SSE_ROWS][4];
            if (VEC && x + 3 < p.rw) {
#pragma unroll
                for (int r = 0; r < METRIC_SSE_ROWS; ++r) {
                    const int y = min(y0 + r, p.rh - 1);
                    const F32x4U qa = *reinterpret_cast<const F32x4U *>(static_cast<const float *>(p.a.data) + sa + (long)y * p.a.stride + x);
                    const F32x4U qb = *reinterpret_cast<const F32x4U *>(static_cast<const float *>(p.b.data) + sb + (long)y * p.b.stride + x);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        va[r][e] = (double)qa.v[e];
                        vb[r][e] = (double)qb.v[e];
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < METRIC_SSE_ROWS; ++r) {
                    const int y = min(y0 + r, p.rh - 1);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int xe = min(x + e, p.rw - 1);
                        va[r][e] = metric_value<LUMA>(p.a, sa + (long)y * p.a.stride + (long)xe * p.a.px_step, p);
                        vb[r][e] = metric_value<LUMA>(p.b, sb + (long)y * p.b.stride + (long)xe * p.b.px_step, p);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < METRIC_SSE_ROWS; ++r) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double d = va[r][e] - vb[r][e];
                    acc = acc + ((y0 + r < p.rh && x + e < p.rw) ? d * d : 0.0);
                }
            }
        }
        const double total = tree_sum<256>(red, acc);
        if (t == 0) p.sse_part[(long)z * p.n_sse + k] = total;
    }
}

// form: 0 the element-wise loads, 1 with a luma, 2 VEC
__global__ __launch_bounds__(256) void metric_sse_kernel(const MetricArgs p, int form)
{
    __shared__ double red[256];
    if (form == 1)
        sse_rows<true, false>(p, red);
    else if (form == 2)
        sse_rows<false, true>(p, red);
    else
        sse_rows<false, false>(p, red);
}

// ---- SSIM: one wave per workgroup, lane = source column, a register ring of 11 rows --------------------------------------
// acc = g_0 v_0, then fma(g_j, v_j, acc), j ascending
#define METRIC_TAPS(dst, expr)                                          \
    do {                                                                \
        { constexpr int j = 0; dst = p.g[0] * (expr); }                 \
        _Pragma("unroll") for (int j = 1; j < METRIC_WIN; ++j) dst = __builtin_fma(p.g[j], (expr), dst); \
    } while (0)

template <bool LUMA>
__device__ __forceinline__ void ssim_tiles(const MetricArgs &p, double (*vbuf)[64])
{
    const int lane = threadIdx.x;
    const int wc = p.rw - (METRIC_WIN - 1), wr = p.rh - (METRIC_WIN - 1);      // windows per row, per column
    const int ct = blockIdx.x;
    const int x = min(ct * METRIC_T + lane, p.rw - 1);      // (a clamped column feeds no counted window)
    const bool counted = lane < METRIC_T && ct * METRIC_T + lane < wc;
    for (int z = blockIdx.z; z < p.n_planes; z += gridDim.z) {
        long sa, sb;
        plane_offsets(p, z, LUMA, &sa, &sb);
        const long ca = sa + (long)x * p.a.px_step, cb = sb + (long)x * p.b.px_step;
        for (int bt = blockIdx.y; bt < p.n_bt; bt += gridDim.y) {
            const int r0 = bt * METRIC_B;                                    // first window row = first source row of the band
            const int nrows = min(METRIC_B, wr - r0) + (METRIC_WIN - 1);     // source rows r0 .. r0 + nrows - 1 <= rh - 1
            double ra[METRIC_WIN], rb[METRIC_WIN];
            double sum = 0.0;
            // the row after the one being worked on is already on its way
            double na = metric_value<LUMA>(p.a, ca + (long)r0 * p.a.stride, p);
            double nb = metric_value<LUMA>(p.b, cb + (long)r0 * p.b.stride, p);
            for (int base = 0; base < nrows; base += METRIC_WIN) {
#pragma unroll
                for (int k = 0; k < METRIC_WIN; ++k) {
                    const int r = base + k;      // (beyond the band's last row: the last row again, and nothing counted)
                    const int rn = r0 + min(r + 1, nrows - 1);
                    const double pa = metric_value<LUMA>(p.a, ca + (long)rn * p.a.stride, p);
                    const double pb = metric_value<LUMA>(p.b, cb + (long)rn * p.b.stride, p);
                    ra[k] = na;
                    rb[k] = nb;
                    if (r >= METRIC_WIN - 1 && r < nrows) {
                        // rows r - 10 .. r lie in ring slots (k + 1) % 11 .. k: the five vertical sums of this lane's column
                        double va, vb, vaa, vbb, vab;
                        METRIC_TAPS(va, ra[(k + 1 + j) % METRIC_WIN]);
                        METRIC_TAPS(vb, rb[(k + 1 + j) % METRIC_WIN]);
                        METRIC_TAPS(vaa, ra[(k + 1 + j) % METRIC_WIN] * ra[(k + 1 + j) % METRIC_WIN]);
                        METRIC_TAPS(vbb, rb[(k + 1 + j) % METRIC_WIN] * rb[(k + 1 + j) % METRIC_WIN]);
                        METRIC_TAPS(vab, ra[(k + 1 + j) % METRIC_WIN] * rb[(k + 1 + j) % METRIC_WIN]);
                        vbuf[0][lane] = va;
                        vbuf[1][lane] = vb;
                        vbuf[2][lane] = vaa;
                        vbuf[3][lane] = vbb;
                        vbuf[4][lane] = vab;
                        __syncthreads();
                        if (counted) {      // lane + 10 <= 63
                            double ma, mb, eaa, ebb, eab;
                            METRIC_TAPS(ma, vbuf[0][lane + j]);
                            METRIC_TAPS(mb, vbuf[1][lane + j]);
                            METRIC_TAPS(eaa, vbuf[2][lane + j]);
                            METRIC_TAPS(ebb, vbuf[3][lane + j]);
                            METRIC_TAPS(eab, vbuf[4][lane + j]);
                            const double mab = ma * mb;
                            const double num = (2.0 * mab + p.c1) * (2.0 * (eab - mab) + p.c2);
                            const double den = ((ma * ma + mb * mb) + p.c1) * (((eaa - ma * ma) + (ebb - mb * mb)) + p.c2);
                            sum = sum + num / den;
                        }
                        __syncthreads();      // the next row's sums overwrite what the lanes just read
                    }
                    na = pa;
                    nb = pb;
                }
            }
            const double total = tree_sum<64>(vbuf[0], sum);
            if (lane == 0) p.ssim_part[(long)z * p.n_ssim + (long)bt * p.n_ct + ct] = total;
        }
    }
}

__global__ __launch_bounds__(64) void metric_ssim_kernel(const MetricArgs p, int luma)
{
    __shared__ double vbuf[5][64];
    if (luma)
        ssim_tiles<true>(p, vbuf);
    else
        ssim_tiles<false>(p, vbuf);
}

// ---- the finish: a plane's partials in a fixed order, and the four doubles of the plane ---------------------------------
__device__ __forceinline__ double partial_sum(const double *part, long n, double *red)
{
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) acc = acc + part[i];
    return tree_sum<256>(red, acc);
}

__global__ __launch_bounds__(256) void metric_finish_kernel(const MetricArgs p)
{
    __shared__ double red[256];
    for (int z = blockIdx.x; z < p.n_planes; z += gridDim.x) {
        double sse = 0.0, n_px = 0.0, ssim = 0.0, n_win = 0.0;
        if (p.flags & METRIC_FLAG_SSE) {
            sse = partial_sum(p.sse_part + (long)z * p.n_sse, p.n_sse, red);
            n_px = (double)p.rw * (double)p.rh;
        }
        if (p.flags & METRIC_FLAG_SSIM) {
            ssim = partial_sum(p.ssim_part + (long)z * p.n_ssim, p.n_ssim, red);
            n_win = (double)(p.rw - (METRIC_WIN - 1)) * (double)(p.rh - (METRIC_WIN - 1));
        }
        if (threadIdx.x == 0) {
            double *o = p.out + 4 * (long)z;
            o[0] = sse;
            o[1] = n_px;
            o[2] = ssim;
            o[3] = n_win;
        }
    }
}

unsigned metric_grid_cap(long v) { return (unsigned)(v < 65535 ? v : 65535); }      // grid y and z: the kernels walk what lies beyond

}  // namespace

hipError_t launch_metrics(const ImageRef &a, const ImageRef &b, int rw, int rh, int channels, int n_frames, const float *luma,
                          const double gauss[METRIC_WIN], double c1, double c2, int flags, double *work, double *out, hipStream_t st)
{
    const int per_frame = luma ? 1 : channels;
    if (rw <= 0 || rh <= 0 || (channels != 1 && channels != 3) || (luma && channels != 3) || n_frames <= 0 ||
        (long)per_frame * n_frames > 0x7fffffffL || !flags || (flags & ~(METRIC_FLAG_SSE | METRIC_FLAG_SSIM)) || !work || !out || !gauss)
        return hipErrorInvalidValue;
    MetricArgs p{};
    p.a = a;
    p.b = b;
    p.rw = rw;
    p.rh = rh;
    p.per_frame = per_frame;
    p.n_planes = per_frame * n_frames;
    for (int k = 0; k < 4; ++k) p.lw[k] = luma ? luma[k] : 0.f;
    for (int k = 0; k < METRIC_WIN; ++k) p.g[k] = gauss[k];
    p.c1 = c1;
    p.c2 = c2;
    p.n_sse = (flags & METRIC_FLAG_SSE) ? metric_sse_partials(rh) : 0;
    p.n_ssim = (flags & METRIC_FLAG_SSIM) ? metric_ssim_partials(rw, rh) : 0;
    if ((flags & METRIC_FLAG_SSIM) && p.n_ssim == 0) return hipErrorInvalidValue;      // no window fits
    if (p.n_ssim) {
        p.n_ct = (rw - METRIC_WIN + 1 + METRIC_T - 1) / METRIC_T;
        p.n_bt = (rh - METRIC_WIN + 1 + METRIC_B - 1) / METRIC_B;
    }
    p.sse_part = work;
    p.ssim_part = work + (long)p.n_planes * p.n_sse;
    p.flags = flags;
    p.out = out;
    const unsigned gz = metric_grid_cap(p.n_planes);
    const bool vec = !luma && image_is_planar_f32(a) && image_is_planar_f32(b);
    if (p.n_sse) hipLaunchKernelGGL(metric_sse_kernel, dim3((unsigned)p.n_sse, 1, gz), dim3(256), 0, st, p, luma ? 1 : vec ? 2 : 0);
    if (p.n_ssim)
        hipLaunchKernelGGL(metric_ssim_kernel, dim3((unsigned)p.n_ct, metric_grid_cap(p.n_bt), gz), dim3(64), 0, st, p, luma ? 1 : 0);
    hipLaunchKernelGGL(metric_finish_kernel, dim3(gz), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace srcnn
