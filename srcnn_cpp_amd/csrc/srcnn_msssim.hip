// srcnn_msssim.hip -- MS-SSIM on two stored images (srcnn_msssim_image_dev): the per-scale sums of the contrast-structure term
// and of the SSIM of Wang, Simoncelli and Bovik 2003, on the channel planes or on a luma, with a border shaved off at scale 0.
// Semantics: include/srcnn_amd.h.  Geometry (MsssimPlan) and the launcher's type: srcnn_image.h.  Host layer: srcnn_image.cpp.
//
// Scale 0 is read where the pictures lie through image_load (srcnn_image.h), widened to float64 at once; scales >= 1 are
// packed float64 planes in the context's workspace, each made from the scale before it by msssim_pyramid_kernel.  This unit is
// built without FMA contraction: the luma, the 2 x 2 mean and the two formulas are the products and sums of the header, each
// rounded on its own.  The 11-tap window sums are the explicit fused multiply-adds of srcnn_metrics.hip (acc = g_0 v_0, then
// acc = fma(g_j, v_j, acc), j ascending), the same sequence for every one of the five quantities.
// A unit of its own: srcnn_metrics.hip holds exactly the three kernels of srcnn_metrics_image_dev and stays as it is.
//
// No floating-point atomic anywhere: a workgroup of msssim_window_kernel adds its lanes' two sums by a fixed tree in LDS and
// writes ONE partial of each, and msssim_finish_kernel adds a scale's partials by a fixed stride-256 pass and the same tree.
#include "srcnn_image.h"

namespace srcnn {
namespace {

enum { SRC_IMAGE = 0, SRC_LUMA = 1, SRC_PLANES = 2 };      // what a launch reads: uniform over it

// one launch of the pyramid or the window kernel: ONE scale of every plane
struct MsLevelArgs {
    ImageRef a, b;                 // SRC_IMAGE, SRC_LUMA: the region, element (0, 0) the first pixel inside the border
    const double *pa, *pb;         // SRC_PLANES: this scale's packed planes of result 0, `plane_pitch` doubles between results
    long plane_pitch;
    int sw, sh;                    // the size of the scale that is read
    int per_frame, n_planes;       // results per frame (1 with a luma, else the channel count), and per call
    float lw[4];                   // the luma row (SRC_LUMA)
    double g[METRIC_WIN];          // the window, normalised
    double c1, c2;
    int n_ct, n_bt, band;          // window kernel: column tiles and row bands of one plane at this scale, window rows of a band
    double *part;                  // ... its partials: [n_planes] x part_pitch, this scale's cs at 0 .., its ssim at n_ct n_bt ..
    long part_pitch;
    double *qa, *qb;               // pyramid kernel: the next scale's packed planes of result 0 (ceil(sw / 2) x ceil(sh / 2))
};

struct MsFinishArgs {
    int n_scales, n_planes;
    long n_part[MSSSIM_MAX_SCALES], part_off[MSSSIM_MAX_SCALES];      // partials of one sum of a scale; where its cs partials begin
    double n_win[MSSSIM_MAX_SCALES];
    const double *part;
    long part_pitch;
    double *out;                   // [n_planes][n_scales][3]
};

// where plane z of a stored image begins
__device__ __forceinline__ void image_plane_offsets(const MsLevelArgs &p, int z, bool luma, long *sa, long *sb)
{
    const int frame = z / p.per_frame, ch = luma ? 0 : z - frame * p.per_frame;
    *sa = frame * p.a.frame_pitch + ch * p.a.ch_pitch;
    *sb = frame * p.b.frame_pitch + ch * p.b.ch_pitch;
}

// One picture of one plane at the scale a launch reads: value(y, x) in float64.  SRC_IMAGE: the loaded element; SRC_LUMA:
// ((w0 c0 + w1 c1) + w2 c2) + offset; SRC_PLANES: the double of the packed plane.
template <int SRC>
struct MsSource {
    const ImageRef *im;
    const float *lw;
    const double *plane;
    long base, stride, px_step;
    __device__ __forceinline__ double at(int y, int x) const
    {
        const long o = base + (long)y * stride + (long)x * px_step;
        if (SRC == SRC_PLANES) return plane[o];
        if (SRC == SRC_IMAGE) return (double)image_load(*im, o);
        const double c0 = (double)image_load(*im, o), c1 = (double)image_load(*im, o + im->ch_pitch);
        const double c2 = (double)image_load(*im, o + 2 * im->ch_pitch);
        return (((double)lw[0] * c0 + (double)lw[1] * c1) + (double)lw[2] * c2) + (double)lw[3];
    }
};

template <int SRC>
__device__ __forceinline__ void ms_sources(const MsLevelArgs &p, int z, MsSource<SRC> *a, MsSource<SRC> *b)
{
    if (SRC == SRC_PLANES) {
        *a = MsSource<SRC>{nullptr, nullptr, p.pa, (long)z * p.plane_pitch, (long)p.sw, 1};
        *b = MsSource<SRC>{nullptr, nullptr, p.pb, (long)z * p.plane_pitch, (long)p.sw, 1};
    } else {
        long sa, sb;
        image_plane_offsets(p, z, SRC == SRC_LUMA, &sa, &sb);
        *a = MsSource<SRC>{&p.a, p.lw, nullptr, sa, p.a.stride, p.a.px_step};
        *b = MsSource<SRC>{&p.b, p.lw, nullptr, sb, p.b.stride, p.b.px_step};
    }
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

// ---- the pyramid: out(y, x) = ((p(2y, 2x) + p(2y, 2x+1)) + (p(2y+1, 2x) + p(2y+1, 2x+1))) * 0.25, odd ends paired with themselves ----
// A workgroup of 256 threads makes MSSSIM_PYR_ROWS rows x 64 columns of the next scale, of both pictures.
template <int SRC>
__device__ __forceinline__ void pyramid_tiles(const MsLevelArgs &p)
{
    const int ow = (p.sw + 1) / 2, oh = (p.sh + 1) / 2;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    if (x >= ow) return;
    const int x0 = 2 * x, x1 = min(2 * x + 1, p.sw - 1);
    const int n_rt = (oh + MSSSIM_PYR_ROWS - 1) / MSSSIM_PYR_ROWS;
    for (int z = blockIdx.z; z < p.n_planes; z += gridDim.z) {
        MsSource<SRC> a, b;
        ms_sources<SRC>(p, z, &a, &b);
        for (int rt = blockIdx.y; rt < n_rt; rt += gridDim.y) {
            const int y = rt * MSSSIM_PYR_ROWS + (threadIdx.x >> 6);
            if (y >= oh) continue;
            const int y0 = 2 * y, y1 = min(2 * y + 1, p.sh - 1);
            const double a00 = a.at(y0, x0), a01 = a.at(y0, x1), a10 = a.at(y1, x0), a11 = a.at(y1, x1);
            const double b00 = b.at(y0, x0), b01 = b.at(y0, x1), b10 = b.at(y1, x0), b11 = b.at(y1, x1);
            const long o = (long)z * p.plane_pitch + (long)y * ow + x;
            p.qa[o] = ((a00 + a01) + (a10 + a11)) * 0.25;
            p.qb[o] = ((b00 + b01) + (b10 + b11)) * 0.25;
        }
    }
}

__global__ __launch_bounds__(256) void msssim_pyramid_kernel(const MsLevelArgs p, int src)
{
    if (src == SRC_LUMA)
        pyramid_tiles<SRC_LUMA>(p);
    else if (src == SRC_PLANES)
        pyramid_tiles<SRC_PLANES>(p);
    else
        pyramid_tiles<SRC_IMAGE>(p);
}

// ---- the windows: one wave per workgroup, lane = source column, a register ring of 11 rows (metric_ssim_kernel's shape) ------
// acc = g_0 v_0, then fma(g_j, v_j, acc), j ascending
#define MSSSIM_TAPS(dst, expr)                                          \
    do {                                                                \
        { constexpr int j = 0; dst = p.g[0] * (expr); }                 \
        _Pragma("unroll") for (int j = 1; j < METRIC_WIN; ++j) dst = __builtin_fma(p.g[j], (expr), dst); \
    } while (0)

template <int SRC>
__device__ __forceinline__ void window_tiles(const MsLevelArgs &p, double (*vbuf)[64])
{
    const int lane = threadIdx.x;
    const int wc = p.sw - (METRIC_WIN - 1), wr = p.sh - (METRIC_WIN - 1);      // windows per row, per column
    const int ct = blockIdx.x;
    const int x = min(ct * MSSSIM_T + lane, p.sw - 1);      // (a clamped column feeds no counted window)
    const bool counted = lane < MSSSIM_T && ct * MSSSIM_T + lane < wc;
    const long n_tiles = (long)p.n_ct * p.n_bt;
    for (int z = blockIdx.z; z < p.n_planes; z += gridDim.z) {
        MsSource<SRC> a, b;
        ms_sources<SRC>(p, z, &a, &b);
        for (int bt = blockIdx.y; bt < p.n_bt; bt += gridDim.y) {
            const int r0 = bt * p.band;                                      // first window row = first source row of the band
            const int nrows = min(p.band, wr - r0) + (METRIC_WIN - 1);       // source rows r0 .. r0 + nrows - 1 <= sh - 1
            double ra[METRIC_WIN], rb[METRIC_WIN];
            double cs_sum = 0.0, ssim_sum = 0.0;
            // the row after the one being worked on is already on its way
            double na = a.at(r0, x), nb = b.at(r0, x);
            for (int base = 0; base < nrows; base += METRIC_WIN) {
#pragma unroll
                for (int k = 0; k < METRIC_WIN; ++k) {
                    const int r = base + k;      // (beyond the band's last row: the last row again, and nothing counted)
                    const int rn = r0 + min(r + 1, nrows - 1);
                    const double pa = a.at(rn, x), pb = b.at(rn, x);
                    ra[k] = na;
                    rb[k] = nb;
                    if (r >= METRIC_WIN - 1 && r < nrows) {
                        // rows r - 10 .. r lie in ring slots (k + 1) % 11 .. k: the five vertical sums of this lane's column
                        double va, vb, vaa, vbb, vab;
                        MSSSIM_TAPS(va, ra[(k + 1 + j) % METRIC_WIN]);
                        MSSSIM_TAPS(vb, rb[(k + 1 + j) % METRIC_WIN]);
                        MSSSIM_TAPS(vaa, ra[(k + 1 + j) % METRIC_WIN] * ra[(k + 1 + j) % METRIC_WIN]);
                        MSSSIM_TAPS(vbb, rb[(k + 1 + j) % METRIC_WIN] * rb[(k + 1 + j) % METRIC_WIN]);
                        MSSSIM_TAPS(vab, ra[(k + 1 + j) % METRIC_WIN] * rb[(k + 1 + j) % METRIC_WIN]);
                        vbuf[0][lane] = va;
                        vbuf[1][lane] = vb;
                        vbuf[2][lane] = vaa;
                        vbuf[3][lane] = vbb;
                        vbuf[4][lane] = vab;
                        __syncthreads();
                        if (counted) {      // lane + 10 <= 63
                            double ma, mb, eaa, ebb, eab;
                            MSSSIM_TAPS(ma, vbuf[0][lane + j]);
                            MSSSIM_TAPS(mb, vbuf[1][lane + j]);
                            MSSSIM_TAPS(eaa, vbuf[2][lane + j]);
                            MSSSIM_TAPS(ebb, vbuf[3][lane + j]);
                            MSSSIM_TAPS(eab, vbuf[4][lane + j]);
                            const double mab = ma * mb;
                            const double cs_num = 2.0 * (eab - mab) + p.c2;
                            const double cs_den = ((eaa - ma * ma) + (ebb - mb * mb)) + p.c2;
                            const double num = (2.0 * mab + p.c1) * cs_num;
                            const double den = ((ma * ma + mb * mb) + p.c1) * cs_den;
                            cs_sum = cs_sum + cs_num / cs_den;
                            ssim_sum = ssim_sum + num / den;
                        }
                        __syncthreads();      // the next row's sums overwrite what the lanes just read
                    }
                    na = pa;
                    nb = pb;
                }
            }
            const double cs_total = tree_sum<64>(vbuf[0], cs_sum);
            const double ssim_total = tree_sum<64>(vbuf[0], ssim_sum);
            if (lane == 0) {
                double *part = p.part + (long)z * p.part_pitch + (long)bt * p.n_ct + ct;
                part[0] = cs_total;
                part[n_tiles] = ssim_total;
            }
        }
    }
}

__global__ __launch_bounds__(64) void msssim_window_kernel(const MsLevelArgs p, int src)
{
    __shared__ double vbuf[5][64];
    if (src == SRC_LUMA)
        window_tiles<SRC_LUMA>(p, vbuf);
    else if (src == SRC_PLANES)
        window_tiles<SRC_PLANES>(p, vbuf);
    else
        window_tiles<SRC_IMAGE>(p, vbuf);
}

// ---- the finish: a scale's partials in a fixed order, and the 3 S doubles of a result --------------------------------------
__device__ __forceinline__ double partial_sum(const double *part, long n, double *red)
{
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) acc = acc + part[i];
    return tree_sum<256>(red, acc);
}

__global__ __launch_bounds__(256) void msssim_finish_kernel(const MsFinishArgs p)
{
    __shared__ double red[256];
    const int s = blockIdx.y;      // one workgroup per (result, scale)
    for (int z = blockIdx.x; z < p.n_planes; z += gridDim.x) {
        const double *part = p.part + (long)z * p.part_pitch + p.part_off[s];
        const double cs = partial_sum(part, p.n_part[s], red);
        const double ssim = partial_sum(part + p.n_part[s], p.n_part[s], red);
        if (threadIdx.x == 0) {
            double *o = p.out + ((long)z * p.n_scales + s) * 3;
            o[0] = cs;
            o[1] = ssim;
            o[2] = p.n_win[s];
        }
    }
}

unsigned grid_cap(long v) { return (unsigned)(v < 65535 ? v : 65535); }      // grid y and z: the kernels walk what lies beyond

hipError_t launch_msssim(const ImageRef &a, const ImageRef &b, int rw, int rh, int channels, int n_frames, const float *luma,
                         const double gauss[METRIC_WIN], double c1, double c2, int n_scales, double *planes, double *parts,
                         double *out, hipStream_t st)
{
    const int per_frame = luma ? 1 : channels;
    MsssimPlan plan;
    if ((channels != 1 && channels != 3) || (luma && channels != 3) || n_frames <= 0 || (long)per_frame * n_frames > 0x7fffffffL ||
        !msssim_plan(rw, rh, n_scales, &plan) || !parts || !out || !gauss || (n_scales > 1 && !planes))
        return hipErrorInvalidValue;
    MsLevelArgs p{};
    p.a = a;
    p.b = b;
    p.plane_pitch = plan.plane_doubles;
    p.per_frame = per_frame;
    p.n_planes = per_frame * n_frames;
    for (int k = 0; k < 4; ++k) p.lw[k] = luma ? luma[k] : 0.f;
    for (int k = 0; k < METRIC_WIN; ++k) p.g[k] = gauss[k];
    p.c1 = c1;
    p.c2 = c2;
    p.part_pitch = plan.part_doubles;
    const unsigned gz = grid_cap(p.n_planes);
    // picture a's planes of every result and scale lie first, picture b's after them
    double *planes_b = planes + (long)p.n_planes * plan.plane_doubles;
    for (int s = 0; s < n_scales; ++s) {
        const int src = s ? SRC_PLANES : luma ? SRC_LUMA : SRC_IMAGE;
        p.sw = plan.w[s];
        p.sh = plan.h[s];
        p.pa = s ? planes + plan.plane_off[s] : nullptr;
        p.pb = s ? planes_b + plan.plane_off[s] : nullptr;
        p.n_ct = (int)plan.n_ct[s];
        p.n_bt = (int)plan.n_bt[s];
        p.band = msssim_band(s);
        p.part = parts + plan.part_off[s];
        p.qa = p.qb = nullptr;
        if (s + 1 < n_scales) {
            p.qa = planes + plan.plane_off[s + 1];
            p.qb = planes_b + plan.plane_off[s + 1];
            const int ow = plan.w[s + 1], oh = plan.h[s + 1];
            hipLaunchKernelGGL(msssim_pyramid_kernel, dim3((unsigned)((ow + 63) / 64), grid_cap((oh + MSSSIM_PYR_ROWS - 1) / MSSSIM_PYR_ROWS), gz),
                               dim3(256), 0, st, p, src);
        }
        hipLaunchKernelGGL(msssim_window_kernel, dim3((unsigned)p.n_ct, grid_cap(p.n_bt), gz), dim3(64), 0, st, p, src);
    }
    MsFinishArgs f{};
    f.n_scales = n_scales;
    f.n_planes = p.n_planes;
    for (int s = 0; s < n_scales; ++s) {
        f.n_part[s] = plan.n_ct[s] * plan.n_bt[s];
        f.part_off[s] = plan.part_off[s];
        f.n_win[s] = (double)(plan.w[s] - (METRIC_WIN - 1)) * (double)(plan.h[s] - (METRIC_WIN - 1));
    }
    f.part = parts;
    f.part_pitch = plan.part_doubles;
    f.out = out;
    hipLaunchKernelGGL(msssim_finish_kernel, dim3(gz, (unsigned)n_scales), dim3(256), 0, st, f);
    return hipGetLastError();
}

}  // namespace

// the host layer's way to the launcher (srcnn_image.h): handed over once, when the library is loaded
__attribute__((constructor)) static void hand_over_msssim_launcher() { set_msssim_launcher(launch_msssim); }

}  // namespace srcnn
