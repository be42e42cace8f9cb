// srcnn_pipeline.hip -- the steps either side of the conv path in the
// reference's pipeline driver, as HBM-bound
// byte kernels:
//   cvtColor BGR->YCrCb + split     src/srcnn.cpp:509,540
//   resize INTER_CUBIC (3 planes)   src/srcnn.cpp:568-583
//   merge + cvtColor YCrCb->BGR     src/srcnn.cpp:639,657
// The arithmetic is OpenCV 4.x's 8-bit integer definition (fixed-point colour
// coefficients, 11-bit cubic coefficients, (sum + 2^21) >> 22), restated in
// oracle/opencv_steps.c; it is integer work, so the kernels are bit-exact
// against that restatement.  One byte in, one byte out per element: no reuse,
// no LDS, consecutive lanes on consecutive bytes.
// At the end of the file: the cubic resize of float32 planes, torch's bicubic
// (srcnn_resize_cubic_f32*, the step in front of the float image path), and the
// two kernels of srcnn_process_rgb_f32* built from its tile; then the accessor
// forms of those four kernels for images as they are stored (srcnn_*_image_dev).
#include "srcnn_image.h"

// No FMA contraction anywhere in this file (also given on the command line, srcnn_cpp_amd/build.py): the vertical pass of
// the resize reproduces OpenCV's separately rounded float32 products and sums.
#pragma clang fp contract(off)

namespace srcnn {

__device__ __forceinline__ int descale14(int x) { return (x + (1 << 13)) >> 14; }
__device__ __forceinline__ uint8_t sat8(int v) { return (uint8_t)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void bgr2ycrcb_kernel(const uint8_t *__restrict__ bgr, long stride, int w, int h,
                                                        uint8_t *__restrict__ planes, long pstride, long ppitch)
{
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c >= w || r >= h) return;
    const uint8_t *p = bgr + (long)r * stride + 3L * c;
    const int B = p[0], G = p[1], R = p[2];
    const int Y = descale14(B * 1868 + G * 9617 + R * 4899);
    const long o = (long)r * pstride + c;
    planes[o] = sat8(Y);
    planes[ppitch + o] = sat8(descale14((R - Y) * 11682 + (128 << 14)));
    planes[2 * ppitch + o] = sat8(descale14((B - Y) * 9241 + (128 << 14)));
}

__global__ __launch_bounds__(256) void ycrcb2bgr_kernel(const uint8_t *__restrict__ yp, long ystride,
                                                        const uint8_t *__restrict__ crcb, long pstride, long ppitch,
                                                        int w, int h, uint8_t *__restrict__ bgr, long stride)
{
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c >= w || r >= h) return;
    const int Y = yp[(long)r * ystride + c];
    const long o = (long)r * pstride + c;
    const int Cr = crcb[o] - 128, Cb = crcb[ppitch + o] - 128;
    uint8_t *p = bgr + (long)r * stride + 3L * c;
    p[0] = sat8(Y + descale14(Cb * 29049));
    p[1] = sat8(Y + descale14(Cb * -5636 + Cr * -11698));
    p[2] = sat8(Y + descale14(Cr * 22987));
}

// Vertical pass of cv::resize(INTER_CUBIC), 8-bit (OpenCV 4.x modules/imgproc/src/resize.cpp, x86 baseline build).
// h0..h3 are the int sums of the horizontal pass for the four source rows, b0..b3 the 11-bit row coefficients.
// Columns below dw - dw % 8 go through the SIMD functor VResizeCubicVec_32s8u, which works in float32:
//   r = h3*(b3*2^-22);  r = h2*(b2*2^-22) + r;  r = h1*(b1*2^-22) + r;  r = h0*(b0*2^-22) + r
// with every product and every sum rounded on its own (the SSE baseline's v_muladd is mul + add: no contraction
// here either), then round-to-nearest-even and saturate; the remaining dw % 8 columns take the scalar fixed-point
// cast (sum + 2^21) >> 22.  This is the variant that reproduces the reference's published picture bit for bit
// (oracle/opencv_steps.c, tests/test_pipeline_oracle.py).
__device__ __forceinline__ unsigned vresize_px(int h0, int h1, int h2, int h3, int b0, int b1, int b2, int b3, bool simd)
{
    if (simd) {
        const float sc = 1.0f / (2048.0f * 2048.0f);
        float r = __fmul_rn((float)h3, (float)b3 * sc);
        r = __fadd_rn(__fmul_rn((float)h2, (float)b2 * sc), r);
        r = __fadd_rn(__fmul_rn((float)h1, (float)b1 * sc), r);
        r = __fadd_rn(__fmul_rn((float)h0, (float)b0 * sc), r);
        return sat8(__float2int_rn(r));
    }
    return sat8((h0 * b0 + h1 * b1 + h2 * b2 + h3 * b3 + (1 << 21)) >> 22);
}

// dst(dy,dx) = vresize_px( sum_kx alpha[dx][kx] * src[clamp(yofs[dy]-1+ky)][clamp(xofs[dx]-1+kx)], beta[dy][ky] );
// blockIdx.z = plane
__global__ __launch_bounds__(256) void resize_cubic_kernel(const uint8_t *__restrict__ src, long sstride, long spitch,
                                                           int sw, int sh, uint8_t *__restrict__ dst, long dstride,
                                                           long dpitch, int dw, int dh,
                                                           const int *__restrict__ xofs, const short *__restrict__ alpha,
                                                           const int *__restrict__ yofs, const short *__restrict__ beta)
{
    const int dx = blockIdx.x * 256 + threadIdx.x, dy = blockIdx.y;
    if (dx >= dw || dy >= dh) return;
    const uint8_t *s = src + (long)blockIdx.z * spitch;
    const int x0 = xofs[dx] - 1, y0 = yofs[dy] - 1;
    int a[4], xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a[k] = alpha[4 * dx + k];
        xs[k] = min(max(x0 + k, 0), sw - 1);
    }
    int hs[4];
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
        const uint8_t *row = s + (long)min(max(y0 + ky, 0), sh - 1) * sstride;
        int t = 0;
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) t += row[xs[kx]] * a[kx];
        hs[ky] = t;
    }
    const short *b = beta + 4 * dy;
    dst[(long)blockIdx.z * dpitch + (long)dy * dstride + dx] =
        (uint8_t)vresize_px(hs[0], hs[1], hs[2], hs[3], b[0], b[1], b[2], b[3], dx < dw - dw % 8);
}

// Tiled variant for up-scaling (and mild down-scaling): a workgroup produces RT output rows x 256
// columns.  The horizontal pass of every source row the tile touches is done ONCE into LDS (as the
// int sums OpenCV's HResize produces), the vertical pass then reads LDS: ~4 byte loads per output
// pixel instead of 16.  Same integer arithmetic, bit-identical results.
// (RT = 8 output rows per workgroup from at most RMAX = 16 source rows x SMAX = 288 source columns: srcnn_kernels.h, where
// resize_variant() checks a geometry against them before this kernel is chosen)

__global__ __launch_bounds__(256) void resize_cubic_tiled_kernel(const uint8_t *__restrict__ src, long sstride,
                                                                 long spitch, int sw, int sh,
                                                                 uint8_t *__restrict__ dst, long dstride, long dpitch,
                                                                 int dw, int dh, const int *__restrict__ xofs,
                                                                 const short *__restrict__ alpha,
                                                                 const int *__restrict__ yofs,
                                                                 const short *__restrict__ beta)
{
    __shared__ int hbuf[RMAX][256];
    __shared__ uint8_t sbuf[RMAX][SMAX];   // the source rows of the tile (replicate border applied), bytes
    const int dx0 = blockIdx.x * 256, dx = dx0 + threadIdx.x;
    const int dy0 = blockIdx.y * RT, dy1 = min(dy0 + RT, dh);
    const uint8_t *s = src + (long)blockIdx.z * spitch;
    const int r_lo = yofs[dy0] - 1, r_hi = yofs[dy1 - 1] + 2;     // unclamped source rows of this tile
    const int c_lo = xofs[dx0] - 1, c_hi = xofs[min(dx0 + 255, dw - 1)] + 2;   // ... and columns
    const int ncol = c_hi - c_lo + 1, nrow = r_hi - r_lo + 1;
    // stage: consecutive lanes fetch consecutive source bytes of a row
    for (int e = threadIdx.x; e < nrow * ncol; e += 256) {
        const int rr = e / ncol, cc = e - rr * ncol;
        sbuf[rr][cc] = s[(long)min(max(r_lo + rr, 0), sh - 1) * sstride + min(max(c_lo + cc, 0), sw - 1)];
    }
    __syncthreads();
    const int dxc = min(dx, dw - 1);
    const int x0 = xofs[dxc] - 1 - c_lo;
    int a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = alpha[4 * dxc + k];
    for (int rr = 0; rr < nrow; ++rr) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) t += sbuf[rr][x0 + k] * a[k];
        hbuf[rr][threadIdx.x] = t;
    }
    // every thread only reads back its own hbuf column: no second barrier needed
    if (dx >= dw) return;
    for (int dy = dy0; dy < dy1; ++dy) {
        const int j = yofs[dy] - 1 - r_lo;
        const short *b = beta + 4 * dy;
        dst[(long)blockIdx.z * dpitch + (long)dy * dstride + dx] =
            (uint8_t)vresize_px(hbuf[j][threadIdx.x], hbuf[j + 1][threadIdx.x], hbuf[j + 2][threadIdx.x],
                                hbuf[j + 3][threadIdx.x], b[0], b[1], b[2], b[3], dx < dw - dw % 8);
    }
}

// vertical pass of output row dy, columns dx .. dx+3 (thread tx of the tile), packed one byte per pixel.
// hbuf holds the horizontal sums as floats (exact); see vresize_px() for the two arithmetic variants.
__device__ __forceinline__ unsigned vpass4(const float (*hbuf)[256], int tx, int j, const short *__restrict__ b, int dx, int dw)
{
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = *reinterpret_cast<const f32x4 *>(&hbuf[j + k][4 * tx]);
    unsigned r = 0;
    if (dx + 3 < dw - dw % 8) {            // all four columns in the SIMD functor's range: float32, every product and sum rounded
        const float sc = 1.0f / (2048.0f * 2048.0f);
        const float b0 = (float)b[0] * sc, b1 = (float)b[1] * sc, b2 = (float)b[2] * sc, b3 = (float)b[3] * sc;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v = __fmul_rn(h[3][c], b3);
            v = __fadd_rn(__fmul_rn(h[2][c], b2), v);
            v = __fadd_rn(__fmul_rn(h[1][c], b1), v);
            v = __fadd_rn(__fmul_rn(h[0][c], b0), v);
            r |= (unsigned)sat8(__float2int_rn(v)) << (8 * c);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            r |= vresize_px((int)h[0][c], (int)h[1][c], (int)h[2][c], (int)h[3][c], b[0], b[1], b[2], b[3], dx + c < dw - dw % 8) << (8 * c);
    }
    return r;
}

// Second tiling: a workgroup produces a 256 x 32 output tile and every thread FOUR adjacent pixels of 8 rows, so
// the vertical pass reads its taps as one 16-byte LDS word per row and stores one dword per row: a quarter of the
// store and LDS instructions of the kernel above (which remains the fallback for small scales / odd strides).
// Same arithmetic, bit-identical results.
// (RT4 = 32 rows, RPT = 8 per thread, at most RMAX4 = 28 source rows: srcnn_kernels.h, resize_variant())

__global__ __launch_bounds__(256) void resize_cubic_tiled4_kernel(const uint8_t *__restrict__ src, long sstride,
                                                                  long spitch, int sw, int sh,
                                                                  uint8_t *__restrict__ dst, long dstride, long dpitch,
                                                                  int dw, int dh, const int *__restrict__ xofs,
                                                                  const short *__restrict__ alpha,
                                                                  const int *__restrict__ yofs,
                                                                  const short *__restrict__ beta)
{
    __shared__ __attribute__((aligned(16))) float hbuf[RMAX4][256];
    __shared__ uint8_t sbuf[RMAX4][SMAX];
    const int tid = threadIdx.x;
    const int dx0 = blockIdx.x * 256;
    const int dy0 = blockIdx.y * RT4, dy1 = min(dy0 + RT4, dh);
    const uint8_t *s = src + (long)blockIdx.z * spitch;
    const int r_lo = yofs[dy0] - 1, r_hi = yofs[dy1 - 1] + 2;
    const int c_lo = xofs[dx0] - 1, c_hi = xofs[min(dx0 + 255, dw - 1)] + 2;
    const int ncol = c_hi - c_lo + 1, nrow = r_hi - r_lo + 1;
    for (int e = tid; e < nrow * ncol; e += 256) {
        const int rr = e / ncol, cc = e - rr * ncol;
        sbuf[rr][cc] = s[(long)min(max(r_lo + rr, 0), sh - 1) * sstride + min(max(c_lo + cc, 0), sw - 1)];
    }
    __syncthreads();
    {   // horizontal pass: thread = output column, all source rows of the tile
        const int dxc = min(dx0 + tid, dw - 1);
        const int x0 = xofs[dxc] - 1 - c_lo;
        int a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = alpha[4 * dxc + k];
        for (int rr = 0; rr < nrow; ++rr) {
            int t = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) t += sbuf[rr][x0 + k] * a[k];
            hbuf[rr][tid] = (float)t;      // exact (|t| < 2^24)
        }
    }
    __syncthreads();
    // vertical pass: thread (tx, ty) = columns 4tx..4tx+3 of rows dy0 + 8ty .. +7
    const int tx = tid & 63, ty = tid >> 6;
    const int dx = dx0 + 4 * tx;
    if (dx >= dw) return;
    for (int r = 0; r < RPT; ++r) {
        const int dy = dy0 + RPT * ty + r;
        if (dy >= dy1) break;
        const unsigned v = vpass4(hbuf, tx, yofs[dy] - 1 - r_lo, beta + 4 * dy, dx, dw);
        uint8_t *o = dst + (long)blockIdx.z * dpitch + (long)dy * dstride + dx;
        if (dx + 3 < dw) *reinterpret_cast<unsigned *>(o) = v;
        else
            for (int c = 0; c < 4 && dx + c < dw; ++c) o[c] = (uint8_t)(v >> (8 * c));
    }
}

// ---- the whole pipeline step in two launches (srcnn_process_bgr[_dev]) ------------------------------------------
// cvtColor + split + 3 x resize + (conv path) + merge + cvtColor as the reference runs them (src/srcnn.cpp:509-657) touch
// every plane twice more than needed: the low-resolution Y / Cr / Cb planes only feed the resize, the resized Cr / Cb only
// the final conversion.  bgr_to_y_resized_kernel converts while it stages its source tile (BGR in, up-sampled Y out);
// resize_merge_kernel does the same for Cr and Cb and turns them, with the conv path's Y, straight into BGR.  The
// arithmetic per value is that of the three separate kernels above -- bit-identical -- in the tiled4 layout
// (256 x 32 output tile per workgroup, four adjacent pixels of eight rows per thread).
__device__ __forceinline__ int bgr_to_comp(const uint8_t *px, int comp)
{
    const int B = px[0], G = px[1], R = px[2];
    const int Y = descale14(B * 1868 + G * 9617 + R * 4899);
    if (comp == 0) return sat8(Y);
    if (comp == 1) return sat8(descale14((R - Y) * 11682 + (128 << 14)));
    return sat8(descale14((B - Y) * 9241 + (128 << 14)));
}

struct TileGeom {
    int dx0, dy0, dy1, r_lo, c_lo, ncol, nrow;
};

// stage component `comp` of the BGR source tile into sbuf, horizontal pass into hbuf (both barriers included)
__device__ __forceinline__ void stage_and_hpass(const uint8_t *__restrict__ bgr, long stride, int sw, int sh, int dw, int comp,
                                                const TileGeom &g, const int *__restrict__ xofs,
                                                const short *__restrict__ alpha, uint8_t (*sbuf)[SMAX], float (*hbuf)[256])
{
    const int tid = threadIdx.x;
    for (int e = tid; e < g.nrow * g.ncol; e += 256) {
        const int rr = e / g.ncol, cc = e - rr * g.ncol;
        sbuf[rr][cc] = (uint8_t)bgr_to_comp(bgr + (long)min(max(g.r_lo + rr, 0), sh - 1) * stride + 3L * min(max(g.c_lo + cc, 0), sw - 1), comp);
    }
    __syncthreads();
    const int dxc = min(g.dx0 + tid, dw - 1);
    const int x0 = xofs[dxc] - 1 - g.c_lo;
    int a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = alpha[4 * dxc + k];
    for (int rr = 0; rr < g.nrow; ++rr) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) t += sbuf[rr][x0 + k] * a[k];
        hbuf[rr][tid] = (float)t;          // |t| < 2^24: exact; converted once per source row instead of once per output row
    }
    __syncthreads();
}

__device__ __forceinline__ TileGeom tile_geom(int dw, int dh, const int *__restrict__ xofs, const int *__restrict__ yofs)
{
    TileGeom g;
    g.dx0 = blockIdx.x * 256;
    g.dy0 = blockIdx.y * RT4;
    g.dy1 = min(g.dy0 + RT4, dh);
    g.r_lo = yofs[g.dy0] - 1;
    g.c_lo = xofs[g.dx0] - 1;
    g.ncol = xofs[min(g.dx0 + 255, dw - 1)] + 2 - g.c_lo + 1;
    g.nrow = yofs[g.dy1 - 1] + 2 - g.r_lo + 1;
    return g;
}

__global__ __launch_bounds__(256) void bgr_to_y_resized_kernel(const uint8_t *__restrict__ bgr, long stride, int sw, int sh,
                                                               uint8_t *__restrict__ dst, long dstride, int dw, int dh,
                                                               const int *__restrict__ xofs, const short *__restrict__ alpha,
                                                               const int *__restrict__ yofs, const short *__restrict__ beta)
{
    __shared__ __attribute__((aligned(16))) float hbuf[RMAX4][256];
    __shared__ uint8_t sbuf[RMAX4][SMAX];
    const TileGeom g = tile_geom(dw, dh, xofs, yofs);
    stage_and_hpass(bgr, stride, sw, sh, dw, 0, g, xofs, alpha, sbuf, hbuf);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, dx = g.dx0 + 4 * tx;
    if (dx >= dw) return;
    for (int r = 0; r < RPT; ++r) {
        const int dy = g.dy0 + RPT * ty + r;
        if (dy >= g.dy1) break;
        const unsigned v = vpass4(hbuf, tx, yofs[dy] - 1 - g.r_lo, beta + 4 * dy, dx, dw);
        uint8_t *o = dst + (long)dy * dstride + dx;
        if (dx + 3 < dw) *reinterpret_cast<unsigned *>(o) = v;
        else
            for (int c = 0; c < 4 && dx + c < dw; ++c) o[c] = (uint8_t)(v >> (8 * c));
    }
}

__global__ __launch_bounds__(256) void resize_merge_kernel(const uint8_t *__restrict__ bgr, long stride, int sw, int sh,
                                                           const uint8_t *__restrict__ ysr, long ystride,
                                                           uint8_t *__restrict__ out, long ostride, int dw, int dh,
                                                           const int *__restrict__ xofs, const short *__restrict__ alpha,
                                                           const int *__restrict__ yofs, const short *__restrict__ beta)
{
    __shared__ __attribute__((aligned(16))) float hbuf[RMAX4][256];
    __shared__ uint8_t sbuf[RMAX4][SMAX];
    const TileGeom g = tile_geom(dw, dh, xofs, yofs);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, dx = g.dx0 + 4 * tx;
    unsigned crcb[2][RPT];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        if (pl) __syncthreads();            // every thread has finished reading plane 0's sums
        stage_and_hpass(bgr, stride, sw, sh, dw, 1 + pl, g, xofs, alpha, sbuf, hbuf);
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int dy = min(g.dy0 + RPT * ty + r, g.dy1 - 1);
            crcb[pl][r] = vpass4(hbuf, tx, yofs[dy] - 1 - g.r_lo, beta + 4 * dy, min(dx, dw - 1), dw);
        }
    }
    if (dx >= dw) return;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int dy = g.dy0 + RPT * ty + r;
        if (dy >= g.dy1) break;
        const uint8_t *yrow = ysr + (long)dy * ystride + dx;
        uint8_t *o = out + (long)dy * ostride + 3L * dx;
        const bool vec = dx + 3 < dw;
        unsigned yv = 0;
        if (vec) yv = *reinterpret_cast<const unsigned *>(yrow);
        else
            for (int c = 0; c < 4 && dx + c < dw; ++c) yv |= (unsigned)yrow[c] << (8 * c);
        uint8_t px[12];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int Y = (yv >> (8 * c)) & 255, Cr = (int)((crcb[0][r] >> (8 * c)) & 255) - 128,
                      Cb = (int)((crcb[1][r] >> (8 * c)) & 255) - 128;
            px[3 * c + 0] = sat8(Y + descale14(Cb * 29049));
            px[3 * c + 1] = sat8(Y + descale14(Cb * -5636 + Cr * -11698));
            px[3 * c + 2] = sat8(Y + descale14(Cr * 22987));
        }
        if (vec) {
            unsigned *o4 = reinterpret_cast<unsigned *>(o);
#pragma unroll
            for (int q = 0; q < 3; ++q)
                o4[q] = px[4 * q] | (px[4 * q + 1] << 8) | (px[4 * q + 2] << 16) | ((unsigned)px[4 * q + 3] << 24);
        } else {
            for (int c = 0; c < 4 && dx + c < dw; ++c)
                for (int q = 0; q < 3; ++q) o[3 * c + q] = px[3 * c + q];
        }
    }
}

// true when the two fused launches apply (the tiled4 geometry limits, dword-aligned rows)
bool fused_pipeline_ok(int sw, int sh, int dw, int dh, const void *y_hi, long ystride, const void *out, long ostride)
{
    const bool aligned = ((reinterpret_cast<uintptr_t>(y_hi) | (uintptr_t)ystride | reinterpret_cast<uintptr_t>(out) | (uintptr_t)ostride) & 3) == 0;
    return resize_variant(sw, sh, dw, dh, aligned) == RESIZE_TILED4;
}

hipError_t launch_bgr_to_y_resized(const uint8_t *bgr, long stride, int sw, int sh, uint8_t *dst, long dstride, int dw, int dh,
                                   const int *xofs, const short *alpha, const int *yofs, const short *beta, hipStream_t st)
{
    hipLaunchKernelGGL(bgr_to_y_resized_kernel, dim3((dw + 255) / 256, (dh + RT4 - 1) / RT4), dim3(256), 0, st, bgr, stride, sw,
                       sh, dst, dstride, dw, dh, xofs, alpha, yofs, beta);
    return hipGetLastError();
}

hipError_t launch_resize_merge(const uint8_t *bgr, long stride, int sw, int sh, const uint8_t *ysr, long ystride, uint8_t *out,
                               long ostride, int dw, int dh, const int *xofs, const short *alpha, const int *yofs,
                               const short *beta, hipStream_t st)
{
    hipLaunchKernelGGL(resize_merge_kernel, dim3((dw + 255) / 256, (dh + RT4 - 1) / RT4), dim3(256), 0, st, bgr, stride, sw, sh,
                       ysr, ystride, out, ostride, dw, dh, xofs, alpha, yofs, beta);
    return hipGetLastError();
}

// A few rows of a byte plane, device to device on ONE device, as a kernel: the striped step's band assembly (12 + 12 rows per
// step).  A launch is queued like the kernels around it and never blocks the host; hipMemcpy2DAsync between device buffers was
// seen to, once a process keeps more streams busy than the device has hardware queues (profiles/r03/stripe_overhead.txt).
__global__ __launch_bounds__(256) void copy_rows_kernel(uint8_t *__restrict__ dst, long dstride, const uint8_t *__restrict__ src,
                                                        long sstride, int width)
{
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x >= width) return;
    const uint8_t *s = src + (long)blockIdx.y * sstride + x;
    uint8_t *d = dst + (long)blockIdx.y * dstride + x;
    if (x + 4 <= width && (((size_t)s | (size_t)d) & 3) == 0) {
        *reinterpret_cast<unsigned *>(d) = *reinterpret_cast<const unsigned *>(s);
    } else {
        for (int b = 0; b < 4 && x + b < width; ++b) d[b] = s[b];
    }
}

// The unsigned 8-bit kernels of this file take a row (or a row tile) from blockIdx.y and a plane from blockIdx.z and do not walk:
// a geometry whose grid would pass the limit of 65,535 is refused here, before anything is launched (the host layer words the
// refusal for the public calls that can reach one: srcnn_host.cpp, u8_rows_refusal).
static bool u8_grid_ok(long y, long z = 1) { return y <= kMaxGridYZ && z <= kMaxGridYZ; }

hipError_t launch_copy_rows(uint8_t *dst, long dstride, const uint8_t *src, long sstride, int width, int rows, hipStream_t st)
{
    if (width <= 0 || rows <= 0) return hipSuccess;
    if (!u8_grid_ok(rows)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)((width + 1023) / 1024), (unsigned)rows), dim3(256), 0, st, dst, dstride, src,
                       sstride, width);
    return hipGetLastError();
}

hipError_t launch_bgr2ycrcb(const uint8_t *bgr, long stride, int w, int h, uint8_t *planes, long pstride,
                            long ppitch, hipStream_t st)
{
    if (!u8_grid_ok(h)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bgr2ycrcb_kernel, dim3((w + 255) / 256, h), dim3(256), 0, st, bgr, stride, w, h, planes,
                       pstride, ppitch);
    return hipGetLastError();
}

hipError_t launch_ycrcb2bgr(const uint8_t *y, long ystride, const uint8_t *crcb, long pstride, long ppitch, int w,
                            int h, uint8_t *bgr, long stride, hipStream_t st)
{
    if (!u8_grid_ok(h)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ycrcb2bgr_kernel, dim3((w + 255) / 256, h), dim3(256), 0, st, y, ystride, crcb, pstride,
                       ppitch, w, h, bgr, stride);
    return hipGetLastError();
}

hipError_t launch_resize_cubic(const uint8_t *src, long sstride, long spitch, int sw, int sh, uint8_t *dst,
                               long dstride, long dpitch, int dw, int dh, int n_planes, const int *xofs,
                               const short *alpha, const int *yofs, const short *beta, hipStream_t st)
{
    const bool dword_ok = ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)dstride | (uintptr_t)dpitch) & 3) == 0;
    const int variant = resize_variant(sw, sh, dw, dh, dword_ok);      // the tiles' LDS limits: srcnn_kernels.h
    if (!u8_grid_ok(resize_grid_rows(variant, dh), n_planes)) return hipErrorInvalidValue;
    if (variant == RESIZE_TILED4)
        hipLaunchKernelGGL(resize_cubic_tiled4_kernel, dim3((dw + 255) / 256, (dh + RT4 - 1) / RT4, n_planes), dim3(256),
                           0, st, src, sstride, spitch, sw, sh, dst, dstride, dpitch, dw, dh, xofs, alpha, yofs, beta);
    else if (variant == RESIZE_TILED)
        hipLaunchKernelGGL(resize_cubic_tiled_kernel, dim3((dw + 255) / 256, (dh + RT - 1) / RT, n_planes), dim3(256),
                           0, st, src, sstride, spitch, sw, sh, dst, dstride, dpitch, dw, dh, xofs, alpha, yofs, beta);
    else
        hipLaunchKernelGGL(resize_cubic_kernel, dim3((dw + 255) / 256, dh, n_planes), dim3(256), 0, st, src, sstride,
                           spitch, sw, sh, dst, dstride, dpitch, dw, dh, xofs, alpha, yofs, beta);
    return hipGetLastError();
}

// ---- cubic resize of float32 planes (srcnn_resize_cubic_f32*, srcnn_process_f32*) --------------------------------------
// torch.nn.functional.interpolate(mode="bicubic", align_corners=False, antialias=False) on planar float32: Keys cubic,
// A = -0.75, half-pixel centres, tap indices clamped to the plane.  The first-tap indices and the coefficients come from the
// host in tables (srcnn_cubic_f32_taps: float64 arithmetic, coefficients rounded once to float32).
// Summation order, the same in both kernels: the horizontal pass first, then the vertical pass, each four products summed in
// ascending tap order, ((c0 s0 + c1 s1) + c2 s2) + c3 s3, all float32.  The sums are SEPARATE multiplies and adds, every
// product and every sum rounded on its own (this unit is built without FMA contraction), so both kernels give the same bits.
// Nothing is clamped but the tap INDEX: the output may overshoot the input's range, and a non-finite input spreads over the
// outputs whose 4 x 4 support holds it and no further.
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float cubic_sum4(float s0, float s1, float s2, float s3, const f32x4 c)
{
    float r = __fmul_rn(s0, c[0]);
    r = __fadd_rn(r, __fmul_rn(s1, c[1]));
    r = __fadd_rn(r, __fmul_rn(s2, c[2]));
    return __fadd_rn(r, __fmul_rn(s3, c[3]));
}

// Where the planes of a call lie: plane z = frame * channels + channel (strides and pitches in floats)
struct F32ResizeArgs {
    const float *src;
    long sstride, sch_pitch, sframe_pitch;
    int sw, sh;
    float *dst;
    long dstride, dch_pitch, dframe_pitch;
    int dw, dh;
    int channels, n_planes;
    const int *xfirst, *yfirst;
    const float *xcoef, *ycoef;     // 16-byte aligned: one f32x4 per output column / row
};

// Direct form: one output element per lane, the 16 taps from global memory.  Every index is clamped before it is used; lanes
// beyond the last column do nothing.  Rows and planes beyond the grid's y / z limits are walked by the same blocks.
__global__ __launch_bounds__(256) void resize_cubic_f32_direct_kernel(const F32ResizeArgs p)
{
    const int dx = blockIdx.x * 256 + threadIdx.x;
    if (dx >= p.dw) return;
    const int x0 = p.xfirst[dx] - 1;
    int xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xs[k] = min(max(x0 + k, 0), p.sw - 1);
    const f32x4 a = *reinterpret_cast<const f32x4 *>(p.xcoef + 4L * dx);
    for (int z = blockIdx.z; z < p.n_planes; z += gridDim.z) {
        const int frame = z / p.channels, ch = z - frame * p.channels;
        const float *s = p.src + frame * p.sframe_pitch + ch * p.sch_pitch;
        float *d = p.dst + frame * p.dframe_pitch + ch * p.dch_pitch;
        for (int dy = blockIdx.y; dy < p.dh; dy += gridDim.y) {
            const int y0 = p.yfirst[dy] - 1;
            float hs[4];
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const float *row = s + (long)min(max(y0 + ky, 0), p.sh - 1) * p.sstride;
                hs[ky] = cubic_sum4(row[xs[0]], row[xs[1]], row[xs[2]], row[xs[3]], a);
            }
            d[(long)dy * p.dstride + dx] = cubic_sum4(hs[0], hs[1], hs[2], hs[3], *reinterpret_cast<const f32x4 *>(p.ycoef + 4L * dy));
        }
    }
}

// Tiled form: a workgroup produces F32_RT output rows x 256 columns.  The source rows and columns the tile spans are loaded
// into LDS once (consecutive lanes on consecutive floats, the replicate border applied by clamping the index), the horizontal
// pass of every one of those rows is done once from LDS (thread = output column), the vertical pass reads the horizontal
// results (thread = four adjacent columns of F32_RPT rows) and stores 16 bytes per lane where the address allows it: scalar
// stores at a ragged right edge and wherever base, stride and column leave the four floats unaligned.
// (at most F32_RMAX source rows x F32_SMAX source columns: srcnn_kernels.h, where resize_f32_variant() checks a geometry
// against them before this kernel is chosen)
// The three steps are functions of their own, shared with the two kernels of srcnn_process_rgb_f32* below: the fill may
// compute the luma of three planes instead of loading one, and the vertical pass may add a term to what it stores.

// What srcnn_process_rgb_f32* adds to a resize.  Y = ((w0 x0 + w1 x1) + w2 x2) + off at the source resolution, the three
// planes sch_pitch apart; out_c = U_c + (Ysr - Yup) g, then min(max(., lo), hi) when clamp is set.  Every product and every
// sum is rounded on its own, like the resize's (this unit is built without FMA contraction).
struct F32LumaArgs {
    float w0, w1, w2, off;
    float g, lo, hi;
    int clamp;
    const float *ysr, *yup;         // the model's output and its input, dw x dh each (merge kernel only)
    long ysr_stride, ysr_frame_pitch, yup_stride, yup_frame_pitch;
};

// the columns of a tile: what a thread keeps for every row tile and plane it walks
struct F32TileCols {
    int c_lo, ncol;      // unclamped first source column of the tile, and how many it spans
    int x0;              // horizontal pass, thread = output column: its first tap in sbuf, and its coefficients
    f32x4 a;
    int tx, ty, dx;      // vertical pass: four columns from dx, rows F32_RPT * ty ...
};

__device__ __forceinline__ F32TileCols f32_tile_cols(const F32ResizeArgs &p)
{
    F32TileCols t;
    const int tid = threadIdx.x;
    const int dx0 = blockIdx.x * 256;
    t.c_lo = p.xfirst[dx0] - 1;
    const int c_hi = p.xfirst[min(dx0 + 255, p.dw - 1)] + 2;     // unclamped source columns of the tile
    t.ncol = c_hi - t.c_lo + 1;
    const int dxc = min(dx0 + tid, p.dw - 1);
    t.x0 = p.xfirst[dxc] - 1 - t.c_lo;
    t.a = *reinterpret_cast<const f32x4 *>(p.xcoef + 4L * dxc);
    t.tx = tid & 63;
    t.ty = tid >> 6;
    t.dx = dx0 + 4 * t.tx;
    return t;
}

// source rows [r_lo, r_lo + nrow) x columns [c_lo, c_lo + ncol) into sbuf, every index clamped to the plane before it is
// used.  LUMA: the element is the luma of the three planes at that place (three loads), not the plane's own.
template <bool LUMA>
__device__ __forceinline__ void f32_tile_fill(float (*sbuf)[F32_SMAX], const float *s, const F32ResizeArgs &p, const F32LumaArgs &q,
                                              int r_lo, int nrow, int c_lo, int ncol)
{
    for (int e = threadIdx.x; e < nrow * ncol; e += 256) {
        const int rr = e / ncol, cc = e - rr * ncol;
        const long at = (long)min(max(r_lo + rr, 0), p.sh - 1) * p.sstride + min(max(c_lo + cc, 0), p.sw - 1);
        if (LUMA) {
            float y = __fadd_rn(__fmul_rn(q.w0, s[at]), __fmul_rn(q.w1, s[at + p.sch_pitch]));
            y = __fadd_rn(y, __fmul_rn(q.w2, s[at + 2 * p.sch_pitch]));
            sbuf[rr][cc] = __fadd_rn(y, q.off);
        } else {
            sbuf[rr][cc] = s[at];
        }
    }
}

__device__ __forceinline__ void f32_tile_hpass(float (*hbuf)[256], const float (*sbuf)[F32_SMAX], int nrow, const F32TileCols t)
{
    for (int rr = 0; rr < nrow; ++rr)
        hbuf[rr][threadIdx.x] = cubic_sum4(sbuf[rr][t.x0], sbuf[rr][t.x0 + 1], sbuf[rr][t.x0 + 2], sbuf[rr][t.x0 + 3], t.a);
}

// four floats of a row from o, of which the first n (1 .. 4 and more) exist: one 16-byte load where all four exist and the
// address is aligned, else a load per float that exists (the others 0)
__device__ __forceinline__ f32x4 f32_load4(const float *o, int n)
{
    if (n >= 4 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) return *reinterpret_cast<const f32x4 *>(o);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < n) v[c] = o[c];
    return v;
}

// The vertical pass of the thread's rows of the tile [dy0, dy1) into plane d.  MERGE: add[r] is added to row r's four sums
// and the result clamped when q.clamp is set (a NaN stays a NaN, as in numpy and torch).
template <bool MERGE>
__device__ __forceinline__ void f32_tile_vpass(const float (*hbuf)[256], float *d, const F32ResizeArgs &p, const F32LumaArgs &q,
                                               const f32x4 *add, int dy0, int dy1, int r_lo, const F32TileCols t)
{
    if (t.dx < p.dw) {
#pragma unroll
        for (int r = 0; r < F32_RPT; ++r) {
            const int dy = dy0 + F32_RPT * t.ty + r;
            if (dy >= dy1) break;
            const int j = p.yfirst[dy] - 1 - r_lo;
            const f32x4 b = *reinterpret_cast<const f32x4 *>(p.ycoef + 4L * dy);
            f32x4 h[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) h[k] = *reinterpret_cast<const f32x4 *>(&hbuf[j + k][4 * t.tx]);
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = cubic_sum4(h[0][c], h[1][c], h[2][c], h[3][c], b);
            if (MERGE) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float m = __fadd_rn(v[c], add[r][c]);
                    if (q.clamp) {
                        m = m < q.lo ? q.lo : m;
                        m = m > q.hi ? q.hi : m;
                    }
                    v[c] = m;
                }
            }
            float *o = d + (long)dy * p.dstride + t.dx;
            if (t.dx + 3 < p.dw && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
                *reinterpret_cast<f32x4 *>(o) = v;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (t.dx + c < p.dw) o[c] = v[c];
            }
        }
    }
}

// the resize of p.n_planes planes, tile after tile; LUMA: every "plane" is the luma of the frame's three (p.channels = 1)
template <bool LUMA>
__device__ __forceinline__ void resize_f32_tiled(const F32ResizeArgs p, const F32LumaArgs q, float (*hbuf)[256],
                                                 float (*sbuf)[F32_SMAX])
{
    const F32TileCols t = f32_tile_cols(p);
    const int n_row_tiles = (p.dh + F32_RT - 1) / F32_RT;
    for (int z = blockIdx.z; z < p.n_planes; z += gridDim.z) {
        const int frame = z / p.channels, ch = z - frame * p.channels;
        const float *s = p.src + frame * p.sframe_pitch + ch * p.sch_pitch;
        float *d = p.dst + frame * p.dframe_pitch + ch * p.dch_pitch;
        for (int rt = blockIdx.y; rt < n_row_tiles; rt += gridDim.y) {
            const int dy0 = rt * F32_RT, dy1 = min(dy0 + F32_RT, p.dh);
            const int r_lo = p.yfirst[dy0] - 1, r_hi = p.yfirst[dy1 - 1] + 2;              // ... and rows
            const int nrow = r_hi - r_lo + 1;
            // (a thread still in the vertical pass of the tile before has not reached the barrier below: hbuf is not written
            // yet, and sbuf was last read before that tile's second barrier)
            f32_tile_fill<LUMA>(sbuf, s, p, q, r_lo, nrow, t.c_lo, t.ncol);
            __syncthreads();
            f32_tile_hpass(hbuf, sbuf, nrow, t);
            __syncthreads();
            f32_tile_vpass<false>(hbuf, d, p, q, nullptr, dy0, dy1, r_lo, t);
        }
    }
}

__global__ __launch_bounds__(256) void resize_cubic_f32_tiled_kernel(const F32ResizeArgs p)
{
    __shared__ __attribute__((aligned(16))) float hbuf[F32_RMAX][256];
    __shared__ float sbuf[F32_RMAX][F32_SMAX];
    resize_f32_tiled<false>(p, F32LumaArgs{}, hbuf, sbuf);
}

// ---- a 3-plane float image through a 1-channel model (srcnn_process_rgb_f32*) -------------------------------------------
// out_c = up(x_c) + g (Ysr - Yup), Yup = up(Y_lr), Ysr = model(Yup): two kernels around the banded path, both the tiled resize
// above (a call never shrinks the image, so every geometry fits the tile).
// Front: the tiled resize whose fill computes Y_lr from the frame's three planes; one plane out, Yup.
__global__ __launch_bounds__(256) void luma_resize_f32_kernel(const F32ResizeArgs p, const F32LumaArgs q)
{
    __shared__ __attribute__((aligned(16))) float hbuf[F32_RMAX][256];
    __shared__ float sbuf[F32_RMAX][F32_SMAX];
    resize_f32_tiled<true>(p, q, hbuf, sbuf);
}

// Back: a workgroup produces its tile of all three output planes in turn.  (Ysr - Yup) g of the thread's F32_RPT rows x 4
// columns is loaded once and kept in registers; then, channel after channel, fill, horizontal pass and a vertical pass that
// adds it.  p.n_planes counts FRAMES here (grid z), p.channels is 3.
// (between two channels no barrier is needed beyond the two of a tile, for the reason given in resize_f32_tiled: a thread
// that refills sbuf has left the vertical pass, which reads hbuf only, and nobody writes hbuf before the next first barrier)
__global__ __launch_bounds__(256) void resize_merge_f32_kernel(const F32ResizeArgs p, const F32LumaArgs q)
{
    __shared__ __attribute__((aligned(16))) float hbuf[F32_RMAX][256];
    __shared__ float sbuf[F32_RMAX][F32_SMAX];
    const F32TileCols t = f32_tile_cols(p);
    const int n_row_tiles = (p.dh + F32_RT - 1) / F32_RT;
    for (int z = blockIdx.z; z < p.n_planes; z += gridDim.z) {
        const float *s = p.src + z * p.sframe_pitch;
        float *d = p.dst + z * p.dframe_pitch;
        const float *ysr = q.ysr + z * q.ysr_frame_pitch, *yup = q.yup + z * q.yup_frame_pitch;
        for (int rt = blockIdx.y; rt < n_row_tiles; rt += gridDim.y) {
            const int dy0 = rt * F32_RT, dy1 = min(dy0 + F32_RT, p.dh);
            const int r_lo = p.yfirst[dy0] - 1, r_hi = p.yfirst[dy1 - 1] + 2;
            const int nrow = r_hi - r_lo + 1;
            f32x4 add[F32_RPT];
#pragma unroll
            for (int r = 0; r < F32_RPT; ++r) {
                const int dy = dy0 + F32_RPT * t.ty + r;
                add[r] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (t.dx < p.dw && dy < dy1) {
                    const f32x4 sr = f32_load4(ysr + (long)dy * q.ysr_stride + t.dx, p.dw - t.dx);
                    const f32x4 up = f32_load4(yup + (long)dy * q.yup_stride + t.dx, p.dw - t.dx);
#pragma unroll
                    for (int c = 0; c < 4; ++c) add[r][c] = __fmul_rn(__fsub_rn(sr[c], up[c]), q.g);
                }
            }
#pragma unroll 1
            for (int ch = 0; ch < 3; ++ch) {
                f32_tile_fill<false>(sbuf, s + ch * p.sch_pitch, p, q, r_lo, nrow, t.c_lo, t.ncol);
                __syncthreads();
                f32_tile_hpass(hbuf, sbuf, nrow, t);
                __syncthreads();
                f32_tile_vpass<true>(hbuf, d + ch * p.dch_pitch, p, q, add, dy0, dy1, r_lo, t);
            }
        }
    }
}

// ---- images as they are stored (srcnn_*_image_dev): accessor forms of the four kernels above ------------------------------
// The same tables, tile (F32_RT, F32_RMAX, F32_SMAX: the same LDS), variant choice and cubic_sum4 order; f32_tile_cols and
// f32_tile_hpass are the ones above.  Only the fill's load and the vertical pass's store differ: they go through an ImageRef.
// The element kind is a workgroup-uniform switch, not a template parameter: 4 source x 4 destination kinds x 4 kernels would be
// 64 kernels for a branch that is scalar (s_cmp on a kernel argument) and sits beside a global load or store.
// Everything between load and store is float32 as above, so a call equals store(f32 call(load(x))) bit for bit.
// (image_load: srcnn_image.h, shared with the metric kernels of srcnn_metrics.hip)

// float32 -> bfloat16 bits, round to nearest even; a NaN stays a NaN (quiet, sign kept)
__device__ __forceinline__ unsigned bf16_bits(float v)
{
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// float32 -> float16 bits: v_cvt_f16_f32, round to nearest even, overflow to +-inf, f16 subnormals kept
__device__ __forceinline__ unsigned f16_bits(float v)
{
    const _Float16 h = (_Float16)v;
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}
// float32 -> byte: rint_half_even(min(max(v scale, 0), 255)), 0 for a NaN (neither comparison holds for one)
__device__ __forceinline__ unsigned u8_bits(float v, float scale)
{
    float t = __fmul_rn(v, scale);
    t = t >= 0.f ? t : 0.f;
    t = t > 255.f ? 255.f : t;
    return (unsigned)(int)rintf(t);
}

__device__ __forceinline__ void image_store(const ImageRef &im, long at, float v)
{
    switch (im.elem) {
    case ELEM_F32: static_cast<float *>(im.data)[at] = v; break;
    case ELEM_F16: static_cast<uint16_t *>(im.data)[at] = (uint16_t)f16_bits(v); break;
    case ELEM_BF16: static_cast<uint16_t *>(im.data)[at] = (uint16_t)bf16_bits(v); break;
    default: static_cast<uint8_t *>(im.data)[at] = (uint8_t)u8_bits(v, im.scale); break;
    }
}

// Four CONTIGUOUS elements from element offset `at`: one store of 16 (F32), 8 (F16, BF16) or 4 (U8) bytes where the ADDRESS
// is aligned to that, else element by element.
__device__ __forceinline__ void image_store_run4(const ImageRef &im, long at, const f32x4 v)
{
    if (im.elem == ELEM_F32) {
        float *o = static_cast<float *>(im.data) + at;
        if ((reinterpret_cast<uintptr_t>(o) & 15) == 0) { *reinterpret_cast<f32x4 *>(o) = v; return; }
    } else if (im.elem == ELEM_U8) {
        uint8_t *o = static_cast<uint8_t *>(im.data) + at;
        if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            *reinterpret_cast<unsigned *>(o) = u8_bits(v[0], im.scale) | u8_bits(v[1], im.scale) << 8 |
                                               u8_bits(v[2], im.scale) << 16 | u8_bits(v[3], im.scale) << 24;
            return;
        }
    } else {
        uint16_t *o = static_cast<uint16_t *>(im.data) + at;
        if ((reinterpret_cast<uintptr_t>(o) & 7) == 0) {
            const bool h = im.elem == ELEM_F16;
            uint2 w;
            w.x = (h ? f16_bits(v[0]) : bf16_bits(v[0])) | (h ? f16_bits(v[1]) : bf16_bits(v[1])) << 16;
            w.y = (h ? f16_bits(v[2]) : bf16_bits(v[2])) | (h ? f16_bits(v[3]) : bf16_bits(v[3])) << 16;
            *reinterpret_cast<uint2 *>(o) = w;
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) image_store(im, at + c, v[c]);
}

// ... and the load of four contiguous elements, by the same rule
__device__ __forceinline__ f32x4 image_load_run4(const ImageRef &im, long at)
{
    f32x4 v;
    if (im.elem == ELEM_F32) {
        const float *o = static_cast<const float *>(im.data) + at;
        if ((reinterpret_cast<uintptr_t>(o) & 15) == 0) return *reinterpret_cast<const f32x4 *>(o);
    } else if (im.elem == ELEM_U8) {
        const uint8_t *o = static_cast<const uint8_t *>(im.data) + at;
        if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            const unsigned w = *reinterpret_cast<const unsigned *>(o);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = __fmul_rn((float)((w >> (8 * c)) & 0xffu), im.scale);
            return v;
        }
    } else {
        const uint16_t *o = static_cast<const uint16_t *>(im.data) + at;
        if ((reinterpret_cast<uintptr_t>(o) & 7) == 0) {
            const uint2 w = *reinterpret_cast<const uint2 *>(o);
            const unsigned b[4] = {w.x & 0xffffu, w.x >> 16, w.y & 0xffffu, w.y >> 16};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                v[c] = im.elem == ELEM_F16 ? (float)__builtin_bit_cast(_Float16, (unsigned short)b[c]) : __uint_as_float(b[c] << 16);
            return v;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = image_load(im, at + c);
    return v;
}

// Four columns of a row from element offset `at`, px_step apart, of which the first n (>= 1) exist: planar rows (px_step 1)
// with all four present as one run, everything else element by element.
__device__ __forceinline__ void image_store4(const ImageRef &im, long at, const f32x4 v, int n)
{
    if (im.px_step == 1 && n >= 4) {
        image_store_run4(im, at, v);
        return;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < n) image_store(im, at + c * im.px_step, v[c]);
}

// Four pixels of three channels (v[channel][column]) into an image whose pixels are three adjacent elements (px_step 3,
// ch_pitch 1): twelve contiguous elements from `at`, as three runs
__device__ __forceinline__ void image_store_pixels4(const ImageRef &im, long at, const f32x4 v0, const f32x4 v1, const f32x4 v2)
{
    image_store_run4(im, at, f32x4{v0[0], v1[0], v2[0], v0[1]});
    image_store_run4(im, at + 4, f32x4{v1[1], v2[1], v0[2], v1[2]});
    image_store_run4(im, at + 8, f32x4{v2[2], v0[3], v1[3], v2[3]});
}
__host__ __device__ __forceinline__ bool image_pixels_of_3(const ImageRef &im) { return im.px_step == 3 && im.ch_pitch == 1; }

// geometry and tables as the kernels above take them (g.src, g.dst and their strides: not read by the image kernels), and the
// two images
struct ImageResizeArgs {
    F32ResizeArgs g;
    ImageRef src, dst;
};

__global__ __launch_bounds__(256) void resize_cubic_image_direct_kernel(const ImageResizeArgs a)
{
    const F32ResizeArgs &p = a.g;
    const int dx = blockIdx.x * 256 + threadIdx.x;
    if (dx >= p.dw) return;
    const int x0 = p.xfirst[dx] - 1;
    long xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xs[k] = (long)min(max(x0 + k, 0), p.sw - 1) * a.src.px_step;
    const f32x4 ca = *reinterpret_cast<const f32x4 *>(p.xcoef + 4L * dx);
    for (int z = blockIdx.z; z < p.n_planes; z += gridDim.z) {
        const int frame = z / p.channels, ch = z - frame * p.channels;
        const long s = frame * a.src.frame_pitch + ch * a.src.ch_pitch;
        const long d = frame * a.dst.frame_pitch + ch * a.dst.ch_pitch + dx * a.dst.px_step;
        for (int dy = blockIdx.y; dy < p.dh; dy += gridDim.y) {
            const int y0 = p.yfirst[dy] - 1;
            float hs[4];
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const long row = s + (long)min(max(y0 + ky, 0), p.sh - 1) * a.src.stride;
                hs[ky] = cubic_sum4(image_load(a.src, row + xs[0]), image_load(a.src, row + xs[1]), image_load(a.src, row + xs[2]),
                                    image_load(a.src, row + xs[3]), ca);
            }
            image_store(a.dst, d + (long)dy * a.dst.stride,
                        cubic_sum4(hs[0], hs[1], hs[2], hs[3], *reinterpret_cast<const f32x4 *>(p.ycoef + 4L * dy)));
        }
    }
}

// f32_tile_fill through the accessor; s: element offset of the plane (LUMA: of the first of the pixel's three channels, which
// lie ch_pitch apart -- adjacent in an interleaved image).  Consecutive lanes take consecutive columns: memory order.
template <bool LUMA>
__device__ __forceinline__ void image_tile_fill(float (*sbuf)[F32_SMAX], const ImageRef &im, long s, const F32ResizeArgs &p,
                                                const F32LumaArgs &q, int r_lo, int nrow, int c_lo, int ncol)
{
    for (int e = threadIdx.x; e < nrow * ncol; e += 256) {
        const int rr = e / ncol, cc = e - rr * ncol;
        const long at = s + (long)min(max(r_lo + rr, 0), p.sh - 1) * im.stride + (long)min(max(c_lo + cc, 0), p.sw - 1) * im.px_step;
        if (LUMA) {
            float y = __fadd_rn(__fmul_rn(q.w0, image_load(im, at)), __fmul_rn(q.w1, image_load(im, at + im.ch_pitch)));
            y = __fadd_rn(y, __fmul_rn(q.w2, image_load(im, at + 2 * im.ch_pitch)));
            sbuf[rr][cc] = __fadd_rn(y, q.off);
        } else {
            sbuf[rr][cc] = image_load(im, at);
        }
    }
}

// The vertical pass of f32_tile_vpass for one row dy of the thread's four columns (r: its place among the thread's rows)
template <bool MERGE>
__device__ __forceinline__ f32x4 image_tile_vsum(const float (*hbuf)[256], const F32ResizeArgs &p, const F32LumaArgs &q,
                                                 const f32x4 *add, int r, int dy, int r_lo, const F32TileCols &t)
{
    const int j = p.yfirst[dy] - 1 - r_lo;
    const f32x4 b = *reinterpret_cast<const f32x4 *>(p.ycoef + 4L * dy);
    f32x4 h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = *reinterpret_cast<const f32x4 *>(&hbuf[j + k][4 * t.tx]);
    f32x4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = cubic_sum4(h[0][c], h[1][c], h[2][c], h[3][c], b);
    if (MERGE) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float m = __fadd_rn(v[c], add[r][c]);
            if (q.clamp) {
                m = m < q.lo ? q.lo : m;
                m = m > q.hi ? q.hi : m;
            }
            v[c] = m;
        }
    }
    return v;
}

// f32_tile_vpass through the accessor; d: element offset of the plane in im
template <bool MERGE>
__device__ __forceinline__ void image_tile_vpass(const float (*hbuf)[256], const ImageRef &im, long d, const F32ResizeArgs &p,
                                                 const F32LumaArgs &q, const f32x4 *add, int dy0, int dy1, int r_lo,
                                                 const F32TileCols t)
{
    if (t.dx < p.dw) {
#pragma unroll
        for (int r = 0; r < F32_RPT; ++r) {
            const int dy = dy0 + F32_RPT * t.ty + r;
            if (dy >= dy1) break;
            image_store4(im, d + (long)dy * im.stride + t.dx * im.px_step, image_tile_vsum<MERGE>(hbuf, p, q, add, r, dy, r_lo, t),
                         p.dw - t.dx);
        }
    }
}

template <bool LUMA>
__device__ __forceinline__ void resize_image_tiled(const ImageResizeArgs &a, const F32LumaArgs q, float (*hbuf)[256],
                                                   float (*sbuf)[F32_SMAX])
{
    const F32ResizeArgs &p = a.g;
    const F32TileCols t = f32_tile_cols(p);
    const int n_row_tiles = (p.dh + F32_RT - 1) / F32_RT;
    for (int z = blockIdx.z; z < p.n_planes; z += gridDim.z) {
        const int frame = z / p.channels, ch = z - frame * p.channels;
        const long s = frame * a.src.frame_pitch + ch * a.src.ch_pitch;
        const long d = frame * a.dst.frame_pitch + ch * a.dst.ch_pitch;
        for (int rt = blockIdx.y; rt < n_row_tiles; rt += gridDim.y) {
            const int dy0 = rt * F32_RT, dy1 = min(dy0 + F32_RT, p.dh);
            const int r_lo = p.yfirst[dy0] - 1, r_hi = p.yfirst[dy1 - 1] + 2;
            const int nrow = r_hi - r_lo + 1;
            image_tile_fill<LUMA>(sbuf, a.src, s, p, q, r_lo, nrow, t.c_lo, t.ncol);      // (barriers: as in resize_f32_tiled)
            __syncthreads();
            f32_tile_hpass(hbuf, sbuf, nrow, t);
            __syncthreads();
            image_tile_vpass<false>(hbuf, a.dst, d, p, q, nullptr, dy0, dy1, r_lo, t);
        }
    }
}

__global__ __launch_bounds__(256) void resize_cubic_image_tiled_kernel(const ImageResizeArgs a)
{
    __shared__ __attribute__((aligned(16))) float hbuf[F32_RMAX][256];
    __shared__ float sbuf[F32_RMAX][F32_SMAX];
    resize_image_tiled<false>(a, F32LumaArgs{}, hbuf, sbuf);
}

// Front of srcnn_process_rgb_image_dev: Yup (a packed float32 plane, a.dst) from the luma of the stored image
__global__ __launch_bounds__(256) void luma_resize_image_kernel(const ImageResizeArgs a, const F32LumaArgs q)
{
    __shared__ __attribute__((aligned(16))) float hbuf[F32_RMAX][256];
    __shared__ float sbuf[F32_RMAX][F32_SMAX];
    resize_image_tiled<true>(a, q, hbuf, sbuf);
}

// Back: as resize_merge_f32_kernel, in one of two store orders.  PIXELS false: channel after channel, each channel's tile
// stored on its own pass (any destination).  PIXELS true, for a destination whose pixels are three adjacent elements: the three
// channels' results of the thread's F32_RPT rows x 4 columns are kept in registers and stored pixel-contiguous, twelve elements per row as three runs.  Same sums in the same order either way.
template <bool PIXELS>
__device__ __forceinline__ void resize_merge_image(const ImageResizeArgs &a, const F32LumaArgs &q, float (*hbuf)[256],
                                                   float (*sbuf)[F32_SMAX])
{
    const F32ResizeArgs &p = a.g;
    const F32TileCols t = f32_tile_cols(p);
    const int n_row_tiles = (p.dh + F32_RT - 1) / F32_RT;
    for (int z = blockIdx.z; z < p.n_planes; z += gridDim.z) {
        const long s = z * a.src.frame_pitch, d = z * a.dst.frame_pitch;
        const float *ysr = q.ysr + z * q.ysr_frame_pitch, *yup = q.yup + z * q.yup_frame_pitch;
        for (int rt = blockIdx.y; rt < n_row_tiles; rt += gridDim.y) {
            const int dy0 = rt * F32_RT, dy1 = min(dy0 + F32_RT, p.dh);
            const int r_lo = p.yfirst[dy0] - 1, r_hi = p.yfirst[dy1 - 1] + 2;
            const int nrow = r_hi - r_lo + 1;
            f32x4 add[F32_RPT];
#pragma unroll
            for (int r = 0; r < F32_RPT; ++r) {
                const int dy = dy0 + F32_RPT * t.ty + r;
                add[r] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (t.dx < p.dw && dy < dy1) {
                    const f32x4 sr = f32_load4(ysr + (long)dy * q.ysr_stride + t.dx, p.dw - t.dx);
                    const f32x4 up = f32_load4(yup + (long)dy * q.yup_stride + t.dx, p.dw - t.dx);
#pragma unroll
                    for (int c = 0; c < 4; ++c) add[r][c] = __fmul_rn(__fsub_rn(sr[c], up[c]), q.g);
                }
            }
            if constexpr (PIXELS) {
                // (the channel loop stays rolled -- unrolled it takes more than 256 registers -- and the results shift through
                // three register sets instead of being indexed by the channel: k0 ends as channel 0, k2 as channel 2)
                f32x4 k0[F32_RPT], k1[F32_RPT], k2[F32_RPT];
#pragma unroll
                for (int r = 0; r < F32_RPT; ++r) k0[r] = k1[r] = k2[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
                for (int ch = 0; ch < 3; ++ch) {
                    image_tile_fill<false>(sbuf, a.src, s + ch * a.src.ch_pitch, p, q, r_lo, nrow, t.c_lo, t.ncol);
                    __syncthreads();
                    f32_tile_hpass(hbuf, sbuf, nrow, t);
                    __syncthreads();
#pragma unroll
                    for (int r = 0; r < F32_RPT; ++r) {
                        const int dy = min(dy0 + F32_RPT * t.ty + r, dy1 - 1);      // (rows beyond the tile: computed, not stored)
                        k0[r] = k1[r];
                        k1[r] = k2[r];
                        k2[r] = image_tile_vsum<true>(hbuf, p, q, add, r, dy, r_lo, t);
                    }
                }
                if (t.dx < p.dw) {
#pragma unroll
                    for (int r = 0; r < F32_RPT; ++r) {
                        const int dy = dy0 + F32_RPT * t.ty + r;
                        if (dy >= dy1) break;
                        const long at = d + (long)dy * a.dst.stride + 3L * t.dx;
                        if (t.dx + 3 < p.dw) {
                            image_store_pixels4(a.dst, at, k0[r], k1[r], k2[r]);
                        } else {
                            image_store4(a.dst, at, k0[r], p.dw - t.dx);
                            image_store4(a.dst, at + 1, k1[r], p.dw - t.dx);
                            image_store4(a.dst, at + 2, k2[r], p.dw - t.dx);
                        }
                    }
                }
            } else {
#pragma unroll 1
                for (int ch = 0; ch < 3; ++ch) {
                    image_tile_fill<false>(sbuf, a.src, s + ch * a.src.ch_pitch, p, q, r_lo, nrow, t.c_lo, t.ncol);
                    __syncthreads();
                    f32_tile_hpass(hbuf, sbuf, nrow, t);
                    __syncthreads();
                    image_tile_vpass<true>(hbuf, a.dst, d + ch * a.dst.ch_pitch, p, q, add, dy0, dy1, r_lo, t);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void resize_merge_image_kernel(const ImageResizeArgs a, const F32LumaArgs q)
{
    __shared__ __attribute__((aligned(16))) float hbuf[F32_RMAX][256];
    __shared__ float sbuf[F32_RMAX][F32_SMAX];
    resize_merge_image<false>(a, q, hbuf, sbuf);
}

__global__ __launch_bounds__(256) void resize_merge_image_pixels_kernel(const ImageResizeArgs a, const F32LumaArgs q)
{
    __shared__ __attribute__((aligned(16))) float hbuf[F32_RMAX][256];
    __shared__ float sbuf[F32_RMAX][F32_SMAX];
    resize_merge_image<true>(a, q, hbuf, sbuf);
}

// dst = store(load(src)) for images of C = 1 or 3 channels: a lane converts four adjacent pixels of every channel.  A side
// whose pixels are C adjacent elements is read / written as 4 C contiguous elements (C runs of four), a planar side as a run of
// four per channel, each run one access of 4 ... 16 bytes where its address is aligned; any other layout, and the last columns
// of a row, element by element.  Rows and frames beyond the grid's limits are walked by the same blocks.
template <int C>
__global__ __launch_bounds__(256) void convert_image_kernel(const ImageRef src, const ImageRef dst, int width, int height, int n_frames)
{
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x >= width) return;
    const int n = width - x;
    const bool s_px = C > 1 && src.px_step == C && src.ch_pitch == 1, d_px = C > 1 && dst.px_step == C && dst.ch_pitch == 1;
    for (int f = blockIdx.z; f < n_frames; f += gridDim.z) {
        for (int y = blockIdx.y; y < height; y += gridDim.y) {
            const long s = f * src.frame_pitch + y * src.stride + x * src.px_step;
            const long d = f * dst.frame_pitch + y * dst.stride + x * dst.px_step;
            f32x4 v[C];      // v[channel][column]
            if (n >= 4 && s_px) {
                float e[4 * C];
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    const f32x4 r = image_load_run4(src, s + 4 * k);
#pragma unroll
                    for (int c = 0; c < 4; ++c) e[4 * k + c] = r[c];
                }
#pragma unroll
                for (int ch = 0; ch < C; ++ch)
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[ch][c] = e[c * C + ch];
            } else if (n >= 4 && src.px_step == 1) {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) v[ch] = image_load_run4(src, s + ch * src.ch_pitch);
            } else {
#pragma unroll
                for (int ch = 0; ch < C; ++ch)
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[ch][c] = c < n ? image_load(src, s + ch * src.ch_pitch + c * src.px_step) : 0.f;
            }
            if (n >= 4 && d_px) {
                float e[4 * C];
#pragma unroll
                for (int ch = 0; ch < C; ++ch)
#pragma unroll
                    for (int c = 0; c < 4; ++c) e[c * C + ch] = v[ch][c];
#pragma unroll
                for (int k = 0; k < C; ++k) image_store_run4(dst, d + 4 * k, f32x4{e[4 * k], e[4 * k + 1], e[4 * k + 2], e[4 * k + 3]});
            } else {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) image_store4(dst, d + ch * dst.ch_pitch, v[ch], n);
            }
        }
    }
}

// Which store order the merge kernel takes for a destination of 3-element pixels (DESIGN.md 4.14 has both orders' times);
// -DSRCNN_MERGE_CHANNEL_PASSES builds the other one for an A/B run
#ifdef SRCNN_MERGE_CHANNEL_PASSES
constexpr bool kMergePixelOrder = false;
#else
constexpr bool kMergePixelOrder = true;
#endif

static unsigned grid_cap(int v) { return (unsigned)(v < 65535 ? v : 65535); }      // grid y and z: the kernels walk what lies beyond

// The arguments of a launch.  g carries the geometry and the tables for every kernel, and the planes' pointers and strides for
// the float32 kernels, which a launcher takes exactly when both sides are planar float32 (srcnn_image_check's layouts: any
// row stride and pitches); every other pair of descriptors takes the image kernels, which read the ImageRefs.
static ImageResizeArgs image_args(const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels, int n_planes,
                                  const int *xfirst, const float *xcoef, const int *yfirst, const float *ycoef)
{
    return ImageResizeArgs{F32ResizeArgs{static_cast<const float *>(src.data), src.stride, src.ch_pitch, src.frame_pitch, sw, sh,
                                         static_cast<float *>(dst.data), dst.stride, dst.ch_pitch, dst.frame_pitch, dw, dh, channels,
                                         n_planes, xfirst, yfirst, xcoef, ycoef}, src, dst};
}
static bool both_planar_f32(const ImageResizeArgs &a) { return image_is_planar_f32(a.src) && image_is_planar_f32(a.dst); }
static dim3 tile_grid(int dw, int dh, int nz) { return dim3((dw + 255) / 256, grid_cap((dh + F32_RT - 1) / F32_RT), grid_cap(nz)); }

hipError_t launch_resize_cubic_image(const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels,
                                     int n_frames, const int *xfirst, const float *xcoef, const int *yfirst, const float *ycoef,
                                     hipStream_t st)
{
    if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || channels <= 0 || n_frames <= 0 || (long)channels * n_frames > 0x7fffffffL)
        return hipErrorInvalidValue;
    const ImageResizeArgs a = image_args(src, sw, sh, dst, dw, dh, channels, channels * n_frames, xfirst, xcoef, yfirst, ycoef);
    const bool f32 = both_planar_f32(a);
    if (resize_f32_variant(sw, sh, dw, dh) == RESIZE_F32_TILED) {      // the tile's LDS limits: srcnn_kernels.h
        const dim3 grid = tile_grid(dw, dh, a.g.n_planes);
        if (f32) hipLaunchKernelGGL(resize_cubic_f32_tiled_kernel, grid, dim3(256), 0, st, a.g);
        else hipLaunchKernelGGL(resize_cubic_image_tiled_kernel, grid, dim3(256), 0, st, a);
    } else {
        const dim3 grid((dw + 255) / 256, grid_cap(dh), grid_cap(a.g.n_planes));
        if (f32) hipLaunchKernelGGL(resize_cubic_f32_direct_kernel, grid, dim3(256), 0, st, a.g);
        else hipLaunchKernelGGL(resize_cubic_image_direct_kernel, grid, dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

// the two launches of srcnn_process_rgb_* for n_frames frames: hipErrorInvalidValue for a geometry outside the tile
static bool rgb_f32_geometry_ok(int sw, int sh, int dw, int dh, int n_frames)
{
    return sw > 0 && sh > 0 && dw > 0 && dh > 0 && n_frames > 0 && resize_f32_variant(sw, sh, dw, dh) == RESIZE_F32_TILED;
}

hipError_t launch_luma_resize_image(const ImageRef &src, int sw, int sh, float *yup, long ystride, long yframe_pitch, int dw, int dh,
                                    int n_frames, const float luma[4], const int *xfirst, const float *xcoef, const int *yfirst,
                                    const float *ycoef, hipStream_t st)
{
    if (!rgb_f32_geometry_ok(sw, sh, dw, dh, n_frames)) return hipErrorInvalidValue;
    const ImageRef dst{yup, ELEM_F32, 0.f, 1, ystride, 0, yframe_pitch};
    const ImageResizeArgs a = image_args(src, sw, sh, dst, dw, dh, 1, n_frames, xfirst, xcoef, yfirst, ycoef);
    F32LumaArgs q{};
    q.w0 = luma[0]; q.w1 = luma[1]; q.w2 = luma[2]; q.off = luma[3];
    if (both_planar_f32(a)) hipLaunchKernelGGL(luma_resize_f32_kernel, tile_grid(dw, dh, n_frames), dim3(256), 0, st, a.g, q);
    else hipLaunchKernelGGL(luma_resize_image_kernel, tile_grid(dw, dh, n_frames), dim3(256), 0, st, a, q);
    return hipGetLastError();
}

hipError_t launch_resize_merge_image(const ImageRef &src, int sw, int sh, const float *ysr, long ysr_stride, long ysr_frame_pitch,
                                     const float *yup, long yup_stride, long yup_frame_pitch, const ImageRef &dst, int dw, int dh,
                                     int n_frames, float g, const float *clamp, const int *xfirst, const float *xcoef,
                                     const int *yfirst, const float *ycoef, hipStream_t st)
{
    if (!rgb_f32_geometry_ok(sw, sh, dw, dh, n_frames)) return hipErrorInvalidValue;
    const ImageResizeArgs a = image_args(src, sw, sh, dst, dw, dh, 3, n_frames, xfirst, xcoef, yfirst, ycoef);
    F32LumaArgs q{};
    q.g = g;
    q.clamp = clamp != nullptr;
    if (clamp) { q.lo = clamp[0]; q.hi = clamp[1]; }
    q.ysr = ysr; q.ysr_stride = ysr_stride; q.ysr_frame_pitch = ysr_frame_pitch;
    q.yup = yup; q.yup_stride = yup_stride; q.yup_frame_pitch = yup_frame_pitch;
    const dim3 grid = tile_grid(dw, dh, n_frames);
    if (both_planar_f32(a))
        hipLaunchKernelGGL(resize_merge_f32_kernel, grid, dim3(256), 0, st, a.g, q);
    else if (kMergePixelOrder && image_pixels_of_3(dst))
        hipLaunchKernelGGL(resize_merge_image_pixels_kernel, grid, dim3(256), 0, st, a, q);
    else
        hipLaunchKernelGGL(resize_merge_image_kernel, grid, dim3(256), 0, st, a, q);
    return hipGetLastError();
}

hipError_t launch_convert_image(const ImageRef &src, const ImageRef &dst, int width, int height, int channels, int n_frames,
                                hipStream_t st)
{
    if (width <= 0 || height <= 0 || (channels != 1 && channels != 3) || n_frames <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((width + 1023) / 1024), grid_cap(height), grid_cap(n_frames));
    if (channels == 1)
        hipLaunchKernelGGL(convert_image_kernel<1>, grid, dim3(256), 0, st, src, dst, width, height, n_frames);
    else
        hipLaunchKernelGGL(convert_image_kernel<3>, grid, dim3(256), 0, st, src, dst, width, height, n_frames);
    return hipGetLastError();
}

// ---- the antialiased cubic resize (srcnn_resize_cubic_aa_*): resample_aa_* kernels ----------------------------------------
// Per axis a table gives every output sample its first source sample, its tap count and its coefficients (srcnn_cubic_aa_f32_taps:
// first + count never leaves the plane, so no index is clamped).  Horizontal pass first, then the vertical one; each computes
// acc = x_0 w_0, then acc = acc + x_j w_j for j ascending over exactly `count` taps, every product and sum rounded on its own
// (this unit is built without FMA contraction).  The intermediate is float32.  Tile geometry and the two forms: srcnn_image.h.
// In both passes a LANE is an output COLUMN.  Horizontal: neighbouring lanes read source columns rho apart with overlapping
// supports, so the taps of one row come out of the same few cache lines, and the coefficient table is tap-major so that a tap's
// coefficients are one coalesced load.  Vertical: the row and with it `first`, `count` and the coefficients are the same for a
// whole wave (scalar loads), and the lanes read neighbouring floats of the intermediate: no LDS bank is hit twice.
// The source's element kind is a workgroup-uniform switch AROUND the horizontal pass (one kernel, four bodies of its tap loop);
// the destination's is the switch inside image_store.
struct AaArgs {
    ImageRef src, dst;
    int sw, sh, dw, dh, channels, n_planes;
    ResampleAaTables t;
    float *work;      // general form: n_planes x sh x dw floats
};

template <int ELEM>
__device__ __forceinline__ float aa_load(const ImageRef &im, long at)      // image_load of a known element kind
{
    if (ELEM == ELEM_F32) return static_cast<const float *>(im.data)[at];
    if (ELEM == ELEM_F16) return (float)static_cast<const _Float16 *>(im.data)[at];
    if (ELEM == ELEM_BF16) return __uint_as_float((unsigned)static_cast<const uint16_t *>(im.data)[at] << 16);
    return __fmul_rn((float)static_cast<const uint8_t *>(im.data)[at], im.scale);
}

// Horizontal pass of a tile: source rows [r_lo, r_lo + nrow) of the plane at element offset s, output column dxc (the lane's,
// clamped to the plane) -> hbuf[row][lane].  Wave w takes rows w, w + 4, ...; four of them at a time share a coefficient load.
template <int ELEM>
__device__ __forceinline__ void aa_tile_hpass(float (*hbuf)[AA_TC], const AaArgs &a, long s, int r_lo, int nrow, int dxc)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cnt = a.t.xcount[dxc];
    const float *coef = a.t.xcoef + dxc;
    const long col = s + (long)a.t.xfirst[dxc] * a.src.px_step;
    for (int r0 = w; r0 < nrow; r0 += 16) {
        long row[4];
        float acc[4];
        const float w0 = coef[0];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            row[k] = col + (long)min(r_lo + r0 + 4 * k, a.sh - 1) * a.src.stride;      // (rows beyond the tile: computed, not kept)
            acc[k] = __fmul_rn(aa_load<ELEM>(a.src, row[k]), w0);
        }
        for (int j = 1; j < cnt; ++j) {
            const float wj = coef[(long)j * a.dw];
            const long o = (long)j * a.src.px_step;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(aa_load<ELEM>(a.src, row[k] + o), wj));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (r0 + 4 * k < nrow) hbuf[r0 + 4 * k][lane] = acc[k];
    }
}

// Vertical pass of a tile: output rows [dy0, dy1), wave w takes dy0 + w, dy0 + w + 4, ...; column dx of the plane at element
// offset d of the destination
__device__ __forceinline__ void aa_tile_vpass(const float (*hbuf)[AA_TC], const AaArgs &a, long d, int dy0, int dy1, int r_lo, int dx)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int dy = dy0 + w; dy < dy1; dy += 4) {
        const int j0 = a.t.yfirst[dy] - r_lo, cnt = a.t.ycount[dy];
        const float *coef = a.t.ycoef + (long)dy * a.t.ky;
        float acc = __fmul_rn(hbuf[j0][lane], coef[0]);
        for (int j = 1; j < cnt; ++j) acc = __fadd_rn(acc, __fmul_rn(hbuf[j0 + j][lane], coef[j]));
        if (dx < a.dw) image_store(a.dst, d + (long)dy * a.dst.stride + (long)dx * a.dst.px_step, acc);
    }
}

__global__ __launch_bounds__(256) void resample_aa_tiled_kernel(const AaArgs a)
{
    __shared__ float hbuf[AA_RMAX][AA_TC];
    const int dx = blockIdx.x * AA_TC + (threadIdx.x & 63);
    const int dxc = min(dx, a.dw - 1);
    const int n_row_tiles = (a.dh + AA_TR - 1) / AA_TR;
    for (int z = blockIdx.z; z < a.n_planes; z += gridDim.z) {
        const int frame = z / a.channels, ch = z - frame * a.channels;
        const long s = frame * a.src.frame_pitch + ch * a.src.ch_pitch;
        const long d = frame * a.dst.frame_pitch + ch * a.dst.ch_pitch;
        for (int rt = blockIdx.y; rt < n_row_tiles; rt += gridDim.y) {
            const int dy0 = rt * AA_TR, dy1 = min(dy0 + AA_TR, a.dh);
            const int r_lo = a.t.yfirst[dy0];
            const int nrow = a.t.yfirst[dy1 - 1] + a.t.ycount[dy1 - 1] - r_lo;      // <= AA_RMAX: resample_aa_variant()
            switch (a.src.elem) {
            case ELEM_F32: aa_tile_hpass<ELEM_F32>(hbuf, a, s, r_lo, nrow, dxc); break;
            case ELEM_F16: aa_tile_hpass<ELEM_F16>(hbuf, a, s, r_lo, nrow, dxc); break;
            case ELEM_BF16: aa_tile_hpass<ELEM_BF16>(hbuf, a, s, r_lo, nrow, dxc); break;
            default: aa_tile_hpass<ELEM_U8>(hbuf, a, s, r_lo, nrow, dxc); break;
            }
            __syncthreads();
            aa_tile_vpass(hbuf, a, d, dy0, dy1, r_lo, dx);
            __syncthreads();      // the next tile's horizontal pass overwrites what this vertical pass reads
        }
    }
}

// General form, first launch: the horizontal pass of every source row into the workspace (thread = output column)
template <int ELEM>
__device__ __forceinline__ void aa_rows_hpass(const AaArgs &a, int dx)
{
    const int cnt = a.t.xcount[dx];
    const float *coef = a.t.xcoef + dx;
    const float w0 = coef[0];
    const long col = (long)a.t.xfirst[dx] * a.src.px_step;
    for (int z = blockIdx.z; z < a.n_planes; z += gridDim.z) {
        const int frame = z / a.channels, ch = z - frame * a.channels;
        const long s = frame * a.src.frame_pitch + ch * a.src.ch_pitch + col;
        float *o = a.work + (long)z * a.sh * a.dw + dx;
        for (int y = blockIdx.y; y < a.sh; y += gridDim.y) {
            const long row = s + (long)y * a.src.stride;
            float acc = __fmul_rn(aa_load<ELEM>(a.src, row), w0);
            for (int j = 1; j < cnt; ++j)
                acc = __fadd_rn(acc, __fmul_rn(aa_load<ELEM>(a.src, row + (long)j * a.src.px_step), coef[(long)j * a.dw]));
            o[(long)y * a.dw] = acc;
        }
    }
}

__global__ __launch_bounds__(256) void resample_aa_h_kernel(const AaArgs a)
{
    const int dx = blockIdx.x * 256 + threadIdx.x;
    if (dx >= a.dw) return;
    switch (a.src.elem) {
    case ELEM_F32: aa_rows_hpass<ELEM_F32>(a, dx); break;
    case ELEM_F16: aa_rows_hpass<ELEM_F16>(a, dx); break;
    case ELEM_BF16: aa_rows_hpass<ELEM_BF16>(a, dx); break;
    default: aa_rows_hpass<ELEM_U8>(a, dx); break;
    }
}

// ... second launch: the vertical pass out of the workspace (thread = output column, a block's row is blockIdx.y's)
__global__ __launch_bounds__(256) void resample_aa_v_kernel(const AaArgs a)
{
    const int dx = blockIdx.x * 256 + threadIdx.x;
    if (dx >= a.dw) return;
    for (int z = blockIdx.z; z < a.n_planes; z += gridDim.z) {
        const int frame = z / a.channels, ch = z - frame * a.channels;
        const float *h = a.work + (long)z * a.sh * a.dw + dx;
        const long d = frame * a.dst.frame_pitch + ch * a.dst.ch_pitch + (long)dx * a.dst.px_step;
        for (int dy = blockIdx.y; dy < a.dh; dy += gridDim.y) {
            const int cnt = a.t.ycount[dy];
            const float *coef = a.t.ycoef + (long)dy * a.t.ky;
            const float *p = h + (long)a.t.yfirst[dy] * a.dw;
            float acc = __fmul_rn(p[0], coef[0]);
            for (int j = 1; j < cnt; ++j) acc = __fadd_rn(acc, __fmul_rn(p[(long)j * a.dw], coef[j]));
            image_store(a.dst, d + (long)dy * a.dst.stride, acc);
        }
    }
}

hipError_t launch_resample_aa(const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels, int n_frames,
                              const ResampleAaTables &t, int variant, float *work, hipStream_t st)
{
    if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || channels <= 0 || n_frames <= 0 || (long)channels * n_frames > 0x7fffffffL ||
        t.kx <= 0 || t.ky <= 0)
        return hipErrorInvalidValue;
    const AaArgs a{src, dst, sw, sh, dw, dh, channels, channels * n_frames, t, work};
    const unsigned gz = grid_cap(a.n_planes);
    if (variant == RESAMPLE_AA_TILED) {
        if (resample_aa_variant(sw, sh, dw, dh, t.kx, t.ky) != RESAMPLE_AA_TILED) return hipErrorInvalidValue;
        hipLaunchKernelGGL(resample_aa_tiled_kernel, dim3((dw + AA_TC - 1) / AA_TC, grid_cap((dh + AA_TR - 1) / AA_TR), gz), dim3(256),
                           0, st, a);
        return hipGetLastError();
    }
    if (!work) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_aa_h_kernel, dim3((dw + 255) / 256, grid_cap(sh), gz), dim3(256), 0, st, a);
    hipLaunchKernelGGL(resample_aa_v_kernel, dim3((dw + 255) / 256, grid_cap(dh), gz), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---- Pillow's resize of uint8 images (srcnn_resize_pil_image_dev): resample_pil_* kernels -----------------------------------
// The resample_aa_* kernels' shape on integers.  Per axis a table gives every output sample its first source sample, its tap
// count and its int32 coefficients with PIL_BITS fractional bits (srcnn_pil_taps; an axis that keeps its length has the identity
// table, one tap of 1 << PIL_BITS, which returns the byte untouched: (b << 22 + (1 << 21)) >> 22 = b).  A pass computes
// acc = 1 << 21, acc += byte * c_j for j ascending, out = min(max(acc >> 22, 0), 255): a uint8 after the horizontal pass (in LDS
// or in the workspace) and again after the vertical one.  The host has checked sum |c_j| < 2^23 for every output sample of the
// tables it hands over, so every |c_j| fits the signed 24-bit multiply and |acc| <= 2^21 + 255 (2^23 - 1) < 2^31.
// Both sides are SRCNN_ELEM_U8 descriptors whose scale is not read; lanes, loads and the tap-major x table are resample_aa's.
struct PilArgs {
    ImageRef src, dst;
    int sw, sh, dw, dh, channels, n_planes;
    ResamplePilTables t;
    uint8_t *work;      // general form: n_planes x sh x dw bytes
};

__device__ __forceinline__ int pil_clip8(int acc) { return min(max(acc >> PIL_BITS, 0), 255); }
constexpr int kPilHalf = 1 << (PIL_BITS - 1);

// Horizontal pass of a tile: source rows [r_lo, r_lo + nrow) of the plane at element offset s, output column dxc (the lane's,
// clamped to the plane) -> hbuf[row][lane], a byte.  Wave w takes rows w, w + 4, ...; four of them share a coefficient load.
__device__ __forceinline__ void pil_tile_hpass(uint8_t (*hbuf)[PIL_TC], const PilArgs &a, long s, int r_lo, int nrow, int dxc)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint8_t *p = static_cast<const uint8_t *>(a.src.data);
    const int cnt = a.t.xcount[dxc];
    const int *coef = a.t.xcoef + dxc;
    const long col = s + (long)a.t.xfirst[dxc] * a.src.px_step;
    for (int r0 = w; r0 < nrow; r0 += 16) {
        long row[4];
        int acc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            row[k] = col + (long)min(r_lo + r0 + 4 * k, a.sh - 1) * a.src.stride;      // (rows beyond the tile: computed, not kept)
            acc[k] = kPilHalf;
        }
        for (int j = 0; j < cnt; ++j) {
            const int cj = coef[(long)j * a.dw];
            const long o = (long)j * a.src.px_step;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += __mul24((int)p[row[k] + o], cj);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (r0 + 4 * k < nrow) hbuf[r0 + 4 * k][lane] = (uint8_t)pil_clip8(acc[k]);
    }
}

// Vertical pass of a tile: output rows [dy0, dy1), wave w takes dy0 + w, dy0 + w + 4, ...; column dx of the plane at element
// offset d of the destination
__device__ __forceinline__ void pil_tile_vpass(const uint8_t (*hbuf)[PIL_TC], const PilArgs &a, long d, int dy0, int dy1, int r_lo, int dx)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *q = static_cast<uint8_t *>(a.dst.data);
    for (int dy = dy0 + w; dy < dy1; dy += 4) {
        const int j0 = a.t.yfirst[dy] - r_lo, cnt = a.t.ycount[dy];
        const int *coef = a.t.ycoef + (long)dy * a.t.ky;
        int acc = kPilHalf;
        for (int j = 0; j < cnt; ++j) acc += __mul24((int)hbuf[j0 + j][lane], coef[j]);
        if (dx < a.dw) q[d + (long)dy * a.dst.stride + (long)dx * a.dst.px_step] = (uint8_t)pil_clip8(acc);
    }
}

__global__ __launch_bounds__(256) void resample_pil_tiled_kernel(const PilArgs a)
{
    __shared__ uint8_t hbuf[PIL_RMAX][PIL_TC];
    const int dx = blockIdx.x * PIL_TC + (threadIdx.x & 63);
    const int dxc = min(dx, a.dw - 1);
    const int n_row_tiles = (a.dh + PIL_TR - 1) / PIL_TR;
    for (int z = blockIdx.z; z < a.n_planes; z += gridDim.z) {
        const int frame = z / a.channels, ch = z - frame * a.channels;
        const long s = frame * a.src.frame_pitch + ch * a.src.ch_pitch;
        const long d = frame * a.dst.frame_pitch + ch * a.dst.ch_pitch;
        for (int rt = blockIdx.y; rt < n_row_tiles; rt += gridDim.y) {
            const int dy0 = rt * PIL_TR, dy1 = min(dy0 + PIL_TR, a.dh);
            const int r_lo = a.t.yfirst[dy0];
            const int nrow = a.t.yfirst[dy1 - 1] + a.t.ycount[dy1 - 1] - r_lo;      // <= t.tile_span <= PIL_RMAX: launch_resample_pil()
            pil_tile_hpass(hbuf, a, s, r_lo, nrow, dxc);
            __syncthreads();
            pil_tile_vpass(hbuf, a, d, dy0, dy1, r_lo, dx);
            __syncthreads();      // the next tile's horizontal pass overwrites what this vertical pass reads
        }
    }
}

// General form, first launch: the horizontal pass of every source row into the byte workspace (thread = output column)
__global__ __launch_bounds__(PIL_HC) void resample_pil_h_kernel(const PilArgs a)
{
    const int dx = blockIdx.x * PIL_HC + threadIdx.x;
    if (dx >= a.dw) return;
    const uint8_t *p = static_cast<const uint8_t *>(a.src.data);
    const int cnt = a.t.xcount[dx];
    const int *coef = a.t.xcoef + dx;
    const long col = (long)a.t.xfirst[dx] * a.src.px_step;
    for (int z = blockIdx.z; z < a.n_planes; z += gridDim.z) {
        const int frame = z / a.channels, ch = z - frame * a.channels;
        const long s = frame * a.src.frame_pitch + ch * a.src.ch_pitch + col;
        uint8_t *o = a.work + (long)z * a.sh * a.dw + dx;
        for (int y = blockIdx.y; y < a.sh; y += gridDim.y) {
            const long row = s + (long)y * a.src.stride;
            int acc = kPilHalf;
            for (int j = 0; j < cnt; ++j) acc += __mul24((int)p[row + (long)j * a.src.px_step], coef[(long)j * a.dw]);
            o[(long)y * a.dw] = (uint8_t)pil_clip8(acc);
        }
    }
}

// ... second launch: the vertical pass out of the workspace (thread = output column, a block's row is blockIdx.y's)
__global__ __launch_bounds__(PIL_HC) void resample_pil_v_kernel(const PilArgs a)
{
    const int dx = blockIdx.x * PIL_HC + threadIdx.x;
    if (dx >= a.dw) return;
    uint8_t *q = static_cast<uint8_t *>(a.dst.data);
    for (int z = blockIdx.z; z < a.n_planes; z += gridDim.z) {
        const int frame = z / a.channels, ch = z - frame * a.channels;
        const uint8_t *h = a.work + (long)z * a.sh * a.dw + dx;
        const long d = frame * a.dst.frame_pitch + ch * a.dst.ch_pitch + (long)dx * a.dst.px_step;
        for (int dy = blockIdx.y; dy < a.dh; dy += gridDim.y) {
            const int cnt = a.t.ycount[dy];
            const int *coef = a.t.ycoef + (long)dy * a.t.ky;
            const uint8_t *r = h + (long)a.t.yfirst[dy] * a.dw;
            int acc = kPilHalf;
            for (int j = 0; j < cnt; ++j) acc += __mul24((int)r[(long)j * a.dw], coef[j]);
            q[d + (long)dy * a.dst.stride] = (uint8_t)pil_clip8(acc);
        }
    }
}

hipError_t launch_resample_pil(const ImageRef &src, int sw, int sh, const ImageRef &dst, int dw, int dh, int channels, int n_frames,
                               const ResamplePilTables &t, int variant, uint8_t *work, hipStream_t st)
{
    if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || channels <= 0 || n_frames <= 0 || (long)channels * n_frames > 0x7fffffffL ||
        t.kx <= 0 || t.ky <= 0 || src.elem != ELEM_U8 || dst.elem != ELEM_U8)
        return hipErrorInvalidValue;
    const PilArgs a{src, dst, sw, sh, dw, dh, channels, channels * n_frames, t, work};
    const unsigned gz = grid_cap(a.n_planes);
    if (variant == RESAMPLE_PIL_TILED) {
        // the rows a tile spans, as the tables themselves have them (t.tile_span: the host's walk over yfirst / ycount)
        if (t.tile_span <= 0 || t.tile_span > PIL_RMAX) return hipErrorInvalidValue;
        hipLaunchKernelGGL(resample_pil_tiled_kernel, dim3((dw + PIL_TC - 1) / PIL_TC, grid_cap((dh + PIL_TR - 1) / PIL_TR), gz),
                           dim3(256), 0, st, a);
        return hipGetLastError();
    }
    if (!work) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_pil_h_kernel, dim3((dw + PIL_HC - 1) / PIL_HC, grid_cap(sh), gz), dim3(PIL_HC), 0, st, a);
    hipLaunchKernelGGL(resample_pil_v_kernel, dim3((dw + PIL_HC - 1) / PIL_HC, grid_cap(dh), gz), dim3(PIL_HC), 0, st, a);
    return hipGetLastError();
}

}  // namespace srcnn
