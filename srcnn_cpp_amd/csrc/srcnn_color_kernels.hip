// srcnn_color_kernels.hip -- layers 1 and 3 of the colour SRCNN models (srcnn_set_model_color: 3 input and 3 output channels,
// 9-f2-5, f2 = 1, 3, 5), for gfx950.
//
// A colour model runs on the banded path of the 9-3-5 / 9-5-5 models (srcnn_color.cpp), three launches per row band:
//
//   color_l1_kernel     3 u8 channels -> 64 planar f32 maps (layer 1, + bias, ReLU): the maps spatial_l1_kernel writes
//   spatial_l2_kernel   64 maps -> 32 maps (srcnn_spatial_kernels.hip), unchanged
//   color_l3_kernel     32 maps -> 3 channels (layer 3, + b3[c], truncate, clamp): interleaved u8 and pre-clamp floats
//
// The input is read at src[y * sstride + x * px_step + c * ch_step]: px_step = 3, ch_step = 1 for interleaved 3-byte pixels
// (srcnn_forward_color*), px_step = 1, ch_step = plane pitch for the three resized planes of srcnn_process_bgr.  Model channel c
// reads byte c of a pixel and writes byte c of an output pixel.
//
// Both kernels use v_mfma_f32_32x32x2_f32 as srcnn_spatial_kernels.hip does (weights as A, one pixel per lane as B).
// Padding: each layer pads its own input.  ZERO = false (replicate): layer 1 clamps the image coordinates, layer 3 reads
// clamped map rows and columns; ZERO = true: layer 1 stages 0 outside the image, layer 3 zeroes the tap partials of map
// pixels outside the image (as spatial_l3z_kernel does).
//
// Summation order (each MFMA is a 2-term fmaf chain, srcnn_mfma.hip):
//   layer 1, channel k:  0 + sum over c = 0, 1, 2 of (w1[k][c][0] x0 + ... + w1[k][c][80] x80 + t_c), taps row-major,
//                        where t_0 = t_1 = 0 * 1 (a zero tap) and t_2 = b1[k] * 1 (the bias tap)
//   layer 2:             srcnn_spatial_kernels.hip
//   layer 3, channel o:  per map pixel the tap partials T[tap] = sum_c w3[o][c][tap] F_c (channel pairs ascending), summed
//                        down the 5 tap rows (m ascending), then ((((V_0 + V_1) + V_2) + V_3) + V_4) + b3[o]
#include "srcnn_kernels.h"

namespace srcnn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define CMFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int cclamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- layer 1 ----------------------------------------------------------------------------------------------------------
// Workgroup: 4 waves, a tile of CL1_COLS columns x CL1_ROWS rows, as spatial_l1_kernel.  Per row 246 MFMAs per wave (3
// channels x 2 channel tiles x 41 k-steps of 2 taps).  LDS: the three channels' A fragments (COLOR_NFRAG_L1 x 64 floats,
// 61.5 KiB) and the u8 window of the three channels (6.4 KiB): 68 KiB, two workgroups per CU.
constexpr int CL1_COLS = 128, CL1_ROWS = 8;
constexpr int CL1_YP = CL1_COLS + 8, CL1_YR = CL1_ROWS + 8, CL1_YC = CL1_YR * CL1_YP;
constexpr size_t CL1_LDS = (size_t)COLOR_NFRAG_L1 * 64 * sizeof(float) + 3 * CL1_YC;

template <bool ZERO>
__global__ __launch_bounds__(256) void color_l1_kernel(const uint8_t *__restrict__ src, long sstride, int px_step, long ch_step,
                                                       int W, int H, int m0, int m1, const float *__restrict__ frag,
                                                       float *__restrict__ map, long mpitch)
{
    extern __shared__ float lds[];
    float *as = lds;
    uint8_t *ys = reinterpret_cast<uint8_t *>(lds + COLOR_NFRAG_L1 * 64);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * CL1_COLS, y0 = m0 + blockIdx.y * CL1_ROWS;
    // the window, channel fastest (consecutive bytes of interleaved pixels go to consecutive threads)
    for (int e = tid; e < 3 * CL1_YC; e += 256) {
        const int rr = e / (3 * CL1_YP), rem = e - rr * (3 * CL1_YP), cc = rem / 3, ch = rem - 3 * cc;
        const int yy = cclamp(y0 - 4 + rr, 0, H - 1), xx = cclamp(x0 - 4 + cc, 0, W - 1);
        const int v = src[(long)yy * sstride + (long)xx * px_step + ch * ch_step];
        // ZERO: 0 where the load was clamped, by a multiply (no branch around the load, as in spatial_l1_kernel)
        if constexpr (ZERO) ys[ch * CL1_YC + rr * CL1_YP + cc] = (uint8_t)(v * (int)(yy == y0 - 4 + rr && xx == x0 - 4 + cc));
        else ys[ch * CL1_YC + rr * CL1_YP + cc] = (uint8_t)v;
    }
    const float4 *fa = reinterpret_cast<const float4 *>(frag);
    for (int e = tid; e < COLOR_NFRAG_L1 * 16; e += 256) reinterpret_cast<float4 *>(as)[e] = fa[e];
    __syncthreads();
    const int j = lane & 31, kk = lane >> 5;
    const int x = x0 + 32 * wave + j;
    for (int r = 0; r < CL1_ROWS; ++r) {
        const int y = y0 + r;
        if (y >= m1) break;                        // uniform over the workgroup
        f32x16 acc0 = {0}, acc1 = {0};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint8_t *yc = ys + ch * CL1_YC + r * CL1_YP + 32 * wave + j;
            const float *ac = as + ch * (2 * 41 * 64) + lane;
#pragma unroll
            for (int s = 0; s < 41; ++s) {
                const int tap = 2 * s + kk;        // 81: the zero / bias tap, B = 1
                const int ty = tap / 9, tx = tap - 9 * (tap / 9);
                const float b = tap < 81 ? (float)yc[ty * CL1_YP + tx] : 1.f;
                acc0 = CMFMA(ac[s * 64], b, acc0);
                acc1 = CMFMA(ac[(41 + s) * 64], b, acc1);
            }
        }
        if (x < W) {
            float *o = map + (long)(y - m0) * W + x;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int ch = acc_row(q, kk);
                o[(long)ch * mpitch] = __builtin_fmaxf(acc0[q], 0.f);
                o[(long)(32 + ch) * mpitch] = __builtin_fmaxf(acc1[q], 0.f);
            }
        }
    }
}

// ---- layer 3 ----------------------------------------------------------------------------------------------------------
// spatial_l3z_kernel with three A sets: workgroup of 4 waves, a strip of CL3_COLS = 128 map columns (image columns
// 124 bx - 2 ..), the middle CL3_OUT = 124 of them output, and a segment of CL3_SEG output rows; wave w owns map columns
// 32w .. 32w + 31 and walks the map rows y0 - 2 .. y1 + 1.  Per map row 3 x 16 MFMAs give the 75 tap partials (3 output
// channels x 25 taps; A set o: W3[o] with the rows of l3_row_tap()); the loads are clamped to the band's rows and the image's
// columns, which is replicate padding, and ZERO sets the partials of a map pixel outside the image to 0.  The 5 tap rows are
// summed down register chains, the per-tap-column sums V_n of the three channels cross lanes through a double-buffered LDS
// row, and a lane of half 0 finishes its pixel's three channels.  The map read (128 B per pixel) is the one of spatial_l3z.
constexpr int CL3_COLS = 128, CL3_OUT = CL3_COLS - 4, CL3_SEG = 16, CL3_XCDS = 8;
constexpr int CL3_AHEAD = 2;        // map rows in flight per wave (48 MFMAs per row cover the loads)

template <bool PRE, bool ZERO>
__global__ __launch_bounds__(256) void color_l3_kernel(const float *__restrict__ map, long mpitch, int o0, int o1, int W, int H,
                                                       int b0, int b1, int nx, int n_tiles, const float *__restrict__ frag,
                                                       float b30, float b31, float b32, uint8_t *__restrict__ dst, long dstride,
                                                       float *__restrict__ pre)
{
    __shared__ float vt[2][3][5][CL3_COLS];
    const int per = (n_tiles + CL3_XCDS - 1) / CL3_XCDS;
    const int tile = (int)(blockIdx.x % CL3_XCDS) * per + (int)(blockIdx.x / CL3_XCDS);
    if (tile >= n_tiles) return;                   // uniform over the workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, kk = lane >> 5;
    const int ty = tile / nx, tx = tile - ty * nx;
    const int c = 32 * wave + j, x = tx * CL3_OUT - 2 + c;
    const int y0 = b0 + ty * CL3_SEG, y1 = min(b1, y0 + CL3_SEG), r_end = y1 + 2;
    const bool col_ok = x >= 0 && x < W;
    const float b3[3] = {b30, b31, b32};
    float a[3][16];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int s = 0; s < 16; ++s) a[o][s] = frag[(o * 16 + s) * 64 + lane];
    // channels 2s + kk of map row r at the lane's column, from a clamped (always valid) address: no branch between the loads
    const float *colp = map + (long)kk * mpitch + cclamp(x, 0, W - 1);
    auto load = [&](int r, float *v) {
        const float *p = colp + (long)(cclamp(r, o0, o1 - 1) - o0) * W;
#pragma unroll
        for (int s = 0; s < 16; ++s) v[s] = p[(long)(2 * s) * mpitch];
    };
    float xr[CL3_AHEAD][16], chn[3][3][4];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int k = 0; k < 4; ++k) chn[o][s][k] = 0.f;
#pragma unroll
    for (int d = 0; d < CL3_AHEAD; ++d)
        if (y0 - 2 + d < r_end) load(y0 - 2 + d, xr[d]);
    for (int rb = y0 - 2; rb < r_end; rb += CL3_AHEAD) {
#pragma unroll
        for (int d = 0; d < CL3_AHEAD; ++d) {
            const int r = rb + d;
            if (r >= r_end) break;                 // uniform over the workgroup
            f32x16 t[3];
#pragma unroll
            for (int o = 0; o < 3; ++o) t[o] = (f32x16){0};
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int o = 0; o < 3; ++o) t[o] = CMFMA(a[o][s], xr[d][s], t[o]);
            if (r + CL3_AHEAD < r_end) load(r + CL3_AHEAD, xr[d]);
            const bool ok = !ZERO || (col_ok && r >= 0 && r < H);
            float v[3][3];
#pragma unroll
            for (int o = 0; o < 3; ++o)
#pragma unroll
                for (int s = 0; s < 3; ++s) {          // chn[o][s][k]: tap rows 0 .. k of output row r + 1 - k
                    v[o][s] = chn[o][s][3] + (ok ? t[o][5 * s + 4] : 0.f);
                    chn[o][s][3] = chn[o][s][2] + (ok ? t[o][5 * s + 3] : 0.f);
                    chn[o][s][2] = chn[o][s][1] + (ok ? t[o][5 * s + 2] : 0.f);
                    chn[o][s][1] = chn[o][s][0] + (ok ? t[o][5 * s + 1] : 0.f);
                    chn[o][s][0] = ok ? t[o][5 * s] : 0.f;
                }
            const int y = r - 2;
            if (y >= y0) {                             // uniform over the workgroup
                float *vr = &vt[r & 1][0][0][0];
#pragma unroll
                for (int o = 0; o < 3; ++o)
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        const int n = kk ? 3 + s : s;
                        if (n < 5) vr[(o * 5 + n) * CL3_COLS + c] = v[o][s];
                    }
                __syncthreads();
                if (kk == 0 && c >= 2 && c < CL3_COLS - 2 && x < W) {
                    const long ob = (long)y * dstride + 3L * x;
#pragma unroll
                    for (int o = 0; o < 3; ++o) {
                        const float *vo = vr + o * 5 * CL3_COLS;
                        const float sum = (((vo[c - 2] + vo[CL3_COLS + c - 1]) + vo[2 * CL3_COLS + c]) + vo[3 * CL3_COLS + c + 1]) +
                                          vo[4 * CL3_COLS + c + 2];
                        const float val = sum + b3[o];
                        dst[ob + o] = (uint8_t)cclamp((int)val, 0, 255);
                        if constexpr (PRE) pre[ob + o] = val;
                    }
                }
            }
        }
    }
}

hipError_t launch_color_l1(bool zero, const uint8_t *src, long sstride, int px_step, long ch_step, int W, int H, int m0, int m1,
                           const float *frag, float *map, long mpitch, hipStream_t st)
{
    const dim3 grid((unsigned)((W + CL1_COLS - 1) / CL1_COLS), (unsigned)((m1 - m0 + CL1_ROWS - 1) / CL1_ROWS));
    // (68 KiB exceed the default dynamic-LDS limit; set per call: the attribute is per device)
    if (zero) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(color_l1_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)CL1_LDS);
        hipLaunchKernelGGL(color_l1_kernel<true>, grid, dim3(256), CL1_LDS, st, src, sstride, px_step, ch_step, W, H, m0, m1, frag,
                           map, mpitch);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(color_l1_kernel<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)CL1_LDS);
        hipLaunchKernelGGL(color_l1_kernel<false>, grid, dim3(256), CL1_LDS, st, src, sstride, px_step, ch_step, W, H, m0, m1, frag,
                           map, mpitch);
    }
    return hipGetLastError();
}

template <bool PRE, bool ZERO>
static void launch_l3(dim3 grid, const float *map, long mpitch, int o0, int o1, int W, int H, int b0, int b1, int nx, int n_tiles,
                      const float *frag, const float *b3, uint8_t *dst, long dstride, float *pre, hipStream_t st)
{
    hipLaunchKernelGGL((color_l3_kernel<PRE, ZERO>), grid, dim3(256), 0, st, map, mpitch, o0, o1, W, H, b0, b1, nx, n_tiles, frag,
                       b3[0], b3[1], b3[2], dst, dstride, pre);
}

hipError_t launch_color_l3(bool zero, const float *map, long mpitch, int o0, int o1, int W, int H, int b0, int b1,
                           const float *frag, const float *b3, uint8_t *dst, long dstride, float *pre, hipStream_t st)
{
    const int nx = (W + CL3_OUT - 1) / CL3_OUT, ny = (b1 - b0 + CL3_SEG - 1) / CL3_SEG, n_tiles = nx * ny;
    const dim3 grid((unsigned)(CL3_XCDS * ((n_tiles + CL3_XCDS - 1) / CL3_XCDS)));
    if (pre && zero) launch_l3<true, true>(grid, map, mpitch, o0, o1, W, H, b0, b1, nx, n_tiles, frag, b3, dst, dstride, pre, st);
    else if (pre) launch_l3<true, false>(grid, map, mpitch, o0, o1, W, H, b0, b1, nx, n_tiles, frag, b3, dst, dstride, pre, st);
    else if (zero) launch_l3<false, true>(grid, map, mpitch, o0, o1, W, H, b0, b1, nx, n_tiles, frag, b3, dst, dstride, pre, st);
    else launch_l3<false, false>(grid, map, mpitch, o0, o1, W, H, b0, b1, nx, n_tiles, frag, b3, dst, dstride, pre, st);
    return hipGetLastError();
}

// ---- srcnn_process_bgr: interleaved BGR -> three planes (before the planar bicubic resize) ------------------------------
__global__ __launch_bounds__(256) void split3_kernel(const uint8_t *__restrict__ src, long sstride, int W, uint8_t *__restrict__ planes,
                                                     long ppitch)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const uint8_t *p = src + (long)y * sstride + 3L * x;
    uint8_t *q = planes + (long)y * W + x;
    q[0] = p[0];
    q[ppitch] = p[1];
    q[2 * ppitch] = p[2];
}

hipError_t launch_split3(const uint8_t *src, long sstride, int W, int H, uint8_t *planes, long ppitch, hipStream_t st)
{
    hipLaunchKernelGGL(split3_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)H), dim3(256), 0, st, src, sstride, W, planes,
                       ppitch);
    return hipGetLastError();
}

}  // namespace srcnn
