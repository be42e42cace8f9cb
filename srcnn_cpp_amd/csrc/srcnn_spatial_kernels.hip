// srcnn_spatial_kernels.hip -- layers 1 and 2 of the 9-3-5 / 9-5-5 SRCNN models (srcnn_set_model, f2 = 3 or 5), and the banded
// path of every model under zero padding (srcnn_set_padding), for gfx950.
//
// A spatial layer 2 (32 x 64 x f2 x f2) is 10 or 28 times the work of the 9-1-5 model's 1x1 layer and needs an f2 x f2 window
// of the 64-channel layer-1 map, which at 256 B per pixel does not fit beside the strip kernels' rings in LDS.  The path is
// therefore three launches per row band (srcnn_spatial.cpp):
//
//   spatial_l1_kernel   u8 luma -> 64 planar f32 maps (layer 1, + bias, ReLU)
//   spatial_l2_kernel   64 maps -> 32 planar f32 maps (layer 2, + bias, ReLU), in exactly the layout MODE_L3 reads
//   MODE_L3 strip kernel (srcnn_mfma.hip), unchanged: layer 3, truncate, clamp
//
// Both kernels use v_mfma_f32_32x32x2_f32 with the weights as the A operand (output channel on the accumulator ROW) and one
// pixel per lane as the B operand; accumulator register r of lane-half h holds output channel acc_row(r, h), lane & 31 the pixel.
// Each layer pads ITS OWN input.  Replicate padding (the default, ZERO = false): layer 1 clamps luma coordinates, layer 2 clamps
// layer-1 map coordinates, and layer 3 is MODE_L3.  Zero padding (srcnn_set_padding(SRCNN_PAD_ZERO), ZERO = true; also for
// f2 = 1): layers 1 and 2 stage 0 for every luma / map value outside the image, and layer 3 is spatial_l3z_kernel below,
// because MODE_L3 builds the replicate border into its column offsets and vertical chains.
//
// Summation order (each MFMA is a 2-term fmaf chain, srcnn_mfma.hip):
//   layer 1, channel c:  0 + w1[c][0] y0 + w1[c][1] y1 + ... + w1[c][80] y80 + b1[c]   (taps row-major, the bias tap last)
//   layer 2, channel k:  b2[k], then the input channels in chunks of 8 (ascending); inside a chunk the taps (kh, kw)
//                        row-major, inside a tap the channel pairs ascending, channel 2p before 2p + 1.
#include "srcnn_kernels.h"

namespace srcnn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define SMFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int sclamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- layer 1 ----------------------------------------------------------------------------------------------------------
// Workgroup: 4 waves, a tile of SL1_COLS columns x SL1_ROWS rows.  Wave w owns columns 32w .. 32w + 31 of the tile and walks
// its rows; per row 82 MFMAs (2 channel tiles x 41 k-steps of 2 taps).  LDS: the luma window (f32) and the 82 A fragments.
constexpr int SL1_COLS = 128, SL1_ROWS = 8;
constexpr int SL1_YP = SL1_COLS + 8, SL1_YR = SL1_ROWS + 8;

template <bool ZERO>
__global__ __launch_bounds__(256) void spatial_l1_kernel(const uint8_t *__restrict__ src, long sstride, int W, int H,
                                                         int m0, int m1, const float *__restrict__ frag,
                                                         float *__restrict__ map, long mpitch)
{
    __shared__ float ys[SL1_YR * SL1_YP];
    __shared__ float as[SPATIAL_NFRAG_L1 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * SL1_COLS, y0 = m0 + blockIdx.y * SL1_ROWS;
    for (int e = tid; e < SL1_YR * SL1_YP; e += 256) {
        const int rr = e / SL1_YP, cc = e - rr * SL1_YP;
        const int yy = sclamp(y0 - 4 + rr, 0, H - 1), xx = sclamp(x0 - 4 + cc, 0, W - 1);
        const float v = (float)src[(long)yy * sstride + xx];
        // ZERO: 0 where the load was clamped, by a multiply: a select lets the compiler branch around the load (measured slower)
        if constexpr (ZERO) ys[e] = v * ((yy == y0 - 4 + rr && xx == x0 - 4 + cc) ? 1.f : 0.f);
        else ys[e] = v;
    }
    for (int e = tid; e < SPATIAL_NFRAG_L1 * 64; e += 256) as[e] = frag[e];
    __syncthreads();
    const int j = lane & 31, kk = lane >> 5;
    const int x = x0 + 32 * wave + j;
    for (int r = 0; r < SL1_ROWS; ++r) {
        const int y = y0 + r;
        if (y >= m1) break;                        // uniform over the workgroup
        f32x16 acc0 = {0}, acc1 = {0};
#pragma unroll
        for (int s = 0; s < 41; ++s) {
            const int tap = 2 * s + kk;            // 81: the bias tap, B = 1
            const int ty = tap / 9, tx = tap - 9 * (tap / 9);
            const float b = tap < 81 ? ys[(r + ty) * SL1_YP + 32 * wave + j + tx] : 1.f;
            acc0 = SMFMA(as[s * 64 + lane], b, acc0);
            acc1 = SMFMA(as[(41 + s) * 64 + lane], b, acc1);
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

// ---- layer 2 ----------------------------------------------------------------------------------------------------------
// Workgroup: 4 waves, a tile of SL2_COLS = 64 columns x SL2_ROWS = 16 output rows.  Wave w owns rows 4w .. 4w + 3 and both
// 32-column units of each: 8 accumulators, so every A fragment read from LDS feeds 8 MFMAs.  The K loop walks the 64 input
// channels in chunks of SL2_CC = 8: per chunk the 8 channels' (16 + 2 r2) x (64 + 2 r2) window (replicate-clamped at the image
// edges) and the chunk's f2 x f2 x 4 A fragments are staged in LDS, then 8 x f2^2 x 4 MFMAs run per wave.
// A channel plane of the window is SL2_PS floats, = 32 mod 64: the two lane-halves (channels 2p, 2p + 1) read disjoint banks.
constexpr int SL2_COLS = 64, SL2_ROWS = 16, SL2_CC = 8, SL2_XP = 72;
__host__ __device__ constexpr int sl2_ps(int r2) { return ((((SL2_ROWS + 2 * r2) * SL2_XP) + 31) / 64) * 64 + 32; }
size_t spatial_l2_lds_bytes(int f2)
{
    return ((size_t)SL2_CC * sl2_ps((f2 - 1) / 2) + (size_t)f2 * f2 * (SL2_CC / 2) * 64) * sizeof(float);
}

template <int F2, bool ZERO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void spatial_l2_kernel(const float *__restrict__ map, long mpitch, int m0, int m1,
                                                         int W, int H, int o0, int o1, const float *__restrict__ frag,
                                                         const float *__restrict__ bias, float *__restrict__ out, long opitch)
{
    constexpr int R = (F2 - 1) / 2, PS = sl2_ps(R), WR = SL2_ROWS + 2 * R, WC = SL2_COLS + 2 * R;
    constexpr int NA = F2 * F2 * (SL2_CC / 2) * 64;          // A floats per chunk
    extern __shared__ float lds[];
    float *xs = lds, *as = lds + SL2_CC * PS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, kk = lane >> 5;
    const int x0 = blockIdx.x * SL2_COLS, y0 = o0 + blockIdx.y * SL2_ROWS;
    f32x16 acc[8];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float b = bias[acc_row(q, kk)];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u][q] = b;
    }
    for (int chunk = 0; chunk < 64 / SL2_CC; ++chunk) {
        __syncthreads();
        for (int e = tid; e < SL2_CC * WR * WC; e += 256) {
            const int c = e / (WR * WC), rem = e - c * (WR * WC), rr = rem / WC, cc = rem - rr * WC;
            // image row, replicate-clamped, then kept inside the rows the map holds (only rows that are not stored differ)
            const int yy = sclamp(sclamp(y0 - R + rr, 0, H - 1), m0, m1 - 1), xx = sclamp(x0 - R + cc, 0, W - 1);
            const float v = map[(long)(SL2_CC * chunk + c) * mpitch + (long)(yy - m0) * W + xx];
            if constexpr (ZERO) {   // 0 outside the image: the replicate load times 0 (as in layer 1: no branch around the load)
                const int iy = y0 - R + rr, ix = x0 - R + cc;
                xs[c * PS + rr * SL2_XP + cc] = v * ((iy >= 0 && iy < H && ix >= 0 && ix < W) ? 1.f : 0.f);
            } else {
                xs[c * PS + rr * SL2_XP + cc] = v;
            }
        }
        const float4 *fa = reinterpret_cast<const float4 *>(frag + (size_t)chunk * NA);
        for (int e = tid; e < NA / 4; e += 256) reinterpret_cast<float4 *>(as)[e] = fa[e];
        __syncthreads();
        const float *xb = xs + kk * PS + (4 * wave) * SL2_XP + j;
        for (int kh = 0; kh < F2; ++kh) {
#pragma unroll
            for (int kw = 0; kw < F2; ++kw) {
#pragma unroll
                for (int pp = 0; pp < SL2_CC / 2; ++pp) {
                    const float a = as[((kh * F2 + kw) * (SL2_CC / 2) + pp) * 64 + lane];
                    const float *xq = xb + 2 * pp * PS + kh * SL2_XP + kw;
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc[u] = SMFMA(a, xq[(u >> 1) * SL2_XP + 32 * (u & 1)], acc[u]);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int y = y0 + 4 * wave + (u >> 1), x = x0 + 32 * (u & 1) + j;
        if (y < o1 && x < W) {
            float *o = out + (long)(y - o0) * W + x;
#pragma unroll
            for (int q = 0; q < 16; ++q) o[(long)acc_row(q, kk) * opitch] = __builtin_fmaxf(acc[u][q], 0.f);
        }
    }
}

// ---- layer 3 under zero padding ---------------------------------------------------------------------------------------
// Workgroup: 4 waves, a strip of SL3_COLS = 128 map columns (image columns 124 bx - 2 ..), of which the middle SL3_OUT = 124
// are output, and a segment of SL3_SEG output rows; wave w owns map columns 32w .. 32w + 31 and walks the map rows
// y0 - 2 .. y1 + 1.  Per map row 16 MFMAs give the 25 tap partials T[tap] = sum_c W3[c][tap] F_c (A: W3 with the rows of
// l3_row_tap(); B: the 32 channels of the lane's pixel; the partials of a pixel outside the image are set to 0), so register
// 5s + m of lane-half h holds tap (m, n = s (h = 0) or 3 + s (h = 1)).  Each wave keeps SL3_AHEAD map rows of loads in
// flight (the kernel is bound by the 128 B per pixel it reads).  The 5 tap rows are summed down register chains, m ascending; the finished
// per-tap-column sums V_n cross lanes through a double-buffered LDS row, and
//   out(y, x) = (V_0(x - 2) + V_1(x - 1) + V_2(x) + V_3(x + 1) + V_4(x + 2)) + b3,  truncated, clamped to 0..255
// (the epilogue of MODE_L3).  Zero padding needs no clamp in the sums: a feature outside the image contributes T = 0.
// The map rows outside the band that the image holds are inside [o0, o1) (srcnn_spatial.cpp); the tiles are handed out
// XCD by XCD (block b runs on XCD b % 8), so horizontally neighbouring strips share their halo columns in one L2.
constexpr int SL3_COLS = 128, SL3_OUT = SL3_COLS - 4, SL3_SEG = 16, SL3_XCDS = 8;
constexpr int SL3_AHEAD = 4;        // map rows in flight per wave: a ring of SL3_AHEAD x 16 registers

template <bool PRE>
__global__ __launch_bounds__(256) void spatial_l3z_kernel(const float *__restrict__ map, long mpitch, int o0, int o1, int W,
                                                          int H, int b0, int b1, int nx, int n_tiles,
                                                          const float *__restrict__ frag, float b3, uint8_t *__restrict__ dst,
                                                          long dstride, float *__restrict__ pre)
{
    __shared__ float vt[2][5][SL3_COLS];
    const int per = (n_tiles + SL3_XCDS - 1) / SL3_XCDS;
    const int tile = (int)(blockIdx.x % SL3_XCDS) * per + (int)(blockIdx.x / SL3_XCDS);
    if (tile >= n_tiles) return;                   // uniform over the workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, kk = lane >> 5;
    const int ty = tile / nx, tx = tile - ty * nx;
    const int c = 32 * wave + j, x = tx * SL3_OUT - 2 + c;
    const int y0 = b0 + ty * SL3_SEG, y1 = min(b1, y0 + SL3_SEG), r_end = y1 + 2;
    const bool col_ok = x >= 0 && x < W;
    float a[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) a[s] = frag[s * 64 + lane];
    // channels 2s + kk of map row r at the lane's column, from a clamped (always valid) address: no branch between the loads;
    // the rows and columns outside the image are zeroed in the tap partials instead
    const float *colp = map + (long)kk * mpitch + sclamp(x, 0, W - 1);
    auto load = [&](int r, float *v) {
        const float *p = colp + (long)(sclamp(r, o0, o1 - 1) - o0) * W;
#pragma unroll
        for (int s = 0; s < 16; ++s) v[s] = p[(long)(2 * s) * mpitch];
    };
    float xr[SL3_AHEAD][16], ch[3][4];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int k = 0; k < 4; ++k) ch[s][k] = 0.f;
#pragma unroll
    for (int d = 0; d < SL3_AHEAD; ++d)
        if (y0 - 2 + d < r_end) load(y0 - 2 + d, xr[d]);
    for (int rb = y0 - 2; rb < r_end; rb += SL3_AHEAD) {
#pragma unroll
        for (int d = 0; d < SL3_AHEAD; ++d) {
            const int r = rb + d;
            if (r >= r_end) break;                 // uniform over the workgroup
            f32x16 t = {0};
#pragma unroll
            for (int s = 0; s < 16; ++s) t = SMFMA(a[s], xr[d][s], t);
            if (r + SL3_AHEAD < r_end) load(r + SL3_AHEAD, xr[d]);
            const bool ok = col_ok && r >= 0 && r < H;   // zero padding: a feature outside the image contributes nothing
            float v[3];
#pragma unroll
            for (int s = 0; s < 3; ++s) {              // ch[s][k]: tap rows 0 .. k of output row r + 1 - k
                v[s] = ch[s][3] + (ok ? t[5 * s + 4] : 0.f);
                ch[s][3] = ch[s][2] + (ok ? t[5 * s + 3] : 0.f);
                ch[s][2] = ch[s][1] + (ok ? t[5 * s + 2] : 0.f);
                ch[s][1] = ch[s][0] + (ok ? t[5 * s + 1] : 0.f);
                ch[s][0] = ok ? t[5 * s] : 0.f;
            }
            const int y = r - 2;
            if (y >= y0) {                             // uniform over the workgroup
                float *vr = &vt[r & 1][0][0];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int n = kk ? 3 + s : s;
                    if (n < 5) vr[n * SL3_COLS + c] = v[s];
                }
                __syncthreads();
                if (kk == 0 && c >= 2 && c < SL3_COLS - 2 && x < W) {
                    const float sum = (((vr[c - 2] + vr[SL3_COLS + c - 1]) + vr[2 * SL3_COLS + c]) + vr[3 * SL3_COLS + c + 1]) +
                                      vr[4 * SL3_COLS + c + 2];
                    const float val = sum + b3;
                    const long o = (long)y * dstride + x;
                    dst[o] = (uint8_t)sclamp((int)val, 0, 255);
                    if constexpr (PRE) pre[o] = val;
                }
            }
        }
    }
}

hipError_t launch_spatial_l1(bool zero, const uint8_t *src, long sstride, int W, int H, int m0, int m1, const float *frag,
                             float *map, long mpitch, hipStream_t st)
{
    const dim3 grid((unsigned)((W + SL1_COLS - 1) / SL1_COLS), (unsigned)((m1 - m0 + SL1_ROWS - 1) / SL1_ROWS));
    if (zero) hipLaunchKernelGGL(spatial_l1_kernel<true>, grid, dim3(256), 0, st, src, sstride, W, H, m0, m1, frag, map, mpitch);
    else hipLaunchKernelGGL(spatial_l1_kernel<false>, grid, dim3(256), 0, st, src, sstride, W, H, m0, m1, frag, map, mpitch);
    return hipGetLastError();
}

template <int F2, bool ZERO>
static void launch_l2(dim3 grid, size_t lds, const float *map, long mpitch, int m0, int m1, int W, int H, int o0, int o1,
                      const float *frag, const float *bias, float *out, long opitch, hipStream_t st)
{
    // (the 9-5-5 kernel's 70 KB exceed the default dynamic-LDS limit; set per call: the attribute is per device)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(spatial_l2_kernel<F2, ZERO>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL((spatial_l2_kernel<F2, ZERO>), grid, dim3(256), lds, st, map, mpitch, m0, m1, W, H, o0, o1, frag, bias, out,
                       opitch);
}

hipError_t launch_spatial_l2(int f2, bool zero, const float *map, long mpitch, int m0, int m1, int W, int H, int o0, int o1,
                             const float *frag, const float *bias, float *out, long opitch, hipStream_t st)
{
    const dim3 grid((unsigned)((W + SL2_COLS - 1) / SL2_COLS), (unsigned)((o1 - o0 + SL2_ROWS - 1) / SL2_ROWS));
    const size_t lds = spatial_l2_lds_bytes(f2);
    if (f2 == 1 && !zero) launch_l2<1, false>(grid, lds, map, mpitch, m0, m1, W, H, o0, o1, frag, bias, out, opitch, st);
    else if (f2 == 3 && !zero) launch_l2<3, false>(grid, lds, map, mpitch, m0, m1, W, H, o0, o1, frag, bias, out, opitch, st);
    else if (f2 == 5 && !zero) launch_l2<5, false>(grid, lds, map, mpitch, m0, m1, W, H, o0, o1, frag, bias, out, opitch, st);
    else if (f2 == 1 && zero) launch_l2<1, true>(grid, lds, map, mpitch, m0, m1, W, H, o0, o1, frag, bias, out, opitch, st);
    else if (f2 == 3 && zero) launch_l2<3, true>(grid, lds, map, mpitch, m0, m1, W, H, o0, o1, frag, bias, out, opitch, st);
    else if (f2 == 5 && zero) launch_l2<5, true>(grid, lds, map, mpitch, m0, m1, W, H, o0, o1, frag, bias, out, opitch, st);
    else return hipErrorInvalidValue;
    // (f2 = 1 under replicate padding: the colour 9-1-5 model; the 1-channel one runs on the strip kernels)
    return hipGetLastError();
}

hipError_t launch_spatial_l3z(const float *map, long mpitch, int o0, int o1, int W, int H, int b0, int b1, const float *frag,
                              float b3, uint8_t *dst, long dstride, float *pre, hipStream_t st)
{
    const int nx = (W + SL3_OUT - 1) / SL3_OUT, ny = (b1 - b0 + SL3_SEG - 1) / SL3_SEG, n_tiles = nx * ny;
    const dim3 grid((unsigned)(SL3_XCDS * ((n_tiles + SL3_XCDS - 1) / SL3_XCDS)));
    if (pre)
        hipLaunchKernelGGL(spatial_l3z_kernel<true>, grid, dim3(256), 0, st, map, mpitch, o0, o1, W, H, b0, b1, nx, n_tiles, frag,
                           b3, dst, dstride, pre);
    else
        hipLaunchKernelGGL(spatial_l3z_kernel<false>, grid, dim3(256), 0, st, map, mpitch, o0, o1, W, H, b0, b1, nx, n_tiles, frag,
                           b3, dst, dstride, pre);
    return hipGetLastError();
}

}  // namespace srcnn
