// srcnn_spatial_kernels.hip -- layers 1 and 2 of the 9-3-5 / 9-5-5 SRCNN models (srcnn_set_model, f2 = 3 or 5) for gfx950.
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
// Each layer replicate-pads ITS OWN input: layer 1 clamps luma coordinates, layer 2 clamps layer-1 map coordinates.
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
        ys[e] = (float)src[(long)yy * sstride + xx];
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

template <int F2>
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
            xs[c * PS + rr * SL2_XP + cc] = map[(long)(SL2_CC * chunk + c) * mpitch + (long)(yy - m0) * W + xx];
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

hipError_t launch_spatial_l1(const uint8_t *src, long sstride, int W, int H, int m0, int m1, const float *frag, float *map,
                             long mpitch, hipStream_t st)
{
    const dim3 grid((unsigned)((W + SL1_COLS - 1) / SL1_COLS), (unsigned)((m1 - m0 + SL1_ROWS - 1) / SL1_ROWS));
    hipLaunchKernelGGL(spatial_l1_kernel, grid, dim3(256), 0, st, src, sstride, W, H, m0, m1, frag, map, mpitch);
    return hipGetLastError();
}

hipError_t launch_spatial_l2(int f2, const float *map, long mpitch, int m0, int m1, int W, int H, int o0, int o1,
                             const float *frag, const float *bias, float *out, long opitch, hipStream_t st)
{
    const dim3 grid((unsigned)((W + SL2_COLS - 1) / SL2_COLS), (unsigned)((o1 - o0 + SL2_ROWS - 1) / SL2_ROWS));
    const size_t lds = spatial_l2_lds_bytes(f2);
    // (the 9-5-5 kernel's 70 KB exceed the default dynamic-LDS limit; set per call: the attribute is per device)
    if (f2 == 3) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(spatial_l2_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(spatial_l2_kernel<3>, grid, dim3(256), lds, st, map, mpitch, m0, m1, W, H, o0, o1, frag, bias, out, opitch);
    } else if (f2 == 5) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(spatial_l2_kernel<5>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(spatial_l2_kernel<5>, grid, dim3(256), lds, st, map, mpitch, m0, m1, W, H, o0, o1, frag, bias, out, opitch);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace srcnn
