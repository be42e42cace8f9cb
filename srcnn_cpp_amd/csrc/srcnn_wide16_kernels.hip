// srcnn_wide16_kernels.hip -- layer 2 of a wide model (srcnn_set_model_shape: n1p = 128 or n2p = 64) in split f16, for gfx950:
// what srcnn_set_wide_split16(ctx, 1) runs in SRCNN_MODE_MFMA instead of wide_l2_kernel (srcnn_wide_kernels.hip).
//
//   wide_l2h_kernel<F2, ZERO>    the split map of n1p channels -> n2p planar f32 maps (layer 2, + bias, ReLU): spatial_l2h_kernel
//                                (srcnn_spatial_kernels.hip) over n1p / 16 K steps (a kernel argument) instead of 4, one group of
//                                32 output channels per blockIdx.z.  It stands to spatial_l2h_kernel as wide_l2_kernel stands to
//                                spatial_l2_kernel.
//
// Layers 1 and 3 need nothing new.  Layer 1 is n1p / 64 launches of spatial_l1_kernel<C, ZERO, float>, the split-output
// epilogue, each with its group's table and its 64 channels of the map (8 planes of 32-byte pixels), all with the model's one
// scale; layer 3 reads the n2p planar f32 maps this kernel writes, as it reads wide_l2_kernel's.
//
// The arithmetic is that of SRCNN_MODE_BANDED16: on v_mfma_f32_32x32x16_f16 with both float32 operands split into f16 (hi, lo)
// pairs,
//   w * 2^e2 = w_hi + w_lo   (host, round to nearest: srcnn_spatial.cpp)      a * 2^e1 = a_hi + a_lo   (spatial_l1_kernel<C, ZERO, float>)
//   w a 2^(e1 + e2) ~= w_hi a_hi + w_lo a_hi + w_hi a_lo                      (the dropped w_lo a_lo is <= 2^-22 |w a|)
// with the two power-of-two scales made over the whole padded model (all n1p channels, the whole padded W2).
// Summation order of a layer-2 value: the accumulators start at 0; the K steps ascending over all n1p / 16 (step s: layer-1
// channels 64 (s >> 2) + spatial_l2h_channel(s & 3, h, e)); inside a step the taps (kh, kw) row-major; per tap three MFMAs, hi hi,
// then lo hi, then hi lo; the epilogue is max(fma(acc, 2^-(e1 + e2), b2[k]), 0).  For n1p = 64 and n2p = 32 that is
// spatial_l2h_kernel's order exactly.  A padded channel is 0 after its ReLU, both halves of its pair are 0 and its weights are 0:
// every product it adds is an exact 0, so a 64 / 32 model embedded in wider tensors gives the floats of SRCNN_MODE_BANDED16.
//
// Every load goes through a clamped, always valid address; every store is guarded by the image and band bounds.
#include "srcnn_kernels.h"

#include <type_traits>

namespace srcnn {

typedef float hf32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 hf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned hu32x4 __attribute__((ext_vector_type(4)));
#define WHMFMA(a, b, c) \
    __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(hf16x8, (a)), __builtin_bit_cast(hf16x8, (b)), (c), 0, 0, 0)

__device__ __forceinline__ int hclamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The tile, the window and the LDS layout of spatial_l2h_kernel (wide_l2h_lds_bytes(f2) of dynamic LDS: 66 / 93 / 135 KiB for
// f2 = 1 / 3 / 5, one workgroup per CU for f2 = 3, 5): 4 waves, 64 columns x 16 output rows, wave w rows 4w .. 4w + 3 and both
// 32-column units of each (8 accumulators); per K step the two planes' (16 + 2 r2) x (64 + 2 r2) window as four LDS planes
// [plane][hi, lo] of 16-byte words and the step's A fragments beside it, 18 ds_read_b128 per 24 MFMAs; step s + 1 is fetched
// into registers while step s computes.  K step s reads planes 2s and 2s + 1 of the whole map: plane p is plane p % 8 of layer-1
// group p / 8, at map + 2 p mpitch words.  blockIdx.z = g: output channels 32g .. 32g + 31, whose fragments
// [n_steps][f2 x f2][hi, lo][64] start at frag + g * n_steps * NA, biases at bias + 32g and planes at out + 32g * opitch.  The
// window is staged once per output group.
constexpr int WH_COLS = 64, WH_ROWS = 16;

template <int F2, bool ZERO>
__global__ __launch_bounds__(256) void wide_l2h_kernel(const uint4 *__restrict__ map_, long mpitch, int m0, int m1, int W, int H,
                                                       int o0, int o1, const uint4 *__restrict__ frag_,
                                                       const float *__restrict__ bias, float unscale, int n_steps,
                                                       float *__restrict__ out, long opitch)
{
    constexpr int R = (F2 - 1) / 2, PS = wide_l2h_ps(R), WR = WH_ROWS + 2 * R, WC = WH_COLS + 2 * R;
    constexpr int NA = F2 * F2 * 2 * 64, NAK = (NA + 255) / 256;     // A words (16 B) per step, and per thread
    // a window LINE is one row of one plane, 2 WC words [column][hi, lo] as the map has them; wave w stages lines w, w + 4, ..
    constexpr int LW = 2 * WC, NK = (LW + 63) / 64, NL = 2 * WR / 4;
    static_assert(2 * WR % 4 == 0, "the lines divide among the 4 waves");
    static_assert(((size_t)4 * PS + NA) * sizeof(uint4) == wide_l2h_lds_bytes(F2), "the launcher's LDS size is this layout's");
    extern __shared__ uint4 lds16[];
    const int group = blockIdx.z;
    const hu32x4 *map = reinterpret_cast<const hu32x4 *>(map_);
    const hu32x4 *frag = reinterpret_cast<const hu32x4 *>(frag_) + (size_t)group * n_steps * NA;
    bias += 32 * group;
    out += (long)(32 * group) * opitch;
    hu32x4 *xs = reinterpret_cast<hu32x4 *>(lds16), *as = xs + 4 * PS;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kk = lane >> 5;
    const int x0 = blockIdx.x * WH_COLS, y0 = o0 + blockIdx.y * WH_ROWS;
    // the lane's words of a line (the same in every line): word min(lane + 64 k, LW - 1) -- past the end the last word again,
    // which stores the same value to the same place; its offset in a map row (column replicate-clamped) and in an LDS plane pair
    int goff[NK], loff[NK];
    unsigned keep[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int idx = min(lane + 64 * k, LW - 1), part = idx & 1, cc = idx >> 1, ix = x0 - R + cc;
        goff[k] = 2 * hclamp(ix, 0, W - 1) + part;
        loff[k] = part * PS + cc;
        keep[k] = (ix >= 0 && ix < W) ? ~0u : 0u;
    }
    // Step s + 1 is fetched into registers while step s computes, and goes to LDS between two barriers: the global loads
    // have a whole step of MFMAs to land.
    hu32x4 wreg[NL][NK], areg[NAK];
    auto fetch = [&](int s) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int line = wave + 4 * n, g = line / WR, rr = line - g * WR;
            // image row, replicate-clamped, then kept inside the rows the map holds (only rows that are not stored differ)
            const int yy = hclamp(hclamp(y0 - R + rr, 0, H - 1), m0, m1 - 1);
            const hu32x4 *row = map + 2 * ((long)(2 * s + g) * mpitch + (long)(yy - m0) * W);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                wreg[n][k] = row[goff[k]];
            }
        }
#pragma unroll
        for (int i = 0; i < NAK; ++i) areg[i] = frag[(size_t)s * NA + min(tid + 256 * i, NA - 1)];
    };
    hf32x16 acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = (hf32x16){0};
    fetch(0);
    for (int s = 0; s < n_steps; ++s) {
        __syncthreads();
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int line = wave + 4 * n, g = line / WR, rr = line - g * WR;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                // ZERO: 0 outside the image, the replicate load under a mask (as in layer 1: no branch around the load)
                if constexpr (ZERO) wreg[n][k] &= (y0 - R + rr >= 0 && y0 - R + rr < H) ? keep[k] : 0u;
                xs[2 * g * PS + rr * WC + loff[k]] = wreg[n][k];
            }
        }
#pragma unroll
        for (int i = 0; i < NAK; ++i) as[min(tid + 256 * i, NA - 1)] = areg[i];
        __syncthreads();
        if (s + 1 < n_steps) fetch(s + 1);
        const hu32x4 *xb = xs + 2 * kk * PS + (4 * wave) * WC + j;
        for (int kh = 0; kh < F2; ++kh) {
#pragma unroll 1
            for (int kw = 0; kw < F2; ++kw) {     // (not unrolled: the next step's words live in registers across this loop)
                const hu32x4 a_hi = as[((kh * F2 + kw) * 2) * 64 + lane], a_lo = as[((kh * F2 + kw) * 2 + 1) * 64 + lane];
                const hu32x4 *xq = xb + kh * WC + kw;
                hu32x4 b_hi[8], b_lo[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    b_hi[u] = xq[(u >> 1) * WC + 32 * (u & 1)];
                    b_lo[u] = xq[PS + (u >> 1) * WC + 32 * (u & 1)];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = WHMFMA(a_hi, b_hi[u], acc[u]);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = WHMFMA(a_lo, b_hi[u], acc[u]);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = WHMFMA(a_hi, b_lo[u], acc[u]);
            }
        }
    }
    float b[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) b[q] = bias[acc_row(q, kk)];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int y = y0 + 4 * wave + (u >> 1), x = x0 + 32 * (u & 1) + j;
        if (y < o1 && x < W) {
            float *o = out + (long)(y - o0) * W + x;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                o[(long)acc_row(q, kk) * opitch] = __builtin_fmaxf(__builtin_fmaf(acc[u][q], unscale, b[q]), 0.f);
        }
    }
}

// ---- the launcher (srcnn_kernels.h states what it reads and writes) -----------------------------------------------------------
static hipError_t launch_wide_l2h(int f2, bool zero, const void *map, long mpitch, int m0, int m1, int W, int H, int o0, int o1,
                                  const void *frag, const float *bias, float unscale, int n_steps, int n_groups, float *out, long opitch,
                                  hipStream_t st)
{
    if ((n_steps != 4 && n_steps != 8) || n_groups < 1 || n_groups > 2) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((W + WH_COLS - 1) / WH_COLS), (unsigned)((o1 - o0 + WH_ROWS - 1) / WH_ROWS), (unsigned)n_groups);
    // (f2, zero) as compile-time constants, as in srcnn_spatial_kernels.hip: f2 is none of 1, 3, 5: hipErrorInvalidValue
    hipError_t e = hipErrorInvalidValue;
    auto one = [&](auto F2, auto ZERO) {
        auto *kernel = wide_l2h_kernel<decltype(F2)::value, decltype(ZERO)::value>;
        // (every form exceeds the default dynamic-LDS limit; set per call: the attribute is per device)
        const size_t lds = wide_l2h_lds_bytes(F2);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, static_cast<const uint4 *>(map), mpitch, m0, m1, W, H, o0, o1,
                           static_cast<const uint4 *>(frag), bias, unscale, n_steps, out, opitch);
        e = hipGetLastError();
    };
    auto form = [&](auto F2) {
        if (f2 == F2.value) zero ? one(F2, std::true_type{}) : one(F2, std::false_type{});
    };
    form(std::integral_constant<int, 1>{});
    form(std::integral_constant<int, 3>{});
    form(std::integral_constant<int, 5>{});
    return e;
}

// the host layer's way to the launcher (srcnn_kernels.h): handed over once, when the library is loaded
__attribute__((constructor)) static void hand_over_wide16_launcher() { set_wide16_launcher(launch_wide_l2h); }

}  // namespace srcnn
