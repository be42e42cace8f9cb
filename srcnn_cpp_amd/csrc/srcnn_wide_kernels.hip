// srcnn_wide_kernels.hip -- the banded path for models of other widths (srcnn_set_model_shape: n1 <= 128 filters in layer 1,
// n2 <= 64 in layer 2), for gfx950.  The host pads the widths to n1p = 64 or 128 and n2p = 32 or 64 with zero weights and zero
// biases (srcnn_spatial.cpp); a model with n1p = 64 and n2p = 32 is an ordinary model and never gets here.
//
// Layer 1 needs no kernel of its own: its output channels are independent, so n1p / 64 launches of spatial_l1_kernel
// (srcnn_spatial_kernels.hip), each with its own fragment table and its own 64 planes of the map, write the n1p maps.  The two
// kernels here are the layer-2 and layer-3 kernels of that unit over more maps, with the same tiles, the same MFMA
// (v_mfma_f32_32x32x2_f32, weights as the A operand, one pixel per lane as the B operand) and the same summation order,
// continued:
//
//   wide_l2_kernel<F2, ZERO>         n1p maps -> n2p planar f32 maps (layer 2, + bias, ReLU): the chunk loop of spatial_l2_kernel
//                                    over n1p / 8 chunks (a kernel argument), one group of 32 output channels per blockIdx.z
//   wide_l3_kernel<C, PRE, ZERO, Out>   64 maps -> C channels (layer 3, + b3[c]): spatial_l3_kernel with 32 k-steps instead of
//                                    16; bytes (with or without the pre-clamp floats) or float planes, C = 1 under replicate
//                                    padding included (the 32-map unit leaves those bytes to the MODE_L3 strip kernel)
//
// Summation order (each MFMA is a 2-term fmaf chain, srcnn_mfma.hip):
//   layer 2, channel k:  b2[k], then the input channels in chunks of 8 (ascending, n1p / 8 of them); inside a chunk the taps
//                        (kh, kw) row-major, inside a tap the channel pairs ascending, channel 2p before 2p + 1.
//   layer 3, channel o:  per map pixel the tap partials T[tap] = sum_c w3[o][c][tap] F_c (channel pairs ascending, n2p / 2 of
//                        them), summed down the 5 tap rows (m ascending), then ((((V_0 + V_1) + V_2) + V_3) + V_4) + b3[o]
// A padded channel is 0 after its ReLU and carries zero weights downstream: every term it adds is an exact 0, so a 64/32 model
// embedded in wider tensors gives the floats of the 32-map kernels.
//
// Every load goes through a clamped, always valid address; every store is guarded by the image and band bounds.
#include "srcnn_kernels.h"

#include <type_traits>

namespace srcnn {

typedef float wf32x16 __attribute__((ext_vector_type(16)));
#define WMFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int wclamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- layer 2 ----------------------------------------------------------------------------------------------------------
// The tile, the window and the LDS layout of spatial_l2_kernel (spatial_l2_lds_bytes(f2) of dynamic LDS): 4 waves, 64 columns x
// 16 output rows, wave w rows 4w .. 4w + 3 and both 32-column units of each (8 accumulators); per chunk of 8 input channels
// the (16 + 2 r2) x (64 + 2 r2) window and the chunk's f2 x f2 x 4 A fragments are staged, then 8 x f2^2 x 4 MFMAs per wave.
// blockIdx.z = g: output channels 32g .. 32g + 31, whose fragments [n_chunks][f2 x f2][4][64] start at frag + g * n_chunks * NA,
// biases at bias + 32g and planes at out + 32g * opitch.  The window is staged once per output group.
constexpr int WL2_COLS = 64, WL2_ROWS = 16, WL2_CC = 8, WL2_XP = 72;
__host__ __device__ constexpr int wl2_ps(int r2) { return ((((WL2_ROWS + 2 * r2) * WL2_XP) + 31) / 64) * 64 + 32; }

template <int F2, bool ZERO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void wide_l2_kernel(const float *__restrict__ map, long mpitch, int m0, int m1,
                                                      int W, int H, int o0, int o1, const float *__restrict__ frag,
                                                      const float *__restrict__ bias, int n_chunks, float *__restrict__ out, long opitch)
{
    constexpr int R = (F2 - 1) / 2, PS = wl2_ps(R), WR = WL2_ROWS + 2 * R, WC = WL2_COLS + 2 * R;
    constexpr int NA = F2 * F2 * (WL2_CC / 2) * 64;          // A floats per chunk
    extern __shared__ float lds[];
    float *xs = lds, *as = lds + WL2_CC * PS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, kk = lane >> 5;
    const int x0 = blockIdx.x * WL2_COLS, y0 = o0 + blockIdx.y * WL2_ROWS;
    const int group = blockIdx.z;
    frag += (size_t)group * n_chunks * NA;
    bias += 32 * group;
    out += (long)(32 * group) * opitch;
    wf32x16 acc[8];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float b = bias[acc_row(q, kk)];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u][q] = b;
    }
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        __syncthreads();
        for (int e = tid; e < WL2_CC * WR * WC; e += 256) {
            const int c = e / (WR * WC), rem = e - c * (WR * WC), rr = rem / WC, cc = rem - rr * WC;
            // image row, replicate-clamped, then kept inside the rows the map holds (only rows that are not stored differ)
            const int yy = wclamp(wclamp(y0 - R + rr, 0, H - 1), m0, m1 - 1), xx = wclamp(x0 - R + cc, 0, W - 1);
            const float v = map[(long)(WL2_CC * chunk + c) * mpitch + (long)(yy - m0) * W + xx];
            if constexpr (ZERO) {   // 0 outside the image: the replicate load times 0 (no branch around the load)
                const int iy = y0 - R + rr, ix = x0 - R + cc;
                xs[c * PS + rr * WL2_XP + cc] = v * ((iy >= 0 && iy < H && ix >= 0 && ix < W) ? 1.f : 0.f);
            } else {
                xs[c * PS + rr * WL2_XP + cc] = v;
            }
        }
        const float4 *fa = reinterpret_cast<const float4 *>(frag + (size_t)chunk * NA);
        for (int e = tid; e < NA / 4; e += 256) reinterpret_cast<float4 *>(as)[e] = fa[e];
        __syncthreads();
        const float *xb = xs + kk * PS + (4 * wave) * WL2_XP + j;
        for (int kh = 0; kh < F2; ++kh) {
#pragma unroll
            for (int kw = 0; kw < F2; ++kw) {
#pragma unroll
                for (int pp = 0; pp < WL2_CC / 2; ++pp) {
                    const float a = as[((kh * F2 + kw) * (WL2_CC / 2) + pp) * 64 + lane];
                    const float *xq = xb + 2 * pp * PS + kh * WL2_XP + kw;
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc[u] = WMFMA(a, xq[(u >> 1) * WL2_XP + 32 * (u & 1)], acc[u]);
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

// ---- layer 3 ----------------------------------------------------------------------------------------------------------
// The strip, the chains, the LDS row and the epilogues of spatial_l3_kernel: 4 waves, a strip of 128 map columns of which the
// middle 124 are output, a segment of 16 output rows; wave w owns map columns 32w .. 32w + 31 and walks the map rows
// y0 - 2 .. y1 + 1.  Per map row C x 32 MFMAs over the 64 maps (k-step s: channels 2s and 2s + 1 on the two lane-halves) give
// the C x 25 tap partials.  The loads are clamped to the band's rows and the image's columns, which is replicate padding; ZERO
// sets the partials of a map pixel outside the image to 0.  Each wave keeps wl3_ahead(C) map rows of 32 loads in flight.
constexpr int WL3_COLS = 128, WL3_OUT = WL3_COLS - 4, WL3_SEG = 16, WL3_XCDS = 8, WL3_K = 32;
__host__ __device__ constexpr int wl3_ahead(int C) { return C == 1 ? 4 : 2; }   // a ring of wl3_ahead x 32 registers

// Out = float: `last` is the channel pitch of C float planes (a long), and a finished value goes to
// dst[y * dstride + x + o * ch_pitch] as it is; Out = uint8_t: `last` is the pre-clamp plane (PRE) or unused.
typedef float *__restrict__ wl3_pre_ptr;
template <typename Out> using wl3_last_arg = std::conditional_t<std::is_same_v<Out, float>, long, wl3_pre_ptr>;

template <int C, bool PRE, bool ZERO, typename Out>
__global__ __launch_bounds__(256) void wide_l3_kernel(const float *__restrict__ map, long mpitch, int o0, int o1, int W, int H,
                                                      int b0, int b1, int nx, int n_tiles, const float *__restrict__ frag,
                                                      float b3_0, float b3_1, float b3_2, Out *__restrict__ dst, long dstride,
                                                      wl3_last_arg<Out> pre)
{
    static_assert(!(std::is_same_v<Out, float> && PRE), "the float form has no second output");
    constexpr int AHEAD = wl3_ahead(C);
    __shared__ float vt[2][C][5][WL3_COLS];
    const int per = (n_tiles + WL3_XCDS - 1) / WL3_XCDS;
    const int tile = (int)(blockIdx.x % WL3_XCDS) * per + (int)(blockIdx.x / WL3_XCDS);
    if (tile >= n_tiles) return;                   // uniform over the workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, kk = lane >> 5;
    const int ty = tile / nx, tx = tile - ty * nx;
    const int c = 32 * wave + j, x = tx * WL3_OUT - 2 + c;
    const int y0 = b0 + ty * WL3_SEG, y1 = min(b1, y0 + WL3_SEG), r_end = y1 + 2;
    const bool col_ok = x >= 0 && x < W;
    const float b3v[3] = {b3_0, b3_1, b3_2};
    float a[C][WL3_K];
#pragma unroll
    for (int o = 0; o < C; ++o)
#pragma unroll
        for (int s = 0; s < WL3_K; ++s) a[o][s] = frag[(o * WL3_K + s) * 64 + lane];
    // channels 2s + kk of map row r at the lane's column, from a clamped (always valid) address: no branch between the loads
    const float *colp = map + (long)kk * mpitch + wclamp(x, 0, W - 1);
    auto load = [&](int r, float *v) {
        const float *p = colp + (long)(wclamp(r, o0, o1 - 1) - o0) * W;
#pragma unroll
        for (int s = 0; s < WL3_K; ++s) v[s] = p[(long)(2 * s) * mpitch];
    };
    float xr[AHEAD][WL3_K], chn[C][3][4];
#pragma unroll
    for (int o = 0; o < C; ++o)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int k = 0; k < 4; ++k) chn[o][s][k] = 0.f;
#pragma unroll
    for (int d = 0; d < AHEAD; ++d)
        if (y0 - 2 + d < r_end) load(y0 - 2 + d, xr[d]);
    for (int rb = y0 - 2; rb < r_end; rb += AHEAD) {
#pragma unroll
        for (int d = 0; d < AHEAD; ++d) {
            const int r = rb + d;
            if (r >= r_end) break;                 // uniform over the workgroup
            wf32x16 t[C];
#pragma unroll
            for (int o = 0; o < C; ++o) t[o] = (wf32x16){0};
#pragma unroll
            for (int s = 0; s < WL3_K; ++s)
#pragma unroll
                for (int o = 0; o < C; ++o) t[o] = WMFMA(a[o][s], xr[d][s], t[o]);
            if (r + AHEAD < r_end) load(r + AHEAD, xr[d]);
            const bool ok = !ZERO || (col_ok && r >= 0 && r < H);
            float v[C][3];
#pragma unroll
            for (int o = 0; o < C; ++o)
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
                for (int o = 0; o < C; ++o)
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        const int n = kk ? 3 + s : s;
                        if (n < 5) vr[(o * 5 + n) * WL3_COLS + c] = v[o][s];
                    }
                __syncthreads();
                if (kk == 0 && c >= 2 && c < WL3_COLS - 2 && x < W) {
#pragma unroll
                    for (int o = 0; o < C; ++o) {
                        const float *vo = vr + o * 5 * WL3_COLS;
                        const float sum = (((vo[c - 2] + vo[WL3_COLS + c - 1]) + vo[2 * WL3_COLS + c]) + vo[3 * WL3_COLS + c + 1]) +
                                          vo[4 * WL3_COLS + c + 2];
                        const float val = sum + b3v[o];
                        if constexpr (std::is_same_v<Out, float>) {
                            dst[(long)y * dstride + x + o * pre] = val;
                        } else {
                            const long ob = (long)y * dstride + (long)C * x + o;
                            dst[ob] = (uint8_t)wclamp((int)val, 0, 255);
                            if constexpr (PRE) pre[ob] = val;
                        }
                    }
                }
            }
        }
    }
}

// ---- the launchers (srcnn_kernels.h states what each one reads and writes) ----------------------------------------------------
// (n, zero) as compile-time constants, as in srcnn_spatial_kernels.hip: n is none of Ns: hipErrorInvalidValue
template <int... Ns, typename F>
static hipError_t wide_form(int n, bool zero, F f)
{
    hipError_t e = hipErrorInvalidValue;
    auto one = [&](auto N) {
        if (n == N.value) e = zero ? f(N, std::true_type{}) : f(N, std::false_type{});
    };
    (one(std::integral_constant<int, Ns>{}), ...);
    return e;
}

static hipError_t launch_wide_l2(int f2, bool zero, const float *map, long mpitch, int m0, int m1, int W, int H, int o0, int o1,
                                 const float *frag, const float *bias, int n_chunks, int n_groups, float *out, long opitch, hipStream_t st)
{
    if (n_chunks < 1 || n_groups < 1 || n_groups > 2) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((W + WL2_COLS - 1) / WL2_COLS), (unsigned)((o1 - o0 + WL2_ROWS - 1) / WL2_ROWS), (unsigned)n_groups);
    return wide_form<1, 3, 5>(f2, zero, [&](auto F2, auto ZERO) {
        auto *kernel = wide_l2_kernel<decltype(F2)::value, decltype(ZERO)::value>;
        // (the f2 = 5 kernel's 70 KB exceeds the default dynamic-LDS limit; set per call: the attribute is per device)
        const size_t lds = spatial_l2_lds_bytes(F2);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, map, mpitch, m0, m1, W, H, o0, o1, frag, bias, n_chunks, out, opitch);
        return hipGetLastError();
    });
}

static hipError_t launch_wide_l3(int channels, bool zero, const float *map, long mpitch, int o0, int o1, int W, int H, int b0, int b1,
                                 const float *frag, const float *b3, const L3Output &out, hipStream_t st)
{
    const int nx = (W + WL3_OUT - 1) / WL3_OUT, ny = (b1 - b0 + WL3_SEG - 1) / WL3_SEG, n_tiles = nx * ny;
    const dim3 grid((unsigned)(WL3_XCDS * ((n_tiles + WL3_XCDS - 1) / WL3_XCDS)));
    return wide_form<1, 3>(channels, zero, [&](auto C, auto ZERO) -> hipError_t {
        constexpr int c = decltype(C)::value;
        constexpr bool z = decltype(ZERO)::value;
        const float b1v = c == 3 ? b3[1] : 0.f, b2v = c == 3 ? b3[2] : 0.f;
        auto launch = [&](auto PRE, auto *dst, auto last) {
            using Out = std::remove_pointer_t<decltype(dst)>;
            hipLaunchKernelGGL((wide_l3_kernel<c, decltype(PRE)::value, z, Out>), grid, dim3(256), 0, st, map, mpitch, o0, o1, W, H, b0,
                               b1, nx, n_tiles, frag, b3[0], b1v, b2v, dst, out.dstride, last);
            return hipGetLastError();
        };
        if (out.f32) return launch(std::false_type{}, static_cast<float *>(out.dst), out.ch_pitch);
        if (out.pre) return launch(std::true_type{}, static_cast<uint8_t *>(out.dst), out.pre);
        return launch(std::false_type{}, static_cast<uint8_t *>(out.dst), out.pre);
    });
}

// the host layer's way to the two launchers (srcnn_kernels.h): handed over once, when the library is loaded
__attribute__((constructor)) static void hand_over_wide_launchers() { set_wide_launchers({launch_wide_l2, launch_wide_l3}); }

}  // namespace srcnn
