// srcnn_spatial_kernels.hip -- the banded path, for gfx950: the 9-3-5 / 9-5-5 models (srcnn_set_model, f2 = 3 or 5), every
// model under zero padding (srcnn_set_padding), and the colour models (srcnn_set_model_color: 3 input and 3 output channels,
// 9-f2-5, f2 = 1, 3, 5).
//
// A spatial layer 2 (32 x 64 x f2 x f2) is 10 or 28 times the work of the 9-1-5 model's 1x1 layer and needs an f2 x f2 window
// of the 64-channel layer-1 map, which at 256 B per pixel does not fit beside the strip kernels' rings in LDS.  The path is
// therefore three launches per row band (srcnn_spatial.cpp), for a model of C = 1 or 3 channels:
//
//   spatial_l1_kernel<C>   C u8 channels -> 64 planar f32 maps (layer 1, + bias, ReLU)
//   spatial_l2_kernel      64 maps -> 32 planar f32 maps (layer 2, + bias, ReLU), in exactly the layout MODE_L3 reads
//   spatial_l3_kernel<C>   32 maps -> C channels (layer 3, + b3[c], truncate, clamp): u8 pixels of C bytes, pre-clamp floats;
//                          the 1-channel model under replicate padding runs the MODE_L3 strip kernel (srcnn_mfma.hip) instead
//
// The float image path (srcnn_forward_f32*: float32 planes in the model's own units in, the value before truncation out) runs
// the same launches with two more compile-time forms: spatial_l1_kernel<C, ZERO, Scale, float> reads C float planes at
// src[y * sstride + x + c * ch_step] (the window is f32 for C = 3 too: 87 KiB of LDS, one workgroup per CU), and
// spatial_l3_kernel<C, false, ZERO, float> stores val = sum + b3[o] to C float planes, dst[y * dstride + x + o * ch_pitch], and
// no byte; C = 1 under replicate padding included (the u8 path of that model stays on MODE_L3).  Same arithmetic, same order:
// on integer-valued input the planes equal the pre-clamp floats of the byte path bit for bit.  Inputs must be finite: the
// zero-padding form multiplies a clamped load by 0, and inf * 0 is NaN.
//
// SRCNN_MODE_BANDED16 runs the same three launches with layer 2 in split f16: spatial_l1_kernel<C, ZERO, float> writes the
// layer-1 map as f16 (hi, lo) pairs (the same bytes), spatial_l2h_kernel reads it on v_mfma_f32_32x32x16_f16 and writes the same
// 32 planar f32 maps, layer 3 is unchanged.
//
// Models of other widths (srcnn_set_model_shape: n1 <= 128 filters in layer 1, n2 <= 64 in layer 2) run the same kernels.  The
// host pads the widths to n1p = 64 or 128 and n2p = 32 or 64 with zero weights and zero biases (srcnn_spatial.cpp); 64 / 32 is
// an ordinary model.  Layer 1 needs no form of its own: its output channels are independent, so n1p / 64 launches of
// spatial_l1_kernel, each with its own fragment table and its own 64 planes of the map, write the n1p maps (split: 8 planes of
// 32-byte pixels per launch, all with the model's one scale).  Layers 2 and 3 have WIDE forms, the same bodies over more maps:
//
//   spatial_l2_kernel<F2, ZERO, int>    n1p maps -> n2p planar f32 maps: the chunk loop over n1p / 8 chunks (a kernel argument
//                                       instead of the compile-time 8), one group of 32 output channels per blockIdx.z
//   spatial_l2h_kernel<F2, ZERO, int>   the split map of n1p channels -> n2p planar f32 maps (srcnn_set_wide_split16): n1p / 16
//                                       K steps (a kernel argument) instead of 4, one group of 32 output channels per blockIdx.z
//   spatial_l3_kernel<C, 32, ...>       64 maps -> C channels: 32 k-steps instead of 16; bytes (with or without the pre-clamp
//                                       floats) or float planes, C = 1 under replicate padding included (from 32 maps those
//                                       bytes are left to the MODE_L3 strip kernel)
//
// A padded channel is 0 after its ReLU (split: both halves of its pair are 0) and carries zero weights downstream: every term it
// adds is an exact 0, so a 64 / 32 model embedded in wider tensors gives the floats of the forms with compile-time counts.
//
// Row stripes (srcnn_model_rows_dev, srcnn_model_rows_halo_dev, srcnn_model_striped*) run the same launches on a row range of
// the image with one more compile-time form of layer 1, spatial_l1_kernel<1, ZERO, Scale, uint8_t, L1Rows>: the image's rows
// come from up to three buffers, and no row outside the ones the launch's map rows need is read.  Layers 2 and 3 read the
// context's own band maps only and have no such form.  The stripes of a colour model and of float planes
// (srcnn_model_color_rows*_dev, srcnn_model_rows*_f32_dev, srcnn_model_color_striped*, srcnn_model_striped_f32*) are the same
// with the forms spatial_l1_kernel<C, ZERO, Scale, In, L1RowsCF> for 3 interleaved byte channels and for 1 or 3 float planes.
//
// Every form lives in this one translation unit, 79 kernels behind the three launchers at its end (srcnn_kernels.h), which
// choose the form from what they are given.  Every load goes through a clamped, always valid address; every store is guarded by
// the image and band bounds.
//
// The input is read at src[y * sstride + x * px_step + c * ch_step]: px_step = 3, ch_step = 1 for interleaved 3-byte pixels
// (srcnn_forward_color*), px_step = 1, ch_step = plane pitch for the three resized planes of srcnn_process_bgr, and a plain
// plane for C = 1.  Model channel c reads byte c of a pixel and writes byte c of an output pixel.
//
// The kernels use v_mfma_f32_32x32x2_f32 with the weights as the A operand (output channel on the accumulator ROW) and one
// pixel per lane as the B operand; accumulator register r of lane-half h holds output channel acc_row(r, h), lane & 31 the pixel.
// Each layer pads ITS OWN input.  Replicate padding (the default, ZERO = false): layer 1 clamps the image coordinates, layer 2
// clamps layer-1 map coordinates, layer 3 reads clamped map rows and columns (1 channel: MODE_L3, which builds the replicate
// border into its column offsets and vertical chains).  Zero padding (srcnn_set_padding(SRCNN_PAD_ZERO), ZERO = true; also for
// f2 = 1): layers 1 and 2 stage 0 for every input value outside the image, and layer 3 zeroes the tap partials of map pixels
// outside the image.
//
// Summation order (each MFMA is a 2-term fmaf chain, srcnn_mfma.hip):
//   layer 1, channel k:  0 + sum over c = 0 .. C - 1 of (w1[k][c][0] x0 + ... + w1[k][c][80] x80 + t_c), taps row-major,
//                        where t_c = 0 * 1 (a zero tap) for c < C - 1 and t_{C-1} = b1[k] * 1 (the bias tap); for C = 1:
//                        0 + w1[k][0] y0 + w1[k][1] y1 + ... + w1[k][80] y80 + b1[k]
//   layer 2, channel k:  b2[k], then the input channels in chunks of 8 (ascending, n1p / 8 of them); inside a chunk the taps
//                        (kh, kw) row-major, inside a tap the channel pairs ascending, channel 2p before 2p + 1.
//   layer 3, channel o:  per map pixel the tap partials T[tap] = sum_c w3[o][c][tap] F_c (channel pairs ascending, n2p / 2 of
//                        them), summed down the 5 tap rows (m ascending), then ((((V_0 + V_1) + V_2) + V_3) + V_4) + b3[o]
// (layer 2 in split f16: the order stated above spatial_l2h_kernel.)  The wide forms continue the order of a 64 / 32 model.
#include "srcnn_kernels.h"

#include <type_traits>

namespace srcnn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define SMFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int sclamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- layer 1 ----------------------------------------------------------------------------------------------------------
// Workgroup: 4 waves, a tile of SL1_COLS columns x SL1_ROWS rows.  Wave w owns columns 32w .. 32w + 31 of the tile and walks
// its rows; per row C x 82 MFMAs (channels x 2 channel tiles x 41 k-steps of 2 taps).  LDS: the C channels' A fragments and
// the window.  C = 1: an f32 window, all LDS static (29 KiB).  C = 3: the three tables (61.5 KiB) and a u8 window of the three
// channels (6.4 KiB), dynamic (68 KiB, two workgroups per CU); no static LDS may sit ahead of it and shift its float4 stores.
constexpr int SL1_COLS = 128, SL1_ROWS = 8;
constexpr int SL1_YP = SL1_COLS + 8, SL1_YR = SL1_ROWS + 8, SL1_YC = SL1_YR * SL1_YP;
constexpr size_t SL1_LDS3 = (size_t)3 * SPATIAL_NFRAG_L1 * 64 * sizeof(float) + 3 * SL1_YC;
// 3 float planes: the three tables and an f32 window of the three channels, 61.5 + 25.5 KiB, one workgroup per CU
constexpr size_t SL1_LDS3F = (size_t)3 * SPATIAL_NFRAG_L1 * 64 * sizeof(float) + 3 * SL1_YC * sizeof(float);

// Kernel arguments are passed as they always were, so that each form compiles to the instructions it had: layer 1 takes the
// steps of the input (int px_step, long ch_step) for 3 channels and none for 1, layer 3 takes its C biases as C floats (from 64
// maps: always three, of which it reads C), the wide forms of layer 2 their loop count between the bias and the output.
// Channel c of input pixel (y, x) (a byte, or a float of the float image path), without and with steps:
template <typename In>
__device__ __forceinline__ In l1_at(const In *p, long stride, int y, int x, int) { return p[(long)y * stride + x]; }
template <typename In>
__device__ __forceinline__ In l1_at(const In *p, long stride, int y, int x, int c, int px_step, long ch_step)
{
    return p[(long)y * stride + (long)x * px_step + c * ch_step];
}

// SPLIT (Scale = float, SRCNN_MODE_BANDED16): the epilogue writes the map for spatial_l2h_kernel instead.  Every ReLU'd activation a, times the
// power-of-two `scale` of the model (exact), becomes the f16 pair a_hi = rtz_f16(a), a_lo = f16(a - a_hi) (a - a_hi is exact in
// f32; the split of srcnn_split16.hip): the same 4 bytes per value.  The map is 8 planes of 32-byte pixels (plane pitch mpitch
// pixels, row stride W pixels): plane g = 4a + 2t + h holds the 8 channels that lane-half h keeps in registers 8t .. 8t + 7 of
// accumulator a -- channel 32a + acc_row(8t + e, h), e = 0 .. 7 -- as [8 x a_hi][8 x a_lo], so a lane stores 32 consecutive bytes
// per plane, and a lane of the layer-2 MFMA (K = 16: planes 2s and 2s + 1 on its two lane-halves) reads its 8 K values of one
// pixel as one 16-byte word.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void l1_store_split(uint4 *o, const f32x16 &acc, int t, float scale)
{
    f16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const float a0 = __builtin_fmaxf(acc[8 * t + e], 0.f) * scale, a1 = __builtin_fmaxf(acc[8 * t + e + 1], 0.f) * scale;
        const f16x2 h = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(a0, a1));
        hi[e] = h[0];
        hi[e + 1] = h[1];
        lo[e] = (_Float16)(a0 - (float)h[0]);
        lo[e + 1] = (_Float16)(a1 - (float)h[1]);
    }
    o[0] = __builtin_bit_cast(uint4, hi);
    o[1] = __builtin_bit_cast(uint4, lo);
}

struct NoScale {};         // the last argument of the forms that write plain f32 maps: nothing

// The stripe forms' row source, a kernel argument (launch_spatial_l1 fills it from an L1Input with `rows`).  L1Rows, one byte
// channel: src (row stride sstride) starts at image row src_row0; with `top` the halo_rows rows above src_row0 come from it,
// with `bot` the halo_rows rows from src_row1 on, both with row stride halo_stride (a null pointer: no buffer on that side, src
// holds those rows too).
struct L1Rows {
    const uint8_t *top, *bot;
    long halo_stride;
    int src_row0, src_row1, halo_rows;
};
// L1RowsCF is L1Rows for the three other inputs of layer 1, every stride and pitch in ELEMENTS of the input (bytes, or floats):
//   3 byte channels   a row holds interleaved pixels (byte c of pixel x at row[3 x + c]); the channel pitches are unused
//   1 float plane     a plain plane; the channel pitches are unused
//   3 float planes    channel c of a row of src at + c * src_ch_pitch, of a row of a halo buffer at + c * halo_ch_pitch: a
//                     halo buffer has a pitch of its own, so that a neighbour's stripe can be read where it lies
struct L1RowsCF {
    const void *top, *bot;
    long halo_stride, halo_ch_pitch, src_ch_pitch;
    int src_row0, src_row1, halo_rows;
};

// The stripe form (Steps = L1Rows): where image row y lives -- the R rows above src_row0 in `top`, the R rows
// from src_row1 on in `bot` (a null pointer: no such buffer, the row is in src), every other row in src, whose first row is
// image row src_row0.  y is uniform over the workgroup, so the select and the row's base address are scalar.
__device__ __forceinline__ const uint8_t *l1_row(const uint8_t *src, long sstride, int y, const L1Rows &rs)
{
    if (rs.top && y < rs.src_row0) return rs.top + (long)(y - (rs.src_row0 - rs.halo_rows)) * rs.halo_stride;
    if (rs.bot && y >= rs.src_row1) return rs.bot + (long)(y - rs.src_row1) * rs.halo_stride;
    return src + (long)(y - rs.src_row0) * sstride;
}
__device__ __forceinline__ const L1Rows &l1_rows_of(const L1Rows &rs) { return rs; }
// ... and for the three other inputs (Steps = L1RowsCF: 3 interleaved byte channels, 1 or 3 float planes; strides in elements):
// the row's base address and, in *ch_pitch, the channel pitch of the buffer it lives in (float planes)
template <typename In>
__device__ __forceinline__ const In *l1_row(const In *src, long sstride, int y, const L1RowsCF &rs, long *ch_pitch)
{
    if (rs.top && y < rs.src_row0) {
        *ch_pitch = rs.halo_ch_pitch;
        return static_cast<const In *>(rs.top) + (long)(y - (rs.src_row0 - rs.halo_rows)) * rs.halo_stride;
    }
    if (rs.bot && y >= rs.src_row1) {
        *ch_pitch = rs.halo_ch_pitch;
        return static_cast<const In *>(rs.bot) + (long)(y - rs.src_row1) * rs.halo_stride;
    }
    *ch_pitch = rs.src_ch_pitch;
    return src + (long)(y - rs.src_row0) * sstride;
}
__device__ __forceinline__ const L1RowsCF &l1_rows_of(const L1RowsCF &rs) { return rs; }

template <int C, bool ZERO, typename Scale, typename In, typename... Steps>
__global__ __launch_bounds__(256) void spatial_l1_kernel(const In *__restrict__ src, long sstride, Steps... steps, int W, int H,
                                                         int m0, int m1, const float *__restrict__ frag, float *__restrict__ map,
                                                         long mpitch, Scale scale)
{
    constexpr bool SPLIT = std::is_same_v<Scale, float>;
    constexpr bool F32 = std::is_same_v<In, float>;            // float planes in (px_step = 1, ch_step = the plane pitch)
    constexpr bool ROWS = (std::is_same_v<Steps, L1Rows> || ...);    // the stripe form: rows from src and two halo buffers
    constexpr bool ROWS_CF = (std::is_same_v<Steps, L1RowsCF> || ...);   // ... of 3 byte channels, of 1 or 3 float planes
    static_assert(ROWS_CF ? (sizeof...(Steps) == 1 && (C == 3 || F32))
                          : ROWS ? (sizeof...(Steps) == 1 && C == 1 && !F32) : sizeof...(Steps) == (C == 1 ? 0 : 2),
                  "px_step and ch_step for 3 channels only; L1Rows for one byte channel only, L1RowsCF for the other inputs");
    using T = std::conditional_t<C == 1 || F32, float, uint8_t>;      // the window's element type
    float *as;
    T *ys;
    if constexpr (C == 1) {
        __shared__ float win[SL1_YC], afr[SPATIAL_NFRAG_L1 * 64];
        ys = win;
        as = afr;
    } else {
        extern __shared__ float lds[];
        as = lds;
        ys = reinterpret_cast<T *>(lds + C * SPATIAL_NFRAG_L1 * 64);
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * SL1_COLS, y0 = m0 + blockIdx.y * SL1_ROWS;
    if constexpr (ROWS_CF) {
        // The stripe form of the other inputs: the rows as below (image row y0 - 4 + rr, clamped to the image, then to y_last; the
        // select is uniform over the workgroup), the elements of a row in the order of the whole-image form of the same input --
        // bytes channel fastest (consecutive threads read consecutive bytes of the row's interleaved pixels),
        // float planes channel slowest (consecutive floats of a plane's row) -- into the same places of the same window.
        const L1RowsCF &rs = l1_rows_of(steps...);
        const int y_last = min(H - 1, m1 + 3);
        for (int rr = 0; rr < SL1_YR; ++rr) {
            const int yi = sclamp(y0 - 4 + rr, 0, H - 1);
            long chp;
            const In *row = l1_row(src, sstride, min(yi, y_last), rs, &chp);     // uniform over the workgroup
            for (int e = tid; e < C * SL1_YP; e += 256) {
                int cc, ch;
                if constexpr (F32) {
                    ch = e / SL1_YP;
                    cc = e - ch * SL1_YP;
                } else {
                    cc = e / C;
                    ch = e - C * cc;
                }
                const int xx = sclamp(x0 - 4 + cc, 0, W - 1);
                const T v = F32 ? row[xx + (C == 1 ? 0 : ch * chp)] : row[(long)xx * C + ch];
                if constexpr (ZERO) ys[ch * SL1_YC + rr * SL1_YP + cc] = (T)(v * ((yi == y0 - 4 + rr && xx == x0 - 4 + cc) ? (T)1 : (T)0));
                else ys[ch * SL1_YC + rr * SL1_YP + cc] = v;
            }
        }
    } else if constexpr (ROWS) {
        // The stripe form stages the window row by row: window row rr is image row y0 - 4 + rr, clamped to the IMAGE (yi: what
        // replicate and zero padding refer to, exactly as below), and then to y_last, the last input row this launch may read.
        // Computed row y reads window rows y - y0 .. y - y0 + 8, i.e. image rows y - 4 .. y + 4, and the row loop below stops at
        // y = m1 - 1: image rows beyond y_last = m1 + 3 feed no computed row (they are there when m1 - m0 is no multiple of
        // SL1_ROWS).  Their window rows hold copies of row y_last, and nothing reads them.  At the other end y0 >= m0, so no
        // window row lies above m0 - 4: the rows read are [max(0, m0 - 4), min(H, m1 + 4)), what the caller of a stripe provides.
        const L1Rows &rs = l1_rows_of(steps...);
        const int y_last = min(H - 1, m1 + 3);
        const int cc = tid, xx = sclamp(x0 - 4 + cc, 0, W - 1);
        for (int rr = 0; rr < SL1_YR; ++rr) {
            const int yi = sclamp(y0 - 4 + rr, 0, H - 1);
            const uint8_t *row = l1_row(src, sstride, min(yi, y_last), rs);     // uniform over the workgroup
            if (cc < SL1_YP) {
                const T v = row[xx];
                if constexpr (ZERO) ys[rr * SL1_YP + cc] = (T)(v * ((yi == y0 - 4 + rr && xx == x0 - 4 + cc) ? (T)1 : (T)0));
                else ys[rr * SL1_YP + cc] = v;
            }
        }
    } else {
        // the window, channel fastest (consecutive bytes of interleaved pixels go to consecutive threads); float planes: channel
        // slowest (consecutive floats of a plane's row)
        for (int e = tid; e < C * SL1_YC; e += 256) {
            int rr, cc, ch;
            if constexpr (F32 && C > 1) {
                ch = e / SL1_YC;
                rr = (e - ch * SL1_YC) / SL1_YP;
                cc = e - ch * SL1_YC - rr * SL1_YP;
            } else {
                rr = e / (C * SL1_YP);
                const int rem = e - rr * (C * SL1_YP);
                cc = rem / C;
                ch = rem - C * cc;
            }
            const int yy = sclamp(y0 - 4 + rr, 0, H - 1), xx = sclamp(x0 - 4 + cc, 0, W - 1);
            const T v = l1_at(src, sstride, yy, xx, ch, steps...);
            // ZERO: 0 where the load was clamped, by a multiply: a select lets the compiler branch around the load (measured slower)
            if constexpr (ZERO) ys[ch * SL1_YC + rr * SL1_YP + cc] = (T)(v * ((yy == y0 - 4 + rr && xx == x0 - 4 + cc) ? (T)1 : (T)0));
            else ys[ch * SL1_YC + rr * SL1_YP + cc] = v;
        }
    }
    if constexpr (C == 1) {
        for (int e = tid; e < SPATIAL_NFRAG_L1 * 64; e += 256) as[e] = frag[e];
    } else {
        const float4 *fa = reinterpret_cast<const float4 *>(frag);
        for (int e = tid; e < C * SPATIAL_NFRAG_L1 * 16; e += 256) reinterpret_cast<float4 *>(as)[e] = fa[e];
    }
    __syncthreads();
    const int j = lane & 31, kk = lane >> 5;
    const int x = x0 + 32 * wave + j;
    for (int r = 0; r < SL1_ROWS; ++r) {
        const int y = y0 + r;
        if (y >= m1) break;                        // uniform over the workgroup
        f32x16 acc0 = {0}, acc1 = {0};
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const T *yc = ys + ch * SL1_YC + r * SL1_YP + 32 * wave + j;
            const float *ac = as + ch * (SPATIAL_NFRAG_L1 * 64) + lane;
#pragma unroll
            for (int s = 0; s < 41; ++s) {
                const int tap = 2 * s + kk;        // 81: the zero / bias tap, B = 1
                const int ty = tap / 9, tx = tap - 9 * (tap / 9);
                // (one address, written per form as each kernel had it: the two writings compile differently)
                const float b = tap < 81 ? (float)(C == 1 ? ys[(r + ty) * SL1_YP + 32 * wave + j + tx] : yc[ty * SL1_YP + tx]) : 1.f;
                acc0 = SMFMA(ac[s * 64], b, acc0);
                acc1 = SMFMA(ac[(41 + s) * 64], b, acc1);
            }
        }
        if (x < W) {
            if constexpr (SPLIT) {
                uint4 *o = reinterpret_cast<uint4 *>(map) + 2 * ((long)kk * mpitch + (long)(y - m0) * W + x);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    l1_store_split(o + 2 * (2 * t) * mpitch, acc0, t, scale);
                    l1_store_split(o + 2 * (4 + 2 * t) * mpitch, acc1, t, scale);
                }
            } else {
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
}

// ---- layer 2 ----------------------------------------------------------------------------------------------------------
// The loop count of a layer-2 kernel: the compile-time count of a 64 / 32 model, or the one kernel argument of a wide form
__device__ __forceinline__ constexpr int wide_count(int narrow) { return narrow; }
__device__ __forceinline__ constexpr int wide_count(int, int wide) { return wide; }

// Workgroup: 4 waves, a tile of SL2_COLS = 64 columns x SL2_ROWS = 16 output rows.  Wave w owns rows 4w .. 4w + 3 and both
// 32-column units of each: 8 accumulators, so every A fragment read from LDS feeds 8 MFMAs.  The K loop walks the 64 input
// channels in chunks of SL2_CC = 8: per chunk the 8 channels' (16 + 2 r2) x (64 + 2 r2) window (replicate-clamped at the image
// edges) and the chunk's f2 x f2 x 4 A fragments are staged in LDS, then 8 x f2^2 x 4 MFMAs run per wave.
// A channel plane of the window is SL2_PS floats, = 32 mod 64: the two lane-halves (channels 2p, 2p + 1) read disjoint banks.
// A wide form (Wide = int, the chunk count n1p / 8): blockIdx.z = g computes output channels 32g .. 32g + 31, whose fragments
// [n_chunks][f2 x f2][4][64] start at frag + g * n_chunks * NA, biases at bias + 32g and planes at out + 32g * opitch; the window
// is staged once per output group.
constexpr int SL2_COLS = 64, SL2_ROWS = 16, SL2_CC = 8, SL2_XP = 72;
__host__ __device__ constexpr int sl2_ps(int r2) { return ((((SL2_ROWS + 2 * r2) * SL2_XP) + 31) / 64) * 64 + 32; }
size_t spatial_l2_lds_bytes(int f2)
{
    return ((size_t)SL2_CC * sl2_ps((f2 - 1) / 2) + (size_t)f2 * f2 * (SL2_CC / 2) * 64) * sizeof(float);
}

template <int F2, bool ZERO, typename... Wide>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void spatial_l2_kernel(const float *__restrict__ map, long mpitch, int m0, int m1,
                                                         int W, int H, int o0, int o1, const float *__restrict__ frag,
                                                         const float *__restrict__ bias, Wide... wide, float *__restrict__ out,
                                                         long opitch)
{
    static_assert(sizeof...(Wide) <= 1, "nothing, or the chunk count of a wide model");
    constexpr int R = (F2 - 1) / 2, PS = sl2_ps(R), WR = SL2_ROWS + 2 * R, WC = SL2_COLS + 2 * R;
    constexpr int NA = F2 * F2 * (SL2_CC / 2) * 64;          // A floats per chunk
    extern __shared__ float lds[];
    float *xs = lds, *as = lds + SL2_CC * PS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, kk = lane >> 5;
    const int x0 = blockIdx.x * SL2_COLS, y0 = o0 + blockIdx.y * SL2_ROWS;
    const int n_chunks = wide_count(64 / SL2_CC, wide...);
    if constexpr (sizeof...(Wide) > 0) {
        const int group = blockIdx.z;
        frag += (size_t)group * n_chunks * NA;
        bias += 32 * group;
        out += (long)(32 * group) * opitch;
    }
    f32x16 acc[8];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float b = bias[acc_row(q, kk)];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u][q] = b;
    }
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
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

// ---- layer 2 in split f16 (SRCNN_MODE_BANDED16) ------------------------------------------------------------------------------
// The same implicit GEMM on v_mfma_f32_32x32x16_f16 (16 K values per instruction at half the cycles of the f32 one), with both
// float32 operands split into f16 (hi, lo) pairs as in srcnn_split16.hip:
//   w * 2^e2 = w_hi + w_lo   (host, round to nearest: srcnn_spatial.cpp)      a * 2^e1 = a_hi + a_lo   (spatial_l1_kernel<C, ZERO, float>)
//   w a 2^(e1 + e2) ~= w_hi a_hi + w_lo a_hi + w_hi a_lo                      (the dropped w_lo a_lo is <= 2^-22 |w a|)
// f16 x f16 products are exact in the f32 accumulation.  The accumulators start at 0; the epilogue is
// max(fma(acc, 2^-(e1 + e2), b2[k]), 0), and the output is the 32 planar f32 maps of spatial_l2_kernel.  The power-of-two
// scales (per model, exact) put the largest layer-1 activation any 8-bit input can give and max |W2| in [2^14, 2^15), so the hi
// parts of all but vanishing values are normal f16 numbers.
// Summation order: the input channels in n1p / 16 steps of 16 (ascending; 4 for a 64 / 32 model; step s: layer-1 channels
// 64 (s >> 2) + spatial_l2h_channel(s & 3, h, e)); inside a step the taps (kh, kw) row-major; per tap three MFMAs, hi hi, then
// lo hi, then hi lo.  The order of the 16 products inside one MFMA is the hardware's (not documented), so
// there is no bitwise CPU model of this kernel: it is held to the tolerance of the f32 path.
// Workgroup and tile as spatial_l2_kernel: 4 waves, 64 columns x 16 rows, wave w rows 4w .. 4w + 3 and both 32-column units, so
// each A fragment pair (w_hi, w_lo: 2 x 16 B per lane) feeds 24 MFMAs, with 16 B-operand reads: 18 ds_read_b128 per 24 MFMAs.
// K step s reads map planes 2s (lane-half 0) and 2s + 1 (lane-half 1), i.e. K slot 8h + e is layer-1 channel
// 32 (s >> 1) + acc_row(8 (s & 1) + e, h); the A table is packed in that order: [4 steps][f2 x f2 taps][hi, lo][64 lanes][8 f16],
// lane l: output channel l & 31, K slots 8 (l >> 5) ...  Per step the two planes' (16 + 2 r2) x (64 + 2 r2) window is staged as
// four LDS planes [plane][hi, lo] of 16-byte words, so the 16 lanes the LDS serves together read 256 consecutive bytes (no bank
// conflict), and the step's A fragments beside it: spatial_l2h_lds_bytes(f2) (srcnn_kernels.h), 66 / 93 / 135 KiB for f2 = 1 / 3 /
// 5, one workgroup per CU for f2 = 3, 5.  Plane p of the whole map is plane p % 8 of layer-1 group p / 8, at map + 2 p mpitch
// words.  A wide form (Wide = int, the step count): blockIdx.z = g computes output channels 32g .. 32g + 31, whose fragments
// [n_steps][f2 x f2][hi, lo][64] start at frag + g * n_steps * NA, biases at bias + 32g and planes at out + 32g * opitch; the
// window is staged once per output group.
// With one wave per SIMD nothing else hides the global loads, so step s + 1 is fetched into registers while step s computes.
#define HMFMA(a, b, c) \
    __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, (a)), __builtin_bit_cast(f16x8, (b)), (c), 0, 0, 0)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int F2, bool ZERO, typename... Wide>
__global__ __launch_bounds__(256) void spatial_l2h_kernel(const uint4 *__restrict__ map_, long mpitch, int m0, int m1, int W, int H,
                                                          int o0, int o1, const uint4 *__restrict__ frag_,
                                                          const float *__restrict__ bias, float unscale, Wide... wide,
                                                          float *__restrict__ out, long opitch)
{
    static_assert(sizeof...(Wide) <= 1, "nothing, or the K-step count of a wide model");
    constexpr int R = (F2 - 1) / 2, PS = spatial_l2h_ps(R), WR = SL2_ROWS + 2 * R, WC = SL2_COLS + 2 * R;
    constexpr int NA = F2 * F2 * 2 * 64, NAK = (NA + 255) / 256;     // A words (16 B) per step, and per thread
    // a window LINE is one row of one plane, 2 WC words [column][hi, lo] as the map has them; wave w stages lines w, w + 4, ..
    constexpr int LW = 2 * WC, NK = (LW + 63) / 64, NL = 2 * WR / 4;
    static_assert(2 * WR % 4 == 0, "the lines divide among the 4 waves");
    static_assert(PS >= WR * WC && ((size_t)4 * PS + NA) * sizeof(uint4) == spatial_l2h_lds_bytes(F2),
                  "the header's plane holds this tile's window, and the launcher's LDS size is this layout's");
    extern __shared__ uint4 lds16[];
    const int n_steps = wide_count(4, wide...);
    const u32x4 *map = reinterpret_cast<const u32x4 *>(map_), *frag = reinterpret_cast<const u32x4 *>(frag_);
    if constexpr (sizeof...(Wide) > 0) {
        const int group = blockIdx.z;
        frag += (size_t)group * n_steps * NA;
        bias += 32 * group;
        out += (long)(32 * group) * opitch;
    }
    u32x4 *xs = reinterpret_cast<u32x4 *>(lds16), *as = xs + 4 * PS;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kk = lane >> 5;
    const int x0 = blockIdx.x * SL2_COLS, y0 = o0 + blockIdx.y * SL2_ROWS;
    // the lane's words of a line (the same in every line): word min(lane + 64 k, LW - 1) -- past the end the last word again,
    // which stores the same value to the same place; its offset in a map row (column replicate-clamped) and in an LDS plane pair
    int goff[NK], loff[NK];
    unsigned keep[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int idx = min(lane + 64 * k, LW - 1), part = idx & 1, cc = idx >> 1, ix = x0 - R + cc;
        goff[k] = 2 * sclamp(ix, 0, W - 1) + part;
        loff[k] = part * PS + cc;
        keep[k] = (ix >= 0 && ix < W) ? ~0u : 0u;
    }
    // Step s + 1 is fetched into registers while step s computes, and goes to LDS between two barriers: the global loads
    // have a whole step of MFMAs to land.
    u32x4 wreg[NL][NK], areg[NAK];
    auto fetch = [&](int s) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int line = wave + 4 * n, g = line / WR, rr = line - g * WR;
            // image row, replicate-clamped, then kept inside the rows the map holds (only rows that are not stored differ)
            const int yy = sclamp(sclamp(y0 - R + rr, 0, H - 1), m0, m1 - 1);
            const u32x4 *row = map + 2 * ((long)(2 * s + g) * mpitch + (long)(yy - m0) * W);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                wreg[n][k] = row[goff[k]];
            }
        }
#pragma unroll
        for (int i = 0; i < NAK; ++i) areg[i] = frag[(size_t)s * NA + min(tid + 256 * i, NA - 1)];
    };
    f32x16 acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = (f32x16){0};
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
        const u32x4 *xb = xs + 2 * kk * PS + (4 * wave) * WC + j;
        for (int kh = 0; kh < F2; ++kh) {
#pragma unroll 1
            for (int kw = 0; kw < F2; ++kw) {     // (not unrolled: the next step's words live in registers across this loop)
                const u32x4 a_hi = as[((kh * F2 + kw) * 2) * 64 + lane], a_lo = as[((kh * F2 + kw) * 2 + 1) * 64 + lane];
                const u32x4 *xq = xb + kh * WC + kw;
                u32x4 b_hi[8], b_lo[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    b_hi[u] = xq[(u >> 1) * WC + 32 * (u & 1)];
                    b_lo[u] = xq[PS + (u >> 1) * WC + 32 * (u & 1)];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = HMFMA(a_hi, b_hi[u], acc[u]);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = HMFMA(a_lo, b_hi[u], acc[u]);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = HMFMA(a_hi, b_lo[u], acc[u]);
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

// ---- layer 3 ----------------------------------------------------------------------------------------------------------
// Workgroup: 4 waves, a strip of SL3_COLS = 128 map columns (image columns 124 bx - 2 ..), of which the middle SL3_OUT = 124
// are output, and a segment of SL3_SEG output rows; wave w owns map columns 32w .. 32w + 31 and walks the map rows
// y0 - 2 .. y1 + 1.  Per map row C x K MFMAs (K = 16 k-steps over 32 maps, 32 over the 64 of a wide model; k-step s: channels 2s
// and 2s + 1 on the two lane-halves) give the C x 25 tap partials T[tap] = sum_c W3[o][c][tap] F_c (A set o: W3[o]
// with the rows of l3_row_tap(); B: the channels of the lane's pixel), so register 5s + m of lane-half h holds tap (m, n = s
// (h = 0) or 3 + s (h = 1)).  The loads are clamped to the band's rows and the image's columns, which is replicate padding;
// ZERO sets the partials of a map pixel outside the image to 0 (a feature outside the image contributes nothing, so the sums
// need no clamp).  Each wave keeps sl3_ahead(C) map rows of loads in flight: the 1-channel kernel is bound by the 128 B per
// pixel it reads, and 48 MFMAs per row cover the loads of the 3-channel one.  The 5 tap rows are summed down register chains,
// m ascending; the finished per-tap-column sums V_n of the C channels cross lanes through a double-buffered LDS row, and a lane
// of half 0 finishes its pixel's channels:
//   out(y, x)[o] = (V_0(x - 2) + V_1(x - 1) + V_2(x) + V_3(x + 1) + V_4(x + 2)) + b3[o],  truncated, clamped to 0..255
// (the epilogue of MODE_L3).  The map rows outside the band that the image holds are inside [o0, o1) (srcnn_spatial.cpp); the
// tiles are handed out XCD by XCD (block b runs on XCD b % 8), so horizontally neighbouring strips share their halo columns in
// one L2.
constexpr int SL3_COLS = 128, SL3_OUT = SL3_COLS - 4, SL3_SEG = 16, SL3_XCDS = 8;
__host__ __device__ constexpr int sl3_ahead(int C) { return C == 1 ? 4 : 2; }   // a ring of sl3_ahead x K registers

// Out = float (the float image path): the last argument is the channel pitch of C float planes, and a finished value goes to
// dst[y * dstride + x + o * ch_pitch] as it is -- no truncation, no clamp, no byte.
typedef float *__restrict__ l3_pre_ptr;
template <typename Out> using l3_last_arg = std::conditional_t<std::is_same_v<Out, float>, long, l3_pre_ptr>;

template <int C, int K, bool PRE, bool ZERO, typename Out, typename... B3>
__global__ __launch_bounds__(256) void spatial_l3_kernel(const float *__restrict__ map, long mpitch, int o0, int o1, int W, int H,
                                                         int b0, int b1, int nx, int n_tiles, const float *__restrict__ frag,
                                                         B3... b3, Out *__restrict__ dst, long dstride, l3_last_arg<Out> pre)
{
    static_assert((K == 16 || K == 32) && sizeof...(B3) >= C, "k-steps over 32 or 64 maps; a bias per output channel");
    static_assert(!(std::is_same_v<Out, float> && PRE), "the float form has no second output");
    constexpr int AHEAD = sl3_ahead(C);
    __shared__ float vt[2][C][5][SL3_COLS];
    const int per = (n_tiles + SL3_XCDS - 1) / SL3_XCDS;
    const int tile = (int)(blockIdx.x % SL3_XCDS) * per + (int)(blockIdx.x / SL3_XCDS);
    if (tile >= n_tiles) return;                   // uniform over the workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, kk = lane >> 5;
    const int ty = tile / nx, tx = tile - ty * nx;
    const int c = 32 * wave + j, x = tx * SL3_OUT - 2 + c;
    const int y0 = b0 + ty * SL3_SEG, y1 = min(b1, y0 + SL3_SEG), r_end = y1 + 2;
    const bool col_ok = x >= 0 && x < W;
    const float bias[] = {b3...};
    float a[C][K];
#pragma unroll
    for (int o = 0; o < C; ++o)
#pragma unroll
        for (int s = 0; s < K; ++s) a[o][s] = frag[(o * K + s) * 64 + lane];
    // channels 2s + kk of map row r at the lane's column, from a clamped (always valid) address: no branch between the loads
    const float *colp = map + (long)kk * mpitch + sclamp(x, 0, W - 1);
    auto load = [&](int r, float *v) {
        const float *p = colp + (long)(sclamp(r, o0, o1 - 1) - o0) * W;
#pragma unroll
        for (int s = 0; s < K; ++s) v[s] = p[(long)(2 * s) * mpitch];
    };
    float xr[AHEAD][K], chn[C][3][4];
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
            f32x16 t[C];
#pragma unroll
            for (int o = 0; o < C; ++o) t[o] = (f32x16){0};
#pragma unroll
            for (int s = 0; s < K; ++s)
#pragma unroll
                for (int o = 0; o < C; ++o) t[o] = SMFMA(a[o][s], xr[d][s], t[o]);
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
                        if (n < 5) vr[(o * 5 + n) * SL3_COLS + c] = v[o][s];
                    }
                __syncthreads();
                if (kk == 0 && c >= 2 && c < SL3_COLS - 2 && x < W) {
                    constexpr bool F32 = std::is_same_v<Out, float>;
                    // (one offset, formed per family where each kernel had it: before the sums from 32 maps, after each sum from 64.
                    // Either writing alone leaves the other family's listing reordered around the epilogue, and timed on the GPU
                    // some rows of the reordered family fell outside the run-to-run gap of the parent: DESIGN.md 4.6)
                    const long row = K == 16 ? (long)y * dstride + (F32 ? x : (long)C * x) : 0;
#pragma unroll
                    for (int o = 0; o < C; ++o) {
                        const float *vo = vr + o * 5 * SL3_COLS;
                        const float sum = (((vo[c - 2] + vo[SL3_COLS + c - 1]) + vo[2 * SL3_COLS + c]) + vo[3 * SL3_COLS + c + 1]) +
                                          vo[4 * SL3_COLS + c + 2];
                        const float val = sum + bias[o];
                        long ob;
                        if constexpr (F32) ob = K == 16 ? row + o * pre : (long)y * dstride + x + o * pre;
                        else ob = K == 16 ? row + o : (long)y * dstride + (long)C * x + o;
                        if constexpr (F32) {
                            dst[ob] = val;
                        } else {
                            dst[ob] = (uint8_t)sclamp((int)val, 0, 255);
                            if constexpr (PRE) pre[ob] = val;
                        }
                    }
                }
            }
        }
    }
}

// ---- the launchers (srcnn_kernels.h states what each one reads and writes) ----------------------------------------------------
// (n, zero) as compile-time constants: calls f(std::integral_constant<int, n>, std::bool_constant<zero>) for the one of Ns that
// n is and returns what f returns; n is none of them: hipErrorInvalidValue, there is no such kernel
template <int... Ns, typename F>
static hipError_t with_form(int n, bool zero, F f)
{
    hipError_t e = hipErrorInvalidValue;
    auto one = [&](auto N) {
        if (n == N.value) e = zero ? f(N, std::true_type{}) : f(N, std::false_type{});
    };
    (one(std::integral_constant<int, Ns>{}), ...);
    return e;
}

hipError_t launch_spatial_l1(const L1Input &in, bool zero, bool split, float scale, int W, int H, int m0, int m1, const float *frag,
                             void *map, long mpitch, hipStream_t st)
{
    const dim3 grid((unsigned)((W + SL1_COLS - 1) / SL1_COLS), (unsigned)((m1 - m0 + SL1_ROWS - 1) / SL1_ROWS));
    // one form: spatial_l1_kernel<C, ZERO, Scale, In, Steps...> by the types of sc, src and steps
    auto launch = [&](auto C, auto ZERO, auto sc, auto *src, auto... steps) {
        using In = std::remove_const_t<std::remove_pointer_t<decltype(src)>>;
        auto *kernel = spatial_l1_kernel<decltype(C)::value, decltype(ZERO)::value, decltype(sc), In, decltype(steps)...>;
        // (3 channels: 68 KiB for bytes, 87 KiB for floats exceed the default dynamic-LDS limit; set per call: the attribute is
        // per device)
        const size_t lds = decltype(C)::value == 1 ? 0 : std::is_same_v<In, float> ? SL1_LDS3F : SL1_LDS3;
        if (lds) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, src, in.sstride, steps..., W, H, m0, m1, frag, static_cast<float *>(map),
                           mpitch, sc);
        return hipGetLastError();
    };
    const uint8_t *bytes = static_cast<const uint8_t *>(in.src);
    const float *floats = static_cast<const float *>(in.src);
    // the form of the input, for a map of one kind (sc: the scale of the split map, or NoScale)
    auto input = [&](auto C, auto ZERO, auto sc) -> hipError_t {
        constexpr bool one = decltype(C)::value == 1;
        if (in.rows) {
            const L1RowsCF cf{in.top, in.bot, in.halo_stride, in.halo_ch_pitch, in.ch_step, in.src_row0, in.src_row1, in.halo_rows};
            if (in.f32) return launch(C, ZERO, sc, floats, cf);
            if constexpr (one)
                return launch(C, ZERO, sc, bytes, L1Rows{static_cast<const uint8_t *>(in.top), static_cast<const uint8_t *>(in.bot),
                                                         in.halo_stride, in.src_row0, in.src_row1, in.halo_rows});
            else       // (3 byte planes have no stripe form)
                return in.px_step == 3 && in.ch_step == 1 ? launch(C, ZERO, sc, bytes, cf) : hipErrorInvalidValue;
        }
        if constexpr (one) return in.f32 ? launch(C, ZERO, sc, floats) : launch(C, ZERO, sc, bytes);
        else return in.f32 ? launch(C, ZERO, sc, floats, 1, in.ch_step) : launch(C, ZERO, sc, bytes, in.px_step, in.ch_step);
    };
    return with_form<1, 3>(in.channels, zero,
                           [&](auto C, auto ZERO) { return split ? input(C, ZERO, scale) : input(C, ZERO, NoScale{}); });
}

hipError_t launch_spatial_l2(int f2, bool zero, bool split, const void *map, long mpitch, int m0, int m1, int W, int H, int o0, int o1,
                             const void *frag, const float *bias, float unscale, float *out, long opitch, int n1p, int n2p,
                             hipStream_t st)
{
    if ((n1p != 64 && n1p != 128) || (n2p != 32 && n2p != 64)) return hipErrorInvalidValue;
    const bool wide = n1p != 64 || n2p != 32;      // the count as an argument, a group of 32 output planes per grid z
    const dim3 grid((unsigned)((W + SL2_COLS - 1) / SL2_COLS), (unsigned)((o1 - o0 + SL2_ROWS - 1) / SL2_ROWS), (unsigned)(n2p / 32));
    // (f2 = 1 under replicate padding: the colour 9-1-5 model and the wide ones; the 1-channel one runs on the strip kernels)
    return with_form<1, 3, 5>(f2, zero, [&](auto F2, auto ZERO) {
        // (the 9-5-5 kernel's 70 KB and every split form exceed the default dynamic-LDS limit; set per call: the attribute is
        // per device)
        auto launch = [&](auto *kernel, size_t lds, auto... args) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, args...);
            return hipGetLastError();
        };
        // one form: the kernel with `count...` (nothing, or the K steps or chunks of a wide model) between its bias and its output
        constexpr int f = decltype(F2)::value;
        constexpr bool z = decltype(ZERO)::value;
        auto f16 = [&](auto... count) {
            const size_t lds = spatial_l2h_lds_bytes(f);
            return launch(spatial_l2h_kernel<f, z, decltype(count)...>, lds, static_cast<const uint4 *>(map), mpitch, m0, m1, W, H, o0, o1,
                          static_cast<const uint4 *>(frag), bias, unscale, count..., out, opitch);
        };
        auto f32 = [&](auto... count) {
            const size_t lds = spatial_l2_lds_bytes(f);
            return launch(spatial_l2_kernel<f, z, decltype(count)...>, lds, static_cast<const float *>(map), mpitch, m0, m1, W, H, o0, o1,
                          static_cast<const float *>(frag), bias, count..., out, opitch);
        };
        if (split) return wide ? f16(n1p / 16) : f16();
        return wide ? f32(n1p / 8) : f32();
    });
}

hipError_t launch_spatial_l3(int channels, bool zero, const float *map, long mpitch, int o0, int o1, int W, int H, int b0, int b1,
                             const float *frag, const float *b3, const L3Output &out, int n2p, hipStream_t st)
{
    if (n2p != 32 && n2p != 64) return hipErrorInvalidValue;
    const int nx = (W + SL3_OUT - 1) / SL3_OUT, ny = (b1 - b0 + SL3_SEG - 1) / SL3_SEG, n_tiles = nx * ny;
    const dim3 grid((unsigned)(SL3_XCDS * ((n_tiles + SL3_XCDS - 1) / SL3_XCDS)));
    // one form: spatial_l3_kernel<C, K, PRE, ZERO, Out, float...> by the type of dst; last: the kernel's last argument
    auto launch = [&](auto C, auto K, auto ZERO, auto PRE, auto *dst, auto last, auto... b) {
        using Out = std::remove_pointer_t<decltype(dst)>;
        hipLaunchKernelGGL((spatial_l3_kernel<decltype(C)::value, decltype(K)::value, decltype(PRE)::value, decltype(ZERO)::value, Out,
                                              decltype(b)...>),
                           grid, dim3(256), 0, st, map, mpitch, o0, o1, W, H, b0, b1, nx, n_tiles, frag, b..., dst, out.dstride, last);
        return hipGetLastError();
    };
    return with_form<1, 3>(channels, zero, [&](auto C, auto ZERO) -> hipError_t {
        constexpr int c = decltype(C)::value;
        // the kernel from 32 maps takes its C biases, the one from 64 maps always three (as each always did)
        auto biases = [&](auto K, auto PRE, auto *dst, auto last) {
            if constexpr (decltype(K)::value == 32) return launch(C, K, ZERO, PRE, dst, last, b3[0], c == 3 ? b3[1] : 0.f, c == 3 ? b3[2] : 0.f);
            else if constexpr (c == 1) return launch(C, K, ZERO, PRE, dst, last, b3[0]);
            else return launch(C, K, ZERO, PRE, dst, last, b3[0], b3[1], b3[2]);
        };
        auto output = [&](auto K) -> hipError_t {
            if (out.f32) return biases(K, std::false_type{}, static_cast<float *>(out.dst), out.ch_pitch);
            if constexpr (decltype(K)::value == 16 && c == 1 && !decltype(ZERO)::value) return hipErrorInvalidValue;      // (MODE_L3 runs it)
            else if (out.pre) return biases(K, std::true_type{}, static_cast<uint8_t *>(out.dst), out.pre);
            else return biases(K, std::false_type{}, static_cast<uint8_t *>(out.dst), out.pre);
        };
        return n2p == 64 ? output(std::integral_constant<int, 32>{}) : output(std::integral_constant<int, 16>{});
    });
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
