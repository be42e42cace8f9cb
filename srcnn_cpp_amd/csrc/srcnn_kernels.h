// Internal interface between the C-ABI layer (srcnn_api.cpp and its sibling units, see srcnn_ctx.h) and the HIP
// kernels.  Not installed; the public boundary is include/srcnn_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace srcnn {

// ---- geometry of the strip kernels (srcnn_mfma.hip) ------------------------
constexpr int FW = 128;            // feature columns per strip (4 waves x 32 lanes-columns)
constexpr int YP = FW + 8;         // Y ring pitch: strip + 4-pixel layer-1 border each side
constexpr int YR = 16;             // Y ring rows (each stored twice, see kernel)
constexpr int NWAVES = FW / 32;    // one 32-pixel unit per wave per feature row
constexpr int NTHREADS = NWAVES * 64;

enum StripMode { MODE_FUSED = 0, MODE_L12 = 1, MODE_L3 = 2 };

// Packed MFMA A-operand fragments, [NFRAG][64 lanes] floats (see pack_fragments()).
// The layers are SCALED by exact powers of two so that every activation lies in [-1, 1] for any 8-bit input
// (layer 1 by 2^-e1, layer 2 by 2^-e2; pack_fragments() derives e1, e2 from the weights): ReLU is then the clamp
// bit of a packed multiply by 1.0 -- one instruction per TWO registers -- and the scaling changes no result bit
// (a power-of-two factor commutes with every rounding; the layer-3 weights carry 2^e2 back).
constexpr int NFRAG_L1 = 82;       // 2 channel tiles x 41 k-steps (81 taps + bias tap), x 2^-e1
constexpr int NFRAG_L2 = 32;       // 2 x 16 k-steps over the 64 layer-1 channels, x 2^(e1-e2)        (MODE_FUSED)
constexpr int NFRAG_L3 = 16;       // 16 k-steps over the 32 layer-2 channels, rows = 25 taps (+7 zero), x 2^e2 (MODE_FUSED)
constexpr int NFRAG_B2 = 16;       // layer-2 bias laid out like the accumulator (the MFMA chain starts from it), x 2^-e2
constexpr int NFRAG_L2U = 32;      // layer 2 with UNSCALED output, x 2^e1: MODE_L12 stores the reference's map
constexpr int NFRAG_B2U = 16;      // ... and its unscaled bias
constexpr int NFRAG_L3U = 16;      // layer 3 on the unscaled map from HBM (MODE_L3)
constexpr int FRAG_L2 = NFRAG_L1, FRAG_L3 = FRAG_L2 + NFRAG_L2, FRAG_B2 = FRAG_L3 + NFRAG_L3,
              FRAG_L2U = FRAG_B2 + NFRAG_B2, FRAG_B2U = FRAG_L2U + NFRAG_L2U, FRAG_L3U = FRAG_B2U + NFRAG_B2U;
constexpr int NFRAG = FRAG_L3U + NFRAG_L3U;

// MFMA 32x32 accumulator row held by register r on lane-half h, and the
// channel we ASSIGN to accumulator row i so that register r / half h holds
// channel 2r+h (then the next layer's k-steps walk channels in ascending
// order, the reference's summation order).
__host__ __device__ constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__host__ __device__ constexpr int row_chan(int i) { return 2 * ((i & 3) + 4 * (i >> 3)) + ((i >> 2) & 1); }

// Layer-3 tap held by accumulator ROW i: register r = (i&3)+4(i>>3) of lane-half h = (i>>2)&1 holds
// tap (m, n) with r = 5s+m, n = s (half 0) or 3+s (half 1); -1 for the 7 unused rows.  Returns 5m+n.
__host__ __device__ constexpr int l3_row_tap(int i)
{
    const int r = (i & 3) + 4 * (i >> 3), h = (i >> 2) & 1, s = r / 5, m = r % 5, n = h ? 3 + s : s;
    return (r < 15 && n < 5) ? 5 * m + n : -1;
}
// Five of the 7 unused rows -- registers 10..14 of lane-half 1, which the vertical chains and the F tile treat as a sixth tap
// column (plane 5) anyway -- carry the LOCAL SCALE of SRCNN_MODE_REFBYTES' per-pixel flag threshold (round 6): weight
// a_c = max_tap |W3[c][tap]| in every one of them, so that plane 5 of a finished F-tile row holds, at no extra instruction,
// V(y, x) = sum over the 5 feature rows y-2..y+2 of U(., x), U = sum_c a_c * F_c, and the pixel's scale is the 5-term
// horizontal sum S1(y, x) = sum_n V(y, clamp(x + n - 2)).  Nothing else reads those rows: every output byte is as before.
__host__ __device__ constexpr bool l3_row_is_scale(int i)
{
    const int r = (i & 3) + 4 * (i >> 3), h = (i >> 2) & 1;
    return h == 1 && r >= 10 && r < 15;
}

// ---- split-f16 variant (srcnn_split16.hip): A-operand fragments of v_mfma_f32_32x32x16_f16 ----
// [S16_NFRAG][64 lanes][8 halfs]: L1 (tile t, part s = hi|lo, k-block b) at (2t+s)*6+b, L2 (s, b) at
// S16_FRAG_L2 + 4s+b, L3 (s, b) at S16_FRAG_L3 + 2s+b; then float b2[2 lane-halves][16 registers].
constexpr int S16_FRAG_L2 = 24, S16_FRAG_L3 = 32, S16_NFRAG = 36;
constexpr size_t S16_TABLE_BYTES = (size_t)S16_NFRAG * 64 * 16 + 2 * 16 * sizeof(float);
// Layer-1 K slot (k-block b, lane-half h, element e) -> tap 9*i+jj of the 9x9 window, 81 = the bias
// slot (B operand 1.0), -1 = padding (zero weight).  Register n = 4b + e/2 of the lane holds the f16
// pair (e even, e odd): n < 20 -> window row n/5 + 5h, columns 2(n%5), 2(n%5)+1; n = 20..22 -> row 4,
// columns 4h + 2(n-20) + (0,1), of which half 0 owns 0..3 and half 1 owns 4..8; n = 23 -> bias.
__host__ __device__ constexpr int l1s_tap(int b, int h, int e)
{
    const int n = 4 * b + e / 2, u = e & 1;
    if (n < 20) return (2 * (n % 5) + u < 9) ? 9 * (n / 5 + 5 * h) + 2 * (n % 5) + u : -1;
    if (n < 23) {
        const int jj = 4 * h + 2 * (n - 20) + u;
        return (h == 0 ? jj <= 3 : (jj >= 4 && jj <= 8)) ? 36 + jj : -1;
    }
    return (u == 0 && h == 0) ? 81 : -1;
}

struct StripParams {
    // layer-1 input (MODE_FUSED, MODE_L12)
    const uint8_t *src;
    long src_stride, src_frame_pitch;
    int src_row0;
    // Row stripes with their halo rows in SEPARATE buffers (srcnn_forward_y_rows_halo_dev, single frame): src holds image
    // rows [src_row0, src_row1), src_top rows [src_row0 - 6, src_row0), src_bot rows [src_row1, src_row1 + 6), both with
    // row stride halo_stride.  Either may be null when the launch reads no row on that side.  Both null: src holds every row.
    const uint8_t *src_top, *src_bot;
    long halo_stride;
    int src_row1;
    // layer-3 input (MODE_L3) / layer-2 output (MODE_L12): 32 planes in one allocation
    const float *planes_in;
    float *planes_out;
    long pl_stride, pl_pitch, pl_frame_pitch;
    // output (MODE_FUSED, MODE_L3)
    uint8_t *dst;
    float *pre;                     // optional pre-clamp f32, same strides as dst
    long dst_stride, dst_frame_pitch;
    int dst_row0;
    const float *wfrag;
    const uint32_t *wfrag16;        // split-f16 fragments (SRCNN_MODE_SPLIT16), else unused
    float *sink;                    // >= 128 floats of scratch for predicated-off stores
    float b3;
    int width, height;              // full image (border-replication domain)
    int row_begin, row_end;         // output rows produced by this launch
    int seg_rows, n_strips, n_segs; // workgroup decomposition
    const int *items;               // optional explicit work items, ITEM_INTS ints per block: {strip, row_begin,
                                    // row_end, seam above, seam below} (see plan_items()); nullptr = regular grid
    int items_per_frame;            // a batch repeats the plane's items frame after frame: block b = item b % items_per_frame
    int seams_per_frame;            // of frame b / items_per_frame, whose seam ids follow those of the frames before it
    float *seam;                    // seam scratch, SEAM_FLOATS * NTHREADS floats per seam (MODE_FUSED, items only)
    float *cseam;                   // column-seam scratch [frame][strip][row][CSEAM_FLOATS]; non-null = strips without column halo
    int strips_total;               // number of strips of the plane (n_strips is 1 in an items launch)
    int tune;                       // experiment switches (SRCNN_DEBUG_TUNE), 0 in production
    // SRCNN_MODE_REFBYTES (srcnn_exact.hip, "the reference's bytes"): a flag byte beside every output byte, same offsets as dst
    uint8_t *flag;                  // null = no flags
    float fix_delta, fix_scale;     // flag where |v - rint(v)| <= threshold <= fix_delta; code = 1 + (v - rint(v) + delta) * scale, scale = 253 / (2 delta)
    // the per-pixel threshold (float32 MFMA kernel): min(fix_delta, fix_kl * S1 + fix_abs), S1 = the pixel's local scale
    // (l3_row_is_scale()); fix_kl = 0, fix_abs = fix_delta: the one global threshold of rounds 3-5
    float fix_kl, fix_abs;
    unsigned *fix_counters;         // FixParams::counters: the strip kernel's first block zeroes them for the launch
};

// ---- SRCNN_MODE_REFBYTES: fix-up of the pixels whose MFMA value lies within delta of a truncation boundary (srcnn_exact.hip)
// Per-launch counter words (zeroed by the strip kernel), FIX_WORD_STRIDE words = 256 B apart so that atomics on different counters
// do not queue on one line, and the context's running totals (FIX_TOTALS 64-bit words of another buffer).  The work lists are filled in FIX_REGIONS regions, each
// with its own pair of reservation words: a returning atomic on ONE word sustains ~88 per microsecond chip-wide, and
// fix_collect_kernel makes one reservation per workgroup -- 900 of them on a 3840x2160 plane (one word: 16.3 us for the kernel,
// eight: 8.0).
enum { FIX_N_SCAT = 0, FIX_N_DENSE = 1, FIX_N_CHANGED = 2, FIX_MAX_DEV = 3, FIX_N_RERUN = 4,
       FIX_MAX_RATIO = 5,    // the largest |v_mfma - v_reference| / (the pixel's own threshold): what the verdict is taken from
       FIX_TOTALS = 6,
       FIX_WORD_STRIDE = 64,
       FIX_NEXT_ITEM = 6,    // item draw of fix_apply_kernel
       FIX_NEXT_RERUN = 7,   // tile draw of fix_rerun_kernel
       FIX_REGIONS = 8, FIX_REGION0 = 8 * FIX_WORD_STRIDE,      // region r: [FIX_REGION0 + r * FIX_WORD_STRIDE] scattered pixels, [+ 32] dense tiles
       FIX_COUNTERS = FIX_REGION0 + FIX_REGIONS * FIX_WORD_STRIDE };
struct FixParams {
    const uint8_t *src;             // the launch's Y input, as the strip kernel reads it
    long src_stride;
    int src_row0;
    const uint8_t *src_top, *src_bot;   // halo rows in separate buffers (StripParams::src_top), or null
    long halo_stride;
    int src_row1;
    uint8_t *dst;                   // the launch's output plane (already written by the strip and seam kernels)
    const uint8_t *flag;            // flag plane, same offsets as dst
    long dst_stride;
    int dst_row0;
    int width, height, row_begin, row_end;
    const float *wraw;              // b1|W1|b2|W2|b3|W3 in convdata.h order, then W2 transposed [64][32], then W1 transposed [81][64]
    unsigned *counters;             // FIX_COUNTERS words, zeroed by the strip kernel; counter k at counters[k * FIX_WORD_STRIDE]
    unsigned long long *totals;     // FIX_TOTALS 64-bit words, accumulated over every launch of the context (srcnn_fixup_stats)
    unsigned *scat, *dense;         // work lists in FIX_REGIONS equal regions: pixel (frame * height + y) * width + x; tile index
    float delta, code_step;         // code_step = 2 delta / 253
    float kl, abs_term;             // the strip kernel's per-pixel threshold min(delta, kl * S1 + abs_term) (StripParams::fix_kl, fix_abs)
    // The monitor ACTS, on the device: fix_rerun_kernel, queued behind fix_apply_kernel unconditionally, compares the launch's largest
    // |v_mfma - v_reference| / threshold(pixel) with rerun_above (1/2; negative = always: the test hook) and recomputes every pixel
    // of the launch in the reference's arithmetic when it is exceeded.
    float rerun_above;
    // one fix-up for the planes of several single-frame strip launches (srcnn_forward_y_dev): frame k of the batch lies at
    // src + k * src_frame_pitch / dst + k * dst_frame_pitch / flag + k * flag_frame_pitch, same rows in every frame
    int n_frames;
    long src_frame_pitch, dst_frame_pitch, flag_frame_pitch;
};
// SRCNN_MODE_REFBYTES: the flag byte stored beside an output byte (srcnn_kernels.h, srcnn_exact.hip): 0, or 1 + the position of
// v - rint(v) in [-delta, +delta] on a 253-step scale, for the values a rounding difference of the MFMA path could carry across
// a truncation boundary: |v - rint(v)| <= thr and 0.5 < v < 255.5 (the store truncates toward zero and clamps: (-1, 1) -> 0,
// >= 255 -> 255, so there is no boundary at 0 nor above 255).  The range test is ONE unsigned compare on the float's bits.
// thr <= delta is the pixel's own threshold (fix_threshold()); the CODE stays on the scale of the global delta, so the
// fix-up kernels decode every pixel the same way.
__device__ __forceinline__ float fix_threshold(float s1, float delta, float kl, float abs_term)
{
    return __builtin_fminf(delta, __builtin_fmaf(s1, kl, abs_term));
}
__device__ __forceinline__ uint8_t fix_code(float v, float thr, float delta, float scale)
{
    // (device code only; the host translation units include this header for the parameter structs)
    const float dist = v - __builtin_rintf(v);
    const bool live = (__builtin_fabsf(dist) <= thr) & ((__builtin_bit_cast(unsigned, v) - 0x3f000000u) < (0x437f8000u - 0x3f000000u));
    const unsigned code = (unsigned)((dist + delta) * scale + 1.5f);
    return live ? (uint8_t)code : (uint8_t)0;
}

// luma of image row yy, column xx of frame `frame`, wherever the launch keeps that row
__device__ __forceinline__ uint8_t fix_src_at(const FixParams &p, int frame, int yy, int xx)
{
    if (p.src_top && yy < p.src_row0) return p.src_top[(long)(yy - (p.src_row0 - 6)) * p.halo_stride + xx];
    if (p.src_bot && yy >= p.src_row1) return p.src_bot[(long)(yy - p.src_row1) * p.halo_stride + xx];
    return p.src[(long)frame * p.src_frame_pitch + (long)(yy - p.src_row0) * p.src_stride + xx];
}

// fix_collect_kernel, fix_apply_kernel, and behind them fix_rerun_kernel when `with_rerun` (srcnn_set_fixup_strict, the default)
// lds_weights: fix_apply_lds_kernel (both weight tables of layers 1-2 in LDS, 3 workgroups per CU) instead of the scalar-load form
hipError_t launch_fixup(const FixParams &p, int n_cu, bool with_rerun, bool lds_weights, hipStream_t st);
constexpr int FIX_BATCH_FRAMES = 16;      // frames per fix-up launch at most (pixel codes stay below 2^32 up to 16 x 16384 x 16384)
size_t fixup_list_entries(int width, int rows, int n_frames, size_t *dense_entries);

// A SEAM is the boundary between two vertically adjacent work items of a strip.  Instead of recomputing the
// two feature rows either side of it (4 rows per item), the item above hands over its 12 vertical-chain
// registers and the item below the tap partials of its first 4 rows that those chains still need (tap rows
// m > r of row r: 12 + 9 + 6 + 3 values); srcnn_seam_kernel replays those chain steps and finishes the 4 output
// rows around the seam -- same operations in the same order, so the result is bit-identical to the
// halo-recompute form.
constexpr int ITEM_INTS = 5;
constexpr int SEAM_R = 12, SEAM_ROWS = 4;
__host__ __device__ constexpr int seam_t_off(int r) { return SEAM_R + 3 * (r * 4 - r * (r - 1) / 2); }   // 12, 24, 33, 39
constexpr int SEAM_FLOATS = SEAM_R + 3 * (4 + 3 + 2 + 1);     // 42 per thread

size_t strip_lds_bytes(int mode);
hipError_t launch_seams(const StripParams &p, int n_seams, const int *d_seams, hipStream_t stream);

// COLUMN seams: with them a strip produces all FW = 128 columns it computes features for (no 2-column halo each
// side, 30 strips instead of 31 at 3840).  The four output pixels around a strip boundary need layer-3 column
// sums F_n from both strips: every strip exports, per output row, CSEAM_FLOATS values of its two edge columns
// (cseam_terms(): partial 5-term sums in the original order, or single F_n values) and srcnn_cseam_kernel
// completes those pixels -- same additions in the same order, bit-identical.
constexpr int CSEAM_FLOATS = 16;      // 15 used
hipError_t launch_cseams(const StripParams &p, int n_frames, hipStream_t stream);
// both in one launch; `winmap` [strips_total][rows] marks the rows inside a seam window of a strip (srcnn_plan.cpp, plan_items_balanced())
hipError_t launch_seams_merged(const StripParams &p, int n_seams, const int *d_seams, const unsigned char *d_winmap, int n_frames,
                               hipStream_t stream);
hipError_t launch_strip(int mode, const StripParams &p, int n_frames, hipStream_t stream);
// A fused float32 single-plane launch that also carries the seam blocks of the launch BEFORE it (seam deferral, srcnn_mfma.hip):
// blocks [0, first_block) are p's work items, the n_seams + cblocks behind them finish `prev`'s row and column seams.
struct FoldParams {
    StripParams prev;
    const int *seams;               // prev's seam table {strip, row} per seam
    const unsigned char *winmap;    // prev's rows inside a seam window, per strip; null: prev has row seams only (cblocks = 0)
    int n_seams, cblocks, first_block;
};
hipError_t launch_strip_fold(const StripParams &p, const FoldParams &f, hipStream_t stream);
// the same kernels with every MFMA <-> vector-ALU hazard visible to the compiler (srcnn_mfma.hip built with -DSRCNN_SAFE_HAZARDS=1)
hipError_t launch_strip_safe(int mode, const StripParams &p, int n_frames, hipStream_t stream);
// Does this device interlock the inline-asm MFMA -> packed multiply -> MFMA sequences of the fast row body?  Runs them with and
// without wait states (srcnn_probe.hip); returns the number of results that differ (0 = interlocked), negative on a HIP error.
long interlock_probe_mismatches(int device, hipStream_t stream);

size_t split16_lds_bytes();
hipError_t launch_split16(const StripParams &p, int n_frames, hipStream_t stream);

// ---- exact (vector-ALU, reference arithmetic) kernels (srcnn_exact.hip) ----
hipError_t launch_conv99_exact(const uint8_t *src, long sstride, float *dst, long dstride,
                               int w, int h, const float *d_kernel81, float bias, hipStream_t st);
hipError_t launch_conv11_exact(const float *planes, long stride, long pitch, float *dst, long dstride,
                               int w, int h, const float *d_kernel64, float bias, hipStream_t st);
hipError_t launch_conv99x11_exact(const uint8_t *src, long sstride, long src_frame_pitch,
                                  float *planes, long stride, long pitch, long frame_pitch,
                                  int w, int h, int n_frames, const float *d_weights, hipStream_t st);
hipError_t launch_conv55_exact(const float *planes, long stride, long pitch, long frame_pitch,
                               uint8_t *dst, float *pre, long dstride, long dst_frame_pitch,
                               int w, int h, int n_frames, const float *d_kernel800, float bias,
                               hipStream_t st);

// ---- the banded path (srcnn_spatial_kernels.hip): 9-3-5 / 9-5-5 models, every model under zero padding, colour models, and
// models of other widths (srcnn_set_model_shape: n1 <= 128 and n2 <= 64 filters) ----
// The widths of a model are padded with zero channels to n1p = 64 or 128 and n2p = 32 or 64; every model but one of
// srcnn_set_model_shape has 64 / 32, the defaults below.  Fragment table of a model of C = 1 or 3 channels, floats: layer 1
// [n1p / 64 groups][C channels][SPATIAL_NFRAG_L1][64] (group g, per input channel c: fragment t * 41 + s, lane l: output channel
// 64g + 32t + (l & 31), tap 2s + (l >> 5); tap 81: b1 on the last channel, else 0), then layer 2 [n2p / 32 groups][n1p / 8 chunks]
// [f2 * f2 taps][4 pairs][64] (group g, lane l: output channel 32g + (l & 31), input channel 8 chunk + 2 pair + (l >> 5)) and
// b2 [n2p], then layer 3 [C output channels][n2p / 2 k-steps][64] (per output channel o, k-step s, lane l: W3[o][2s + (l >> 5)]
// at the tap of l3_row_tap(l & 31), 0 for the unused rows).  Unscaled: the maps hold the model's own values.
constexpr int SPATIAL_NFRAG_L1 = 82;
__host__ __device__ constexpr size_t spatial_l2_offset(int C, int n1p = 64) { return (size_t)(n1p / 64) * C * SPATIAL_NFRAG_L1 * 64; }
__host__ __device__ constexpr size_t spatial_l2_floats(int f2, int n1p = 64, int n2p = 32) { return (size_t)(n2p / 32) * (n1p / 8) * f2 * f2 * 256; }
__host__ __device__ constexpr size_t spatial_l3_offset(int C, int f2, int n1p = 64, int n2p = 32)
{
    return spatial_l2_offset(C, n1p) + spatial_l2_floats(f2, n1p, n2p) + n2p;
}
__host__ __device__ constexpr size_t spatial_table_floats(int C, int f2, int n1p = 64, int n2p = 32)
{
    return spatial_l3_offset(C, f2, n1p, n2p) + (size_t)C * (n2p / 2) * 64;
}
size_t spatial_l2_lds_bytes(int f2);
// The split W2 table of SRCNN_MODE_BANDED16 and srcnn_set_wide_split16 (spatial_l2h_table_bytes(f2, n1p, n2p)): [n2p / 32 groups]
// [n1p / 16 K steps][f2 * f2 taps][hi, lo][64 lanes][8 f16]; lane l of group g: output channel 32g + (l & 31), element e of step s:
// layer-1 channel 64 (s >> 2) + spatial_l2h_channel(s & 3, l >> 5, e)
__host__ __device__ constexpr int spatial_l2h_channel(int step, int h, int e) { return 32 * (step >> 1) + acc_row(8 * (step & 1) + e, h); }
__host__ __device__ constexpr size_t spatial_l2h_table_bytes(int f2, int n1p = 64, int n2p = 32)
{
    return (size_t)(n2p / 32) * (n1p / 16) * f2 * f2 * 2 * 64 * 16;
}
// The dynamic LDS of spatial_l2h_kernel: four window planes [plane][hi, lo] of spatial_l2h_ps() 16-byte words (a (16 + 2 r2) x
// (64 + 2 r2) window, = 4 mod 8) and one K step's A fragments: 66 / 93 / 135 KiB for f2 = 1 / 3 / 5.  The kernel asserts that this
// is its layout's size, and the launcher asks for it.
__host__ __device__ constexpr int spatial_l2h_ps(int r2) { return (((16 + 2 * r2) * (64 + 2 * r2) + 7) / 8) * 8 + 4; }
__host__ __device__ constexpr size_t spatial_l2h_lds_bytes(int f2) { return ((size_t)4 * spatial_l2h_ps((f2 - 1) / 2) + (size_t)f2 * f2 * 2 * 64) * 16; }
// One launcher per layer; each picks the kernel form from what it is given and returns hipErrorInvalidValue where there is none.
// Every form of a layer does the same arithmetic in the same order.
//
// Where layer 1 reads the image: `channels` = 1 or 3 channels of bytes or (f32) floats in the model's own units (finite values),
// channel c of pixel (y, x) at src[y * sstride + x * px_step + c * ch_step], strides and pitches in elements (1 channel: a plane,
// the steps unused; floats: planes, px_step 1).  rows: a row stripe (one byte channel, 3 interleaved byte channels -- px_step 3,
// ch_step 1 -- or float planes): src starts at image row src_row0; with `top` the halo_rows rows above src_row0 come from it, with
// `bot` the halo_rows rows from src_row1 on, both with row stride halo_stride and, for 3 float planes, a channel pitch of their
// own, halo_ch_pitch, so that a neighbour's stripe can be read where it lies (a null pointer: no buffer on that side, src holds
// those rows too).
struct L1Input {
    const void *src;
    bool f32;
    int channels;
    long sstride;
    int px_step;
    long ch_step;
    bool rows;
    const void *top, *bot;
    long halo_stride, halo_ch_pitch;
    int src_row0, src_row1, halo_rows;
};
// Layer 1: the 64 maps of image rows [m0, m1).  zero: input outside the image is 0 (SRCNN_PAD_ZERO), else replicated; padding
// refers to the image (0, H - 1, 0, W - 1), never to a stripe.  split (SRCNN_MODE_BANDED16): `map` holds 8 planes of 32-byte
// pixels, every activation times `scale` (a power of two) as an f16 (hi, lo) pair; else 64 planar f32 maps (plane pitch mpitch,
// row stride W; the same bytes) and `scale` is unused.  A stripe reads no input row outside [max(0, m0 - 4), min(H, m1 + 4)) and
// no column beyond W - 1.  Layer 1 of a model with n1p = 128 is two calls, each with its group's table and its 64 planes of the
// map (split: all with the model's one scale).
hipError_t launch_spatial_l1(const L1Input &in, bool zero, bool split, float scale, int W, int H, int m0, int m1, const float *frag,
                             void *map, long mpitch, hipStream_t st);
// Layer 2 (f2 = 1, 3, 5): n2p planar f32 maps (row stride W) of rows [o0, o1) from the layer-1 map of n1p channels and rows
// [m0, m1) (which must hold rows o0 - r2 .. o1 + r2 - 1, clamped to the image); zero: the map outside the image is 0, else
// replicated.  split: the f16 pair map, frag = the split W2 table above and unscale = 1 / (layer 1's scale x the W2 scale), on
// the f16 MFMA (spatial_l2h_kernel); else the f32 maps, frag = the layer-2 part of the fragment table, unscale unused.  bias: the
// n2p floats of the fragment table.  n1p = 64 and n2p = 32: the kernels with compile-time loop counts; else (n1p 64 or 128, n2p
// 32 or 64) the forms with the count as an argument, one group of 32 output planes per grid z.
hipError_t launch_spatial_l2(int f2, bool zero, bool split, const void *map, long mpitch, int m0, int m1, int W, int H, int o0, int o1,
                             const void *frag, const float *bias, float unscale, float *out, long opitch, int n1p, int n2p,
                             hipStream_t st);
// What layer 3 writes: pixels of `channels` bytes (row stride dstride; pre: the values before truncation at the same element
// offsets, or null), or (f32) the value before truncation to `channels` float planes, dst[y * dstride + x + o * ch_pitch], and
// no byte.
struct L3Output {
    void *dst;
    bool f32;
    long dstride, ch_pitch;
    float *pre;
};
// Layer 3: rows [b0, b1) of the output from the n2p = 32 or 64 planar maps of rows [o0, o1) (row stride W, plane pitch mpitch),
// which must hold every image row of [b0 - 2, b1 + 2).  frag: the layer-3 part of the table above, b3: `channels` floats.  From 32
// maps, bytes of 1 channel under replicate padding are not a form of this kernel (the MODE_L3 strip kernel runs them); floats of
// it are, and from 64 maps every form is.
hipError_t launch_spatial_l3(int channels, bool zero, const float *map, long mpitch, int o0, int o1, int W, int H, int b0, int b1,
                             const float *frag, const float *b3, const L3Output &out, int n2p, hipStream_t st);

// interleaved 3-byte pixels -> three planes (row stride W, plane pitch ppitch)
hipError_t launch_split3(const uint8_t *src, long sstride, int W, int H, uint8_t *planes, long ppitch, hipStream_t st);

// ---- pipeline steps around the conv path (srcnn_pipeline.hip) ---------------
// Tile geometry of the cubic resize's three kernels.  tiled: a workgroup produces RT output rows x 256 columns from at most
// RMAX source rows x SMAX source columns held in LDS; tiled4 (and the two fused launches, which share its layout): RT4 rows
// (four row groups of RPT rows per thread) x 256 columns from at most RMAX4 x SMAX.
constexpr int RT = 8;        // output rows per workgroup
constexpr int RMAX = 16;     // source rows a tile may span
constexpr int SMAX = 288;    // source columns a 256-wide tile may span
#ifndef SRCNN_RT4
#define SRCNN_RT4 32
#endif
constexpr int RT4 = SRCNN_RT4;          // output rows per workgroup (four row groups of RPT rows)
constexpr int RPT = RT4 / 4;            // rows per thread
constexpr int RMAX4 = RT4 == 32 ? 28 : 20;     // source rows such a tile may span
enum { RESIZE_DIRECT = 0, RESIZE_TILED = 1, RESIZE_TILED4 = 2 };
// Which kernel resizes (sw x sh) -> (dw x dh): the ONE place that keeps a tile inside its LDS arrays.  A tile of T output
// rows spans at most ceil(T * sh / dh) + 4 source rows (4-tap support), 256 output columns at most ceil(256 * sw / dw) + 5
// source columns.  dword_ok: destination base, row stride and plane pitch are multiples of four (tiled4 stores dwords).
inline int resize_variant(int sw, int sh, int dw, int dh, bool dword_ok)
{
    const long span = ((long)RT * sh + dh - 1) / dh + 4;
    const long cspan = (256L * sw + dw - 1) / dw + 5;
    const long span4 = ((long)RT4 * sh + dh - 1) / dh + 4;
    if (span4 <= RMAX4 && cspan <= SMAX && dword_ok) return RESIZE_TILED4;
    if (span <= RMAX && cspan <= SMAX) return RESIZE_TILED;
    return RESIZE_DIRECT;
}
// Grid y of that kernel: one block per output row (direct) or per row tile.  These kernels do not walk rows beyond the grid's
// limit of 65,535, so launch_resize_cubic and the host layer refuse a geometry whose count passes it.
constexpr int kMaxGridYZ = 65535;
inline long resize_grid_rows(int variant, int dh)
{
    return variant == RESIZE_TILED4 ? ((long)dh + RT4 - 1) / RT4 : variant == RESIZE_TILED ? ((long)dh + RT - 1) / RT : (long)dh;
}

// The float32 cubic resize (srcnn_resize_cubic_f32*, torch's bicubic with half-pixel centres) has two forms.  tiled: a workgroup
// produces F32_RT output rows x 256 columns (four row groups of F32_RPT rows, four adjacent columns per thread) from at most
// F32_RMAX source rows x F32_SMAX source columns held in LDS: 2 x 20 KB per workgroup, three workgroups per CU.  direct: one
// output element per lane, its 16 taps from global memory -- every ratio whose tile span does not fit (down-scaling below 1).
constexpr int F32_RT = 16;         // output rows per workgroup
constexpr int F32_RPT = F32_RT / 4;
constexpr int F32_RMAX = 20;       // source rows a tile may span (ratio 1: 16 + 4)
constexpr int F32_SMAX = 264;      // source columns a 256-wide tile may span (ratio 1: 256 + 5)
enum { RESIZE_F32_DIRECT = 0, RESIZE_F32_TILED = 1 };
// Which form resizes (sw x sh) -> (dw x dh): the ONE place that keeps a float tile inside its LDS arrays, by the span bound
// of resize_variant() above (the first tap of output d is floor((d + 0.5) * s / n - 0.5) - 1 on both paths).
inline int resize_f32_variant(int sw, int sh, int dw, int dh)
{
    const long span = ((long)F32_RT * sh + dh - 1) / dh + 4;
    const long cspan = (256L * sw + dw - 1) / dw + 5;
    return (span <= F32_RMAX && cspan <= F32_SMAX) ? RESIZE_F32_TILED : RESIZE_F32_DIRECT;
}
// (the launchers take descriptors, float32 planes among them: srcnn_image.h)

hipError_t launch_copy_rows(uint8_t *dst, long dstride, const uint8_t *src, long sstride, int width, int rows, hipStream_t st);
hipError_t launch_bgr2ycrcb(const uint8_t *bgr, long stride, int w, int h, uint8_t *planes, long pstride,
                            long ppitch, hipStream_t st);
hipError_t launch_ycrcb2bgr(const uint8_t *y, long ystride, const uint8_t *crcb, long pstride, long ppitch, int w,
                            int h, uint8_t *bgr, long stride, hipStream_t st);
hipError_t launch_resize_cubic(const uint8_t *src, long sstride, long spitch, int sw, int sh, uint8_t *dst,
                               long dstride, long dpitch, int dw, int dh, int n_planes, const int *xofs,
                               const short *alpha, const int *yofs, const short *beta, hipStream_t st);

// the pipeline step in two launches: BGR -> up-sampled Y, and BGR + the conv path's Y -> up-sampled BGR
bool fused_pipeline_ok(int sw, int sh, int dw, int dh, const void *y_hi, long ystride, const void *out, long ostride);
hipError_t launch_bgr_to_y_resized(const uint8_t *bgr, long stride, int sw, int sh, uint8_t *dst, long dstride, int dw, int dh,
                                   const int *xofs, const short *alpha, const int *yofs, const short *beta, hipStream_t st);
hipError_t launch_resize_merge(const uint8_t *bgr, long stride, int sw, int sh, const uint8_t *ysr, long ystride, uint8_t *out,
                               long ostride, int dw, int dh, const int *xofs, const short *alpha, const int *yofs,
                               const short *beta, hipStream_t st);

}  // namespace srcnn
