// srcnn_spatial_rows_cf.hip -- the stripe forms of the banded path's layer 1 for a colour model and for float planes, for gfx950
// (srcnn_model_color_rows*_dev, srcnn_model_rows*_f32_dev, srcnn_model_color_striped*, srcnn_model_striped_f32*):
// spatial_l1_kernel<C, ZERO, Scale, In, L1RowsCF> for 3 interleaved byte channels, 1 float plane and 3 float planes, replicate
// and zero padding, f32 and split-f16 map -- 12 kernels behind launch_spatial_l1_rows_cf.  A form takes the image's rows from
// the stripe and from two halo buffers (L1RowsCF, srcnn_kernels.h), stages its window row by row and reads no row beyond the
// ones its map rows need and no column beyond the image's.  The window, the table, the MFMA chains and the epilogues are those
// of the whole-image form of the same input (68 KiB of dynamic LDS for 3 byte channels, 87 KiB for 3 float planes, 29,696 B
// static for 1 float plane).  The template is the one of srcnn_spatial_kernels.hip, included here with its own launchers
// switched off: a translation unit of its own, so the other three units keep exactly the kernels they had.
#define SRCNN_SPATIAL_ROWS_CF_UNIT 1
#include "srcnn_spatial_kernels.hip"

namespace srcnn {

// the three tables and an f32 window of the three channels, as the whole-image float form
constexpr size_t SL1_LDS3F = (size_t)3 * SPATIAL_NFRAG_L1 * 64 * sizeof(float) + 3 * SL1_YC * sizeof(float);

template <int C, bool ZERO, typename In, typename Scale>
static void launch_l1cf(dim3 grid, const In *src, long sstride, const L1RowsCF &rows, int W, int H, int m0, int m1, const float *frag,
                        float *map, long mpitch, Scale scale, hipStream_t st)
{
    if constexpr (C == 1) {
        hipLaunchKernelGGL((spatial_l1_kernel<1, ZERO, Scale, In, L1RowsCF>), grid, dim3(256), 0, st, src, sstride, rows, W, H, m0, m1,
                           frag, map, mpitch, scale);
    } else {
        // (more than the default dynamic-LDS limit; set per call: the attribute is per device)
        constexpr size_t lds = std::is_same_v<In, float> ? SL1_LDS3F : SL1_LDS3;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(spatial_l1_kernel<C, ZERO, Scale, In, L1RowsCF>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((spatial_l1_kernel<C, ZERO, Scale, In, L1RowsCF>), grid, dim3(256), lds, st, src, sstride, rows, W, H, m0,
                           m1, frag, map, mpitch, scale);
    }
}

template <typename Scale>
static hipError_t launch_l1cf_any(int channels, bool zero, bool f32, dim3 grid, const void *src, long sstride, const L1RowsCF &rows,
                                  int W, int H, int m0, int m1, const float *frag, float *map, long mpitch, Scale scale, hipStream_t st)
{
    const float *sf = static_cast<const float *>(src);
    const uint8_t *sb = static_cast<const uint8_t *>(src);
    if (f32 && channels == 1 && !zero) launch_l1cf<1, false>(grid, sf, sstride, rows, W, H, m0, m1, frag, map, mpitch, scale, st);
    else if (f32 && channels == 1) launch_l1cf<1, true>(grid, sf, sstride, rows, W, H, m0, m1, frag, map, mpitch, scale, st);
    else if (f32 && channels == 3 && !zero) launch_l1cf<3, false>(grid, sf, sstride, rows, W, H, m0, m1, frag, map, mpitch, scale, st);
    else if (f32 && channels == 3) launch_l1cf<3, true>(grid, sf, sstride, rows, W, H, m0, m1, frag, map, mpitch, scale, st);
    else if (channels == 3 && !zero) launch_l1cf<3, false>(grid, sb, sstride, rows, W, H, m0, m1, frag, map, mpitch, scale, st);
    else if (channels == 3) launch_l1cf<3, true>(grid, sb, sstride, rows, W, H, m0, m1, frag, map, mpitch, scale, st);
    else return hipErrorInvalidValue;          // (one byte channel: launch_spatial_l1_rows)
    return hipGetLastError();
}

hipError_t launch_spatial_l1_rows_cf(int channels, bool zero, bool split, bool f32, const void *src, long sstride, const L1RowsCF &rows,
                                     int W, int H, int m0, int m1, const float *frag, void *map, long mpitch, float scale,
                                     hipStream_t st)
{
    const dim3 grid((unsigned)((W + SL1_COLS - 1) / SL1_COLS), (unsigned)((m1 - m0 + SL1_ROWS - 1) / SL1_ROWS));
    float *m = static_cast<float *>(map);
    if (split) return launch_l1cf_any(channels, zero, f32, grid, src, sstride, rows, W, H, m0, m1, frag, m, mpitch, scale, st);
    return launch_l1cf_any(channels, zero, f32, grid, src, sstride, rows, W, H, m0, m1, frag, m, mpitch, NoScale{}, st);
}

}  // namespace srcnn
