// srcnn_spatial_rows.hip -- the stripe forms of the banded path's layer 1, for gfx950 (srcnn_model_rows_dev,
// srcnn_model_rows_halo_dev, srcnn_model_striped*): spatial_l1_kernel<1, ZERO, Scale, uint8_t, L1Rows>, replicate and zero
// padding, f32 and split-f16 map, behind launch_spatial_l1_rows.  The form takes the image's rows from the stripe and from two
// halo buffers (L1Rows, srcnn_kernels.h) and reads no row beyond the ones its map rows need.  The template is the one of
// srcnn_spatial_kernels.hip, included here with its own launchers switched off: a translation unit of its own, so that unit and
// srcnn_spatial_f32.hip keep exactly the kernels they had.
#define SRCNN_SPATIAL_ROWS_UNIT 1
#include "srcnn_spatial_kernels.hip"

namespace srcnn {

template <bool ZERO, typename Scale>
static void launch_l1r(dim3 grid, const uint8_t *src, long sstride, const L1Rows &rows, int W, int H, int m0, int m1,
                       const float *frag, float *map, long mpitch, Scale scale, hipStream_t st)
{
    hipLaunchKernelGGL((spatial_l1_kernel<1, ZERO, Scale, uint8_t, L1Rows>), grid, dim3(256), 0, st, src, sstride, rows, W, H, m0, m1,
                       frag, map, mpitch, scale);
}

hipError_t launch_spatial_l1_rows(bool zero, bool split, const uint8_t *src, long sstride, const L1Rows &rows, int W, int H, int m0,
                                  int m1, const float *frag, void *map, long mpitch, float scale, hipStream_t st)
{
    const dim3 grid((unsigned)((W + SL1_COLS - 1) / SL1_COLS), (unsigned)((m1 - m0 + SL1_ROWS - 1) / SL1_ROWS));
    float *m = static_cast<float *>(map);
    if (split && zero) launch_l1r<true>(grid, src, sstride, rows, W, H, m0, m1, frag, m, mpitch, scale, st);
    else if (split) launch_l1r<false>(grid, src, sstride, rows, W, H, m0, m1, frag, m, mpitch, scale, st);
    else if (zero) launch_l1r<true>(grid, src, sstride, rows, W, H, m0, m1, frag, m, mpitch, NoScale{}, st);
    else launch_l1r<false>(grid, src, sstride, rows, W, H, m0, m1, frag, m, mpitch, NoScale{}, st);
    return hipGetLastError();
}

}  // namespace srcnn
