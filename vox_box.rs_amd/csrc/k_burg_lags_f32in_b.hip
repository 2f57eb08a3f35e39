// k_burg_lags_f32in_b.hip -- the one-pass Burg lag kernels (vbx_burg_fast.hpp) and their form on the resampled view
// (vbx_burg_resampled.hpp) on FLOAT32 samples, at orders 13, 14, 16 (two translation units keep the build parallel)
#include "vbx_burg_resampled.hpp"

namespace vbx {

VBX_BURG_FAST_DEFINE_LAGS
VBX_BURG_RESAMPLED_DEFINE
template void launch_burg_lags_p<13, float>(hipStream_t, const float *, long, int, long, const double *, frame_map_t, long, long, double *);
template void launch_burg_lags_resampled_p<13, float>(hipStream_t, const float *, long, int, long, const double *, resample_src_t, frame_map_t, long, long, double *);
template void launch_burg_lags_p<14, float>(hipStream_t, const float *, long, int, long, const double *, frame_map_t, long, long, double *);
template void launch_burg_lags_resampled_p<14, float>(hipStream_t, const float *, long, int, long, const double *, resample_src_t, frame_map_t, long, long, double *);
template void launch_burg_lags_p<16, float>(hipStream_t, const float *, long, int, long, const double *, frame_map_t, long, long, double *);
template void launch_burg_lags_resampled_p<16, float>(hipStream_t, const float *, long, int, long, const double *, resample_src_t, frame_map_t, long, long, double *);

}  // namespace vbx
