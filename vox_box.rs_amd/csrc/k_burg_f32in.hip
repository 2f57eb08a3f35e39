// k_burg_f32in.hip -- Burg's direct recursion (k_burg.hip) and its form on the resampled view (k_burg_resampled.hip) on FLOAT32
// samples with f64 window, arithmetic and coefficients (vbx_analyze_frames_ex_f32in): the same kernels at the template parameters the
// f64 launchers pick for the same length, with float as the sample type.  A sample is widened -- exactly -- where it is loaded, so a
// row is the f64 kernel's on the widened copy of the frames bit for bit.
#include "vbx_burg_direct.hpp"
#include "vbx_burg_resampled_direct.hpp"

namespace vbx {

void launch_burg_f32in(hipStream_t s, const float *x, long F, int n, long stride, const double *window,
                       int p, double *out, int32_t *status, frame_map_t map) {
    launch_burg_t<double, float>(s, x, F, n, stride, window, p, out, status, map);
}
void launch_burg_f32in_list(hipStream_t s, const float *x, long F, int n, long stride, const double *window,
                            int p, double *out, int32_t *status, const int32_t *list, const int32_t *count) {
    launch_burg_list_t<float>(s, x, F, n, stride, window, p, out, status, list, count);
}
void launch_burg_resampled_f32in(hipStream_t s, const float *x, long F, int m, long stride, const double *window,
                                 resample_src_t rs, int p, double *out, int32_t *status, frame_map_t map) {
    launch_burg_resampled_t<float>(s, x, F, m, stride, window, rs, p, out, status, map);
}
void launch_burg_resampled_f32in_list(hipStream_t s, const float *x, long F, int m, long stride, const double *window,
                                      resample_src_t rs, int p, double *out, int32_t *status, const int32_t *list, const int32_t *count) {
    launch_burg_resampled_list_t<float>(s, x, F, m, stride, window, rs, p, out, status, list, count);
}

// ---- frames of any sample type: the form of x.kind ----------------------------------------------------------------------------
void launch_burg(hipStream_t s, frames_t x, long F, int n, long stride, const double *window, int p, double *out, int32_t *status,
                 frame_map_t map) {
    switch (x.kind) {
        case SAMPLE_F64: launch_burg(s, x.f64(), F, n, stride, window, p, out, status, map); break;
        case SAMPLE_PCM16: launch_burg_pcm16(s, x.pcm16(), F, n, stride, window, p, out, status, map); break;
        case SAMPLE_F32: launch_burg_f32in(s, x.f32in(), F, n, stride, window, p, out, status, map); break;
    }
}
void launch_burg_list(hipStream_t s, frames_t x, long F, int n, long stride, const double *window, int p, double *out, int32_t *status,
                      const int32_t *list, const int32_t *count) {
    switch (x.kind) {
        case SAMPLE_F64: launch_burg_list(s, x.f64(), F, n, stride, window, p, out, status, list, count); break;
        case SAMPLE_PCM16: launch_burg_pcm16_list(s, x.pcm16(), F, n, stride, window, p, out, status, list, count); break;
        case SAMPLE_F32: launch_burg_f32in_list(s, x.f32in(), F, n, stride, window, p, out, status, list, count); break;
    }
}
void launch_burg_resampled(hipStream_t s, frames_t x, long F, int m, long stride, const double *window, resample_src_t rs, int p,
                           double *out, int32_t *status, frame_map_t map) {
    if (x.kind == SAMPLE_F32) launch_burg_resampled_f32in(s, x.f32in(), F, m, stride, window, rs, p, out, status, map);
    else launch_burg_resampled(s, x.f64(), x.pcm16(), F, m, stride, window, rs, p, out, status, map);
}
void launch_burg_resampled_list(hipStream_t s, frames_t x, long F, int m, long stride, const double *window, resample_src_t rs, int p,
                                double *out, int32_t *status, const int32_t *list, const int32_t *count) {
    if (x.kind == SAMPLE_F32) launch_burg_resampled_f32in_list(s, x.f32in(), F, m, stride, window, rs, p, out, status, list, count);
    else launch_burg_resampled_list(s, x.f64(), x.pcm16(), F, m, stride, window, rs, p, out, status, list, count);
}

}  // namespace vbx
