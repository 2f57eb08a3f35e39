// k_lists_f32in.hip -- the kernels that go back to a frame's SAMPLES behind the fused analysis kernel, on FLOAT32 samples
// (vbx_analyze_frames_ex_f32in): the direct-sum pitch kernel over the frames the FFT form could not decide (k_pitch.hip), the
// double-double LPC rows of the frames the probe listed (k_lpc_exact.hip) and the crate's own rows under VBX_LPC_POLICY_REFERENCE
// (k_lpc_ref.hip).  Each is that file's kernel with float as the sample type: a sample is widened -- exactly -- where it is loaded,
// everything after that is the f64 kernel's arithmetic.
#include "vbx_pitch_frame.hpp"
#include "vbx_lpc_exact.hpp"
#include "vbx_lpc_ref.hpp"

namespace vbx {

template <bool ALIAS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void pitch_list_f32in_kernel(
    const int32_t *__restrict__ frame_list, const int32_t *__restrict__ list_count,
    const float *__restrict__ frames, int n, long stride, const double *__restrict__ window,
    const double *__restrict__ lag_window, double sample_rate, double threshold, double fmin, double fmax,
    int kmax, int full_off, double *__restrict__ out_cand, long cand_ld, int32_t *__restrict__ out_count,
    int32_t *__restrict__ status, unsigned long long *__restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int count = *list_count;
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
        pitch_frame_mfma<ALIAS, float>(smem, (long)frame_list[i], reinterpret_cast<const double *>(frames), n, stride, window, lag_window,
                                       sample_rate, threshold, fmin, fmax, kmax, full_off, out_cand, cand_ld, out_count, status, work);
        wave_sync();
    }
}

void launch_pitch_list_f32in(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int grid,
                             const float *x, int n, long stride, const double *window,
                             const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                             int kmax, pitch_t *out_cand, long cand_ld, int32_t *out_count, int32_t *status,
                             unsigned long long *work) {
    const size_t base = (pitch_lds_bytes(n) + 15) & ~(size_t)15, extra = pitch_full_list_bytes(n, kmax);
    const int full_off = extra ? (int)base : 0;
    if (n <= AC_MF_NT * AC_MF_TILE)
        hipLaunchKernelGGL((pitch_list_f32in_kernel<true>), dim3((unsigned)grid), dim3(64), base + extra, s,
                           frame_list, list_count, x, n, stride, window, lag_window, sample_rate, threshold, fmin, fmax, kmax,
                           full_off, reinterpret_cast<double *>(out_cand), cand_ld, out_count, status, work);
    else
        hipLaunchKernelGGL((pitch_list_f32in_kernel<false>), dim3((unsigned)grid), dim3(64), base + extra, s,
                           frame_list, list_count, x, n, stride, window, lag_window, sample_rate, threshold, fmin, fmax, kmax,
                           full_off, reinterpret_cast<double *>(out_cand), cand_ld, out_count, status, work);
}

void launch_lpc_exact_list_f32in(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int cus, const float *x, int n,
                                 long stride, const double *window, int p, double *out_lpc, long lpc_ld) {
    const lpc_exact_geom g = lpc_exact_geometry(n, p, cus);
    hipLaunchKernelGGL(lpc_exact_list_kernel<float>, dim3(g.grid), dim3(64), g.lds, s, frame_list, list_count,
                       reinterpret_cast<const double *>(x), n, stride, window, 0, p + 1, out_lpc, lpc_ld);
}

void launch_lpc_ref_f32in(hipStream_t s, const float *x, long F, int n, long stride, const double *window, int n_lags, int p,
                          int normalize, double *out_r, long r_ld, double *out_lpc, long lpc_ld) {
    if (F <= 0) return;
    const lpc_ref_geom g = lpc_ref_geometry(F, n_lags);
    const unsigned grid = g.grid;
    const size_t lds = g.lds;
    if (p == LREF_FIXED_P) hipLaunchKernelGGL((lpc_ref_kernel<false, 12, true>), dim3(grid), dim3(64), lds, s, x, F, n, stride, window, n_lags, p, normalize, out_r, r_ld, out_lpc, lpc_ld);
    else hipLaunchKernelGGL((lpc_ref_kernel<false, 0, true>), dim3(grid), dim3(64), lds, s, x, F, n, stride, window, n_lags, p, normalize, out_r, r_ld, out_lpc, lpc_ld);
}

// ---- frames of any sample type: the form of x.kind (the f64 kernels take PCM through their f64 argument, behind a flag) ----------
void launch_pitch_list(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int grid, frames_t x, int n, long stride,
                       const double *window, const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                       int kmax, pitch_t *out_cand, long cand_ld, int32_t *out_count, int32_t *status, unsigned long long *work) {
    if (x.kind == SAMPLE_F32)
        launch_pitch_list_f32in(s, frame_list, list_count, grid, x.f32in(), n, stride, window, lag_window, sample_rate, threshold, fmin,
                                fmax, kmax, out_cand, cand_ld, out_count, status, work);
    else
        launch_pitch_list(s, frame_list, list_count, grid, static_cast<const double *>(x.p), n, stride, window, lag_window, sample_rate,
                          threshold, fmin, fmax, kmax, out_cand, cand_ld, out_count, status, work, x.kind == SAMPLE_PCM16);
}
void launch_lpc_exact_list(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int cus, frames_t x, int n, long stride,
                           const double *window, int p, double *out_lpc, long lpc_ld) {
    if (x.kind == SAMPLE_F32) launch_lpc_exact_list_f32in(s, frame_list, list_count, cus, x.f32in(), n, stride, window, p, out_lpc, lpc_ld);
    else launch_lpc_exact_list(s, frame_list, list_count, cus, static_cast<const double *>(x.p), n, stride, window, x.kind == SAMPLE_PCM16, p,
                               out_lpc, lpc_ld);
}
void launch_lpc_ref(hipStream_t s, frames_t x, long F, int n, long stride, const double *window, int n_lags, int p, int normalize,
                    double *out_r, long r_ld, double *out_lpc, long lpc_ld) {
    if (x.kind == SAMPLE_F32) launch_lpc_ref_f32in(s, x.f32in(), F, n, stride, window, n_lags, p, normalize, out_r, r_ld, out_lpc, lpc_ld);
    else launch_lpc_ref(s, x.p, x.kind == SAMPLE_PCM16, F, n, stride, window, n_lags, p, normalize, out_r, r_ld, out_lpc, lpc_ld);
}

}  // namespace vbx
