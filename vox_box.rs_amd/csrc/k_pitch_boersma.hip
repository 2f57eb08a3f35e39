// k_pitch_boersma.hip -- vbx_pitch_boersma_f64: Boersma's pitch candidates with an unquantised lag (vbx_pitch_boersma.hpp has the
// per-frame routine, include/voxbox_hip.h the definition).  One wavefront per frame, pitch_kernel's grid and XCD mapping.
#include "vbx_pitch_boersma.hpp"

namespace vbx {

template <bool ALIAS, int G>
__global__ __launch_bounds__(64) void pitch_boersma_kernel(
    const double *__restrict__ frames, long n_frames, int n, long stride, const double *__restrict__ window,
    const double *__restrict__ lag_window, double sample_rate, double threshold, double fmin, double fmax,
    int kmax, double *__restrict__ out_cand, int32_t *__restrict__ out_count, int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const long f = xcd_item(blockIdx.x, n_frames);          // neighbouring frames on the same XCD: their overlap hits its L2
    if (f >= n_frames) return;
    pitch_boersma_frame<ALIAS, G>(smem, f, frames, n, stride, window, lag_window, sample_rate, threshold, fmin, fmax, kmax,
                                  out_cand, out_count, status);
}

size_t pitch_boersma_lds_bytes(int n) {
    const size_t refine = (size_t)(n + Y_PAD + 2 * boersma_list_entries(n) + 4 * 64) * sizeof(double);
    const size_t image = (size_t)((ac_mf_lds_doubles(n) + 1) & ~1) * sizeof(double);
    if (n <= AC_MF_NT * AC_MF_TILE) return image > refine ? image : refine;
    return image + refine;
}

template <bool ALIAS, int G>
static void launch_one(hipStream_t s, size_t lds, const double *x, long F, int n, long stride, const double *window,
                       const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                       int kmax, pitch_t *out_cand, int32_t *out_count, int32_t *status) {
    hipLaunchKernelGGL((pitch_boersma_kernel<ALIAS, G>), dim3((unsigned)F), dim3(64), lds, s,
                       x, F, n, stride, window, lag_window, sample_rate, threshold, fmin, fmax, kmax,
                       reinterpret_cast<double *>(out_cand), out_count, status);
}

void launch_pitch_boersma(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                          const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                          int kmax, int group, pitch_t *out_cand, int32_t *out_count, int32_t *status) {
    const size_t lds = (pitch_boersma_lds_bytes(n) + 15) & ~(size_t)15;
    const bool alias = n <= AC_MF_NT * AC_MF_TILE;
#define VBX_BOERSMA_LAUNCH(A, G) launch_one<A, G>(s, lds, x, F, n, stride, window, lag_window, sample_rate, threshold, fmin, fmax, kmax, out_cand, out_count, status)
    if (group == 16) { if (alias) VBX_BOERSMA_LAUNCH(true, 16); else VBX_BOERSMA_LAUNCH(false, 16); }
    else { if (alias) VBX_BOERSMA_LAUNCH(true, 64); else VBX_BOERSMA_LAUNCH(false, 64); }
#undef VBX_BOERSMA_LAUNCH
}

}  // namespace vbx
