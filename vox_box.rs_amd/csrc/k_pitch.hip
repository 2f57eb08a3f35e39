// k_pitch.hip -- Pitched::pitch (Boersma-style autocorrelation pitch candidates).
//
// Reference: src/periodic.rs:29-87 (interpolate_sinc), :103-188 (brent_maximize),
//            :192-229 (improve_extremum), :362-375 (local_maxima), :396-455 (pitch),
//            src/waves.rs:44-75 (max_amplitude / normalize).  Quirks Q1-Q10 reproduced.
//
// One kernel, one wavefront per frame: (1) the windowed frame is staged in LDS and the all-lag autocorrelation
// runs on the FP64 matrix cores (vbx_autocorr.hpp), giving the normalised / lag-window-divided curve y, which
// replaces the frame in LDS; (2) the candidate peaks are compacted in index order, bounded from above (one lane
// per candidate) and refined best-bound-first, one candidate at a time: every lane runs the reference's Brent
// iteration on identical values (wave sums are bit-identical in all lanes), while each sinc evaluation -- the
// dominant cost, 2*(depth+1) terms -- is spread over the 64 lanes and reduced with DPP.  Candidates that provably
// cannot reach the returned top-kmax are skipped (exact).  The path is FP64 bound (hundreds of flop per byte);
// HBM traffic is the frame's samples in and 16 bytes per kept candidate out.
#include "vbx_pitch_frame.hpp"

namespace vbx {

template <bool ALIAS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void pitch_kernel(
    const double *__restrict__ frames, long n_frames, int n, long stride, const double *__restrict__ window,
    const double *__restrict__ lag_window, double sample_rate, double threshold, double fmin, double fmax,
    int kmax, int full_off, double *__restrict__ out_cand, long cand_ld, int32_t *__restrict__ out_count,
    int32_t *__restrict__ status, unsigned long long *__restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const long f = xcd_item(blockIdx.x, n_frames);          // neighbouring frames on the same XCD: their overlap hits its L2
    if (f >= n_frames) return;
    pitch_frame_mfma<ALIAS>(smem, f, frames, n, stride, window, lag_window, sample_rate, threshold, fmin, fmax, kmax,
                            full_off, out_cand, cand_ld, out_count, status, work);
}

// The same per-frame routine over a list of frame indices: the frames the FFT-based kernel (k_spectral.hip) could not
// decide within its rounding error.  A fixed grid walks the list; *list_count is read on the device.
template <bool ALIAS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void pitch_list_kernel(
    const int32_t *__restrict__ frame_list, const int32_t *__restrict__ list_count,
    const double *__restrict__ frames, int n, long stride, const double *__restrict__ window,
    const double *__restrict__ lag_window, double sample_rate, double threshold, double fmin, double fmax,
    int kmax, int full_off, double *__restrict__ out_cand, long cand_ld, int32_t *__restrict__ out_count,
    int32_t *__restrict__ status, unsigned long long *__restrict__ work, int pcm) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int count = *list_count;
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
        pitch_frame_mfma<ALIAS>(smem, (long)frame_list[i], frames, n, stride, window, lag_window, sample_rate, threshold,
                                fmin, fmax, kmax, full_off, out_cand, cand_ld, out_count, status, work, pcm != 0);
        wave_sync();
    }
}

// ------------------------------------------------------------------------------------------
// interpolate_sinc / improve_extremum at M query points of one curve (PG lanes per point)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void sinc_points_kernel(const double *__restrict__ y, int ylen, int offset, int nx,
                                                         const double *__restrict__ xs, long m, int depth,
                                                         double *__restrict__ out, int32_t *__restrict__ status) {
    const long q = (long)blockIdx.x * PNG + lane_id() / PG;
    const bool have = q < m;
    int st = 0;
    const double v = sinc_interp<PG>(y, ylen, ylen, offset, nx, have ? xs[q] : 0.0, depth, have, st);
    if (have && (lane_id() & (PG - 1)) == 0) {
        out[q] = (st & 4) ? 0.0 : v;
        if (status != nullptr) status[q] = (st & 4) ? 4 : 0;
    }
}

// interp: 0 Interpolation::None, 1 Parabolic, 2 Sinc(depth) (src/periodic.rs:192-229); is_max == 0 negates the interpolant
__global__ __launch_bounds__(64) void extremum_points_kernel(const double *__restrict__ y, int ylen, int offset, int nx,
                                                             const double *__restrict__ ix, long m, int depth,
                                                             double *__restrict__ out_xy, int32_t *__restrict__ status,
                                                             int interp, int is_max) {
    const long q = (long)blockIdx.x * PNG + lane_id() / PG;
    const bool have = q < m;
    int st = 0;
    double xmid = 0., ymid = 0.;
    if (interp == 2) {
        improve_extremum_sinc<PG>(y, ylen, ylen, offset, nx, have ? ix[q] : 1.0, depth, have, xmid, ymid, st, nullptr, nullptr,
                                  -__builtin_inf(), nullptr, is_max == 0);
    } else if (have) {
        const double ixmid = ix[q];
        if (ylen < 1) st |= 4;
        else if (ixmid == 0.) { xmid = 0.; ymid = y[0]; }                                              // :193
        else if (ixmid >= (double)nx) {                                                                // :194
            if (nx < 1 || nx - 1 >= ylen) st |= 4; else { xmid = (double)nx; ymid = y[nx - 1]; }
        } else if (interp == 0) { xmid = 0.; ymid = y[0]; }                                            // :197-199
        else {                                                                                         // :200-207
#pragma clang fp contract(off)
            const double fl = floor(ixmid);
            if (!(fl >= 1.) || !(fl + 1. < (double)ylen)) st |= 4;       // usize underflow / index out of bounds (NaN too)
            else {
                const int i = (int)fl;
                const double diff = y[i + 1] - y[i - 1];
                const double mid = y[i];
                const double dy = 0.5 * diff;
                const double d2y = 2.0 * mid - diff;
                xmid = ixmid + dy / d2y;
                ymid = mid + 0.5 * dy * dy / d2y;
            }
        }
    }
    if (have && (lane_id() & (PG - 1)) == 0) {
        out_xy[2 * q] = (st & 4) ? 0.0 : xmid;
        out_xy[2 * q + 1] = (st & 4) ? 0.0 : ymid;
        if (status != nullptr) status[q] = (st & 4) ? 4 : 0;
    }
}

size_t pitch_lds_bytes(int n) {
    const int nblk = (n + PB - 1) / PB;
    const size_t refine = (size_t)(n + Y_PAD + ((nblk + 2) & ~1)) * sizeof(double) + (size_t)(n / 4 + 8) * (sizeof(float) + sizeof(cand_t));
    const size_t image = (size_t)((ac_mf_lds_doubles(n) + 1) & ~1) * sizeof(double);
    if (n <= AC_MF_NT * AC_MF_TILE) return image > refine ? image : refine;
    return image + refine;
}

// kmax > PITCH_LIST_LANES: the whole candidate Vec is wanted; its entries are parked in an extra LDS region behind
// the frame state (vbx_pitch_refine.hpp, `full`) and rank-sorted at the end of the frame
size_t pitch_full_list_bytes(int n, int kmax) {
    return kmax > PITCH_LIST_LANES ? (size_t)pitch_full_list_entries(n) * sizeof(double2) : 0;
}

void launch_pitch(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                  const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                  int kmax, pitch_t *out_cand, long cand_ld, int32_t *out_count, int32_t *status,
                  unsigned long long *work) {
    const size_t base = (pitch_lds_bytes(n) + 15) & ~(size_t)15, extra = pitch_full_list_bytes(n, kmax);
    const int full_off = extra ? (int)base : 0;
    if (n <= AC_MF_NT * AC_MF_TILE)
        hipLaunchKernelGGL((pitch_kernel<true>), dim3((unsigned)F), dim3(64), base + extra, s,
                           x, F, n, stride, window, lag_window, sample_rate, threshold, fmin, fmax, kmax, full_off,
                           reinterpret_cast<double *>(out_cand), cand_ld, out_count, status, work);
    else
        hipLaunchKernelGGL((pitch_kernel<false>), dim3((unsigned)F), dim3(64), base + extra, s,
                           x, F, n, stride, window, lag_window, sample_rate, threshold, fmin, fmax, kmax, full_off,
                           reinterpret_cast<double *>(out_cand), cand_ld, out_count, status, work);
}

void launch_pitch_list(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int grid,
                       const double *x, int n, long stride, const double *window,
                       const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                       int kmax, pitch_t *out_cand, long cand_ld, int32_t *out_count, int32_t *status,
                       unsigned long long *work, bool pcm) {
    const size_t base = (pitch_lds_bytes(n) + 15) & ~(size_t)15, extra = pitch_full_list_bytes(n, kmax);
    const int full_off = extra ? (int)base : 0;
    if (n <= AC_MF_NT * AC_MF_TILE)
        hipLaunchKernelGGL((pitch_list_kernel<true>), dim3((unsigned)grid), dim3(64), base + extra, s,
                           frame_list, list_count, x, n, stride, window, lag_window, sample_rate, threshold, fmin, fmax, kmax,
                           full_off, reinterpret_cast<double *>(out_cand), cand_ld, out_count, status, work, pcm ? 1 : 0);
    else
        hipLaunchKernelGGL((pitch_list_kernel<false>), dim3((unsigned)grid), dim3(64), base + extra, s,
                           frame_list, list_count, x, n, stride, window, lag_window, sample_rate, threshold, fmin, fmax, kmax,
                           full_off, reinterpret_cast<double *>(out_cand), cand_ld, out_count, status, work, pcm ? 1 : 0);
}

void launch_sinc_points(hipStream_t s, const double *y, int ylen, long offset, long nx, const double *xs, long m,
                        long depth, double *out, int32_t *status) {
    hipLaunchKernelGGL(sinc_points_kernel, dim3((unsigned)((m + PNG - 1) / PNG)), dim3(64), 0, s,
                       y, ylen, (int)offset, (int)nx, xs, m, (int)depth, out, status);
}

void launch_extremum_points(hipStream_t s, const double *y, int ylen, long offset, long nx, const double *ix, long m,
                            long depth, double *out_xy, int32_t *status, int interp, int is_max) {
    hipLaunchKernelGGL(extremum_points_kernel, dim3((unsigned)((m + PNG - 1) / PNG)), dim3(64), 0, s,
                       y, ylen, (int)offset, (int)nx, ix, m, (int)depth, out_xy, status, interp, is_max);
}

}  // namespace vbx
