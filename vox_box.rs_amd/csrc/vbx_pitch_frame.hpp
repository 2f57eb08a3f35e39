// vbx_pitch_frame.hpp -- Pitched::pitch of ONE frame by one wavefront (k_pitch.hip has the description and the f64 / PCM kernels;
// k_lists_f32in.hip the list kernel that reads float samples).
#pragma once

#include <type_traits>
#include "vbx_autocorr.hpp"
#include "vbx_kernels.hpp"
#include "vbx_pitch_refine.hpp"

namespace vbx {

// ------------------------------------------------------------------------------------------
// Pitched::pitch, one wavefront per frame, one kernel (src/periodic.rs:396-455):
//  1) the windowed frame is staged in LDS as the padded image of vbx_autocorr.hpp and
//     r = self.autocorrelate(self.len()) (:403) runs on the FP64 matrix cores;
//  2) y[i] = (r[i] / max|r|) / w_lag[i] (:404-408) replaces the image in LDS (zero padded, standing for
//     resize(2N, 0), :411);
//  a) peak scan, lane-parallel: strict local maxima of y[0..N/2) (Q4), the "parabolic" lag (Q5) and
//     the frequency filter (:439); survivors are compacted in index order into an LDS list.
//     The sinc(30) strength of :433 is dead in the reference (overwritten at :448 for every
//     candidate that passes the filter, dropped otherwise) and is not evaluated.
//  b, c) refinement (improve_extremum_sinc) and the sorted candidate list, see below.
// Phase 1 keeps the matrix pipe busy and phases a-c the vector ALU; the wavefronts resident on a SIMD are in
// different phases of different frames, so both pipes work at the same time.
// ------------------------------------------------------------------------------------------
// ALIAS: a single autocorrelation pass (n <= AC_MF_NT * 256): the lag values wait in registers while y takes the
// image's place in LDS.  Otherwise y has its own region.
// TIN = float: `frames` carries float32 samples, widened on load (k_lists_f32in.hip; the f64 / PCM callers leave the default)
template <bool ALIAS, typename TIN = double>
__device__ __forceinline__ void pitch_frame_mfma(
    double *smem, const long f, const double *__restrict__ frames, int n, long stride, const double *__restrict__ window,
    const double *__restrict__ lag_window, double sample_rate, double threshold, double fmin, double fmax,
    int kmax, int full_off, double *__restrict__ out_cand, long cand_ld, int32_t *__restrict__ out_count,
    int32_t *__restrict__ status, unsigned long long *__restrict__ work, const bool pcm = false) {
    const int lane = lane_id();
    double *zs = smem;                              // padded image of the windowed frame (vbx_autocorr.hpp)
    // refinement state (vbx_pitch_refine.hpp): y[n + Y_PAD] | p16 | keys | candidate list
    double *ys = ALIAS ? smem : smem + ((ac_mf_lds_doubles(n) + 1) & ~1);
    {
        // all of the frame's loads are issued before the first LDS store (nothing else hides their latency here);
        // only the zero margins of the image are cleared, the pad double inside each 16 samples is never read
        const double *xf = frames + f * stride;
        const int16_t *x16 = reinterpret_cast<const int16_t *>(frames) + f * stride;        // the frame when pcm
        const float *x32 = reinterpret_cast<const float *>(frames) + f * stride;            // the frame when TIN = float
        constexpr bool F32 = std::is_same<TIN, float>::value;
        constexpr int NB = 8;
        for (int p = lane; p < ac_mf_phys(0); p += 64) zs[p] = 0.0;
        for (int p = ac_mf_phys(n) + lane; p < ac_mf_lds_doubles(n); p += 64) zs[p] = 0.0;
        for (int i0 = 0; i0 < n; i0 += 64 * NB) {
            double xv[NB], wv[NB];
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const int i = i0 + 64 * j + lane;
                xv[j] = (i < n) ? (F32 ? (double)x32[i] : pcm ? pcm16_value(x16[i]) : xf[i]) : 0.0;
                wv[j] = (window != nullptr && i < n) ? window[i] : 1.0;
            }
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const int i = i0 + 64 * j + lane;
                if (i < n) zs[ac_mf_phys(i)] = (window != nullptr) ? xv[j] * wv[j] : xv[j];
            }
        }
        wave_sync();
    }
    const double x0 = zs[ac_mf_phys(0)];
    double amax = -1.0;                             // max_amplitude over ALL lags (Q2; NaN never wins)
    if (ALIAS) {
        double rv[AC_MF_NT * 4];
        autocorr_mfma(zs, n, n, [&](int slot, int lag, double s) {          // self.autocorrelate(self.len()), :403
            const double r = (lag < n) ? (s - x0 * zs[ac_mf_phys(lag)]) + x0 : 0.0;
            rv[slot] = r;
            const double a = fabs(r);
            amax = (lag < n && a > amax) ? a : amax;
        });
        wave_sync();                                // every lane is done with the image
        amax = wave_max(amax);
        const double scale = 1.0 / amax;            // normalize (:404), then / lag window (:406-408)
#pragma unroll
        for (int slot = 0; slot < AC_MF_NT * 4; slot++) {
            const int lag = (slot >> 2) * AC_MF_TILE + 64 * (slot & 3) + lane;
            if (lag < n) ys[lag] = (rv[slot] * scale) / lag_window[lag];
        }
        if (lane < Y_PAD) ys[n + lane] = 0.0;
    } else {
        autocorr_mfma(zs, n, n, [&](int, int lag, double s) {
            if (lag < n) {
                const double r = (s - x0 * zs[ac_mf_phys(lag)]) + x0;
                ys[lag] = r;
                const double a = fabs(r);
                amax = (a > amax) ? a : amax;
            }
        });
        wave_sync();
        amax = wave_max(amax);
        const double scale = 1.0 / amax;
        for (int i = lane; i < n; i += 64) ys[i] = (ys[i] * scale) / lag_window[i];
        if (lane < Y_PAD) ys[n + lane] = 0.0;
    }
    wave_sync();

    pitch_params_t pp;
    pp.sample_rate = sample_rate; pp.threshold = threshold; pp.fmin = fmin; pp.fmax = fmax; pp.kmax = kmax; pp.full_off = full_off; pp.f32 = 0;
    double2 *full = full_off ? reinterpret_cast<double2 *>(reinterpret_cast<char *>(smem) + full_off) : nullptr;
    pitch_refine_store<0, PITCH_CELL_NB>(ys, n, pp, f, out_cand, cand_ld, out_count, status, work, 0.0, full);
}

}  // namespace vbx
