// k_front_ex.hip -- RMS::rms (src/waves.rs:10-23) of the rectangular frame beside the fused frame loop (vbx_analyze_frames_ex_*,
// examples/formant_extraction/src/main.rs:84), from the f64 view or straight from 16-bit PCM, and -- in a tracked call -- the
// pitch path's local_peak from the same read.  One wavefront per frame; lane l takes samples l, l + 64, ... in that order, as
// rms_kernel (k_front.hip) and frame_peak_kernel (k_pitch_path.hip) both do, so each value is that kernel's bit for bit.
// HBM- / L2-bound stream work (frames of a hop-strided view overlap): coalesced loads, one pass.
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"

namespace vbx {

// TIN = int16_t: the samples widened by pcm16_value (what vbx_pcm16_to_f64 writes); the peak as an integer max widened once
// (frame_peak_pcm16_kernel, k_front.hip)
template <typename TIN, bool PEAK>
__global__ __launch_bounds__(256) void frame_rms_kernel(const TIN *__restrict__ x, long F, int n, long stride,
                                                        double *__restrict__ out_rms, long rms_ld, double *__restrict__ out_peak) {
    constexpr bool PCM = sizeof(TIN) == 2;
    const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= F) return;                                        // wavefront-uniform
    const TIN *row = x + f * stride;
    double s = 0.0;
    double m = __builtin_nan("");                              // fmax(NaN, v) = v: an all-NaN frame stays NaN
    int mi = 0;
    for (int i = lane; i < n; i += 64) {
        double v;
        if constexpr (PCM) {
            const int q = (int)row[i];
            v = pcm16_value(q);
            if constexpr (PEAK) mi = max(mi, abs(q));
        } else {
            v = row[i];
            if constexpr (PEAK) m = fmax(m, fabs(v));
        }
        s = fma(v, v, s);
    }
    s = wave_sum(s);
    if constexpr (PEAK) {
        if constexpr (PCM) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) mi = max(mi, __shfl_xor(mi, d, 64));
            m = pcm16_value(mi);
        } else {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
        }
        if (lane == 0) out_peak[f] = m;
    }
    if (lane == 0) out_rms[f * rms_ld] = sqrt(s / (double)n);
}

void launch_frame_rms(hipStream_t s, const double *x, const int16_t *pcm, long F, int n, long stride, double *out_rms, long rms_ld,
                      double *out_peak) {
    const dim3 g((unsigned)((F + 3) / 4)), b(256);
    if (pcm) {
        if (out_peak) hipLaunchKernelGGL((frame_rms_kernel<int16_t, true>), g, b, 0, s, pcm, F, n, stride, out_rms, rms_ld, out_peak);
        else hipLaunchKernelGGL((frame_rms_kernel<int16_t, false>), g, b, 0, s, pcm, F, n, stride, out_rms, rms_ld, out_peak);
    } else {
        if (out_peak) hipLaunchKernelGGL((frame_rms_kernel<double, true>), g, b, 0, s, x, F, n, stride, out_rms, rms_ld, out_peak);
        else hipLaunchKernelGGL((frame_rms_kernel<double, false>), g, b, 0, s, x, F, n, stride, out_rms, rms_ld, out_peak);
    }
}

}  // namespace vbx
