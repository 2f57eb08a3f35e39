// k_front_f32in.hip -- the front end of the frame loop on FLOAT32 samples (vbx_f32_to_f64, vbx_analyze_frames_ex_f32in):
//   float -> f64    every float is a double: the conversion is exact (subnormals, -0.0, infinities and NaNs arrive as the same values);
//                   the counterpart of pcm16_kernel (k_front.hip).  Only the shapes without a float form of every kernel take it.
//   frame peak      max |x| per frame (the pitch path's local_peak): taken in float and widened once -- widening is monotone and
//                   exact, so this is frame_peak_kernel (k_pitch_path.hip) on the widened samples, with its NaN-ignoring rule
//   frame RMS       frame_rms_kernel (k_front_ex.hip) with each sample widened on load: the same f64 sum in the same order
// HBM- / L2-bound stream work: coalesced loads, one pass.
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"

namespace vbx {

// two samples per lane and step: one 8-byte load (two of 4 bytes where x + head is not 8-byte aligned), one 16-byte store.  A first
// sample alone where `out` is at 8 mod 16, a last one alone where the rest is odd.  size_t indices: n may pass 2^31.
__global__ void f32_to_f64_kernel(const float *__restrict__ x, size_t n, double *__restrict__ out) {
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const size_t head = ((reinterpret_cast<uintptr_t>(out) & 15) != 0 && n > 0) ? 1 : 0;
    const float *xs = x + head;
    double *os = out + head;
    const size_t n2 = (n - head) / 2;
    if (t0 == 0 && head) out[0] = (double)x[0];
    if ((reinterpret_cast<uintptr_t>(xs) & 7) == 0) {
        for (size_t v = t0; v < n2; v += step) {
            const float2 w = reinterpret_cast<const float2 *>(xs)[v];
            reinterpret_cast<double2 *>(os)[v] = make_double2((double)w.x, (double)w.y);
        }
    } else {
        for (size_t v = t0; v < n2; v += step) {
            const float lo = xs[2 * v], hi = xs[2 * v + 1];
            reinterpret_cast<double2 *>(os)[v] = make_double2((double)lo, (double)hi);
        }
    }
    if (t0 == 0 && head + 2 * n2 < n) out[n - 1] = (double)x[n - 1];
}

void launch_f32_to_f64(hipStream_t s, const float *x, size_t n, double *out) {
    size_t blocks = (n / 2 + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(f32_to_f64_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, n, out);
}

// One wavefront per frame, lane l takes samples l, l + 64, ..: frame_peak_kernel's order
__global__ __launch_bounds__(256) void frame_peak_f32in_kernel(const float *__restrict__ x, long F, long n, long stride,
                                                               double *__restrict__ out) {
    const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= F) return;                                        // wavefront-uniform
    const float *row = x + f * stride;
    float m = __builtin_nanf("");                              // fmaxf(NaN, v) = v: an all-NaN frame stays NaN
    for (long i = lane; i < n; i += 64) m = fmaxf(m, fabsf(row[i]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if (lane == 0) out[f] = (double)m;
}

void launch_frame_peak_f32in(hipStream_t s, const float *x, long F, long n, long stride, double *out) {
    hipLaunchKernelGGL(frame_peak_f32in_kernel, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, s, x, F, n, stride, out);
}

template <bool PEAK>
__global__ __launch_bounds__(256) void frame_rms_f32in_kernel(const float *__restrict__ x, long F, int n, long stride,
                                                              double *__restrict__ out_rms, long rms_ld, double *__restrict__ out_peak) {
    const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= F) return;                                        // wavefront-uniform
    const float *row = x + f * stride;
    double s = 0.0;
    float m = __builtin_nanf("");
    for (int i = lane; i < n; i += 64) {
        const float q = row[i];
        const double v = (double)q;
        if constexpr (PEAK) m = fmaxf(m, fabsf(q));
        s = fma(v, v, s);
    }
    s = wave_sum(s);
    if constexpr (PEAK) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
        if (lane == 0) out_peak[f] = (double)m;
    }
    if (lane == 0) out_rms[f * rms_ld] = sqrt(s / (double)n);
}

void launch_frame_rms_f32in(hipStream_t s, const float *x, long F, int n, long stride, double *out_rms, long rms_ld, double *out_peak) {
    const dim3 g((unsigned)((F + 3) / 4)), b(256);
    if (out_peak) hipLaunchKernelGGL((frame_rms_f32in_kernel<true>), g, b, 0, s, x, F, n, stride, out_rms, rms_ld, out_peak);
    else hipLaunchKernelGGL((frame_rms_f32in_kernel<false>), g, b, 0, s, x, F, n, stride, out_rms, rms_ld, out_peak);
}

// ---- frames of any sample type: the form of x.kind ----------------------------------------------------------------------------
void launch_frame_peak(hipStream_t s, frames_t x, long F, long n, long stride, double *out) {
    switch (x.kind) {
        case SAMPLE_F64: launch_frame_peak(s, x.f64(), F, n, stride, out); break;
        case SAMPLE_PCM16: launch_frame_peak_pcm16(s, x.pcm16(), F, n, stride, out); break;
        case SAMPLE_F32: launch_frame_peak_f32in(s, x.f32in(), F, n, stride, out); break;
    }
}
void launch_frame_rms(hipStream_t s, frames_t x, long F, int n, long stride, double *out_rms, long rms_ld, double *out_peak) {
    if (x.kind == SAMPLE_F32) launch_frame_rms_f32in(s, x.f32in(), F, n, stride, out_rms, rms_ld, out_peak);
    else launch_frame_rms(s, x.f64(), x.pcm16(), F, n, stride, out_rms, rms_ld, out_peak);
}

}  // namespace vbx
