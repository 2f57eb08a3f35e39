// k_lpc_ref.hip -- the crate's own f64 arithmetic for the LPC rows computed from frames (VBX_LPC_POLICY_REFERENCE):
//   Autocorrelate::autocorrelate   src/periodic.rs:276-289   r[lag] = fold(x[0], |acc, (a, b)| acc + a * b), i = 1 .. n - lag
//   Normalize::normalize           src/waves.rs:60-76        scale = 1 / max|r|, r * scale
//   LPC::lpc_mut / lpc             src/spectrum.rs:63-92     the Levinson-Durbin recursion
// every operation an IEEE f64 operation in the order the source states, no contraction -- the rows are bit for bit what the
// crate returns (tests/test_gpu_lpc_reference.py holds them to the CPU restatement of the same statements).
//
// A sequential fold cannot be re-associated, split across lanes, done by FFT or put on the matrix cores without changing its
// rounding, so the parallelism is across (frame, lag): one lane per lag of G frames of one wavefront (4 frames x 13 lags = 52
// lanes at order 12), as the f32 instantiation does it (k_f32.hip).  The frames stream through LDS in tiles of LREF_T samples
// plus a halo of 64: x[i] is a broadcast read, x[i + lag] a read of consecutive words.  More than 64 lags (autocorrelate only):
// one frame per wavefront, 64 lags at a time, the lag side staged from x[c + lag0 ..].  Then the normalize and the recursion of
// each frame on one lane: at order 12 in registers, at the other orders with the row in the frame's (then idle) LDS slot.
#include "vbx_lpc_ref.hpp"

namespace vbx {

namespace {

// LPC::lpc_mut on rows of lag sums (vbx_lpc_mut_f64 / vbx_lpc_f64 under the REFERENCE policy): a lane per row.  r may be out.
__global__ void levinson_ref_rows_kernel(const double *__restrict__ r, long n_rows, long r_stride, int p, double *out, long out_ld,
                                         double *__restrict__ out_kc) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    double rr[VBX_MAX_LPC_ORDER_K + 1], ac[VBX_MAX_LPC_ORDER_K + 1], tmp[VBX_MAX_LPC_ORDER_K + 1];
    for (int i = 0; i <= p; i++) rr[i] = r[row * r_stride + i];
    levinson_ref(rr, p, ac, tmp, out_kc != nullptr ? out_kc + row * (long)p : nullptr, 1);
    for (int i = 0; i <= p; i++) out[row * out_ld + i] = ac[i];
}

}  // namespace

// out_r: [F, r_ld] (may be NULL when out_lpc is not), out_lpc: [F, lpc_ld] (NULL: lag sums only, p = 0; n_lags <= n).  p >= 1:
// n_lags = p + 1.
void launch_lpc_ref(hipStream_t s, const void *x, bool pcm, long F, int n, long stride, const double *window, int n_lags, int p,
                    int normalize, double *out_r, long r_ld, double *out_lpc, long lpc_ld) {
    if (F <= 0) return;
    const lpc_ref_geom g = lpc_ref_geometry(F, n_lags);
    const unsigned grid = g.grid;
    const size_t lds = g.lds;
    if (pcm) {
        if (p == LREF_FIXED_P) hipLaunchKernelGGL((lpc_ref_kernel<true, 12>), dim3(grid), dim3(64), lds, s, x, F, n, stride, window, n_lags, p, normalize, out_r, r_ld, out_lpc, lpc_ld);
        else hipLaunchKernelGGL((lpc_ref_kernel<true, 0>), dim3(grid), dim3(64), lds, s, x, F, n, stride, window, n_lags, p, normalize, out_r, r_ld, out_lpc, lpc_ld);
    } else {
        if (p == LREF_FIXED_P) hipLaunchKernelGGL((lpc_ref_kernel<false, 12>), dim3(grid), dim3(64), lds, s, x, F, n, stride, window, n_lags, p, normalize, out_r, r_ld, out_lpc, lpc_ld);
        else hipLaunchKernelGGL((lpc_ref_kernel<false, 0>), dim3(grid), dim3(64), lds, s, x, F, n, stride, window, n_lags, p, normalize, out_r, r_ld, out_lpc, lpc_ld);
    }
}

void launch_levinson_ref_rows(hipStream_t s, const double *r, long rows, long r_stride, int p, double *out, long out_ld, double *out_kc) {
    const int bs = 64;
    hipLaunchKernelGGL(levinson_ref_rows_kernel, dim3((unsigned)((rows + bs - 1) / bs)), dim3(bs), 0, s, r, rows, r_stride, p, out, out_ld, out_kc);
}

}  // namespace vbx
