// k_lpc_exact.hip -- LPC::lpc (src/spectrum.rs:63-84) on Autocorrelate::autocorrelate (src/periodic.rs:276-289) of the frames
// whose Levinson row the fused kernels' probe found ill-conditioned (levinson_probe, vbx_spectral.hpp): the p + 1 lag sums
// accumulated in double-double (Ogita / Rump / Oishi's Dot2: every product split exactly by one FMA, every addition's rounding
// recovered by TwoSum), the recursion in double-double, one rounding at the end.  What comes out is the exact-arithmetic row of
// the f64 frame rounded to f64 -- closer to the exact answer than either f64 recursion (the reference's own included) can be on
// such a frame, and what tests/test_gpu_soak.py holds against the same recursion in long double.
//
// Row A10 of SURVEY 8a.  Cost per listed frame: ~10 instructions per product (13 n products over 64 lanes: 2.4 k at 1200
// samples) + a sixteenth of the serial recursion -- a fifth of a frame of analyze_kernel; the list is ~0.1 % of the synthetic
// signal's frames and ~10 % of real 44.1 kHz speech at order 13 (tools/experiments notes in DESIGN.md section 3).
#include "vbx_lpc_exact.hpp"

namespace vbx {

bool lpc_exact_supported(int n, int p) { return p >= 1 && p + 1 <= LX_NLMAX && n >= 2 && n <= 4096; }

void launch_lpc_exact_list(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int cus, const double *x, int n,
                           long stride, const double *window, bool pcm, int p, double *out_lpc, long lpc_ld) {
    const lpc_exact_geom g = lpc_exact_geometry(n, p, cus);
    hipLaunchKernelGGL(lpc_exact_list_kernel<>, dim3(g.grid), dim3(64), g.lds, s, frame_list, list_count, x, n, stride, window,
                       pcm ? 1 : 0, p + 1, out_lpc, lpc_ld);
}

}  // namespace vbx
