// k_spectral_f32in.hip -- the fused analysis kernel of k_spectral.hip on FLOAT32 samples (vbx_analyze_frames_ex_f32in): the same
// kernel (analyze_kernel<..., float>, vbx_spectral_1200.hpp) with the sample type chosen at compile time, in a translation unit of
// its own so that the f64 / PCM instantiations of k_spectral.hip stay the code they were.  Lane n' needs samples 120 q + 2 n' and
// + 1: one 8-byte load per q where the frame's address is 8-byte aligned, two 4-byte loads otherwise, widened before the window
// product -- from there on the registers hold what the f64 kernel's hold, so the records are that kernel's on the widened copy
// bit for bit and the register budget is the f64 form's (168 registers at three wavefronts per SIMD).
#include "vbx_spectral_1200.hpp"

namespace vbx {

bool launch_analyze_f32in(hipStream_t s, const analyze_choice_t &c, const spectral_args_t &a) {
    return c.waves == 3 ? sp_launch_1200<SP_ANALYZE, 3, float>(s, c, a) : sp_launch_1200<SP_ANALYZE, VBX_SPECTRAL_WAVES, float>(s, c, a);
}

}  // namespace vbx
