// k_spectral_f32in.hip -- the fused analysis kernel of k_spectral.hip on FLOAT32 samples (vbx_analyze_frames_ex_f32in): the same
// kernel (analyze_kernel<..., float>, vbx_spectral_1200.hpp) with the sample type chosen at compile time, in a translation unit of
// its own so that the f64 / PCM instantiations of k_spectral.hip stay the code they were.  Lane n' needs samples 120 q + 2 n' and
// + 1: one 8-byte load per q where the frame's address is 8-byte aligned, two 4-byte loads otherwise, widened before the window
// product -- from there on the registers hold what the f64 kernel's hold, so the records are that kernel's on the widened copy
// bit for bit and the register budget is the f64 form's (168 registers at three wavefronts per SIMD).
#include "vbx_spectral_1200.hpp"

namespace vbx {

void launch_analyze_f32in(hipStream_t s, const spectral_args_1200_t &a, unsigned grid, size_t lds, bool lpc, bool mfcc, bool waves3) {
    const dim3 g(grid), b(64);
#define VBX_SP32_LAUNCH(LPC_, MF_)                                                                                \
    do {                                                                                                           \
        if (waves3) hipLaunchKernelGGL((analyze_kernel<LPC_, MF_, true, SP_ANALYZE, 3, float>), g, b, lds, s, a);                     \
        else hipLaunchKernelGGL((analyze_kernel<LPC_, MF_, true, SP_ANALYZE, VBX_SPECTRAL_WAVES, float>), g, b, lds, s, a);           \
    } while (0)
    if (lpc && mfcc) VBX_SP32_LAUNCH(true, true);
    else if (lpc) VBX_SP32_LAUNCH(true, false);
    else if (mfcc) VBX_SP32_LAUNCH(false, true);
    else VBX_SP32_LAUNCH(false, false);
#undef VBX_SP32_LAUNCH
}

}  // namespace vbx
