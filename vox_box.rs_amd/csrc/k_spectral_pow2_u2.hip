// k_spectral_pow2_u2.hip -- analyze_pow2_kernel<2, ..>: complex FFT of 2048 (vbx_spectral_pow2.hpp)
#include "vbx_spectral_pow2.hpp"

namespace vbx {

#ifdef VBX_POW2_2048_TWO_WAVES
#define VBX_POW2_U2 1, 2
#else
#define VBX_POW2_U2 2
#endif
analyze_choice_t choose_pow2_u2(const spectral_launch_t &L) { return choose_pow2_u<VBX_POW2_U2>(L); }
int launch_pow2_u2(hipStream_t s, const spectral_launch_t &L, const analyze_choice_t &c, spectral_args_t &a) { return launch_pow2_u<VBX_POW2_U2>(s, L, c, a); }
#undef VBX_POW2_U2

}  // namespace vbx
