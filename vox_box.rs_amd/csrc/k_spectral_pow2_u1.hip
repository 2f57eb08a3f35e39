// k_spectral_pow2_u1.hip -- analyze_pow2_kernel<1, ..>: complex FFT of 1024 (vbx_spectral_pow2.hpp)
#include "vbx_spectral_pow2.hpp"

namespace vbx {

analyze_choice_t choose_pow2_u1(const spectral_launch_t &L) { return choose_pow2_u<1>(L); }
int launch_pow2_u1(hipStream_t s, const spectral_launch_t &L, const analyze_choice_t &c, spectral_args_t &a) { return launch_pow2_u<1>(s, L, c, a); }

}  // namespace vbx
