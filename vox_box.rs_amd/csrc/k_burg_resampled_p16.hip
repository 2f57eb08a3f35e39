// k_burg_resampled_p16.hip -- the one-pass Burg lag kernels on the resampled view at order 16 (vbx_burg_resampled.hpp)
#include "vbx_burg_resampled.hpp"

namespace vbx {

VBX_BURG_RESAMPLED_INSTANTIATE(16)

}  // namespace vbx
