// k_burg_resampled_p8.hip -- the one-pass Burg lag kernels on the resampled view at order 8 (vbx_burg_resampled.hpp)
#include "vbx_burg_resampled.hpp"

namespace vbx {

VBX_BURG_RESAMPLED_INSTANTIATE(8)

}  // namespace vbx
