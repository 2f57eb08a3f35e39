// k_burg_resampled_p10.hip -- the one-pass Burg lag kernels on the resampled view at order 10 (vbx_burg_resampled.hpp)
#include "vbx_burg_resampled.hpp"

namespace vbx {

VBX_BURG_RESAMPLED_INSTANTIATE(10)

}  // namespace vbx
