// k_burg.hip -- Burg LPC (LPC::lpc_praat_mut, src/spectrum.rs:101-146, Q12).
//
// G lanes per frame, 64/G frames per wavefront.  A lane keeps b1/b2 elements
// [lig*EPL, (lig+1)*EPL) of its frame in registers, so the reference's shift
//   b2[j] <- b2[j+1] - a*b1[j+1]
// needs ONE neighbour-lane fetch per order (DPP wave_shl) instead of a pass through memory.
// Per order: two group reductions (num, denum; DPP, bit-identical inside the group), the
// coefficient recursion with coefficient t in lane t of the group (the reversed operand aa[i-2-t] by one
// lane permute: no LDS, no serial loop), one fused update sweep.
// The shrinking valid range [0, N-i) is kept by zeroing exactly the element that drops out.
// Short frames use small groups so that the per-order overhead is shared by several frames.
//
// The denominator.  The reference sums b1^2 + b2^2 over the valid range at every order (:118-121).  With mu = 2 num / den
// the updated arrays satisfy, exactly in real arithmetic,
//     den' = (1 - mu^2) den - (b1[last] - mu b2[last])^2 - (b2[0] - mu b1[0])^2
// (the two elements that leave the range: `last` = the one the update zeroes, and the one the shift drops at the front),
// which costs two broadcasts instead of 2 EPL FMAs and a group reduction per order -- a quarter of the kernel's vector
// instructions, and the kernel is vector-issue bound.  Its rounding differs from the direct sums' by ~eps / (1 - mu^2)
// per order (relative; the errors carried so far grow by (1 + mu^2) / (1 - mu^2) with every order: on 48 kHz speech, 1 - mu_1^2 ~ 0.02,
// the coefficients end 1.5e-14 .. 2.4e-13 of the row's largest from the long-double recursion, where the directly summed forms end
// 2e-16 .. 5e-16: tests/test_gpu_accuracy.py), so it is used only while that stays far inside the 1e-6 coefficient tolerance: after an order with
// 1 - mu^2 < 2^-20, or once den' has fallen below 2^-24 of the first order's den (absolute errors ~eps * den_1 would show),
// the next order sums directly again.  The status test `den <= 0` (:123-125) can only fire on a directly summed
// denominator: a recursion value that small has already handed over to the direct sums.  Only the one-frame-per-wavefront
// form (G = 64: frames of more than 1024 samples) does this: there the choice is a scalar branch that depends on the frame
// alone (a frame's result must not depend on which frames share its wavefront), and that is where it pays (measured:
// Burg at N = 1200 23.4 -> 19.5 ms per 4.5 M frames; at N = 512 with four frames per wavefront the permutes cost what the
// FMAs save).
#include "vbx_burg_direct.hpp"

namespace vbx {

bool burg_supported(int n, int p) {
    return n >= 2 && n <= 64 * 64 && p >= 1 && p <= VBX_MAX_LPC_ORDER_K;
}

void launch_burg(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                 int p, double *out, int32_t *status, frame_map_t map) {
    launch_burg_t<double>(s, x, F, n, stride, window, p, out, status, map);
}
void launch_burg_pcm16(hipStream_t s, const int16_t *x, long F, int n, long stride, const double *window,
                       int p, double *out, int32_t *status, frame_map_t map) {
    dim3 b(64);
    const long items = frame_map_items(map, F);
#define VBX_BURG16(GG, E)                                                                                                  \
    hipLaunchKernelGGL((burg_kernel<GG, E, double, int16_t>), dim3((unsigned)((items + (64 / GG) - 1) / (64 / GG))), b, 0, s, \
                       x, F, n, stride, window, p, out, status, map)
    const bool g16 = burg_small_groups_ok(p);
    if (g16 && n <= 16 * 32) VBX_BURG16(16, 32);
    else if (n <= 32 * 32 && burg_half_wave_ok(p)) VBX_BURG16(32, 32);
    else if (n <= 64 * 20) VBX_BURG16(64, 20);
    else if (n <= 64 * 32) VBX_BURG16(64, 32);
    else VBX_BURG16(64, 64);
#undef VBX_BURG16
}
void launch_burg_list(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                      int p, double *out, int32_t *status, const int32_t *list, const int32_t *count) {
    launch_burg_list_t<double>(s, x, F, n, stride, window, p, out, status, list, count);
}
void launch_burg_pcm16_list(hipStream_t s, const int16_t *x, long F, int n, long stride, const double *window,
                            int p, double *out, int32_t *status, const int32_t *list, const int32_t *count) {
    launch_burg_list_t<int16_t>(s, x, F, n, stride, window, p, out, status, list, count);
}

void launch_burg_f32(hipStream_t s, const float *x, long F, int n, long stride, const float *window,
                     int p, float *out, int32_t *status) {
    launch_burg_t<float>(s, x, F, n, stride, window, p, out, status, frame_map_t{0, 0, 0});
}

}  // namespace vbx
