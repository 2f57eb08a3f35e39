// k_burg_lags_f32in.hip -- dispatch of the one-pass Burg lag kernels on FLOAT32 samples by order (k_burg_fast.hip's and
// k_burg_resampled.hip's, for float; the instantiations live in k_burg_lags_f32in_a.hip / _b.hip; launch_burg_recursion runs
// behind either unchanged)
#include "vbx_burg_resampled.hpp"

namespace vbx {

// false: no instantiation at this order, NOTHING was launched (the caller fails the call: burg_fast_supported's list of orders,
// k_burg_fast.hip, and this one have drifted apart, and the recursion behind would read scratch that no kernel wrote)
#define VBX_BF32_DISPATCH(CALL)                                   \
    switch (p) {                                                  \
        case 8: CALL(8); return true;                             \
        case 10: CALL(10); return true;                           \
        case 12: CALL(12); return true;                           \
        case 13: CALL(13); return true;                           \
        case 14: CALL(14); return true;                           \
        case 16: CALL(16); return true;                           \
        default: return false;                                    \
    }

bool launch_burg_lags_f32in(hipStream_t s, const float *x, long F, int n, long stride, const double *window, int p,
                            frame_map_t map, long i0, long m, void *ws) {
#define VBX_BF_CALL(PP) launch_burg_lags_p<PP, float>(s, x, F, n, stride, window, map, i0, m, (double *)ws)
    VBX_BF32_DISPATCH(VBX_BF_CALL)
#undef VBX_BF_CALL
}
bool launch_burg_lags_resampled_f32in(hipStream_t s, const float *x, long F, int m, long stride, const double *window,
                                      resample_src_t rs, int p, frame_map_t map, long i0, long n_items, void *ws) {
#define VBX_BF_CALL(PP) launch_burg_lags_resampled_p<PP, float>(s, x, F, m, stride, window, rs, map, i0, n_items, (double *)ws)
    VBX_BF32_DISPATCH(VBX_BF_CALL)
#undef VBX_BF_CALL
}

// ---- frames of any sample type: the form of x.kind; false as above, whatever the type ------------------------------------------
static bool lag_order(int p) { return p == 8 || p == 10 || p == 12 || p == 13 || p == 14 || p == 16; }

bool launch_burg_lags(hipStream_t s, frames_t x, long F, int n, long stride, const double *window, int p, frame_map_t map, long i0,
                      long m, void *ws) {
    if (!lag_order(p)) return false;
    switch (x.kind) {
        case SAMPLE_F64: launch_burg_lags(s, x.f64(), F, n, stride, window, p, map, i0, m, ws); break;
        case SAMPLE_PCM16: launch_burg_lags_pcm16(s, x.pcm16(), F, n, stride, window, p, map, i0, m, ws); break;
        case SAMPLE_F32: return launch_burg_lags_f32in(s, x.f32in(), F, n, stride, window, p, map, i0, m, ws);
    }
    return true;
}
bool launch_burg_lags_resampled(hipStream_t s, frames_t x, long F, int m, long stride, const double *window, resample_src_t rs, int p,
                                frame_map_t map, long i0, long n_items, void *ws) {
    if (!lag_order(p)) return false;
    if (x.kind == SAMPLE_F32) return launch_burg_lags_resampled_f32in(s, x.f32in(), F, m, stride, window, rs, p, map, i0, n_items, ws);
    launch_burg_lags_resampled(s, x.f64(), x.pcm16(), F, m, stride, window, rs, p, map, i0, n_items, ws);
    return true;
}

}  // namespace vbx
