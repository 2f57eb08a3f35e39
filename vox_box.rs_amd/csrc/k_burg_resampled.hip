// k_burg_resampled.hip -- Burg LPC (LPC::lpc_praat_mut, src/spectrum.rs:101-146) on the RESAMPLED view of the caller's frames
// (find_formants with resample_ratio != 1.0, src/lib.rs:40-64; vbx_burg_resampled.hpp has the contract): burg_kernel of
// k_burg.hip with the resampled sample as its frame source, at the <G, EPL> the dense path's launchers (launch_burg,
// launch_burg_list) pick for the resampled length m -- and the dispatch of the lag kernels by order.
#include "vbx_burg_resampled_direct.hpp"

namespace vbx {

bool burg_resampled_supported(int n_src, int m, int p) {
    // a source frame in the fast kernels' range; a resampled one of 2 .. 1280 samples: every length the direct kernel takes
    // on its own (no one-pass form below 256 samples or off its orders), and the lag kernels that keep a lane's samples in
    // registers.  Longer resampled frames (the segmented lag kernel, the long-frame kernels) take the dense batch.
    return n_src >= 2 && n_src <= VBX_MAX_FRAME_LEN_K && m >= 2 && m <= BURG_RESAMPLED_MAX_M && p >= 1 && p <= VBX_MAX_LPC_ORDER_K;
}


void launch_burg_resampled(hipStream_t s, const double *x, const int16_t *pcm, long F, int m, long stride, const double *window,
                           resample_src_t rs, int p, double *out, int32_t *status, frame_map_t map) {
    if (pcm) launch_burg_resampled_t<int16_t>(s, pcm, F, m, stride, window, rs, p, out, status, map);
    else launch_burg_resampled_t<double>(s, x, F, m, stride, window, rs, p, out, status, map);
}

void launch_burg_resampled_list(hipStream_t s, const double *x, const int16_t *pcm, long F, int m, long stride, const double *window,
                                resample_src_t rs, int p, double *out, int32_t *status, const int32_t *list, const int32_t *count) {
    if (pcm) launch_burg_resampled_list_t<int16_t>(s, pcm, F, m, stride, window, rs, p, out, status, list, count);
    else launch_burg_resampled_list_t<double>(s, x, F, m, stride, window, rs, p, out, status, list, count);
}

// items [i0, i0 + n_items) of the (mapped) batch: lag sums and edge samples of the resampled frames into the scratch of
// k_burg_fast.hip; launch_burg_recursion runs on it unchanged
void launch_burg_lags_resampled(hipStream_t s, const double *x, const int16_t *pcm, long F, int m, long stride, const double *window,
                                resample_src_t rs, int p, frame_map_t map, long i0, long n_items, void *ws) {
#define VBX_BRS_CALL(PP)                                                                                                         \
    if (pcm) launch_burg_lags_resampled_p<PP, int16_t>(s, pcm, F, m, stride, window, rs, map, i0, n_items, (double *)ws);       \
    else launch_burg_lags_resampled_p<PP, double>(s, x, F, m, stride, window, rs, map, i0, n_items, (double *)ws)
    switch (p) {
        case 8: VBX_BRS_CALL(8); break;
        case 10: VBX_BRS_CALL(10); break;
        case 12: VBX_BRS_CALL(12); break;
        case 13: VBX_BRS_CALL(13); break;
        case 14: VBX_BRS_CALL(14); break;
        case 16: VBX_BRS_CALL(16); break;
        default: break;
    }
#undef VBX_BRS_CALL
}

}  // namespace vbx
