// vbx_api_boersma.hip -- vbx_pitch_boersma_f64 (k_pitch_boersma.hip): the argument checks, the lag-window table and the launch.
#include "vbx_ctx.hpp"
#include "vbx_pitch_boersma.hpp"

#include <cmath>
#include <string>

using namespace vbx;

extern "C" {

int vbx_pitch_boersma_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                          const double *window, double sample_rate, double threshold, double fmin, double fmax,
                          size_t kmax, vbx_pitch *out_cand, int32_t *out_count, int32_t *status) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    // every rule is checked before anything is written, an empty batch included
    VBX_REQUIRE(ctx, frame_len >= (size_t)BOERSMA_MIN_FRAME && frame_len <= (size_t)BOERSMA_MAX_FRAME, "frame_len must be in [16, 4096]");
    VBX_REQUIRE(ctx, kmax >= 1 && kmax <= (size_t)BOERSMA_MAX_KMAX, "kmax must be in [1, 63] (the pitch path's cap)");
    VBX_REQUIRE(ctx, std::isfinite(sample_rate) && sample_rate > 0.0, "sample_rate must be finite and > 0");
    VBX_REQUIRE(ctx, fmin < fmax, "fmin must be below fmax");
    VBX_REQUIRE(ctx, n_frames == 0 || (out_cand != nullptr && out_count != nullptr), "null output");
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, (size_t)BOERSMA_MAX_FRAME);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const double *lagw = nullptr; bool lag_rcp = false;
    VBX_HIP(ctx, ctx->tables.window(VBX_WINDOW_HANNING_LAG, frame_len, &lagw, &lag_rcp));
    {
        Prof p(ctx, "pitch_boersma", ctx->stream);
        launch_pitch_boersma(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, lagw, sample_rate, threshold,
                             fmin, fmax, (int)kmax, kmax >= 4 ? ctx->boersma_group : 64, (pitch_t *)out_cand, out_count, status);
    }
    return check_launch(ctx, __func__);
}

}  // extern "C"
