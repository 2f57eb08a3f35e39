// vbx_api_f32.hip -- Sample = f32: the *_f32_wide family and the reference-faithful *_f32 family.
#include "vbx_ctx.hpp"

#include <string>

using namespace vbx;

// ---- Sample = f32, the WIDE forms --------------------------------------------
// The traits are generic over the Sample type (src/periodic.rs:276-289 `T: Sample`, src/spectrum.rs:56 `T: Float`,
// :401-409).  The *_f32_wide entry points take float frames and return float results; samples are widened on load, the
// arithmetic runs in f64 and every result is rounded to f32 once -- more accurate than the reference's own f32 folds and as
// fast as the f64 kernels, but NOT the bits the crate returns at f32.  The reference-faithful forms (every fold in f32, in
// the reference's order) carry the plain *_f32 names, further down; MFCC has only the wide form (its f32 arithmetic lives
// in the un-vendored rustfft).

extern "C" {

int vbx_autocorrelate_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                          size_t stride, const float *window, size_t n_lags, float *out) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, n_lags >= 1 && n_lags <= frame_len, "n_lags must be in [1, frame_len] (the reference panics beyond)");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    if (!fewlags_supported((int)frame_len, (int)n_lags, false) && !ctx->pitch_force_mfma &&
        spectral_plan((int)frame_len) != SPECTRAL_PLAN_NONE && (n_lags >= SPECTRAL_AC_MIN_LAGS || frame_len >= 1024)) {
        // many lags: widen (the windowed product rounded to f32 first), the f64 FFT path, one rounding to f32
        void *wi = nullptr, *wo = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_F32_IN, n_frames * frame_len * sizeof(double), &wi);
        if (rc != VBX_SUCCESS) return rc;
        rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * n_lags * sizeof(double), &wo);
        if (rc != VBX_SUCCESS) return rc;
        { Prof p(ctx, "widen_frames"); launch_widen_frames(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (double *)wi); }
        rc = vbx_autocorrelate_f64(ctx, (const double *)wi, n_frames, frame_len, frame_len, nullptr, n_lags, (double *)wo);
        if (rc != VBX_SUCCESS) return rc;
        { Prof p(ctx, "narrow"); launch_narrow(ctx->stream, (const double *)wo, (long)(n_frames * n_lags), out); }
        return check_launch(ctx, __func__);
    }
    if (fewlags_supported((int)frame_len, (int)n_lags, false)) {
        Prof p(ctx, "autocorr_fewlags_f32");
        launch_autocorr_fewlags_f32(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_lags, 0, out, nullptr);
    } else {
        Prof p(ctx, "autocorr_tiles_f32");
        launch_autocorr_tiles_f32(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_lags, out);
    }
    return check_launch(ctx, __func__);
}

int vbx_normalize_f32(vbx_ctx *ctx, float *data, size_t n_rows, size_t n) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_rows == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, data && n >= 1 && n <= 0x7fffffff && n_rows <= 0x7fffffff, "bad argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "normalize_rows_f32"); launch_normalize_rows_f32(ctx->stream, data, (long)n_rows, (int)n); }
    return check_launch(ctx, __func__);
}

int vbx_lpc_mut_f32_wide(vbx_ctx *ctx, const float *r, size_t n_frames, size_t r_stride, size_t n_coeffs, float *out_ac,
                    float *out_kc) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, r && out_ac, "null argument");
    VBX_REQUIRE(ctx, n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && r_stride >= n_coeffs + 1, "bad order / stride");
    VBX_REQUIRE(ctx, n_frames <= 0x7fffffffull, "too many rows");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "levinson_rows_f32"); launch_levinson_rows_f32(ctx->stream, r, (long)n_frames, (long)r_stride, (int)n_coeffs, out_ac, (long)n_coeffs + 1, out_kc); }
    return check_launch(ctx, __func__);
}

int vbx_autocorr_lpc_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                         size_t stride, const float *window, size_t n_coeffs, int normalize,
                         float *out_r, float *out_lpc) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out_r || out_lpc, "both outputs null");
    VBX_REQUIRE(ctx, n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && n_coeffs + 1 <= frame_len, "bad order");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const int n_lags = (int)n_coeffs + 1;
    hipStream_t st = ctx->stream;
    if (fewlags_supported((int)frame_len, n_lags, out_lpc != nullptr)) {
        Prof p(ctx, "autocorr_lpc_f32", st);
        launch_autocorr_fewlags_f32(st, x, (long)n_frames, (int)frame_len, (long)stride, window, n_lags, normalize, out_r, out_lpc, (long)n_lags);
        return check_launch(ctx, __func__);
    }
    float *r = out_r;
    if (!r) {
        void *w = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * (size_t)n_lags * sizeof(float), &w);
        if (rc != VBX_SUCCESS) return rc;
        r = (float *)w;
    }
    if (fewlags_supported((int)frame_len, n_lags, false)) {
        Prof p(ctx, "autocorr_fewlags_f32", st);
        launch_autocorr_fewlags_f32(st, x, (long)n_frames, (int)frame_len, (long)stride, window, n_lags, 0, r, nullptr);
    } else {
        Prof p(ctx, "autocorr_tiles_f32", st);
        launch_autocorr_tiles_f32(st, x, (long)n_frames, (int)frame_len, (long)stride, window, n_lags, r);
    }
    if (normalize) { Prof p(ctx, "normalize_rows_f32", st); launch_normalize_rows_f32(st, r, (long)n_frames, n_lags); }
    if (out_lpc) { Prof p(ctx, "levinson_rows_f32", st); launch_levinson_rows_f32(st, r, (long)n_frames, n_lags, (int)n_coeffs, out_lpc, (long)n_lags); }
    return check_launch(ctx, __func__);
}

int vbx_lpc_burg_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                     size_t stride, const float *window, size_t n_coeffs, float *out, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, burg_supported((int)frame_len, (int)n_coeffs), "frame_len must be in [2, 4096], order in [1, 62]");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "burg_f32"); launch_burg_f32(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_coeffs, out, status); }
    return check_launch(ctx, __func__);
}

// MFCC is bound by its transforms, not by HBM: the f32 frames are widened into a dense f64 batch (windowed product
// rounded to f32 first) and take the f64 kernels; the coefficients are rounded to f32 on the way out.
int vbx_mfcc_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                 const float *window, size_t num_coeffs, double lo_hz, double hi_hz,
                 double sample_rate, float *out, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr && num_coeffs >= 1, "bad argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    void *wi = nullptr, *wo = nullptr;
    rc = ws_get(ctx, vbx_ctx::WS_F32_IN, n_frames * frame_len * sizeof(double), &wi);
    if (rc != VBX_SUCCESS) return rc;
    rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * num_coeffs * sizeof(double), &wo);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, "widen_frames"); launch_widen_frames(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (double *)wi); }
    rc = run_mfcc(ctx, ctx->stream, (const double *)wi, n_frames, frame_len, frame_len, nullptr, num_coeffs, lo_hz, hi_hz,
                  sample_rate, (double *)wo, num_coeffs, status);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, "narrow"); launch_narrow(ctx->stream, (const double *)wo, (long)(n_frames * num_coeffs), out); }
    return check_launch(ctx, __func__);
}

// Pitched::pitch at S = T = f32 (src/periodic.rs:396-455 is generic over the Sample): the frames are widened (windowed
// product rounded to f32 first), the candidates come from the f64 path and are rounded to f32 once.
int vbx_pitch_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                  const float *window, float sample_rate, float threshold, float fmin, float fmax,
                  size_t kmax, vbx_pitch32 *out_cand, int32_t *out_count, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out_cand != nullptr, "null output");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    void *wi = nullptr, *wo = nullptr;
    rc = ws_get(ctx, vbx_ctx::WS_F32_IN, n_frames * frame_len * sizeof(double), &wi);
    if (rc != VBX_SUCCESS) return rc;
    rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * (kmax ? kmax : 1) * sizeof(vbx_pitch), &wo);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, "widen_frames"); launch_widen_frames(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (double *)wi); }
    rc = run_pitch(ctx, ctx->stream, (const double *)wi, n_frames, frame_len, frame_len, nullptr, (double)sample_rate,
                   (double)threshold, (double)fmin, (double)fmax, kmax, (vbx_pitch *)wo, 2 * kmax, out_count, status);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, "narrow"); launch_narrow(ctx->stream, (const double *)wo, (long)(n_frames * kmax * 2), (float *)out_cand); }
    return check_launch(ctx, __func__);
}


// ---- Sample = f32, reference-faithful (k_f32.hip): every fold in f32 in the reference's order ------------------------

int vbx_autocorrelate_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                          size_t stride, const float *window, size_t n_lags, float *out) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, n_lags >= 1 && n_lags <= frame_len, "n_lags must be in [1, frame_len] (the reference panics beyond)");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "autocorr_f32_exact"); launch_autocorr_f32_exact(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_lags, out); }
    return check_launch(ctx, __func__);
}

int vbx_lpc_mut_f32(vbx_ctx *ctx, const float *r, size_t n_frames, size_t r_stride, size_t n_coeffs, float *out_ac,
                    float *out_kc) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, r && out_ac, "null argument");
    VBX_REQUIRE(ctx, n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && r_stride >= n_coeffs + 1, "bad order / stride");
    VBX_REQUIRE(ctx, n_frames <= 0x7fffffffull, "too many rows");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "levinson_f32_exact"); launch_levinson_f32_exact(ctx->stream, r, (long)n_frames, (long)r_stride, (int)n_coeffs, out_ac, (long)n_coeffs + 1, out_kc); }
    return check_launch(ctx, __func__);
}

int vbx_autocorr_lpc_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                         size_t stride, const float *window, size_t n_coeffs, int normalize,
                         float *out_r, float *out_lpc) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out_r || out_lpc, "both outputs null");
    VBX_REQUIRE(ctx, n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && n_coeffs + 1 <= frame_len, "bad order");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const int n_lags = (int)n_coeffs + 1;
    hipStream_t st = ctx->stream;
    float *r = out_r;
    if (!r) {
        void *w = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * (size_t)n_lags * sizeof(float), &w);
        if (rc != VBX_SUCCESS) return rc;
        r = (float *)w;
    }
    { Prof p(ctx, "autocorr_f32_exact", st); launch_autocorr_f32_exact(st, x, (long)n_frames, (int)frame_len, (long)stride, window, n_lags, r); }
    if (normalize) { Prof p(ctx, "normalize_rows_f32", st); launch_normalize_rows_f32(st, r, (long)n_frames, n_lags); }
    if (out_lpc) { Prof p(ctx, "levinson_f32_exact", st); launch_levinson_f32_exact(st, r, (long)n_frames, n_lags, (int)n_coeffs, out_lpc, (long)n_lags, nullptr); }
    return check_launch(ctx, __func__);
}

int vbx_lpc_burg_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                     size_t stride, const float *window, size_t n_coeffs, float *out, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, burg_supported((int)frame_len, (int)n_coeffs), "frame_len must be in [2, 4096], order in [1, 62]");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    // one lane per frame, b1 / b2 in a context-owned scratch: launches of at most `chunk` frames keep it under 256 MB
    long chunk = (long)((256ull << 20) / (8ull * frame_len)) & ~63L;
    if (chunk < 64) chunk = 64;
    if ((size_t)chunk > n_frames) chunk = (long)((n_frames + 63) & ~(size_t)63);
    void *w = nullptr;
    rc = ws_get(ctx, vbx_ctx::WS_F32_IN, burg_f32_exact_scratch_bytes(chunk, (int)frame_len), &w);
    if (rc != VBX_SUCCESS) return rc;
    batch_count_t batches(ctx, chunk);
    for (long f0 = 0; f0 < (long)n_frames; f0 += chunk) {
        batches.launched();
        const long f1 = (f0 + chunk < (long)n_frames) ? f0 + chunk : (long)n_frames;
        Prof p(ctx, "burg_f32_exact");
        launch_burg_f32_exact(ctx->stream, x, f0, f1, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_coeffs, out, status, (float *)w);
    }
    return check_launch(ctx, __func__);
}

int vbx_pitch_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                  const float *window, float sample_rate, float threshold, float fmin, float fmax,
                  size_t kmax, vbx_pitch32 *out_cand, int32_t *out_count, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out_cand != nullptr, "null output");
    VBX_REQUIRE(ctx, kmax >= 1 && kmax <= VBX_MAX_PITCH_CANDIDATES, "kmax must be in [1, VBX_MAX_PITCH_CANDIDATES]");
    VBX_REQUIRE(ctx, frame_len >= 4, "frame_len must be >= 4");
    VBX_REQUIRE(ctx, pitch_f32_exact_lds_bytes((int)frame_len, (int)kmax) + 16 <= 160 * 1024, "frame does not fit the LDS");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const float *lagw32 = nullptr;
    VBX_HIP(ctx, ctx->tables.lag_window_f32(frame_len, &lagw32));
    void *wo = nullptr;
    rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * kmax * sizeof(vbx_pitch), &wo);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, "pitch_f32_exact");
      launch_pitch_f32_exact(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, lagw32, (double)sample_rate,
                             (double)threshold, (double)fmin, (double)fmax, (int)kmax, (pitch_t *)wo, 2 * (long)kmax, out_count, status); }
    { Prof p(ctx, "narrow"); launch_narrow(ctx->stream, (const double *)wo, (long)(n_frames * kmax * 2), (float *)out_cand); }
    return check_launch(ctx, __func__);
}

}  // extern "C"
