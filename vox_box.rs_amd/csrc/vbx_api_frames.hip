// vbx_api_frames.hip -- the user's frame loop, batched and fused, and its typed entry points.
#include "vbx_ctx.hpp"

#include <cmath>
#include <string>
#include <vector>

using namespace vbx;

// ---- the user's frame loop, batched and fused ------------------------------------------------------------------

namespace vbx {

static int ensure_side_stream(vbx_ctx *ctx) {
    if (ctx->side) return VBX_SUCCESS;
    VBX_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    VBX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    VBX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    VBX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_peak, hipEventDisableTiming));
    for (auto &e : ctx->ev_bf_launch) VBX_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : ctx->ev_bf_free) VBX_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return VBX_SUCCESS;
}

// vbx_analyze_frames_tracked_*: columns 0-1 of the records are the pitch path over the call's own kmax-entry lists
// (defer_path: the lists, counts and peaks only -- vbx_analyze_host runs ONE path over the whole recording behind its last chunk)
struct track_req_t { size_t kmax; vbx_pitch_path_params path; vbx_pitch_track_outputs out; bool defer_path; };
// vbx_analyze_frames_ex_*: find_formants on the frames' resampled view (rp non-null) at formant_rate, and the RMS column
struct ex_req_t { const resample_plan_t *rp; double formant_rate; bool rms; };

// own: the caller's frames, as f64, 16-bit PCM or float32 samples.  PCM and float32 are read directly where EVERY kernel that goes over
// the samples has a form for them (full 1200-sample frames through the fused spectral kernel with nothing beside it but Burg, which
// has one at every length); every other shape takes one widening pass into a context-owned f64 copy of the view and the f64 path.
static int analyze_frames_impl(vbx_ctx *ctx, const char *fn, frames_t own, size_t n_frames, size_t frame_len,
                               size_t stride, const vbx_analysis_params *h_p, const int64_t *h_seg_start, size_t n_segments,
                               double *out_records, size_t record_ld, int32_t *status3, const track_req_t *tk = nullptr,
                               const ex_req_t *ex = nullptr) {
    int rc = check_frames(ctx, fn, own.p, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc == 1 && tk) { ctx->path_redone = nullptr; ctx->path_last = true; }      // an empty batch: an empty path
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, h_p && out_records, "null argument");
    const size_t c_rms = vbx_record_doubles(h_p), rec = c_rms + ((ex && ex->rms) ? 1 : 0);     // RMS: the record's last column
    VBX_REQUIRE(ctx, record_ld >= rec && record_ld % 2 == 0, "record_ld must be even and >= vbx_record_doubles(params)");
    VBX_REQUIRE(ctx, ((uintptr_t)out_records & 15) == 0, "records must be 16-byte aligned");
    VBX_REQUIRE(ctx, !h_p->formant_order || (h_p->n_est >= 1 && h_p->n_est <= VBX_FORMANT_SLOTS), "n_est must be in [1, 6]");
    if (tk || ex) {
        // The tracked form writes its peaks before the parts below look at their own arguments: what they would reject is asked first,
        // through the predicates those parts use themselves.  (The unfused MFCC kernels choose their form from the geometry: the tracked
        // form queues them FIRST on the side stream, below, so that their rejection also precedes every write.)
        if (const char *e = pitch_shape_error(frame_len, tk ? tk->kmax : 1)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": " + e);
        VBX_REQUIRE(ctx, !h_p->formant_order || burg_order_ok((ex && ex->rp) ? ex->rp->m : frame_len, h_p->formant_order), "frame_len must be >= 2, order in [1, 62]");
        VBX_REQUIRE(ctx, !h_p->lpc_order || lpc_order_ok(frame_len, h_p->lpc_order), "bad order");
    }
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    rc = ensure_side_stream(ctx);
    if (rc != VBX_SUCCESS) return rc;
    // One spectral pass for pitch + LPC + MFCC when the shape has a fused kernel (k_spectral.hip); otherwise the LPC
    // and MFCC kernels run on the side stream and the pitch kernel alone on the main one.
    std::vector<int32_t> hb; bool bad_bins = false; const int32_t *d_bins = nullptr;
    const double *dct = nullptr, *slopes = nullptr;
    int nb = 0;
    if (h_p->mfcc_coeffs) {
        VBX_REQUIRE(ctx, h_p->mfcc_coeffs <= 64, "mfcc_coeffs must be in [0, 64]");
        rc = get_bins_dev(ctx, frame_len, h_p->mfcc_coeffs, h_p->mfcc_lo_hz, h_p->mfcc_hi_hz, h_p->sample_rate, &d_bins, hb, bad_bins);
        if (rc != VBX_SUCCESS) return rc;
        nb = hb.back() - hb.front();
    }
    // (MFCC joins the fused kernel when the frame's length divides the transform's: n = 512, 600, 800, 1024, 1200, 2048, 4096 -- and, since
    // round 5, at every other length by interpolated bins, below; LPC only at the order the kernel's register Levinson is built for -- what
    // cannot join runs from its own kernel on the side stream)
    const bool fused = !ctx->pitch_force_mfma && spectral_supported((int)frame_len, 0, 0, 0, 0);
    const bool fused_lpc = fused && h_p->lpc_order == SPECTRAL_LPC_ORDER;
    // the transform: the one its length asks for, or -- if MFCC can join only there -- the one whose length the frame divides
    int plan = fused ? spectral_plan((int)frame_len) : SPECTRAL_PLAN_NONE;
    if (fused && !bad_bins && h_p->mfcc_coeffs) {
        const int pm = spectral_plan_mfcc((int)frame_len);
        if (spectral_supported_plan(pm, (int)frame_len, 0, nb, hb.front(), (int)h_p->mfcc_coeffs)) plan = pm;
    }
    bool fused_mfcc = fused && !bad_bins && h_p->mfcc_coeffs &&
                      spectral_supported_plan(plan, (int)frame_len, 0, nb, hb.front(), (int)h_p->mfcc_coeffs);
    // ... and at the other lengths by interpolating the frame's DFT bins from the transform's (mfcc_interp_t)
    bool interp_mfcc = false;
    mfcc_interp_t ip{};
    if (fused && !fused_mfcc && !bad_bins && h_p->mfcc_coeffs && ctx->mfcc_interp != 0 && plan != SPECTRAL_PLAN_NONE && nb >= 1 && nb <= 4096 && hb.front() >= 0) {
        VBX_HIP(ctx, ctx->tables.interp(plan, (int)frame_len, hb.front(), nb, &ip, &interp_mfcc));
        fused_mfcc = interp_mfcc;
    }
    // x: what the kernels read -- the caller's own samples, or their widened copy (the RMS and peak kernels read `own` either way)
    frames_t x = own;
    const bool native = fused && frame_len == (size_t)SPECTRAL_N && (!h_p->lpc_order || fused_lpc) && (!h_p->mfcc_coeffs || fused_mfcc) &&
                        !(ex && ex->rp && !ex->rp->direct);                // (the dense fallback resamples f64 frames)
    if (own.kind != SAMPLE_F64 && !native) {
        const size_t ns = (n_frames - 1) * stride + frame_len;
        void *w = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_F32_IN, ns * sizeof(double), &w);
        if (rc != VBX_SUCCESS) return rc;
        if (own.kind == SAMPLE_PCM16) { Prof p(ctx, "pcm16"); launch_pcm16(ctx->stream, own.pcm16(), ns, 32767.0, (double *)w); }
        else { Prof p(ctx, "f32_to_f64"); launch_f32_to_f64(ctx->stream, own.f32in(), ns, (double *)w); }
        x = (const double *)w;
    }
    const double *hann = nullptr;
    VBX_HIP(ctx, ctx->tables.window(VBX_WINDOW_HANNING, frame_len, &hann));        // Windower::hanning frames (examples/pitch_detection.rs:23)
    // record columns
    const size_t c_form = 2, c_mfcc = c_form + (h_p->formant_order ? 2 * h_p->n_est : 0),
                 c_lpc = c_mfcc + h_p->mfcc_coeffs;
    int32_t *st_pitch = nullptr, *st_form = nullptr, *st_mfcc = nullptr;
    if (status3) { st_pitch = status3; st_form = status3 + n_frames; st_mfcc = status3 + 2 * n_frames; }
    // the tracked form: the lists, counts and peaks the path reads -- the caller's arrays, or context-owned ones
    vbx_pitch *tk_cand = nullptr; int32_t *tk_count = nullptr; double *tk_peak = nullptr;
    if (tk) {
        tk_cand = tk->out.cand; tk_count = tk->out.count;
        const bool need_peak = tk->path.silence_threshold != 0.0 || tk->out.peak != nullptr;
        tk_peak = need_peak ? tk->out.peak : nullptr;
        const size_t b_cand = tk_cand ? 0 : n_frames * tk->kmax * sizeof(vbx_pitch), b_peak = (need_peak && !tk_peak) ? n_frames * sizeof(double) : 0,
                     b_count = tk_count ? 0 : n_frames * sizeof(int32_t), b_st = st_pitch ? 0 : n_frames * sizeof(int32_t);
        if (b_cand + b_peak + b_count + b_st) {
            void *w = nullptr;
            rc = ws_get(ctx, vbx_ctx::WS_TRACK, b_cand + b_peak + b_count + b_st, &w);
            if (rc != VBX_SUCCESS) return rc;
            char *q = static_cast<char *>(w);
            if (b_cand) { tk_cand = reinterpret_cast<vbx_pitch *>(q); q += b_cand; }
            if (b_peak) { tk_peak = reinterpret_cast<double *>(q); q += b_peak; }
            if (b_count) { tk_count = reinterpret_cast<int32_t *>(q); q += b_count; }
            if (b_st) st_pitch = reinterpret_cast<int32_t *>(q);              // (the path must see the frames the pitch kernel gave up on)
        }
    }
    // fork: the formant chain (Burg -> roots -> the latency-bound tracker scan) and the MFCC run on the side stream,
    // beside the FP64-bound pitch kernel
    VBX_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    // (frames longer than VBX_MAX_FRAME_LEN: everything in order on the context's stream -- the long-frame kernels share one scratch)
    hipStream_t side = frame_len > VBX_MAX_FRAME_LEN ? ctx->stream : ctx->side;
    VBX_HIP(ctx, hipStreamWaitEvent(side, ctx->ev_fork, 0));
    const bool mfcc_beside = h_p->mfcc_coeffs && !fused_mfcc;              // MFCC from its own kernel on the side stream
    if (tk && mfcc_beside) {                                               // (tracked: first, see above; its columns are nobody else's)
        rc = run_mfcc(ctx, side, x.f64(), n_frames, frame_len, stride, hann, h_p->mfcc_coeffs, h_p->mfcc_lo_hz, h_p->mfcc_hi_hz,
                      h_p->sample_rate, out_records + c_mfcc, record_ld, st_mfcc);
        if (rc != VBX_SUCCESS) return rc;
    }
    // RMS::rms of the rectangular frame (examples/formant_extraction/src/main.rs:84), from the caller's own samples -- a PCM
    // recording is never widened for it.  A tracked call that needs the frame peaks takes both from one read, here; otherwise
    // the RMS kernel is the side stream's LAST launch, behind everything that may still reject the call.
    const bool want_rms = ex && ex->rms;
    if (tk_peak && want_rms) {
        { Prof p(ctx, "frame_rms_peak", side);
          launch_frame_rms(side, own, (long)n_frames, (int)frame_len, (long)stride, out_records + c_rms, (long)record_ld, tk_peak); }
        VBX_HIP(ctx, hipEventRecord(ctx->ev_peak, side));
    } else if (tk_peak) {
        // max |x| per frame, first on the side stream: HBM-bound, beside the FP64-bound kernel; the path waits for ev_peak
        static const char *const k_peak_names[3] = {"frame_peak", "frame_peak_pcm16", "frame_peak_f32in"};      // by sample_kind_t
        { Prof p(ctx, k_peak_names[own.kind], side); launch_frame_peak(side, own, (long)n_frames, (long)frame_len, (long)stride, tk_peak); }
        VBX_HIP(ctx, hipEventRecord(ctx->ev_peak, side));
    }
    // Burg's lag sums from the analyze kernel's own wavefronts instead of a second pass over the audio (analyze_kernel<.., BURG>): large
    // calls of full 1200-sample f64 / PCM frames with find_formants at order 12 on the same frames.  The formant chain then runs behind
    // the analyze kernel launch by launch (below, at the launch); the launch itself has the last word (spectral_burg_fusable_call).
    const bool burg_fused_shape = ctx->burg_fused && fused && h_p->formant_order == (size_t)SPECTRAL_BURG_ORDER && frame_len == (size_t)SPECTRAL_N &&
                                  x.p == own.p && (own.kind == SAMPLE_F64 || own.kind == SAMPLE_PCM16) && !(ex && ex->rp) &&
                                  (long)n_frames >= ctx->burg_fused_min_frames && burg_fast_supported((int)frame_len, SPECTRAL_BURG_ORDER) &&
                                  formant_resonances_fast_supported(SPECTRAL_BURG_ORDER);
    auto formants_beside = [&]() -> int {
        vbx_resonance est[VBX_FORMANT_SLOTS];
        for (size_t e = 0; e < h_p->n_est; e++) est[e] = h_p->est_init[e];
        return run_find_formants(ctx, side, x, n_frames, frame_len, stride, ex ? ex->formant_rate : h_p->sample_rate, h_p->formant_order,
                                 h_seg_start, n_segments, est, h_p->n_est, (vbx_resonance *)(out_records + c_form), record_ld,
                                 nullptr, nullptr, nullptr, st_form, ex ? ex->rp : nullptr);
    };
    if (burg_fused_shape) {
        // (decided at the launch, below: every other side-stream kernel of such a call precedes the formant chain either way)
    } else if (h_p->formant_order) {
        rc = formants_beside();
        if (rc != VBX_SUCCESS) return rc;
    } else {
        ctx->last_track.res = nullptr;                        // no tracks in these records: nothing for vbx_track_stitch_f64 to continue
        ctx->last_track.n_est = 0;                            // ... and no row for a communicator to send on
        if (st_form) VBX_HIP(ctx, hipMemsetAsync(st_form, 0, n_frames * sizeof(int32_t), side));
    }
    // (what runs beside the spectral kernel reads f64: `native` is false wherever one of these runs)
    if (h_p->lpc_order && !fused_lpc) {
        rc = run_autocorr_lpc(ctx, side, x.f64(), n_frames, frame_len, stride, hann, h_p->lpc_order, 0, nullptr,
                              out_records + c_lpc, record_ld);
        if (rc != VBX_SUCCESS) return rc;
    }
    if (mfcc_beside && !tk) {
        rc = run_mfcc(ctx, side, x.f64(), n_frames, frame_len, stride, hann, h_p->mfcc_coeffs, h_p->mfcc_lo_hz, h_p->mfcc_hi_hz,
                      h_p->sample_rate, out_records + c_mfcc, record_ld, st_mfcc);
        if (rc != VBX_SUCCESS) return rc;
    }
    if (!h_p->mfcc_coeffs && st_mfcc) VBX_HIP(ctx, hipMemsetAsync(st_mfcc, 0, n_frames * sizeof(int32_t), side));
    if (want_rms && !tk_peak) {
        Prof p(ctx, "frame_rms", side);
        launch_frame_rms(side, own, (long)n_frames, (int)frame_len, (long)stride, out_records + c_rms, (long)record_ld, nullptr);
    }
    if (!burg_fused_shape) VBX_HIP(ctx, hipEventRecord(ctx->ev_join, side));
    if (fused) {
        const double *lagw = nullptr, *tab = nullptr; bool lag_rcp = false;
        VBX_HIP(ctx, ctx->tables.window(VBX_WINDOW_HANNING_LAG, frame_len, &lagw, &lag_rcp));
        VBX_HIP(ctx, ctx->tables.spectral(plan, &tab));
        if (fused_mfcc) {
            VBX_HIP(ctx, ctx->tables.dct(h_p->mfcc_coeffs, &dct));
            VBX_HIP(ctx, ctx->tables.slopes(frame_len, h_p->mfcc_coeffs, h_p->mfcc_lo_hz, h_p->mfcc_hi_hz, h_p->sample_rate, hb, &slopes));
        }
        if (ctx->prof && !ctx->pitch_work) {
            const size_t wb = PITCH_WORK_WORDS * sizeof(unsigned long long);
            VBX_HIP(ctx, hipMalloc((void **)&ctx->pitch_work, wb));
            VBX_HIP(ctx, hipMemsetAsync(ctx->pitch_work, 0, wb, ctx->stream));
        }
        spectral_launch_t L{};
        L.plan = plan; L.n = (int)frame_len;
        L.x = x; L.F = (long)n_frames; L.stride = (long)stride; L.window = hann; L.lag_window = lagw; L.tab = tab;
        L.lag_rcp = lag_rcp;
        L.sample_rate = h_p->sample_rate; L.threshold = h_p->pitch_threshold; L.fmin = h_p->pitch_fmin; L.fmax = h_p->pitch_fmax;
        L.kmax = 1;
        L.whole_curve = ctx->pitch_whole_curve;
        L.out_cand = (pitch_t *)out_records; L.cand_ld = (long)record_ld; L.out_count = nullptr; L.pitch_status = st_pitch;
        if (tk) { L.kmax = (int)tk->kmax; L.out_cand = (pitch_t *)tk_cand; L.cand_ld = 2 * (long)tk->kmax; L.out_count = tk_count; }
        L.work = ctx->prof ? ctx->pitch_work : nullptr;
        if (fused_lpc) { L.out_lpc = out_records + c_lpc; L.lpc_ld = (long)record_ld; }
        if (fused_mfcc) {
            L.out_mfcc = out_records + c_mfcc; L.mfcc_ld = (long)record_ld; L.mfcc_status = st_mfcc;
            L.bins = d_bins; L.slopes = slopes; L.dct = dct; L.num_coeffs = (int)h_p->mfcc_coeffs; L.nb = nb;
            L.interp = interp_mfcc; L.ip = ip;
        }
        if (burg_fused_shape && spectral_burg_fusable_call(ctx, L)) {
            formants_ranges_t R{};
            vbx_resonance est[VBX_FORMANT_SLOTS];
            for (size_t e = 0; e < h_p->n_est; e++) est[e] = h_p->est_init[e];
            rc = find_formants_ranges_begin(ctx, side, x, n_frames, stride, ex ? ex->formant_rate : h_p->sample_rate, h_p->formant_order, h_seg_start,
                                            n_segments, est, h_p->n_est, (vbx_resonance *)(out_records + c_form), record_ld, st_form,
                                            ctx->analyze_launch_frames, &R);
            if (rc != VBX_SUCCESS) return rc;
            analyze_ranges_t rg;
            rg.launch_frames = ctx->analyze_launch_frames < (long)n_frames ? ctx->analyze_launch_frames : (long)n_frames;
            rg.scratch[0] = R.scratch[0]; rg.scratch[1] = R.scratch[1]; rg.burg_window = R.hann;
            // launch j + 2 writes the scratch launch j wrote: behind the recursion that reads it
            rg.before = [&](int j) -> int {
                if (j >= 2) VBX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_bf_free[j & 1], 0));
                return VBX_SUCCESS;
            };
            // ... and the side stream takes launch j's frames from there, beside launch j + 1
            rg.after = [&](int j, long f0, long nf) -> int {
                VBX_HIP(ctx, hipEventRecord(ctx->ev_bf_launch[j & 1], ctx->stream));
                VBX_HIP(ctx, hipStreamWaitEvent(side, ctx->ev_bf_launch[j & 1], 0));
                return find_formants_ranges_step(ctx, &R, j, f0, nf);
            };
            rc = launch_spectral(ctx, ctx->stream, L, "analyze", &rg);
            if (rc != VBX_SUCCESS) return rc;
            rc = find_formants_ranges_end(ctx, &R);
            if (rc != VBX_SUCCESS) return rc;
            VBX_HIP(ctx, hipEventRecord(ctx->ev_join, side));
        } else {
            if (burg_fused_shape) {                           // the launch takes another instance after all: the chain beside it, as for every other call
                rc = formants_beside();
                if (rc != VBX_SUCCESS) return rc;
                VBX_HIP(ctx, hipEventRecord(ctx->ev_join, side));
            }
            rc = launch_spectral(ctx, ctx->stream, L, "analyze");
        }
    } else if (tk) {
        rc = run_pitch(ctx, ctx->stream, x.f64(), n_frames, frame_len, stride, hann, h_p->sample_rate, h_p->pitch_threshold,
                       h_p->pitch_fmin, h_p->pitch_fmax, tk->kmax, tk_cand, 2 * tk->kmax, tk_count, st_pitch);
    } else {
        rc = run_pitch(ctx, ctx->stream, x.f64(), n_frames, frame_len, stride, hann, h_p->sample_rate, h_p->pitch_threshold,
                       h_p->pitch_fmin, h_p->pitch_fmax, 1, (vbx_pitch *)out_records, record_ld, nullptr, st_pitch);
    }
    if (rc != VBX_SUCCESS) return rc;
    if (tk && !tk->defer_path) {
        // the path over those lists, on the context's stream behind the kernel that wrote them: its rows are columns 0-1 of the records
        if (tk_peak) VBX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_peak, 0));
        rc = run_pitch_path(ctx, ctx->stream, tk_cand, tk_count, st_pitch, n_frames, tk->kmax, tk_peak, h_seg_start, n_segments, tk->path,
                            (vbx_pitch *)out_records, record_ld, tk->out.index, fn);
        if (rc != VBX_SUCCESS) return rc;
    }
    VBX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));       // join: the records are complete on ctx's stream
    return VBX_SUCCESS;
}

// find_formants' resample_ratio (src/lib.rs:40-64) as a plan: the checks every entry point that takes a ratio shares, the
// resampled length, the context's (li, frac) table and whether the resampled loaders take the shape.  *have = false: no
// resampling (ratio 0 or 1.0: src/lib.rs:57 compares with 1.0).
int make_resample_plan(vbx_ctx *ctx, const char *fn, double ratio, size_t frame_len, size_t order, resample_plan_t *rp, bool *have) {
    *have = false;
    if (!(ratio >= 0.0) || !std::isfinite(ratio)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": resample_ratio must be finite and >= 0");
    if (ratio == 0.0 || ratio == 1.0) return VBX_SUCCESS;
    if (ratio > 64.0) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": resample_ratio must be in (0, 64]");
    if (order == 0) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": a resample_ratio needs a formant order");
    const size_t m = vbx_resampled_len(frame_len, ratio);
    if (m > 0x3fffffff) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad resampled length");
    if (!burg_order_ok(m, order)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": the resampled frame must have >= 2 samples, order in [1, 62]");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    rp->n_src = frame_len; rp->m = m; rp->rs.n_src = (int)frame_len;
    VBX_HIP(ctx, ctx->tables.resample(frame_len, ratio, m, &rp->rs.li, &rp->rs.frac));
    rp->direct = frame_len <= VBX_MAX_FRAME_LEN && burg_resampled_supported((int)frame_len, (int)m, (int)order);
    *have = true;
    return VBX_SUCCESS;
}

// The frame loop of examples/formant_extraction/src/main.rs:72-88: find_formants at a resample_ratio, the frame's RMS as the
// record's last column.  Everything is checked before anything is launched; an h_ext that asks for nothing is the plain /
// tracked call itself.
int analyze_ex(vbx_ctx *ctx, const char *fn, frames_t x, size_t n_frames, size_t frame_len, size_t stride,
               const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
               const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld, int32_t *status3,
               const vbx_pitch_track_outputs *h_out, bool defer_path /* vbx_analyze_host's chunks: track_req_t */) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null context");
    if (!h_p) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": null argument");
    resample_plan_t rp{}; ex_req_t ex{nullptr, h_p->sample_rate, false};
    const ex_req_t *exp = nullptr;
    if (h_ext) {
        const double ratio = h_ext->formant_resample_ratio, rate = h_ext->formant_sample_rate;
        if (!(rate >= 0.0) || !std::isfinite(rate)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": formant_sample_rate must be finite and >= 0");
        bool have = false;
        if (n_frames != 0 && frame_len >= 1 && frame_len <= VBX_MAX_LONG_FRAME_LEN) {      // (any other frame_len is rejected below)
            int rc = make_resample_plan(ctx, fn, ratio, frame_len, h_p->formant_order, &rp, &have);
            if (rc != VBX_SUCCESS) return rc;
        } else if (!(ratio >= 0.0) || !std::isfinite(ratio) || ratio > 64.0) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": resample_ratio must be in [0, 64]");
        ex.rp = have ? &rp : nullptr;
        ex.formant_rate = rate != 0.0 ? rate : (have ? h_p->sample_rate * ratio : h_p->sample_rate);
        ex.rms = h_ext->rms != 0;
        if (have || ex.rms || rate != 0.0) exp = &ex;
    }
    if (!h_track) return analyze_frames_impl(ctx, fn, x, n_frames, frame_len, stride, h_p, h_seg_start, n_segments, out_records, record_ld,
                                             status3, nullptr, exp);
    track_req_t tk{};
    tk.kmax = h_track->kmax; tk.path = h_track->path;
    if (h_out) tk.out = *h_out;
    tk.defer_path = defer_path;
    if (tk.path.time_step == 0.0) tk.path.time_step = (double)stride / h_p->sample_rate;      // the batch's own hop
    int rc = check_pitch_path(ctx, fn, tk.path, n_frames, tk.kmax, true, h_seg_start, n_segments);
    if (rc != VBX_SUCCESS) return rc;
    return analyze_frames_impl(ctx, fn, x, n_frames, frame_len, stride, h_p, h_seg_start, n_segments, out_records, record_ld, status3, &tk, exp);
}

}  // namespace vbx

extern "C" {

int vbx_analyze_frames_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                           const vbx_analysis_params *h_p, const int64_t *h_seg_start, size_t n_segments,
                           double *out_records, size_t record_ld, int32_t *status3) {
    return analyze_frames_impl(ctx, __func__, x, n_frames, frame_len, stride, h_p, h_seg_start, n_segments, out_records, record_ld, status3);
}

int vbx_analyze_frames_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                             const vbx_analysis_params *h_p, const int64_t *h_seg_start, size_t n_segments,
                             double *out_records, size_t record_ld, int32_t *status3) {
    if (n_frames != 0 && ctx && !pcm) return fail(ctx, VBX_E_INVALID, "vbx_analyze_frames_pcm16: null frame pointer");
    return analyze_frames_impl(ctx, __func__, pcm, n_frames, frame_len, stride, h_p, h_seg_start, n_segments, out_records, record_ld, status3);
}

// The frame loop with the TRACKED contour in columns 0-1 (the fused kernel at the caller's kmax into list buffers, the frame peaks
// beside it, the pitch path behind it): analyze_ex with no extension, behind the two checks that come first here.
int vbx_analyze_frames_tracked_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                                   const vbx_analysis_params *h_p, const vbx_pitch_track_params *h_track,
                                   const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld,
                                   int32_t *status3, const vbx_pitch_track_outputs *h_outputs) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, std::string(__func__) + ": null context");
    if (!h_track) return fail(ctx, VBX_E_INVALID, std::string(__func__) + ": null track parameters");
    return analyze_ex(ctx, __func__, x, n_frames, frame_len, stride, h_p, nullptr, h_track, h_seg_start, n_segments, out_records,
                      record_ld, status3, h_outputs);
}

int vbx_analyze_frames_tracked_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                                     const vbx_analysis_params *h_p, const vbx_pitch_track_params *h_track,
                                     const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld,
                                     int32_t *status3, const vbx_pitch_track_outputs *h_outputs) {
    if (n_frames != 0 && ctx && !pcm) return fail(ctx, VBX_E_INVALID, "vbx_analyze_frames_tracked_pcm16: null frame pointer");
    if (!ctx) return fail(nullptr, VBX_E_INVALID, std::string(__func__) + ": null context");
    if (!h_track) return fail(ctx, VBX_E_INVALID, std::string(__func__) + ": null track parameters");
    return analyze_ex(ctx, __func__, pcm, n_frames, frame_len, stride, h_p, nullptr, h_track, h_seg_start, n_segments, out_records,
                      record_ld, status3, h_outputs);
}

int vbx_analyze_frames_ex_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                              const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                              const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld,
                              int32_t *status3, const vbx_pitch_track_outputs *h_outputs) {
    return analyze_ex(ctx, __func__, x, n_frames, frame_len, stride, h_p, h_ext, h_track, h_seg_start, n_segments, out_records,
                      record_ld, status3, h_outputs);
}

int vbx_analyze_frames_ex_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                                const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                                const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld,
                                int32_t *status3, const vbx_pitch_track_outputs *h_outputs) {
    if (n_frames != 0 && ctx && !pcm) return fail(ctx, VBX_E_INVALID, "vbx_analyze_frames_ex_pcm16: null frame pointer");
    return analyze_ex(ctx, __func__, pcm, n_frames, frame_len, stride, h_p, h_ext, h_track, h_seg_start, n_segments, out_records,
                      record_ld, status3, h_outputs);
}

int vbx_analyze_frames_ex_f32in(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                                const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                                const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld,
                                int32_t *status3, const vbx_pitch_track_outputs *h_outputs) {
    if (n_frames != 0 && ctx && !x) return fail(ctx, VBX_E_INVALID, "vbx_analyze_frames_ex_f32in: null frame pointer");
    return analyze_ex(ctx, __func__, x, n_frames, frame_len, stride, h_p, h_ext, h_track, h_seg_start, n_segments, out_records,
                      record_ld, status3, h_outputs);
}

}  // extern "C"
