// vbx_live.hpp -- what the live families -- the one-channel and the multi-channel session (vbx_api_session.hip), the session pool
// (vbx_api_pool.hip) -- do identically around their own kernels, launches, tables and open-time checks (vbx_api_live.hip): the frame-loop
// call and its chunk-local buffers, the warm-up at open, a push's output checks, a deliver descriptor's source half, the staging ring.
#pragma once

#include "vbx_ctx.hpp"

namespace vbx {

// a failed HIP call while a family's object is being built: behind the queued work, `release` it, report the call
#define LIVE_HIP(ctx, expr, release) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { hipStreamSynchronize((ctx)->stream); release; \
        return vbx::fail(ctx, VBX_E_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)

// what a frame-loop call of a live family runs with, and what it writes before the caller's arrays: the chunk-local records / status
// rows / lists of the largest call and the state rows (2 * VBX_FORMANT_SLOTS doubles each: the formant row of a stream's last frame
// delivered).  The frame loop's own workspaces are the context's.
struct live_core_t {
    vbx_ctx *ctx = nullptr;
    int fmt = 0;
    size_t frame_len = 0, stride = 0;
    vbx_analysis_params p{}; vbx_analysis_ext ext{}; vbx_pitch_track_params track{};
    bool have_ext = false, have_track = false;
    size_t rec = 0, ld_c = 0;
    double *c_rec = nullptr; int32_t *c_st = nullptr;
    vbx_pitch *c_cand = nullptr; int32_t *c_count = nullptr; double *c_peak = nullptr;
    double *state = nullptr;
};

// the format, the family's own rule for channels / channel (checked by the caller, refused here in its place), reserved fields
int live_check_audio(vbx_ctx *ctx, const char *fn, const vbx_host_audio *h_fmt, bool channels_ok, const char *channels_msg);
int live_check_n_est(vbx_ctx *ctx, const char *fn, const vbx_analysis_params *h_p);
live_core_t live_make(vbx_ctx *ctx, int fmt, size_t frame_len, size_t stride, const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext,
                      const vbx_pitch_track_params *h_track);
// the path parameters of the tracked form: time_step == 0 means stride / sample_rate
vbx_pitch_path_params live_path_params(const live_core_t &c);
int live_check_path(const live_core_t &c, const char *fn, size_t call_max);
// the chunk-local buffers for calls of up to nbuf frames and state_rows zeroed state rows; a failure frees what it allocated
int live_alloc(live_core_t &c, size_t nbuf, size_t state_rows);
void live_free(live_core_t &c);

// frames [0, n) of `plane` (the format's plane type) into the chunk-local buffers
int live_analyze(const live_core_t &c, const char *fn, const void *plane, size_t n, const int64_t *seg, size_t n_seg, bool want_peak);
// the chunk-local rows are no track of the caller's: nothing to stitch
inline void live_drop_last_track(vbx_ctx *ctx) { ctx->last_track.res = nullptr; ctx->last_track.n_est = 0; }
// ctx->last_track is the track the frame-loop call of n frames just left over the chunk-local records, for a family's own stitch launch
int live_take_last_track(const live_core_t &c, const char *fn, size_t n);

// the largest call a push can make, on zeroed memory: the context's workspaces and tables are as large as they will ever have to be,
// and what only the frame loop's parts know is rejected here.  A failure releases the family's object and reports the call's own text.
template <class Release>
int live_warm_up(const live_core_t &c, const char *fn, const void *plane, size_t n, const int64_t *seg, size_t n_seg, Release release) {
    vbx_ctx *ctx = c.ctx;
    int rc = live_analyze(c, fn, plane, n, seg, n_seg, true);
    if (rc == VBX_SUCCESS) rc = check_launch(ctx, fn);
    live_drop_last_track(ctx);
    if (rc != VBX_SUCCESS) { const std::string why = ctx->last_error; hipStreamSynchronize(ctx->stream); vbx_sync(ctx); release(); return fail(ctx, rc, why); }
    return VBX_SUCCESS;
}

// One set of a push's output arguments; `name`: what the entry point calls the lists' struct ("h_outputs", "outputs").  The checks
// run in this order, those of `which` only; *want_peak is raised when the lists ask for the peaks.
enum : unsigned { LIVE_OUT_RECORDS = 1, LIVE_OUT_ALIGNED = 2, LIVE_OUT_RECORD_LD = 4, LIVE_OUT_STATUS_LD = 8, LIVE_OUT_LISTS = 16, LIVE_OUT_ALL = 31 };
int live_check_outputs(const live_core_t &c, const char *fn, unsigned which, const char *name, const vbx_channel_outputs &o, size_t record_ld,
                       size_t status_ld, size_t rows, const char *status_ld_msg, bool *want_peak);

// the source half of session_deliver_t, session_deliver_all_t or pool_deliver_t: the chunk-local buffers of a call of src_n frames
template <class D>
void live_deliver_source(D &d, const live_core_t &c, size_t src_n, bool want_peak) {
    d.src = c.c_rec; d.src_ld = c.ld_c; d.c0 = c.have_track ? 2 : 0; d.c1 = c.rec;
    d.src_st = c.c_st; d.src_n = src_n;
    if (c.have_track) {
        d.src_cand = reinterpret_cast<const double *>(c.c_cand); d.kmax = c.track.kmax;
        d.src_count = c.c_count;
        d.src_peak = want_peak ? c.c_peak : nullptr;
    }
    if (c.p.formant_order) { d.state = c.state; d.n_state = 2 * c.p.n_est; }
}

// Two pinned staging buffers with their raw device slots: upload k goes through slot k & 1, on the context's own stream -- no second
// stream to wait for, no host wait for the upload.  staged[i]: slot i's last upload has left its staging buffer.
struct live_ring_t {
    void *stage[2] = {nullptr, nullptr}, *raw[2] = {nullptr, nullptr};
    hipEvent_t staged[2] = {nullptr, nullptr};
    size_t uploads = 0;
    int slot() const { return (int)(uploads & 1); }
    int alloc(vbx_ctx *ctx, size_t stage_bytes, size_t raw_bytes);
    int acquire(vbx_ctx *ctx, char **h_stage);            // the next slot's staging buffer, once the upload of two pushes ago has left it
    int upload(vbx_ctx *ctx, size_t bytes);               // ONE copy of its first `bytes` into the slot, behind the slot's last reader
    void free();
};

void live_drain(vbx_ctx *ctx);                            // close: a family's buffers may still be read by queued work

}  // namespace vbx
