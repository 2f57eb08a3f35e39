// vbx_api_live.hip -- the host-side core of the live families: sessions (vbx_api_session.hip) and the session pool
// (vbx_api_pool.hip).  No kernel and no entry point: what those units do identically around their own launches (vbx_live.hpp).
#include "vbx_live.hpp"

#include <cstring>

namespace vbx {

int live_check_audio(vbx_ctx *ctx, const char *fn, const vbx_host_audio *h_fmt, bool channels_ok, const char *channels_msg) {
    VBX_REQUIRE_FN(ctx, fn, sample_format_ok(h_fmt->format), "unknown sample format");
    VBX_REQUIRE_FN(ctx, fn, channels_ok, channels_msg);
    VBX_REQUIRE_FN(ctx, fn, h_fmt->reserved == 0 && h_fmt->chunk_frames == 0, "reserved and chunk_frames must be 0");
    return VBX_SUCCESS;
}

int live_check_n_est(vbx_ctx *ctx, const char *fn, const vbx_analysis_params *h_p) {
    VBX_REQUIRE_FN(ctx, fn, !h_p->formant_order || (h_p->n_est >= 1 && h_p->n_est <= VBX_FORMANT_SLOTS), "n_est must be in [1, 6]");
    return VBX_SUCCESS;
}

live_core_t live_make(vbx_ctx *ctx, int fmt, size_t frame_len, size_t stride, const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext,
                      const vbx_pitch_track_params *h_track) {
    live_core_t c;
    c.ctx = ctx; c.fmt = fmt; c.frame_len = frame_len; c.stride = stride;
    c.p = *h_p;
    if (h_ext) { c.ext = *h_ext; c.have_ext = true; }
    if (h_track) { c.track = *h_track; c.have_track = true; }
    c.rec = vbx_record_doubles_ex(h_p, h_ext);
    c.ld_c = c.rec + (c.rec & 1);
    return c;
}

vbx_pitch_path_params live_path_params(const live_core_t &c) {
    vbx_pitch_path_params path = c.track.path;
    if (path.time_step == 0.0) path.time_step = (double)c.stride / c.p.sample_rate;
    return path;
}

int live_check_path(const live_core_t &c, const char *fn, size_t call_max) {
    return c.have_track ? check_pitch_path(c.ctx, fn, live_path_params(c), call_max, c.track.kmax, true, nullptr, 0) : VBX_SUCCESS;
}

int live_alloc(live_core_t &c, size_t nbuf, size_t state_rows) {
    vbx_ctx *ctx = c.ctx;
    LIVE_HIP(ctx, hipMalloc((void **)&c.c_rec, nbuf * c.ld_c * sizeof(double)), live_free(c));
    LIVE_HIP(ctx, hipMalloc((void **)&c.c_st, 3 * nbuf * sizeof(int32_t)), live_free(c));
    if (c.have_track) {
        LIVE_HIP(ctx, hipMalloc((void **)&c.c_cand, nbuf * c.track.kmax * sizeof(vbx_pitch)), live_free(c));
        LIVE_HIP(ctx, hipMalloc((void **)&c.c_count, nbuf * sizeof(int32_t)), live_free(c));
        LIVE_HIP(ctx, hipMalloc((void **)&c.c_peak, nbuf * sizeof(double)), live_free(c));
    }
    LIVE_HIP(ctx, hipMalloc((void **)&c.state, state_rows * 2 * VBX_FORMANT_SLOTS * sizeof(double)), live_free(c));
    LIVE_HIP(ctx, hipMemsetAsync(c.state, 0, state_rows * 2 * VBX_FORMANT_SLOTS * sizeof(double), ctx->stream), live_free(c));
    return VBX_SUCCESS;
}

void live_free(live_core_t &c) {
    for (void *m : {(void *)c.c_rec, (void *)c.c_st, (void *)c.c_cand, (void *)c.c_count, (void *)c.c_peak, (void *)c.state}) if (m) hipFree(m);
    c.c_rec = nullptr; c.c_st = nullptr; c.c_cand = nullptr; c.c_count = nullptr; c.c_peak = nullptr; c.state = nullptr;
}

int live_analyze(const live_core_t &c, const char *fn, const void *plane, size_t n, const int64_t *seg, size_t n_seg, bool want_peak) {
    vbx_pitch_track_outputs to{};
    to.cand = c.c_cand; to.count = c.c_count; to.peak = want_peak ? c.c_peak : nullptr;
    return analyze_ex(c.ctx, fn, frames_t(plane, sample_plane_kind(c.fmt)), n, c.frame_len, c.stride, &c.p, c.have_ext ? &c.ext : nullptr,
                      c.have_track ? &c.track : nullptr, seg, n_seg, c.c_rec, c.ld_c, c.c_st, c.have_track ? &to : nullptr, true);
}

int live_take_last_track(const live_core_t &c, const char *fn, size_t n) {
    const auto &lt = c.ctx->last_track;
    if (lt.res == nullptr || lt.out != reinterpret_cast<res_t *>(c.c_rec + 2) || lt.F != (long)n)
        return fail(c.ctx, VBX_E_RUNTIME, std::string(fn) + ": the frame loop left no track to stitch");
    return VBX_SUCCESS;
}

int live_check_outputs(const live_core_t &c, const char *fn, unsigned which, const char *name, const vbx_channel_outputs &o, size_t record_ld,
                       size_t status_ld, size_t rows, const char *status_ld_msg, bool *want_peak) {
    vbx_ctx *ctx = c.ctx;
    if (which & LIVE_OUT_RECORDS) VBX_REQUIRE_FN(ctx, fn, o.records != nullptr, "null argument");
    if (which & LIVE_OUT_ALIGNED) VBX_REQUIRE_FN(ctx, fn, ((uintptr_t)o.records & 15) == 0, "records must be 16-byte aligned");
    if (which & LIVE_OUT_RECORD_LD)
        VBX_REQUIRE_FN(ctx, fn, record_ld >= c.rec && record_ld % 2 == 0, "record_ld must be even and >= vbx_record_doubles(params)");
    if (which & LIVE_OUT_STATUS_LD) VBX_REQUIRE_FN(ctx, fn, o.status3 == nullptr || status_ld >= rows, status_ld_msg);
    if ((which & LIVE_OUT_LISTS) && c.have_track) {
        const vbx_pitch_track_outputs *t = o.outputs;
        const std::string nm(name);
        VBX_REQUIRE_FN(ctx, fn, t != nullptr && t->cand != nullptr && t->count != nullptr, "the tracked form needs " + nm + "->cand and ->count");
        VBX_REQUIRE_FN(ctx, fn, c.track.path.silence_threshold == 0.0 || t->peak != nullptr, "a silence_threshold needs " + nm + "->peak");
        VBX_REQUIRE_FN(ctx, fn, t->index == nullptr, nm + "->index must be NULL: the caller runs the path (vbx_pitch_path_f64)");
        *want_peak = *want_peak || t->peak != nullptr;
    }
    return VBX_SUCCESS;
}

int live_ring_t::alloc(vbx_ctx *ctx, size_t stage_bytes, size_t raw_bytes) {
    for (int i = 0; i < 2; i++) {
        LIVE_HIP(ctx, hipHostMalloc(&stage[i], stage_bytes, hipHostMallocDefault), free());
        LIVE_HIP(ctx, hipMalloc(&raw[i], raw_bytes), free());
        LIVE_HIP(ctx, hipEventCreateWithFlags(&staged[i], hipEventDisableTiming), free());
    }
    return VBX_SUCCESS;
}

int live_ring_t::acquire(vbx_ctx *ctx, char **h_stage) {
    VBX_HIP(ctx, hipEventSynchronize(staged[slot()]));
    *h_stage = static_cast<char *>(stage[slot()]);
    return VBX_SUCCESS;
}

int live_ring_t::upload(vbx_ctx *ctx, size_t bytes) {
    VBX_HIP(ctx, hipMemcpyAsync(raw[slot()], stage[slot()], bytes, hipMemcpyHostToDevice, ctx->stream));
    VBX_HIP(ctx, hipEventRecord(staged[slot()], ctx->stream));
    uploads++;
    return VBX_SUCCESS;
}

void live_ring_t::free() {
    for (int i = 0; i < 2; i++) {
        if (stage[i]) hipHostFree(stage[i]);
        if (raw[i]) hipFree(raw[i]);
        if (staged[i]) hipEventDestroy(staged[i]);
        stage[i] = nullptr; raw[i] = nullptr; staged[i] = nullptr;
    }
}

void live_drain(vbx_ctx *ctx) {
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (ctx->side) hipStreamSynchronize(ctx->side);
    if (ctx->trk) hipStreamSynchronize(ctx->trk);
}

}  // namespace vbx
