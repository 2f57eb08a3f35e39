// vbx_api_session.hip -- live sessions: one channel, or every selected channel, of one stream of audio, analysed block by block.
// What a push shares with a pool's tick -- the chunk-local buffers, the frame-loop call, the output checks, the staging ring -- is the
// live core's (vbx_live.hpp); the carry buffers, the plan, the launches around the frame loop and the path binding are here.
#include "vbx_live.hpp"

#include <cstring>
#include <string>
#include <vector>

using namespace vbx;

// ---- live sessions (header: "live sessions") --------------------------------------------------

extern "C" {

// blocks of up to this many bytes are staged through the session's pinned buffers and uploaded on the context's own stream: a host
// copy of about 10 us at this size, which is what the copy stream's event round trip was measured to add to a push (DESIGN.md
// section 5g); larger blocks take the copy stream, where their upload runs beside the previous block's analysis
#define VBX_SESSION_STAGE_BYTES 131072
static const char *const k_ingest_names[9] = {"", "session_ingest_pcm16", "session_ingest_pcm24", "session_ingest_pcm32", "session_ingest_f32",
                                              "session_ingest_f64", "session_ingest_u8", "session_ingest_ulaw", "session_ingest_alaw"};      // by sample_name_slot
static const char *const k_ingest_all_names[9] = {"", "session_ingest_all_pcm16", "session_ingest_all_pcm24", "session_ingest_all_pcm32",
                                                  "session_ingest_all_f32", "session_ingest_all_f64", "session_ingest_all_u8",
                                                  "session_ingest_all_ulaw", "session_ingest_all_alaw"};

// One channel, or n_sel channels, of one stream of audio, analysed block by block.  The session owns what lives between pushes and
// everything a push writes before the caller's arrays: the two carry buffers (ping-pong: a push's ingest writes the other one), the
// staging ring with the two events per raw slot of the copy stream's uploads, and the core's chunk-local buffers and state rows.
struct vbx_session {
    live_core_t core;
    size_t channels = 1, channel = 0, max_block = 0;
    // the stream so far
    size_t consumed = 0, utt_frame = 0, frames = 0;
    size_t base = 0;                                      // the sample frame element 0 of carry[cur] holds
    size_t keep_from = 0;                                 // the first sample frame a later push may still read (vbx_session_plan)
    int cur = 0;
    void *carry[2] = {nullptr, nullptr};
    // small blocks (a hop, a few hops) go through the ring's pinned buffers on the context's own stream; larger ones straight into
    // the ring's raw slot on the copy stream -- ready: the upload has landed; freed: the slot's last reader is through
    live_ring_t ring;
    size_t stage_bytes = 0;
    hipEvent_t ready[2] = {nullptr, nullptr}, freed[2] = {nullptr, nullptr};
    // vbx_session_open_channels (n_sel >= 1; 0: a one-channel session): the carry buffers hold n_sel planes, plane k = channel
    // sel.ch[k], plane_ld elements apart in carry[cur] (vbx_session_channels_plan), and the state n_sel rows
    size_t n_sel = 0, plane_ld = 0;
    unpack_sel_t sel{};
    std::vector<int64_t> seg;                             // the segment list of the current frame-loop call: [0, Q, 2Q, ...]
    // vbx_session_path_bind / _bind_channels: one online path per channel over the session-owned lists, and where each one's rows go
    bool bound = false;
    std::vector<vbx_path_stream *> paths;
    std::vector<vbx_channel_path_outputs> p_outs;
    size_t p_ld = 0;
};

static void session_free(vbx_session *s) {
    for (int i = 0; i < 2; i++) {
        if (s->carry[i]) hipFree(s->carry[i]);
        if (s->ready[i]) hipEventDestroy(s->ready[i]);
        if (s->freed[i]) hipEventDestroy(s->freed[i]);
    }
    s->ring.free();
    live_free(s->core);
    for (vbx_path_stream *ps : s->paths) path_stream_free(ps);
    delete s;
}

// h_channels == nullptr: vbx_session_open (one channel, h_fmt->channel); else vbx_session_open_channels
static int session_open_impl(vbx_ctx *ctx, const char *fn, const vbx_host_audio *h_fmt, const int32_t *h_channels, size_t n_sel, bool multi,
                             size_t frame_len, size_t stride, const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext,
                             const vbx_pitch_track_params *h_track, size_t max_block, vbx_session **out) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null context");
    VBX_REQUIRE_FN(ctx, fn, out != nullptr, "null output");
    *out = nullptr;
    VBX_REQUIRE_FN(ctx, fn, h_fmt != nullptr && h_p != nullptr, "null argument");
    int rc = live_check_audio(ctx, fn, h_fmt, h_fmt->channels >= 1 && h_fmt->channel >= 0 && h_fmt->channel < h_fmt->channels,
                              "need channels >= 1 and 0 <= channel < channels");
    if (rc != VBX_SUCCESS) return rc;
    unpack_sel_t sel{};
    if (multi) {
        VBX_REQUIRE_FN(ctx, fn, h_fmt->channel == 0, "channel must be 0 (the selection is h_channels)");
        VBX_REQUIRE_FN(ctx, fn, channel_selection_ok(h_channels, n_sel, h_fmt->channels, &sel),
                       "need 1 <= n_sel <= min(channels, VBX_HOST_MAX_CHANNELS) distinct channels in [0, channels)");
    }
    VBX_REQUIRE_FN(ctx, fn, max_block >= 1, "max_block_sample_frames must be >= 1");
    VBX_REQUIRE_FN(ctx, fn, frame_len >= 1 && frame_len <= VBX_MAX_LONG_FRAME_LEN, "frame_len must be in [1, 67108864]");
    VBX_REQUIRE_FN(ctx, fn, stride >= 1, "stride must be >= 1");
    VBX_REQUIRE_FN(ctx, fn, max_block <= ((size_t)1 << 40) && stride <= ((size_t)1 << 40), "max_block_sample_frames or stride too large");
    if ((rc = live_check_n_est(ctx, fn, h_p)) != VBX_SUCCESS) return rc;
    const size_t nmax = session_max_frames(stride, max_block);
    VBX_REQUIRE_FN(ctx, fn, nmax <= 0x7fffffffull, "too many frames for one launch");
    // n_sel planes: the largest a push can make (a plane never holds more than session_carry_samples), and the frames of the one
    // frame-loop call over them
    const size_t cap1 = session_carry_samples(frame_len, stride, max_block);
    size_t q_max = 0, call_max = nmax;
    if (multi) {
        vbx_session_channels_plan_t cp{};
        VBX_REQUIRE_FN(ctx, fn, vbx_session_channels_plan(0, 0, cap1, frame_len, stride, sample_out_bytes(h_fmt->format), n_sel, &cp, nullptr) == VBX_SUCCESS,
                       "bad session plan");
        q_max = cp.plane_frames;
        call_max = (n_sel - 1) * q_max + nmax;
        VBX_REQUIRE_FN(ctx, fn, q_max <= 0x7fffffffull && call_max <= 0x7fffffffull, "too many frames for one launch");
    }
    const live_core_t core = live_make(ctx, h_fmt->format, frame_len, stride, h_p, h_ext, h_track);
    if ((rc = live_check_path(core, fn, call_max)) != VBX_SUCCESS) return rc;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_host_slots(ctx, 0)) != VBX_SUCCESS) return rc;      // (the copy stream; the context's own raw slots stay as they are)
    vbx_session *s = new vbx_session();
    s->core = core; s->channels = (size_t)h_fmt->channels; s->channel = (size_t)h_fmt->channel; s->max_block = max_block;
    if (multi) {
        s->n_sel = n_sel; s->sel = sel; s->plane_ld = q_max * stride;
        s->seg.resize(n_sel);
    }
    const size_t planes = multi ? n_sel : 1;
    const size_t cap = multi ? n_sel * q_max * stride : cap1, ob = sample_out_bytes(core.fmt);
    const size_t raw_bytes = max_block * s->channels * sample_src_bytes(core.fmt);
    s->stage_bytes = raw_bytes < (size_t)VBX_SESSION_STAGE_BYTES ? raw_bytes : (size_t)VBX_SESSION_STAGE_BYTES;
    for (int i = 0; i < 2; i++) {
        LIVE_HIP(ctx, hipMalloc(&s->carry[i], cap * ob), session_free(s));                     // (hipMalloc: 256-byte aligned bases)
        LIVE_HIP(ctx, hipMemsetAsync(s->carry[i], 0, cap * ob, ctx->stream), session_free(s));
        LIVE_HIP(ctx, hipEventCreateWithFlags(&s->ready[i], hipEventDisableTiming), session_free(s));
        LIVE_HIP(ctx, hipEventCreateWithFlags(&s->freed[i], hipEventDisableTiming), session_free(s));
    }
    rc = s->ring.alloc(ctx, s->stage_bytes, raw_bytes);
    if (rc == VBX_SUCCESS) rc = live_alloc(s->core, call_max, planes);
    if (rc != VBX_SUCCESS) { session_free(s); return rc; }
    // the warm-up: the largest shape a push can ask for, on the zeroed carry
    if (multi) for (size_t k = 0; k < n_sel; k++) s->seg[k] = (int64_t)(k * q_max);
    rc = live_warm_up(s->core, fn, s->carry[s->cur], call_max, multi ? s->seg.data() : nullptr, s->n_sel, [&] { session_free(s); });
    if (rc != VBX_SUCCESS) return rc;
    *out = s;
    return VBX_SUCCESS;
}

int vbx_session_open(vbx_ctx *ctx, const vbx_host_audio *h_fmt, size_t frame_len, size_t stride, const vbx_analysis_params *h_p,
                     const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, size_t max_block, vbx_session **out) {
    return session_open_impl(ctx, __func__, h_fmt, nullptr, 0, false, frame_len, stride, h_p, h_ext, h_track, max_block, out);
}

int vbx_session_open_channels(vbx_ctx *ctx, const vbx_host_audio *h_fmt, const int32_t *h_channels, size_t n_sel, size_t frame_len, size_t stride,
                              const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                              size_t max_block, vbx_session **out) {
    return session_open_impl(ctx, __func__, h_fmt, h_channels, n_sel, true, frame_len, stride, h_p, h_ext, h_track, max_block, out);
}

// a host block into the ring's next raw slot; *wait_ready: the upload runs on the copy stream, and the caller waits for
// ready[*slot] before it returns (the block is not read after the call)
static int session_upload(vbx_session *s, const void *block, size_t n, const void **raw, int *slot_out, bool *wait_ready) {
    vbx_ctx *ctx = s->core.ctx;
    live_ring_t &r = s->ring;
    const int slot = r.slot();
    const size_t bytes = n * s->channels * sample_src_bytes(s->core.fmt);
    if (bytes <= s->stage_bytes) {
        // through pinned staging: the caller's block has been read when the host copy returns
        char *stage = nullptr;
        int rc = r.acquire(ctx, &stage);
        if (rc != VBX_SUCCESS) return rc;
        std::memcpy(stage, block, bytes);
        if ((rc = r.upload(ctx, bytes)) != VBX_SUCCESS) return rc;
    } else {                                              // on the copy stream, behind the slot's last reader
        VBX_HIP(ctx, hipStreamWaitEvent(ctx->copy, s->freed[slot], 0));
        VBX_HIP(ctx, hipMemcpyAsync(r.raw[slot], block, bytes, hipMemcpyHostToDevice, ctx->copy));
        VBX_HIP(ctx, hipEventRecord(s->ready[slot], ctx->copy));
        VBX_HIP(ctx, hipStreamWaitEvent(ctx->stream, s->ready[slot], 0));
        *wait_ready = true;
        r.uploads++;
    }
    *raw = r.raw[slot];
    *slot_out = slot;
    return VBX_SUCCESS;
}

// the bound session's path launch: every channel's contour in one launch, or the one channel's
static int session_path_launch(vbx_session *s, const char *fn, const vbx_pitch *cand, const int32_t *count, const int32_t *st, const double *peak,
                               size_t plane_frames, size_t n, int end_utterance) {
    if (s->n_sel) return path_stream_launch_all(s->paths.data(), s->n_sel, fn, cand, count, st, peak, plane_frames, n, end_utterance, s->p_outs.data(), s->p_ld);
    const vbx_channel_path_outputs &po = s->p_outs[0];
    return path_stream_launch(s->paths[0], fn, cand, count, st, peak, n, end_utterance, po.out_path, s->p_ld, po.out_index, po.out_forced, po.d_commit);
}

// One push of either form.  multi: the entry point is a _channels one; outs: one entry per plane (a one-channel session's entry
// points make theirs from their own arguments, and `name` is what they call the lists).  The shape is vbx_session_channels_plan's: a
// one-channel session is its push / base / keep with one plane and no segment list.  The two forms differ in their four launches.
static int session_push_impl(vbx_session *s, const char *fn, bool multi, const void *block, bool on_device, size_t n,
                             const vbx_channel_outputs *outs, size_t record_ld, size_t status_ld, size_t *h_n) {
    if (!s) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null session");
    const live_core_t &c = s->core;
    vbx_ctx *ctx = c.ctx;
    if (h_n) *h_n = 0;
    if (multi) VBX_REQUIRE_FN(ctx, fn, s->n_sel != 0, "the session was opened with vbx_session_open: push with vbx_session_push");
    else VBX_REQUIRE_FN(ctx, fn, s->n_sel == 0, "the session was opened with vbx_session_open_channels: push with vbx_session_push_channels");
    if (n == 0) return VBX_SUCCESS;
    VBX_REQUIRE_FN(ctx, fn, block != nullptr, "null block");
    VBX_REQUIRE_FN(ctx, fn, n <= s->max_block, "the block is larger than the session's max_block_sample_frames");
    VBX_REQUIRE_FN(ctx, fn, !on_device || c.fmt == VBX_SAMPLE_PCM24 || (uintptr_t)block % sample_src_bytes(c.fmt) == 0, "the block needs its type's alignment");
    const size_t K = multi ? s->n_sel : 1;
    vbx_session_channels_plan_t cp{};
    if (vbx_session_channels_plan(s->consumed, s->utt_frame, n, c.frame_len, c.stride, sample_out_bytes(c.fmt), K, &cp, multi ? s->seg.data() : nullptr) != VBX_SUCCESS)
        return fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad session plan");
    const vbx_session_plan_t &pl = cp.push;
    const size_t nf = pl.hi - pl.lo;
    bool want_peak = false;
    auto check = [&](unsigned which, const char *name, const vbx_channel_outputs &o) {
        return live_check_outputs(c, fn, which, name, o, record_ld, status_ld, nf, "status_ld must be >= the frames the push delivers", &want_peak);
    };
    int rc = VBX_SUCCESS;
    if (multi) VBX_REQUIRE_FN(ctx, fn, outs != nullptr, "null outputs");
    if (nf && !multi && (rc = check(LIVE_OUT_ALL, "h_outputs", outs[0])) != VBX_SUCCESS) return rc;
    if (nf && multi) {                                    // (the order these refusals have always had: record_ld first, the alignment after status_ld)
        if ((rc = check(LIVE_OUT_RECORD_LD, "outputs", outs[0])) != VBX_SUCCESS) return rc;
        for (size_t k = 0; k < K; k++) {
            if ((rc = check(LIVE_OUT_RECORDS | LIVE_OUT_STATUS_LD, "outputs", outs[k])) != VBX_SUCCESS) return rc;
            if ((rc = check(LIVE_OUT_ALIGNED, "outputs", outs[k])) != VBX_SUCCESS) return rc;
            for (size_t j = 0; j < k; j++) {              // [n, record_ld] each
                const uintptr_t a = (uintptr_t)outs[j].records, b = (uintptr_t)outs[k].records, len = nf * record_ld * sizeof(double);
                VBX_REQUIRE_FN(ctx, fn, a + len <= b || b + len <= a, "the channels' records overlap");
            }
            if ((rc = check(LIVE_OUT_LISTS, "outputs", outs[k])) != VBX_SUCCESS) return rc;
        }
    }
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const size_t sf_bytes = s->channels * sample_src_bytes(c.fmt);
    const void *raw = block;
    int slot = -1;
    bool wait_ready = false;
    if (!on_device && (rc = session_upload(s, block, n, &raw, &slot, &wait_ready)) != VBX_SUCCESS) return rc;      // ONE upload, whatever n_sel
    // the other carry buffer, every plane from sample frame cp.base on -- what this push's analysis reads first, or, when it completes no
    // frame, what a later one may.  (stride > frame_len: it may lie beyond the carried samples, inside the block; the gap is dropped)
    const size_t at = s->consumed, from_old = at - cp.keep, skip = cp.base > at ? cp.base - at : 0;
    const char *src = static_cast<const char *>(raw) + skip * sf_bytes;
    if (!multi) {
        Prof p(ctx, k_ingest_names[sample_name_slot(c.fmt)]);
        launch_session_ingest(ctx->stream, c.fmt, s->carry[s->cur], from_old - s->base, cp.keep, src, n - skip, s->channels, s->channel, s->carry[s->cur ^ 1]);
    } else {
        Prof p(ctx, k_ingest_all_names[sample_name_slot(c.fmt)]);
        launch_session_ingest_all(ctx->stream, c.fmt, s->carry[s->cur], s->plane_ld, from_old - s->base, cp.keep, src, n - skip, s->channels, s->sel, K,
                                  s->carry[s->cur ^ 1], cp.plane_ld);
    }
    if (slot >= 0) VBX_HIP(ctx, hipEventRecord(s->freed[slot], ctx->stream));
    s->cur ^= 1; s->base = cp.base; s->plane_ld = cp.plane_ld; s->consumed = at + n; s->keep_from = pl.keep_from;
    auto bail = [&](int code) { if (wait_ready) hipEventSynchronize(s->ready[slot]); return code; };      // the block is not read after the call returns
    if (nf) {
        // the frame loop on the new carry buffer (n_sel planes: as one recording, with the segment list the plan wrote)
        const size_t n_call = cp.call_frames;             // (one plane: cp.frames)
        if ((rc = live_analyze(c, fn, s->carry[s->cur], n_call, multi ? s->seg.data() : nullptr, s->n_sel, want_peak)) != VBX_SUCCESS) return bail(rc);
        // the push continues an utterance: every channel's tracker goes on from its true state, the formant row of its last frame delivered
        if (pl.continues_prev && c.p.formant_order) {
            if (!multi) rc = vbx_internal_track_stitch(ctx, nullptr, reinterpret_cast<vbx_resonance *>(c.c_rec + 2), n_call, c.ld_c, pl.warm, n_call, c.state, nullptr);
            else if ((rc = live_take_last_track(c, fn, n_call)) == VBX_SUCCESS) {
                const auto &lt = ctx->last_track;
                Prof p(ctx, "tracker_stitch_all");
                launch_tracker_stitch_all(ctx->stream, lt.res, lt.F, VBX_MAX_RESONANCES, lt.cnt, lt.n_est, lt.st, lt.out, lt.out_ld, (long)cp.plane_frames,
                                          (long)pl.warm, (long)cp.frames, c.state, (long)K);
            }
            if (rc != VBX_SUCCESS) return bail(rc);
        }
        if (!multi) {
            session_deliver_t d{};
            live_deliver_source(d, c, n_call, want_peak);
            d.row0 = pl.warm; d.rows = nf; d.dst = outs[0].records; d.dst_ld = record_ld; d.dst_st = outs[0].status3; d.dst_st_ld = status_ld;
            if (c.have_track) {
                const vbx_pitch_track_outputs *o = outs[0].outputs;
                d.dst_cand = reinterpret_cast<double *>(o->cand); d.dst_count = o->count; d.dst_peak = o->peak;
            }
            Prof p(ctx, "session_deliver");
            launch_session_deliver(ctx->stream, d);
        } else {
            session_deliver_all_t d{};
            live_deliver_source(d, c, n_call, want_peak);
            d.plane_frames = cp.plane_frames; d.row0 = pl.warm; d.rows = nf; d.dst_ld = record_ld; d.dst_st_ld = status_ld;
            for (size_t k = 0; k < K; k++) {
                d.ch[k].rec = outs[k].records; d.ch[k].st = outs[k].status3;
                if (c.have_track) {
                    const vbx_pitch_track_outputs *o = outs[k].outputs;
                    d.ch[k].cand = reinterpret_cast<double *>(o->cand); d.ch[k].count = o->count; d.ch[k].peak = o->peak;
                }
            }
            Prof p(ctx, "session_deliver_all");
            launch_session_deliver_all(ctx->stream, d, K);
        }
        live_drop_last_track(ctx);
        s->frames += nf;
    }
    if (s->bound) {
        // the contours: every channel's online path over its own rows of the session-owned lists, in one launch behind the deliver
        // (a push that completes no frame still reports: n = 0 and what is pending)
        const size_t w = nf ? pl.warm : 0;
        const vbx_pitch *cand = c.c_cand + w * c.track.kmax;
        const double *peak = want_peak ? c.c_peak + w : nullptr;
        if ((rc = session_path_launch(s, fn, cand, c.c_count + w, c.c_st + w, peak, cp.plane_frames, nf, 0)) != VBX_SUCCESS) return bail(rc);
    }
    if ((rc = check_launch(ctx, fn)) != VBX_SUCCESS) return bail(rc);
    if (h_n) *h_n = nf;
    if (wait_ready) VBX_HIP(ctx, hipEventSynchronize(s->ready[slot]));     // the last byte of h_block has been read
    return VBX_SUCCESS;
}

int vbx_session_push(vbx_session *s, const void *h_block, size_t n_sample_frames, double *out_records, size_t record_ld, int32_t *status3,
                     size_t status_ld, const vbx_pitch_track_outputs *h_outputs, size_t *h_n_frames) {
    const vbx_channel_outputs one{out_records, status3, h_outputs};
    return session_push_impl(s, __func__, false, h_block, false, n_sample_frames, &one, record_ld, status_ld, h_n_frames);
}

int vbx_session_push_device(vbx_session *s, const void *d_block, size_t n_sample_frames, double *out_records, size_t record_ld,
                            int32_t *status3, size_t status_ld, const vbx_pitch_track_outputs *h_outputs, size_t *h_n_frames) {
    const vbx_channel_outputs one{out_records, status3, h_outputs};
    return session_push_impl(s, __func__, false, d_block, true, n_sample_frames, &one, record_ld, status_ld, h_n_frames);
}

int vbx_session_push_channels(vbx_session *s, const void *h_block, size_t n_sample_frames, const vbx_channel_outputs *h_out, size_t record_ld,
                              size_t status_ld, size_t *h_n_frames) {
    return session_push_impl(s, __func__, true, h_block, false, n_sample_frames, h_out, record_ld, status_ld, h_n_frames);
}

int vbx_session_push_channels_device(vbx_session *s, const void *d_block, size_t n_sample_frames, const vbx_channel_outputs *h_out,
                                     size_t record_ld, size_t status_ld, size_t *h_n_frames) {
    return session_push_impl(s, __func__, true, d_block, true, n_sample_frames, h_out, record_ld, status_ld, h_n_frames);
}

int vbx_session_mark_utterance(vbx_session *s) {
    if (!s) return fail(nullptr, VBX_E_INVALID, "vbx_session_mark_utterance: null session");
    s->utt_frame = vbx_frame_count(s->consumed, s->core.frame_len, s->core.stride);
    if (!s->bound) return VBX_SUCCESS;
    VBX_HIP(s->core.ctx, hipSetDevice(s->core.ctx->device));
    return session_path_launch(s, __func__, nullptr, nullptr, nullptr, nullptr, 0, 0, 1);      // the rest of the contour now, not when the next frame arrives
}

// what both bindings do once their arguments stand: a bound session takes other destinations only; an unbound one opens its paths,
// or keeps those of before a reset (their state was reset with the session) when nothing about them changes
static int session_bind(vbx_session *s, const char *fn, double peak_ref, size_t max_pending, const vbx_channel_path_outputs *h_out, size_t path_ld) {
    vbx_ctx *ctx = s->core.ctx;
    const size_t K = s->n_sel ? s->n_sel : 1;
    const bool same = !s->paths.empty() && s->paths[0]->max_pending == max_pending && std::memcmp(&peak_ref, &s->paths[0]->peak_ref, sizeof(double)) == 0;
    if (s->bound) {                                       // between pushes: other destinations, the same paths
        VBX_REQUIRE_FN(ctx, fn, same, "a bound session keeps its peak_ref and max_pending (vbx_session_reset drops the binding)");
    } else {
        VBX_REQUIRE_FN(ctx, fn, s->consumed == 0, "bind before the first push or after vbx_session_reset");
        if (!same) {
            const vbx_pitch_path_params path = live_path_params(s->core);
            std::vector<vbx_path_stream *> fresh;
            for (size_t k = 0; k < K; k++) {
                vbx_path_stream *ps = nullptr;
                int rc = path_stream_open(ctx, fn, s->core.track.kmax, path, peak_ref, max_pending, &ps);
                if (rc != VBX_SUCCESS) { for (vbx_path_stream *q : fresh) path_stream_free(q); return rc; }
                fresh.push_back(ps);
            }
            for (vbx_path_stream *q : s->paths) path_stream_free(q);
            s->paths = fresh;
        }
        s->bound = true;
    }
    s->p_outs.assign(h_out, h_out + K);
    s->p_ld = path_ld;
    return VBX_SUCCESS;
}

int vbx_session_path_bind(vbx_session *s, double peak_ref, size_t max_pending, vbx_pitch *out_path, size_t path_ld, int32_t *out_index,
                          uint8_t *out_forced, vbx_path_commit *d_commit) {
    if (!s) return fail(nullptr, VBX_E_INVALID, "vbx_session_path_bind: null session");
    vbx_ctx *ctx = s->core.ctx;
    VBX_REQUIRE(ctx, s->n_sel == 0, "the session was opened with vbx_session_open_channels");
    VBX_REQUIRE(ctx, s->core.have_track, "the session was opened without h_track: it has no candidate lists");
    VBX_REQUIRE(ctx, out_path != nullptr && d_commit != nullptr, "null out_path or d_commit");
    VBX_REQUIRE(ctx, path_ld >= 2, "path_ld must be >= 2");
    const vbx_channel_path_outputs one{out_path, out_index, out_forced, d_commit};
    return session_bind(s, __func__, peak_ref, max_pending, &one, path_ld);
}

int vbx_session_path_bind_channels(vbx_session *s, double peak_ref, size_t max_pending, const vbx_channel_path_outputs *h_out, size_t path_ld) {
    if (!s) return fail(nullptr, VBX_E_INVALID, "vbx_session_path_bind_channels: null session");
    vbx_ctx *ctx = s->core.ctx;
    VBX_REQUIRE(ctx, s->n_sel != 0, "the session was opened with vbx_session_open: bind with vbx_session_path_bind");
    VBX_REQUIRE(ctx, s->core.have_track, "the session was opened without h_track: it has no candidate lists");
    VBX_REQUIRE(ctx, h_out != nullptr, "null outputs");
    for (size_t k = 0; k < s->n_sel; k++) VBX_REQUIRE(ctx, h_out[k].out_path != nullptr && h_out[k].d_commit != nullptr, "null out_path or d_commit");
    VBX_REQUIRE(ctx, path_ld >= 2, "path_ld must be >= 2");
    return session_bind(s, __func__, peak_ref, max_pending, h_out, path_ld);
}

int vbx_session_reset(vbx_session *s) {
    if (!s) return fail(nullptr, VBX_E_INVALID, "vbx_session_reset: null session");
    // (nothing is queued: the next ingest keeps nothing of the carry, and a first push of an utterance stitches from no state)
    s->consumed = 0; s->utt_frame = 0; s->frames = 0; s->base = 0; s->keep_from = 0;
    if (!s->paths.empty()) s->bound = false;              // the paths' state goes, and the binding with it
    for (vbx_path_stream *ps : s->paths) { int rc = path_stream_reset(ps); if (rc != VBX_SUCCESS) return rc; }
    return VBX_SUCCESS;
}

int vbx_session_info(const vbx_session *s, size_t *h_consumed, size_t *h_frames, size_t *h_carried) {
    if (!s) return fail(nullptr, VBX_E_INVALID, "vbx_session_info: null session");
    if (h_consumed) *h_consumed = s->consumed;
    if (h_frames) *h_frames = s->frames;
    if (h_carried) *h_carried = s->consumed - s->keep_from;
    return VBX_SUCCESS;
}

void vbx_session_close(vbx_session *s) {
    if (!s) return;
    live_drain(s->core.ctx);
    if (s->core.ctx->copy) hipStreamSynchronize(s->core.ctx->copy);
    session_free(s);
}

// test hook (tests/test_gpu_session_ingest.py): the ingest kernel on its own, on the context's stream
int vbx_internal_session_ingest(vbx_ctx *ctx, int format, int channels, int channel, const void *d_old, size_t drop, size_t keep,
                                const void *d_raw, size_t n_new, void *d_out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_REQUIRE(ctx, sample_format_ok(format), "unknown sample format");
    VBX_REQUIRE(ctx, channels >= 1 && channel >= 0 && channel < channels, "need channels >= 1 and 0 <= channel < channels");
    if (keep + n_new == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, d_out && (keep == 0 || d_old) && (n_new == 0 || d_raw), "null argument");
    VBX_REQUIRE(ctx, format == VBX_SAMPLE_PCM24 || (uintptr_t)d_raw % sample_src_bytes(format) == 0, "the source needs its type's alignment");
    VBX_REQUIRE(ctx, (uintptr_t)d_out % sample_out_bytes(format) == 0 && (uintptr_t)d_old % sample_out_bytes(format) == 0,
                "the carry buffers need their type's alignment");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, k_ingest_names[sample_name_slot(format)]);
      launch_session_ingest(ctx->stream, format, d_old, drop, keep, d_raw, n_new, (size_t)channels, (size_t)channel, d_out); }
    return check_launch(ctx, __func__);
}

// test hook (tests/test_gpu_session_channels_ingest.py): the multi-plane ingest kernel on its own, on the context's stream
int vbx_internal_session_ingest_channels(vbx_ctx *ctx, int format, int channels, const int32_t *h_channels, size_t n_sel, const void *d_old,
                                         size_t old_ld, size_t drop, size_t keep, const void *d_raw, size_t n_new, void *d_out, size_t out_ld) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_REQUIRE(ctx, sample_format_ok(format), "unknown sample format");
    unpack_sel_t sel{};
    VBX_REQUIRE(ctx, channel_selection_ok(h_channels, n_sel, channels, &sel),
                "need 1 <= n_sel <= min(channels, VBX_HOST_MAX_CHANNELS) distinct channels in [0, channels)");
    VBX_REQUIRE(ctx, keep + n_new <= out_ld && (keep == 0 || drop + keep <= old_ld), "a plane's elements must fit its pitch");
    if (keep + n_new == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, d_out && (keep == 0 || d_old) && (n_new == 0 || d_raw), "null argument");
    VBX_REQUIRE(ctx, format == VBX_SAMPLE_PCM24 || (uintptr_t)d_raw % sample_src_bytes(format) == 0, "the source needs its type's alignment");
    VBX_REQUIRE(ctx, (uintptr_t)d_out % sample_out_bytes(format) == 0 && (uintptr_t)d_old % sample_out_bytes(format) == 0,
                "the carry buffers need their type's alignment");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, k_ingest_all_names[sample_name_slot(format)]);
      launch_session_ingest_all(ctx->stream, format, d_old, old_ld, drop, keep, d_raw, n_new, (size_t)channels, sel, n_sel, d_out, out_ld); }
    return check_launch(ctx, __func__);
}

}  // extern "C"
