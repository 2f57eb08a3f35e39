// vbx_api_session.hip -- live sessions: one channel, or every selected channel, of one stream of audio, analysed block by block.
#include "vbx_ctx.hpp"

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

// One channel of one stream of audio, analysed block by block.  The session owns what lives between pushes and everything a push
// writes before the caller's arrays: the two carry buffers (ping-pong: a push's ingest writes the other one), the two raw staging
// slots with their events, the chunk-local records / status rows / lists and the tracker state.  The frame loop's own workspaces are
// the context's, grown once by the warm-up call of vbx_session_open.
struct vbx_session {
    vbx_ctx *ctx = nullptr;
    int fmt = 0; size_t channels = 1, channel = 0;
    size_t frame_len = 0, stride = 0, max_block = 0;
    vbx_analysis_params p{}; vbx_analysis_ext ext{}; vbx_pitch_track_params track{};
    bool have_ext = false, have_track = false;
    size_t rec = 0, ld_c = 0, nmax = 0;
    // the stream so far
    size_t consumed = 0, utt_frame = 0, frames = 0;
    size_t base = 0;                                      // the sample frame element 0 of carry[cur] holds
    size_t keep_from = 0;                                 // the first sample frame a later push may still read (vbx_session_plan)
    int cur = 0;
    size_t uploads = 0;                                   // host pushes so far: push k stages through raw slot k & 1
    // device memory
    void *carry[2] = {nullptr, nullptr};
    void *raw[2] = {nullptr, nullptr};
    hipEvent_t ready[2] = {nullptr, nullptr}, freed[2] = {nullptr, nullptr};
    // small blocks (a hop, a few hops): two pinned staging buffers the block is copied into on the host, uploaded from on the context's
    // own stream -- no second stream to wait for, no host wait for the upload; staged[i]: slot i's last upload has left it
    void *stage[2] = {nullptr, nullptr};
    size_t stage_bytes = 0;
    hipEvent_t staged[2] = {nullptr, nullptr};
    double *c_rec = nullptr; int32_t *c_st = nullptr;
    vbx_pitch *c_cand = nullptr; int32_t *c_count = nullptr; double *c_peak = nullptr;
    double *state = nullptr;                              // 2 * n_est doubles: the formant row of the last frame delivered
    // vbx_session_path_bind: the online path over the session-owned lists, and where its rows go
    vbx_path_stream *path = nullptr;
    bool bound = false;
    vbx_pitch *p_out = nullptr; size_t p_ld = 0; int32_t *p_index = nullptr; uint8_t *p_forced = nullptr; vbx_path_commit *p_commit = nullptr;
    // vbx_session_open_channels (n_sel >= 1; 0: a one-channel session): the carry buffers hold n_sel planes, plane k = channel
    // sel.ch[k], plane_ld elements apart in carry[cur] (vbx_session_channels_plan); the chunk-local buffers hold call_max frames, the
    // state n_sel rows of 2 * VBX_FORMANT_SLOTS doubles
    size_t n_sel = 0, plane_ld = 0, q_max = 0, call_max = 0;
    unpack_sel_t sel{};
    std::vector<int64_t> seg;                             // the segment list of the current frame-loop call: [0, Q, 2Q, ...]
    // vbx_session_path_bind_channels: one online path per channel (n_sel entries once bound) and where each one's rows go
    std::vector<vbx_path_stream *> paths;
    std::vector<vbx_channel_path_outputs> p_outs;
};

static void session_free(vbx_session *s) {
    for (int i = 0; i < 2; i++) {
        if (s->carry[i]) hipFree(s->carry[i]);
        if (s->raw[i]) hipFree(s->raw[i]);
        if (s->ready[i]) hipEventDestroy(s->ready[i]);
        if (s->freed[i]) hipEventDestroy(s->freed[i]);
        if (s->stage[i]) hipHostFree(s->stage[i]);
        if (s->staged[i]) hipEventDestroy(s->staged[i]);
    }
    if (s->c_rec) hipFree(s->c_rec);
    if (s->c_st) hipFree(s->c_st);
    if (s->c_cand) hipFree(s->c_cand);
    if (s->c_count) hipFree(s->c_count);
    if (s->c_peak) hipFree(s->c_peak);
    if (s->state) hipFree(s->state);
    if (s->path) path_stream_free(s->path);
    for (vbx_path_stream *ps : s->paths) path_stream_free(ps);
    delete s;
}

// the frame loop on frames [0, n) of the session's current carry buffer into the chunk-local buffers (a multi-channel session: over
// all planes as one recording, with the segment list s->seg)
static int session_analyze(vbx_session *s, const char *fn, size_t n, bool want_peak) {
    vbx_pitch_track_outputs to{};
    to.cand = s->c_cand; to.count = s->c_count; to.peak = want_peak ? s->c_peak : nullptr;
    return analyze_ex(s->ctx, fn, frames_t(s->carry[s->cur], sample_plane_kind(s->fmt)), n, s->frame_len, s->stride, &s->p,
                      s->have_ext ? &s->ext : nullptr, s->have_track ? &s->track : nullptr, s->n_sel ? s->seg.data() : nullptr, s->n_sel, s->c_rec,
                      s->ld_c, s->c_st,
                      s->have_track ? &to : nullptr, true);
}

// h_channels == nullptr: vbx_session_open (one channel, h_fmt->channel); else vbx_session_open_channels
static int session_open_impl(vbx_ctx *ctx, const char *fn, const vbx_host_audio *h_fmt, const int32_t *h_channels, size_t n_sel, bool multi,
                             size_t frame_len, size_t stride, const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext,
                             const vbx_pitch_track_params *h_track, size_t max_block, vbx_session **out) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null context");
    VBX_REQUIRE_FN(ctx, fn, out != nullptr, "null output");
    *out = nullptr;
    VBX_REQUIRE_FN(ctx, fn, h_fmt != nullptr && h_p != nullptr, "null argument");
    VBX_REQUIRE_FN(ctx, fn, sample_format_ok(h_fmt->format), "unknown sample format");
    VBX_REQUIRE_FN(ctx, fn, h_fmt->channels >= 1 && h_fmt->channel >= 0 && h_fmt->channel < h_fmt->channels, "need channels >= 1 and 0 <= channel < channels");
    VBX_REQUIRE_FN(ctx, fn, h_fmt->reserved == 0 && h_fmt->chunk_frames == 0, "reserved and chunk_frames must be 0");
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
    VBX_REQUIRE_FN(ctx, fn, !h_p->formant_order || (h_p->n_est >= 1 && h_p->n_est <= VBX_FORMANT_SLOTS), "n_est must be in [1, 6]");
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
    if (h_track) {
        vbx_pitch_path_params path = h_track->path;
        if (path.time_step == 0.0) path.time_step = (double)stride / h_p->sample_rate;
        int rc = check_pitch_path(ctx, fn, path, call_max, h_track->kmax, true, nullptr, 0);
        if (rc != VBX_SUCCESS) return rc;
    }
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_host_slots(ctx, 0);                   // (the copy stream; the context's own raw slots stay as they are)
    if (rc != VBX_SUCCESS) return rc;
    vbx_session *s = new vbx_session();
    s->ctx = ctx; s->fmt = h_fmt->format; s->channels = (size_t)h_fmt->channels; s->channel = (size_t)h_fmt->channel;
    s->frame_len = frame_len; s->stride = stride; s->max_block = max_block;
    s->p = *h_p;
    if (h_ext) { s->ext = *h_ext; s->have_ext = true; }
    if (h_track) { s->track = *h_track; s->have_track = true; }
    s->rec = vbx_record_doubles_ex(h_p, h_ext);
    s->ld_c = s->rec + (s->rec & 1);
    s->nmax = nmax;
    if (multi) {
        s->n_sel = n_sel; s->sel = sel; s->q_max = q_max; s->call_max = call_max; s->plane_ld = q_max * stride;
        s->seg.resize(n_sel);
    }
    const size_t planes = multi ? n_sel : 1, nbuf = multi ? call_max : nmax;
    const size_t cap = multi ? n_sel * q_max * stride : cap1, ob = sample_out_bytes(s->fmt);
    const size_t kmax = h_track ? h_track->kmax : 0;
    const size_t raw_bytes = max_block * s->channels * sample_src_bytes(s->fmt);
    const size_t stage_bytes = raw_bytes < (size_t)VBX_SESSION_STAGE_BYTES ? raw_bytes : (size_t)VBX_SESSION_STAGE_BYTES;
#define SESSION_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { hipStreamSynchronize(ctx->stream); session_free(s); \
        return fail(ctx, VBX_E_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)
    for (int i = 0; i < 2; i++) {
        SESSION_HIP(hipMalloc(&s->carry[i], cap * ob));                     // (hipMalloc: 256-byte aligned bases)
        SESSION_HIP(hipMemsetAsync(s->carry[i], 0, cap * ob, ctx->stream));
        SESSION_HIP(hipMalloc(&s->raw[i], raw_bytes));
        SESSION_HIP(hipEventCreateWithFlags(&s->ready[i], hipEventDisableTiming));
        SESSION_HIP(hipEventCreateWithFlags(&s->freed[i], hipEventDisableTiming));
        SESSION_HIP(hipHostMalloc(&s->stage[i], stage_bytes, hipHostMallocDefault));
        SESSION_HIP(hipEventCreateWithFlags(&s->staged[i], hipEventDisableTiming));
    }
    s->stage_bytes = stage_bytes;
    SESSION_HIP(hipMalloc((void **)&s->c_rec, nbuf * s->ld_c * sizeof(double)));
    SESSION_HIP(hipMalloc((void **)&s->c_st, 3 * nbuf * sizeof(int32_t)));
    if (h_track) {
        SESSION_HIP(hipMalloc((void **)&s->c_cand, nbuf * kmax * sizeof(vbx_pitch)));
        SESSION_HIP(hipMalloc((void **)&s->c_count, nbuf * sizeof(int32_t)));
        SESSION_HIP(hipMalloc((void **)&s->c_peak, nbuf * sizeof(double)));
    }
    SESSION_HIP(hipMalloc((void **)&s->state, planes * 2 * VBX_FORMANT_SLOTS * sizeof(double)));
    SESSION_HIP(hipMemsetAsync(s->state, 0, planes * 2 * VBX_FORMANT_SLOTS * sizeof(double), ctx->stream));
#undef SESSION_HIP
    // the largest shape a push can ask for, on the zeroed carry: the context's workspaces and tables are as large as they will ever
    // have to be, and what only the frame loop's parts know is rejected here
    if (multi) for (size_t k = 0; k < n_sel; k++) s->seg[k] = (int64_t)(k * q_max);
    rc = session_analyze(s, fn, nbuf, true);
    if (rc == VBX_SUCCESS) rc = check_launch(ctx, fn);
    ctx->last_track.res = nullptr;                        // the chunk-local rows are no track of the caller's
    ctx->last_track.n_est = 0;
    if (rc != VBX_SUCCESS) { const std::string why = ctx->last_error; hipStreamSynchronize(ctx->stream); vbx_sync(ctx); session_free(s); return fail(ctx, rc, why); }
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

// a host block into raw slot `*slot` (push k stages through slot k & 1); *wait_ready: the upload runs on the copy stream, and the
// caller waits for ready[*slot] before it returns (the block is not read after the call)
static int session_upload(vbx_session *s, const void *block, size_t n, const void **raw, int *slot_out, bool *wait_ready) {
    vbx_ctx *ctx = s->ctx;
    const int slot = (int)(s->uploads & 1);
    const size_t bytes = n * s->channels * sample_src_bytes(s->fmt);
    if (bytes <= s->stage_bytes) {
        // through pinned staging, on the context's stream: behind the slot's last reader by stream order; the caller's block has
        // been read when the host copy returns (the staging buffer's previous upload, two pushes ago, has long left it)
        VBX_HIP(ctx, hipEventSynchronize(s->staged[slot]));
        std::memcpy(s->stage[slot], block, bytes);
        VBX_HIP(ctx, hipMemcpyAsync(s->raw[slot], s->stage[slot], bytes, hipMemcpyHostToDevice, ctx->stream));
        VBX_HIP(ctx, hipEventRecord(s->staged[slot], ctx->stream));
    } else {                                              // on the copy stream, behind the slot's last reader
        VBX_HIP(ctx, hipStreamWaitEvent(ctx->copy, s->freed[slot], 0));
        VBX_HIP(ctx, hipMemcpyAsync(s->raw[slot], block, bytes, hipMemcpyHostToDevice, ctx->copy));
        VBX_HIP(ctx, hipEventRecord(s->ready[slot], ctx->copy));
        VBX_HIP(ctx, hipStreamWaitEvent(ctx->stream, s->ready[slot], 0));
        *wait_ready = true;
    }
    *raw = s->raw[slot];
    *slot_out = slot;
    s->uploads++;
    return VBX_SUCCESS;
}

static int session_push_impl(vbx_session *s, const char *fn, const void *block, bool on_device, size_t n, double *out_records,
                             size_t record_ld, int32_t *status3, size_t status_ld, const vbx_pitch_track_outputs *h_out, size_t *h_n) {
    if (!s) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null session");
    vbx_ctx *ctx = s->ctx;
    if (h_n) *h_n = 0;
    VBX_REQUIRE_FN(ctx, fn, s->n_sel == 0, "the session was opened with vbx_session_open_channels: push with vbx_session_push_channels");
    if (n == 0) return VBX_SUCCESS;
    VBX_REQUIRE_FN(ctx, fn, block != nullptr, "null block");
    VBX_REQUIRE_FN(ctx, fn, n <= s->max_block, "the block is larger than the session's max_block_sample_frames");
    VBX_REQUIRE_FN(ctx, fn, !on_device || s->fmt == VBX_SAMPLE_PCM24 || (uintptr_t)block % sample_src_bytes(s->fmt) == 0, "the block needs its type's alignment");
    vbx_session_plan_t pl{};
    if (vbx_session_plan(s->consumed, s->utt_frame, n, s->frame_len, s->stride, &pl) != VBX_SUCCESS)
        return fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad session plan");
    const size_t nf = pl.hi - pl.lo;
    bool want_peak = false;
    if (nf) {
        VBX_REQUIRE_FN(ctx, fn, out_records != nullptr, "null argument");
        VBX_REQUIRE_FN(ctx, fn, ((uintptr_t)out_records & 15) == 0, "records must be 16-byte aligned");
        VBX_REQUIRE_FN(ctx, fn, record_ld >= s->rec && record_ld % 2 == 0, "record_ld must be even and >= vbx_record_doubles(params)");
        VBX_REQUIRE_FN(ctx, fn, status3 == nullptr || status_ld >= nf, "status_ld must be >= the frames the push delivers");
        if (s->have_track) {
            VBX_REQUIRE_FN(ctx, fn, h_out != nullptr && h_out->cand != nullptr && h_out->count != nullptr, "the tracked form needs h_outputs->cand and ->count");
            VBX_REQUIRE_FN(ctx, fn, s->track.path.silence_threshold == 0.0 || h_out->peak != nullptr, "a silence_threshold needs h_outputs->peak");
            VBX_REQUIRE_FN(ctx, fn, h_out->index == nullptr, "h_outputs->index must be NULL: the caller runs the path (vbx_pitch_path_f64)");
            want_peak = h_out->peak != nullptr;
        }
    }
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const size_t sf_bytes = s->channels * sample_src_bytes(s->fmt);
    const void *raw = block;
    int slot = -1;
    bool wait_ready = false;
    if (!on_device) {
        int rc = session_upload(s, block, n, &raw, &slot, &wait_ready);
        if (rc != VBX_SUCCESS) return rc;
    }
    // the other carry buffer: from sample frame nb on -- what this push's analysis reads first, or, when it completes no frame, what
    // a later one may.  (stride > frame_len: nb may lie beyond the carried samples, inside the block; the gap's samples are dropped)
    const size_t c = s->consumed, nb = nf ? pl.read_from : pl.keep_from;
    const size_t from_old = nb < c ? nb : c, skip = nb > c ? nb - c : 0;
    { Prof p(ctx, k_ingest_names[sample_name_slot(s->fmt)]);
      launch_session_ingest(ctx->stream, s->fmt, s->carry[s->cur], from_old - s->base, c - from_old,
                            static_cast<const char *>(raw) + skip * sf_bytes, n - skip, s->channels, s->channel, s->carry[s->cur ^ 1]); }
    if (slot >= 0) VBX_HIP(ctx, hipEventRecord(s->freed[slot], ctx->stream));
    s->cur ^= 1; s->base = nb; s->consumed = c + n; s->keep_from = pl.keep_from;
    auto bail = [&](int code) { if (wait_ready) hipEventSynchronize(s->ready[slot]); return code; };      // the block is not read after the call returns
    if (nf) {
        const size_t n_an = pl.warm + nf;
        int rc = session_analyze(s, fn, n_an, want_peak);
        if (rc != VBX_SUCCESS) return bail(rc);
        // the push continues an utterance: the tracker goes on from the true state, the formant row of the last frame delivered
        if (pl.continues_prev && s->p.formant_order) {
            rc = vbx_internal_track_stitch(ctx, nullptr, reinterpret_cast<vbx_resonance *>(s->c_rec + 2), n_an, s->ld_c, pl.warm, n_an, s->state, nullptr);
            if (rc != VBX_SUCCESS) return bail(rc);
        }
        session_deliver_t d{};
        d.src = s->c_rec; d.src_ld = s->ld_c; d.row0 = pl.warm; d.rows = nf; d.c0 = s->have_track ? 2 : 0; d.c1 = s->rec;
        d.dst = out_records; d.dst_ld = record_ld;
        d.src_st = s->c_st; d.src_n = n_an; d.dst_st = status3; d.dst_st_ld = status_ld;
        if (s->have_track) {
            d.src_cand = reinterpret_cast<const double *>(s->c_cand); d.dst_cand = reinterpret_cast<double *>(h_out->cand); d.kmax = s->track.kmax;
            d.src_count = s->c_count; d.dst_count = h_out->count;
            if (want_peak) { d.src_peak = s->c_peak; d.dst_peak = h_out->peak; }
        }
        if (s->p.formant_order) { d.state = s->state; d.n_state = 2 * s->p.n_est; }
        { Prof p(ctx, "session_deliver"); launch_session_deliver(ctx->stream, d); }
        ctx->last_track.res = nullptr;                    // the chunk-local rows are no track of the caller's: nothing to stitch
        ctx->last_track.n_est = 0;
        s->frames += nf;
    }
    if (s->bound) {
        // the contour: the online path over the push's own rows of the session-owned lists, behind session_deliver (a push that
        // completes no frame still reports: n = 0 and what is pending)
        const size_t w = nf ? pl.warm : 0;
        int rc = path_stream_launch(s->path, fn, s->c_cand + w * s->track.kmax, s->c_count + w, s->c_st + w, want_peak ? s->c_peak + w : nullptr,
                                    nf, 0, s->p_out, s->p_ld, s->p_index, s->p_forced, s->p_commit);
        if (rc != VBX_SUCCESS) return bail(rc);
    }
    int rc = check_launch(ctx, fn);
    if (rc != VBX_SUCCESS) return bail(rc);
    if (h_n) *h_n = nf;
    if (wait_ready) VBX_HIP(ctx, hipEventSynchronize(s->ready[slot]));     // the last byte of h_block has been read
    return VBX_SUCCESS;
}

int vbx_session_push(vbx_session *s, const void *h_block, size_t n_sample_frames, double *out_records, size_t record_ld, int32_t *status3,
                     size_t status_ld, const vbx_pitch_track_outputs *h_outputs, size_t *h_n_frames) {
    return session_push_impl(s, __func__, h_block, false, n_sample_frames, out_records, record_ld, status3, status_ld, h_outputs, h_n_frames);
}

int vbx_session_push_device(vbx_session *s, const void *d_block, size_t n_sample_frames, double *out_records, size_t record_ld,
                            int32_t *status3, size_t status_ld, const vbx_pitch_track_outputs *h_outputs, size_t *h_n_frames) {
    return session_push_impl(s, __func__, d_block, true, n_sample_frames, out_records, record_ld, status3, status_ld, h_outputs, h_n_frames);
}

int vbx_session_mark_utterance(vbx_session *s) {
    if (!s) return fail(nullptr, VBX_E_INVALID, "vbx_session_mark_utterance: null session");
    s->utt_frame = vbx_frame_count(s->consumed, s->frame_len, s->stride);
    if (s->bound && s->n_sel) {                           // every channel's contour, in one launch
        VBX_HIP(s->ctx, hipSetDevice(s->ctx->device));
        return path_stream_launch_all(s->paths.data(), s->n_sel, __func__, nullptr, nullptr, nullptr, nullptr, 0, 0, 1, s->p_outs.data(), s->p_ld);
    }
    if (s->bound) {                                       // the rest of the contour now, not when the next frame arrives
        VBX_HIP(s->ctx, hipSetDevice(s->ctx->device));
        return path_stream_launch(s->path, __func__, nullptr, nullptr, nullptr, nullptr, 0, 1, s->p_out, s->p_ld, s->p_index, s->p_forced,
                                  s->p_commit);
    }
    return VBX_SUCCESS;
}

int vbx_session_path_bind(vbx_session *s, double peak_ref, size_t max_pending, vbx_pitch *out_path, size_t path_ld, int32_t *out_index,
                          uint8_t *out_forced, vbx_path_commit *d_commit) {
    if (!s) return fail(nullptr, VBX_E_INVALID, "vbx_session_path_bind: null session");
    vbx_ctx *ctx = s->ctx;
    VBX_REQUIRE(ctx, s->n_sel == 0, "the session was opened with vbx_session_open_channels");
    VBX_REQUIRE(ctx, s->have_track, "the session was opened without h_track: it has no candidate lists");
    VBX_REQUIRE(ctx, out_path != nullptr && d_commit != nullptr, "null out_path or d_commit");
    VBX_REQUIRE(ctx, path_ld >= 2, "path_ld must be >= 2");
    if (s->bound) {                                       // between pushes: other destinations, the same path
        VBX_REQUIRE(ctx, max_pending == s->path->max_pending && std::memcmp(&peak_ref, &s->path->peak_ref, sizeof(double)) == 0,
                    "a bound session keeps its peak_ref and max_pending (vbx_session_reset drops the binding)");
    } else {
        VBX_REQUIRE(ctx, s->consumed == 0, "bind before the first push or after vbx_session_reset");
        vbx_pitch_path_params path = s->track.path;
        if (path.time_step == 0.0) path.time_step = (double)s->stride / s->p.sample_rate;
        // the path of before a reset (its state was reset with the session) serves again when nothing about it changes
        const bool same = s->path != nullptr && s->path->max_pending == max_pending && std::memcmp(&peak_ref, &s->path->peak_ref, sizeof(double)) == 0;
        if (!same) {
            vbx_path_stream *ps = nullptr;
            int rc = path_stream_open(ctx, __func__, s->track.kmax, path, peak_ref, max_pending, &ps);
            if (rc != VBX_SUCCESS) return rc;
            if (s->path) path_stream_free(s->path);
            s->path = ps;
        }
        s->bound = true;
    }
    s->p_out = out_path; s->p_ld = path_ld; s->p_index = out_index; s->p_forced = out_forced; s->p_commit = d_commit;
    return VBX_SUCCESS;
}

int vbx_session_path_bind_channels(vbx_session *s, double peak_ref, size_t max_pending, const vbx_channel_path_outputs *h_out, size_t path_ld) {
    if (!s) return fail(nullptr, VBX_E_INVALID, "vbx_session_path_bind_channels: null session");
    vbx_ctx *ctx = s->ctx;
    VBX_REQUIRE(ctx, s->n_sel != 0, "the session was opened with vbx_session_open: bind with vbx_session_path_bind");
    VBX_REQUIRE(ctx, s->have_track, "the session was opened without h_track: it has no candidate lists");
    VBX_REQUIRE(ctx, h_out != nullptr, "null outputs");
    for (size_t k = 0; k < s->n_sel; k++) VBX_REQUIRE(ctx, h_out[k].out_path != nullptr && h_out[k].d_commit != nullptr, "null out_path or d_commit");
    VBX_REQUIRE(ctx, path_ld >= 2, "path_ld must be >= 2");
    const bool have = !s->paths.empty();
    const bool same = have && s->paths[0]->max_pending == max_pending && std::memcmp(&peak_ref, &s->paths[0]->peak_ref, sizeof(double)) == 0;
    if (s->bound) {                                       // between pushes: other destinations, the same paths
        VBX_REQUIRE(ctx, same, "a bound session keeps its peak_ref and max_pending (vbx_session_reset drops the binding)");
    } else {
        VBX_REQUIRE(ctx, s->consumed == 0, "bind before the first push or after vbx_session_reset");
        if (!same) {                                      // (the paths of before a reset serve again when nothing about them changes)
            vbx_pitch_path_params path = s->track.path;
            if (path.time_step == 0.0) path.time_step = (double)s->stride / s->p.sample_rate;
            std::vector<vbx_path_stream *> fresh;
            for (size_t k = 0; k < s->n_sel; k++) {
                vbx_path_stream *ps = nullptr;
                int rc = path_stream_open(ctx, __func__, s->track.kmax, path, peak_ref, max_pending, &ps);
                if (rc != VBX_SUCCESS) { for (vbx_path_stream *q : fresh) path_stream_free(q); return rc; }
                fresh.push_back(ps);
            }
            for (vbx_path_stream *q : s->paths) path_stream_free(q);
            s->paths = fresh;
        }
        s->bound = true;
    }
    s->p_outs.assign(h_out, h_out + s->n_sel);
    s->p_ld = path_ld;
    return VBX_SUCCESS;
}

int vbx_session_reset(vbx_session *s) {
    if (!s) return fail(nullptr, VBX_E_INVALID, "vbx_session_reset: null session");
    // (nothing is queued: the next ingest keeps nothing of the carry, and a first push of an utterance stitches from no state)
    s->consumed = 0; s->utt_frame = 0; s->frames = 0; s->base = 0; s->keep_from = 0;
    if (s->path) {                                        // the path's state goes, and the binding with it
        s->bound = false;
        return path_stream_reset(s->path);
    }
    if (!s->paths.empty()) {
        s->bound = false;
        for (vbx_path_stream *ps : s->paths) { int rc = path_stream_reset(ps); if (rc != VBX_SUCCESS) return rc; }
    }
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
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);                 // the session's buffers may still be read by queued work
    if (s->ctx->side) hipStreamSynchronize(s->ctx->side);
    if (s->ctx->trk) hipStreamSynchronize(s->ctx->trk);
    if (s->ctx->copy) hipStreamSynchronize(s->ctx->copy);
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

// ---- every selected channel from one session (header: "live sessions over several channels") ----------------------------------

static int session_push_channels_impl(vbx_session *s, const char *fn, const void *block, bool on_device, size_t n,
                                      const vbx_channel_outputs *h_out, size_t record_ld, size_t status_ld, size_t *h_n) {
    if (!s) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null session");
    vbx_ctx *ctx = s->ctx;
    if (h_n) *h_n = 0;
    VBX_REQUIRE_FN(ctx, fn, s->n_sel != 0, "the session was opened with vbx_session_open: push with vbx_session_push");
    if (n == 0) return VBX_SUCCESS;
    VBX_REQUIRE_FN(ctx, fn, block != nullptr, "null block");
    VBX_REQUIRE_FN(ctx, fn, n <= s->max_block, "the block is larger than the session's max_block_sample_frames");
    VBX_REQUIRE_FN(ctx, fn, !on_device || s->fmt == VBX_SAMPLE_PCM24 || (uintptr_t)block % sample_src_bytes(s->fmt) == 0, "the block needs its type's alignment");
    const size_t K = s->n_sel;
    vbx_session_channels_plan_t cp{};
    if (vbx_session_channels_plan(s->consumed, s->utt_frame, n, s->frame_len, s->stride, sample_out_bytes(s->fmt), K, &cp, s->seg.data()) != VBX_SUCCESS)
        return fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad session plan");
    const vbx_session_plan_t &pl = cp.push;
    const size_t nf = pl.hi - pl.lo;
    bool want_peak = false;
    VBX_REQUIRE_FN(ctx, fn, h_out != nullptr, "null outputs");
    if (nf) {
        VBX_REQUIRE_FN(ctx, fn, record_ld >= s->rec && record_ld % 2 == 0, "record_ld must be even and >= vbx_record_doubles(params)");
        for (size_t k = 0; k < K; k++) {
            VBX_REQUIRE_FN(ctx, fn, h_out[k].records != nullptr, "null argument");
            VBX_REQUIRE_FN(ctx, fn, h_out[k].status3 == nullptr || status_ld >= nf, "status_ld must be >= the frames the push delivers");
            VBX_REQUIRE_FN(ctx, fn, ((uintptr_t)h_out[k].records & 15) == 0, "records must be 16-byte aligned");
            for (size_t j = 0; j < k; j++) {              // [n, record_ld] each
                const uintptr_t a = (uintptr_t)h_out[j].records, b = (uintptr_t)h_out[k].records, len = nf * record_ld * sizeof(double);
                VBX_REQUIRE_FN(ctx, fn, a + len <= b || b + len <= a, "the channels' records overlap");
            }
            if (s->have_track) {
                const vbx_pitch_track_outputs *o = h_out[k].outputs;
                VBX_REQUIRE_FN(ctx, fn, o != nullptr && o->cand != nullptr && o->count != nullptr, "the tracked form needs outputs->cand and ->count");
                VBX_REQUIRE_FN(ctx, fn, s->track.path.silence_threshold == 0.0 || o->peak != nullptr, "a silence_threshold needs outputs->peak");
                VBX_REQUIRE_FN(ctx, fn, o->index == nullptr, "outputs->index must be NULL: the caller runs the path (vbx_pitch_path_f64)");
                want_peak = want_peak || o->peak != nullptr;
            }
        }
    }
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const size_t sf_bytes = s->channels * sample_src_bytes(s->fmt);
    const void *raw = block;
    int slot = -1;
    bool wait_ready = false;
    if (!on_device) {                                     // ONE upload, whatever n_sel
        int rc = session_upload(s, block, n, &raw, &slot, &wait_ready);
        if (rc != VBX_SUCCESS) return rc;
    }
    // the other carry buffer, every plane from sample frame cp.base on (session_push_impl's rule, per plane)
    const size_t c = s->consumed, from_old = c - cp.keep, skip = cp.base > c ? cp.base - c : 0;
    { Prof p(ctx, k_ingest_all_names[sample_name_slot(s->fmt)]);
      launch_session_ingest_all(ctx->stream, s->fmt, s->carry[s->cur], s->plane_ld, from_old - s->base, cp.keep,
                                static_cast<const char *>(raw) + skip * sf_bytes, n - skip, s->channels, s->sel, K, s->carry[s->cur ^ 1], cp.plane_ld); }
    if (slot >= 0) VBX_HIP(ctx, hipEventRecord(s->freed[slot], ctx->stream));
    s->cur ^= 1; s->base = cp.base; s->plane_ld = cp.plane_ld; s->consumed = c + n; s->keep_from = pl.keep_from;
    auto bail = [&](int code) { if (wait_ready) hipEventSynchronize(s->ready[slot]); return code; };      // the block is not read after the call returns
    if (nf) {
        const size_t m = cp.frames, Q = cp.plane_frames, n_call = cp.call_frames;
        int rc = session_analyze(s, fn, n_call, want_peak);
        if (rc != VBX_SUCCESS) return bail(rc);
        // the push continues an utterance: every channel's tracker goes on from its true state, the formant row of its last frame delivered
        if (pl.continues_prev && s->p.formant_order) {
            const auto &lt = ctx->last_track;
            if (lt.res == nullptr || lt.out != reinterpret_cast<res_t *>(s->c_rec + 2) || lt.F != (long)n_call)
                return bail(fail(ctx, VBX_E_RUNTIME, std::string(fn) + ": the frame loop left no track to stitch"));
            { Prof p(ctx, "tracker_stitch_all");
              launch_tracker_stitch_all(ctx->stream, lt.res, lt.F, VBX_MAX_RESONANCES, lt.cnt, lt.n_est, lt.st, lt.out, lt.out_ld, (long)Q, (long)pl.warm,
                                        (long)m, s->state, (long)K); }
        }
        session_deliver_all_t d{};
        d.src = s->c_rec; d.src_ld = s->ld_c; d.plane_frames = Q; d.row0 = pl.warm; d.rows = nf; d.c0 = s->have_track ? 2 : 0; d.c1 = s->rec;
        d.dst_ld = record_ld;
        d.src_st = s->c_st; d.src_n = n_call; d.dst_st_ld = status_ld;
        if (s->have_track) {
            d.src_cand = reinterpret_cast<const double *>(s->c_cand); d.kmax = s->track.kmax;
            d.src_count = s->c_count;
            d.src_peak = want_peak ? s->c_peak : nullptr;
        }
        if (s->p.formant_order) { d.state = s->state; d.n_state = 2 * s->p.n_est; }
        for (size_t k = 0; k < K; k++) {
            d.ch[k].rec = h_out[k].records; d.ch[k].st = h_out[k].status3;
            if (s->have_track) {
                const vbx_pitch_track_outputs *o = h_out[k].outputs;
                d.ch[k].cand = reinterpret_cast<double *>(o->cand); d.ch[k].count = o->count; d.ch[k].peak = o->peak;
            }
        }
        { Prof p(ctx, "session_deliver_all"); launch_session_deliver_all(ctx->stream, d, K); }
        ctx->last_track.res = nullptr;                    // the chunk-local rows are no track of the caller's: nothing to stitch
        ctx->last_track.n_est = 0;
        s->frames += nf;
    }
    if (s->bound) {
        // the contours: every channel's online path over its own rows of the session-owned lists, in one launch behind
        // session_deliver_all (a push that completes no frame still reports: n = 0 and what is pending)
        const size_t w = nf ? pl.warm : 0;
        int rc = path_stream_launch_all(s->paths.data(), K, fn, s->c_cand + w * s->track.kmax, s->c_count + w, s->c_st + w,
                                        want_peak ? s->c_peak + w : nullptr, cp.plane_frames, nf, 0, s->p_outs.data(), s->p_ld);
        if (rc != VBX_SUCCESS) return bail(rc);
    }
    int rc = check_launch(ctx, fn);
    if (rc != VBX_SUCCESS) return bail(rc);
    if (h_n) *h_n = nf;
    if (wait_ready) VBX_HIP(ctx, hipEventSynchronize(s->ready[slot]));     // the last byte of h_block has been read
    return VBX_SUCCESS;
}

int vbx_session_push_channels(vbx_session *s, const void *h_block, size_t n_sample_frames, const vbx_channel_outputs *h_out, size_t record_ld,
                              size_t status_ld, size_t *h_n_frames) {
    return session_push_channels_impl(s, __func__, h_block, false, n_sample_frames, h_out, record_ld, status_ld, h_n_frames);
}

int vbx_session_push_channels_device(vbx_session *s, const void *d_block, size_t n_sample_frames, const vbx_channel_outputs *h_out,
                                     size_t record_ld, size_t status_ld, size_t *h_n_frames) {
    return session_push_channels_impl(s, __func__, d_block, true, n_sample_frames, h_out, record_ld, status_ld, h_n_frames);
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
