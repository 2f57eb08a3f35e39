// vbx_api_pool.hip -- a session pool: many independent live streams on one context, analysed from one upload and one launch chain
// per tick (vbx_pool_*).
#include "vbx_ctx.hpp"

#include <cstring>
#include <string>
#include <vector>

using namespace vbx;

// ---- a pool of live streams (header: "a pool of live streams") ---------------------------------

extern "C" {

static const char *const k_pool_ingest_names[9] = {"", "pool_ingest_pcm16", "pool_ingest_pcm24", "pool_ingest_pcm32", "pool_ingest_f32",
                                                   "pool_ingest_f64", "pool_ingest_u8", "pool_ingest_ulaw", "pool_ingest_alaw"};      // by sample_name_slot
static_assert(UNPACK_PCM16 == VBX_SAMPLE_PCM16 && UNPACK_F64 == VBX_SAMPLE_F64 && UNPACK_U8 == VBX_SAMPLE_U8 && UNPACK_ULAW == VBX_SAMPLE_ULAW &&
              UNPACK_ALAW == VBX_SAMPLE_ALAW, "the ingest kernels take the header's formats");
static_assert(sizeof(pool_entry_t) % 16 == 0, "the blocks behind the table start on a 16-byte boundary");

// One slot's timeline: what a one-channel session keeps between pushes.
struct pool_slot_t {
    size_t consumed = 0, utt_frame = 0, frames = 0;
    size_t keep_from = 0;                                 // the sample frame element 0 of the slot's current carry region holds
    int cur = 0;                                          // which of its two carry regions is current
    uint64_t seen = 0;                                    // the last tick that listed the slot
};

// max_streams slots that share a format, a frame shape and a parameter set.  The pool owns everything a tick writes before the
// caller's arrays: the carry regions (slot k's two regions at elements (2 k + b) * carry_cap), the tick's plane, the two pinned
// staging buffers with their raw device slots (table first, the gathered blocks behind it), the chunk-local records / status rows /
// lists of the largest frame-loop call and the state rows.  The frame loop's own workspaces are the context's.
struct vbx_pool {
    vbx_ctx *ctx = nullptr;
    int fmt = 0;
    size_t frame_len = 0, stride = 0, max_streams = 0, max_block = 0, max_tick = 0;
    vbx_analysis_params p{}; vbx_analysis_ext ext{}; vbx_pitch_track_params track{};
    bool have_ext = false, have_track = false;
    size_t rec = 0, ld_c = 0, call_max = 0, plane_cap = 0, carry_cap = 0, raw_bytes = 0;
    std::vector<pool_slot_t> slots;
    uint64_t ticks = 0;                                   // vbx_pool_push calls so far (the duplicate check's stamp)
    size_t uploads = 0;                                   // ticks that uploaded: upload k stages through slot k & 1
    void *carry = nullptr, *plane = nullptr;
    void *stage[2] = {nullptr, nullptr}, *raw[2] = {nullptr, nullptr};
    hipEvent_t staged[2] = {nullptr, nullptr};
    double *c_rec = nullptr; int32_t *c_st = nullptr;
    vbx_pitch *c_cand = nullptr; int32_t *c_count = nullptr; double *c_peak = nullptr;
    double *state = nullptr;                              // max_streams rows of 2 * VBX_FORMANT_SLOTS doubles
    // a tick's host scratch, kept between ticks so that none allocates
    std::vector<size_t> h_consumed, h_utt, h_new;
    std::vector<vbx_pool_plan_row> rows;
    std::vector<pool_entry_t> tab;
    std::vector<int64_t> seg;
};

static void pool_free(vbx_pool *q) {
    for (int i = 0; i < 2; i++) {
        if (q->stage[i]) hipHostFree(q->stage[i]);
        if (q->raw[i]) hipFree(q->raw[i]);
        if (q->staged[i]) hipEventDestroy(q->staged[i]);
    }
    if (q->carry) hipFree(q->carry);
    if (q->plane) hipFree(q->plane);
    if (q->c_rec) hipFree(q->c_rec);
    if (q->c_st) hipFree(q->c_st);
    if (q->c_cand) hipFree(q->c_cand);
    if (q->c_count) hipFree(q->c_count);
    if (q->c_peak) hipFree(q->c_peak);
    if (q->state) hipFree(q->state);
    delete q;
}

// the frame loop on frames [0, n) of the pool's plane into the chunk-local buffers, every entry a segment (q->seg)
static int pool_analyze(vbx_pool *q, const char *fn, size_t n, bool want_peak) {
    vbx_pitch_track_outputs to{};
    to.cand = q->c_cand; to.count = q->c_count; to.peak = want_peak ? q->c_peak : nullptr;
    return analyze_ex(q->ctx, fn, frames_t(q->plane, sample_plane_kind(q->fmt)), n, q->frame_len, q->stride, &q->p,
                      q->have_ext ? &q->ext : nullptr, q->have_track ? &q->track : nullptr, q->seg.data(), q->seg.size(), q->c_rec, q->ld_c,
                      q->c_st, q->have_track ? &to : nullptr, true);
}

int vbx_pool_open(vbx_ctx *ctx, const vbx_host_audio *h_fmt, size_t frame_len, size_t stride, const vbx_analysis_params *h_p,
                  const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, size_t max_streams, size_t max_block,
                  size_t max_tick, vbx_pool **out) {
    const char *fn = __func__;
    if (!ctx) return fail(nullptr, VBX_E_INVALID, "vbx_pool_open: null context");
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    *out = nullptr;
    VBX_REQUIRE(ctx, h_fmt != nullptr && h_p != nullptr, "null argument");
    VBX_REQUIRE(ctx, sample_format_ok(h_fmt->format), "unknown sample format");
    VBX_REQUIRE(ctx, h_fmt->channels == 1 && h_fmt->channel == 0, "a pool's streams are mono: channels must be 1 and channel 0");
    VBX_REQUIRE(ctx, h_fmt->reserved == 0 && h_fmt->chunk_frames == 0, "reserved and chunk_frames must be 0");
    VBX_REQUIRE(ctx, max_streams >= 1, "max_streams must be >= 1");
    VBX_REQUIRE(ctx, max_block >= 1 && max_tick >= max_block, "need 1 <= max_block_sample_frames <= max_tick_sample_frames");
    VBX_REQUIRE(ctx, frame_len >= 1 && frame_len <= VBX_MAX_FRAME_LEN, "frame_len must be in [1, VBX_MAX_FRAME_LEN]: longer frames take one vbx_session per stream");
    VBX_REQUIRE(ctx, stride >= 1 && stride <= ((size_t)1 << 40), "stride must be in [1, 2^40]");
    VBX_REQUIRE(ctx, max_streams <= 0x7fffffffull && max_tick <= ((size_t)1 << 40), "max_streams or max_tick_sample_frames too large");
    VBX_REQUIRE(ctx, !h_p->formant_order || (h_p->n_est >= 1 && h_p->n_est <= VBX_FORMANT_SLOTS), "n_est must be in [1, 6]");
    const size_t call_max = pool_max_call_frames(frame_len, stride, max_streams, max_tick);
    VBX_REQUIRE(ctx, call_max <= 0x7fffffffull, "too many frames for one launch");
    if (h_track) {
        vbx_pitch_path_params path = h_track->path;
        if (path.time_step == 0.0) path.time_step = (double)stride / h_p->sample_rate;
        int rc = check_pitch_path(ctx, fn, path, call_max, h_track->kmax, true, nullptr, 0);
        if (rc != VBX_SUCCESS) return rc;
    }
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    vbx_pool *q = new vbx_pool();
    q->ctx = ctx; q->fmt = h_fmt->format;
    q->frame_len = frame_len; q->stride = stride; q->max_streams = max_streams; q->max_block = max_block; q->max_tick = max_tick;
    q->p = *h_p;
    if (h_ext) { q->ext = *h_ext; q->have_ext = true; }
    if (h_track) { q->track = *h_track; q->have_track = true; }
    q->rec = vbx_record_doubles_ex(h_p, h_ext);
    q->ld_c = q->rec + (q->rec & 1);
    q->call_max = call_max;
    q->plane_cap = call_max * stride + frame_len;
    q->carry_cap = (pool_carry_samples(frame_len, stride) + 7) & ~(size_t)7;      // whole 16-byte groups for every element type
    const size_t e_max = max_streams < max_tick ? max_streams : max_tick;         // entries that hold a sample
    q->raw_bytes = e_max * sizeof(pool_entry_t) + max_tick * sample_src_bytes(q->fmt) + 16 * e_max;
    q->slots.resize(max_streams);
    q->h_consumed.reserve(max_streams); q->h_utt.reserve(max_streams); q->h_new.reserve(max_streams);
    q->rows.reserve(max_streams); q->tab.reserve(e_max); q->seg.reserve(max_streams);
    const size_t ob = sample_out_bytes(q->fmt), kmax = h_track ? h_track->kmax : 0, nbuf = call_max;
#define POOL_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { hipStreamSynchronize(ctx->stream); pool_free(q); \
        return fail(ctx, VBX_E_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)
    POOL_HIP(hipMalloc(&q->carry, 2 * max_streams * q->carry_cap * ob));    // (hipMalloc: 256-byte aligned bases)
    POOL_HIP(hipMemsetAsync(q->carry, 0, 2 * max_streams * q->carry_cap * ob, ctx->stream));
    POOL_HIP(hipMalloc(&q->plane, q->plane_cap * ob));
    POOL_HIP(hipMemsetAsync(q->plane, 0, q->plane_cap * ob, ctx->stream));
    for (int i = 0; i < 2; i++) {
        POOL_HIP(hipHostMalloc(&q->stage[i], q->raw_bytes, hipHostMallocDefault));
        POOL_HIP(hipMalloc(&q->raw[i], q->raw_bytes));
        POOL_HIP(hipEventCreateWithFlags(&q->staged[i], hipEventDisableTiming));
    }
    POOL_HIP(hipMalloc((void **)&q->c_rec, nbuf * q->ld_c * sizeof(double)));
    POOL_HIP(hipMalloc((void **)&q->c_st, 3 * nbuf * sizeof(int32_t)));
    if (h_track) {
        POOL_HIP(hipMalloc((void **)&q->c_cand, nbuf * kmax * sizeof(vbx_pitch)));
        POOL_HIP(hipMalloc((void **)&q->c_count, nbuf * sizeof(int32_t)));
        POOL_HIP(hipMalloc((void **)&q->c_peak, nbuf * sizeof(double)));
    }
    POOL_HIP(hipMalloc((void **)&q->state, max_streams * 2 * VBX_FORMANT_SLOTS * sizeof(double)));
    POOL_HIP(hipMemsetAsync(q->state, 0, max_streams * 2 * VBX_FORMANT_SLOTS * sizeof(double), ctx->stream));
#undef POOL_HIP
    // the largest shape a tick can ask for, on the zeroed plane, with as many segments as a tick can have entries: the context's
    // workspaces and tables are as large as they will ever have to be, and what only the frame loop's parts know is rejected here
    const size_t per = call_max / e_max;
    for (size_t k = 0; k < e_max; k++) q->seg.push_back((int64_t)(k * per));
    int rc = pool_analyze(q, fn, nbuf, true);
    if (rc == VBX_SUCCESS) rc = check_launch(ctx, fn);
    q->seg.clear();
    ctx->last_track.res = nullptr;                        // the chunk-local rows are no track of the caller's
    ctx->last_track.n_est = 0;
    if (rc != VBX_SUCCESS) { const std::string why = ctx->last_error; hipStreamSynchronize(ctx->stream); vbx_sync(ctx); pool_free(q); return fail(ctx, rc, why); }
    *out = q;
    return VBX_SUCCESS;
}

static int pool_push_impl(vbx_pool *q, const char *fn, const vbx_pool_entry *h_entries, bool on_device, size_t n_entries, double *out_records,
                          size_t record_ld, int32_t *status3, size_t status_ld, const vbx_pitch_track_outputs *h_out, vbx_pool_rows *h_rows,
                          size_t *h_total) {
    if (!q) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null pool");
    vbx_ctx *ctx = q->ctx;
    if (h_total) *h_total = 0;
    if (n_entries == 0) return VBX_SUCCESS;
    VBX_REQUIRE_FN(ctx, fn, h_entries != nullptr, "null entries");
    // ---- everything that can be refused, before anything is queued or any slot changes
    const size_t sb = sample_src_bytes(q->fmt), ob = sample_out_bytes(q->fmt);
    const uint64_t stamp = ++q->ticks;
    size_t sum = 0, n_live = 0;
    const char *why = nullptr;
    for (size_t i = 0; i < n_entries && !why; i++) {
        const vbx_pool_entry &e = h_entries[i];
        if (e.stream < 0 || (size_t)e.stream >= q->max_streams) { why = "a stream outside [0, max_streams)"; break; }
        pool_slot_t &s = q->slots[(size_t)e.stream];
        if (s.seen == stamp) { why = "a stream is listed twice in one tick"; break; }
        s.seen = stamp;
        if (e.n_sample_frames == 0) continue;
        if (e.block == nullptr) why = "null block";
        else if (e.n_sample_frames > q->max_block) why = "a block is larger than the pool's max_block_sample_frames";
        else if (e.n_sample_frames > q->max_tick - sum) why = "the tick's blocks are larger than the pool's max_tick_sample_frames";
        else if (on_device && q->fmt != VBX_SAMPLE_PCM24 && (uintptr_t)e.block % sb != 0) why = "a block needs its type's alignment";
        sum += e.n_sample_frames;
        n_live++;
    }
    VBX_REQUIRE_FN(ctx, fn, why == nullptr, why);
    q->h_consumed.resize(n_entries); q->h_utt.resize(n_entries); q->h_new.resize(n_entries); q->rows.resize(n_entries);
    for (size_t i = 0; i < n_entries; i++) {
        const pool_slot_t &s = q->slots[(size_t)h_entries[i].stream];
        q->h_consumed[i] = s.consumed; q->h_utt[i] = s.utt_frame; q->h_new[i] = h_entries[i].n_sample_frames;
    }
    size_t total = 0, call_frames = 0;
    if (vbx_pool_plan(q->h_consumed.data(), q->h_utt.data(), q->h_new.data(), n_entries, q->frame_len, q->stride, q->rows.data(), &total,
                      &call_frames) != VBX_SUCCESS)
        return fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad pool plan");
    VBX_REQUIRE_FN(ctx, fn, call_frames <= q->call_max, "the tick's frame-loop call is larger than the pool was opened for");
    bool want_peak = false;
    if (total) {
        VBX_REQUIRE_FN(ctx, fn, out_records != nullptr, "null argument");
        VBX_REQUIRE_FN(ctx, fn, ((uintptr_t)out_records & 15) == 0, "records must be 16-byte aligned");
        VBX_REQUIRE_FN(ctx, fn, record_ld >= q->rec && record_ld % 2 == 0, "record_ld must be even and >= vbx_record_doubles(params)");
        VBX_REQUIRE_FN(ctx, fn, status3 == nullptr || status_ld >= total, "status_ld must be >= the rows the tick delivers");
        if (q->have_track) {
            VBX_REQUIRE_FN(ctx, fn, h_out != nullptr && h_out->cand != nullptr && h_out->count != nullptr, "the tracked form needs h_outputs->cand and ->count");
            VBX_REQUIRE_FN(ctx, fn, q->track.path.silence_threshold == 0.0 || h_out->peak != nullptr, "a silence_threshold needs h_outputs->peak");
            VBX_REQUIRE_FN(ctx, fn, h_out->index == nullptr, "h_outputs->index must be NULL: the caller runs the path (vbx_pitch_path_f64)");
            want_peak = h_out->peak != nullptr;
        }
    }
    for (size_t i = 0; i < n_entries; i++) if (h_rows) { h_rows[i].row_start = q->rows[i].row_start; h_rows[i].n_rows = q->rows[i].n_rows; }
    if (h_total) *h_total = total;
    if (n_live == 0) return VBX_SUCCESS;                  // nothing but empty blocks: nothing is queued

    // ---- the table, and in the host form the blocks behind it, in one pinned buffer
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const int slot = (int)(q->uploads & 1);
    VBX_HIP(ctx, hipEventSynchronize(q->staged[slot]));   // the upload of two ticks ago has left the staging buffer
    char *stage = static_cast<char *>(q->stage[slot]);
    const char *raw = static_cast<const char *>(q->raw[slot]);
    size_t at = n_live * sizeof(pool_entry_t);            // where the next block goes (16-byte aligned)
    q->tab.clear(); q->seg.clear();
    size_t carry_groups = 0, plane_total = 0, next_off = 0;
    bool any_continues = false;
    const size_t gpe = 16 / ob;                           // elements of a 16-byte group
    for (size_t i = 0; i < n_entries; i++) {
        const vbx_pool_entry &he = h_entries[i];
        if (he.n_sample_frames == 0) continue;
        const pool_slot_t &s = q->slots[(size_t)he.stream];
        const vbx_pool_plan_row &r = q->rows[i];
        const size_t c = s.consumed, n = he.n_sample_frames;
        pool_entry_t e{};
        if (on_device) e.src = he.block;
        else {
            std::memcpy(stage + at, he.block, n * sb);
            e.src = raw + at;
            at = (at + n * sb + 15) & ~(size_t)15;
        }
        char *region = static_cast<char *>(q->carry) + (2 * (size_t)he.stream) * q->carry_cap * ob;
        e.old = region + (size_t)s.cur * q->carry_cap * ob;
        e.carry = region + (size_t)(s.cur ^ 1) * q->carry_cap * ob;
        e.n_new = n; e.old_len = c - s.keep_from;         // (a reset slot: consumed == keep_from == 0, nothing of the stale tail is read)
        e.off = next_off; e.span = 0; e.first = 0;
        e.plane_frame = 0; e.frames = 0; e.warm = 0;
        e.row_start = r.row_start; e.n_rows = r.n_rows;
        e.slot = he.stream; e.continues_prev = 0;
        if (r.n_rows) {
            e.span = ((size_t)r.frames - 1) * q->stride + q->frame_len;
            e.first = (int64_t)r.plan.read_from - (int64_t)c;
            e.plane_frame = r.plane_frame; e.frames = r.frames; e.warm = (int64_t)r.plan.warm;
            e.off = (size_t)r.plane_frame * q->stride;
            e.continues_prev = r.plan.continues_prev;
            any_continues = any_continues || r.plan.continues_prev;
            plane_total = e.off + e.span;
            next_off = e.off + (e.span / q->stride + (e.span % q->stride != 0)) * q->stride;
            q->seg.push_back(r.plane_frame);
        }
        e.carry_first = (int64_t)r.plan.keep_from - (int64_t)c;
        e.carry_len = c + n - r.plan.keep_from;
        e.carry_g0 = carry_groups;
        carry_groups += (e.carry_len + gpe - 1) / gpe;
        if (e.carry_len > q->carry_cap || (e.first < 0 && (uint64_t)(-e.first) > e.old_len) || (e.carry_first < 0 && (uint64_t)(-e.carry_first) > e.old_len) ||
            plane_total > q->plane_cap)
            return fail(ctx, VBX_E_RUNTIME, std::string(fn) + ": the tick does not fit the pool's buffers (internal)");
        q->tab.push_back(e);
    }
    std::memcpy(stage, q->tab.data(), n_live * sizeof(pool_entry_t));
    const size_t up_bytes = on_device ? n_live * sizeof(pool_entry_t) : at;
    VBX_HIP(ctx, hipMemcpyAsync(q->raw[slot], stage, up_bytes, hipMemcpyHostToDevice, ctx->stream));      // ONE upload
    VBX_HIP(ctx, hipEventRecord(q->staged[slot], ctx->stream));
    q->uploads++;
    const pool_entry_t *d_tab = static_cast<const pool_entry_t *>(q->raw[slot]);
    { Prof p(ctx, k_pool_ingest_names[sample_name_slot(q->fmt)]);
      launch_pool_ingest(ctx->stream, q->fmt, d_tab, n_live, plane_total, q->plane, carry_groups); }
    for (size_t i = 0; i < n_entries; i++) {              // the slots' timelines: the tails are where the ingest puts them
        if (h_entries[i].n_sample_frames == 0) continue;
        pool_slot_t &s = q->slots[(size_t)h_entries[i].stream];
        s.cur ^= 1; s.consumed += h_entries[i].n_sample_frames; s.keep_from = q->rows[i].plan.keep_from; s.frames += (size_t)q->rows[i].n_rows;
    }
    if (total) {
        int rc = pool_analyze(q, fn, call_frames, want_peak);
        if (rc != VBX_SUCCESS) return rc;
        // the entries that continue an utterance: their trackers go on from the true state, the formant row of the slot's last frame delivered
        if (any_continues && q->p.formant_order) {
            const auto &lt = ctx->last_track;
            if (lt.res == nullptr || lt.out != reinterpret_cast<res_t *>(q->c_rec + 2) || lt.F != (long)call_frames)
                return fail(ctx, VBX_E_RUNTIME, std::string(fn) + ": the frame loop left no track to stitch");
            { Prof p(ctx, "tracker_stitch_pool");
              launch_tracker_stitch_pool(ctx->stream, lt.res, lt.F, VBX_MAX_RESONANCES, lt.cnt, lt.n_est, lt.st, lt.out, lt.out_ld, d_tab, (long)n_live,
                                         q->state); }
        }
        pool_deliver_t d{};
        d.tab = d_tab; d.n = n_live; d.rows = total;
        d.src = q->c_rec; d.src_ld = q->ld_c; d.c0 = q->have_track ? 2 : 0; d.c1 = q->rec; d.dst = out_records; d.dst_ld = record_ld;
        d.src_st = q->c_st; d.src_n = call_frames;
        for (int k = 0; k < 3; k++) d.dst_st[k] = status3 ? status3 + (size_t)k * status_ld : nullptr;
        if (q->have_track) {
            d.src_cand = reinterpret_cast<const double *>(q->c_cand); d.dst_cand = reinterpret_cast<double *>(h_out->cand); d.kmax = q->track.kmax;
            d.src_count = q->c_count; d.dst_count = h_out->count;
            if (want_peak) { d.src_peak = q->c_peak; d.dst_peak = h_out->peak; }
        }
        if (q->p.formant_order) { d.state = q->state; d.n_state = 2 * q->p.n_est; }
        { Prof p(ctx, "pool_deliver"); launch_pool_deliver(ctx->stream, d); }
        ctx->last_track.res = nullptr;                    // the chunk-local rows are no track of the caller's: nothing to stitch
        ctx->last_track.n_est = 0;
    }
    return check_launch(ctx, fn);
}

int vbx_pool_push(vbx_pool *pool, const vbx_pool_entry *h_entries, size_t n_entries, double *out_records, size_t record_ld, int32_t *status3,
                  size_t status_ld, const vbx_pitch_track_outputs *h_outputs, vbx_pool_rows *h_rows, size_t *h_total_rows) {
    return pool_push_impl(pool, __func__, h_entries, false, n_entries, out_records, record_ld, status3, status_ld, h_outputs, h_rows, h_total_rows);
}

int vbx_pool_push_device(vbx_pool *pool, const vbx_pool_entry *h_entries, size_t n_entries, double *out_records, size_t record_ld,
                         int32_t *status3, size_t status_ld, const vbx_pitch_track_outputs *h_outputs, vbx_pool_rows *h_rows,
                         size_t *h_total_rows) {
    return pool_push_impl(pool, __func__, h_entries, true, n_entries, out_records, record_ld, status3, status_ld, h_outputs, h_rows, h_total_rows);
}

int vbx_pool_mark_utterance(vbx_pool *pool, int32_t stream) {
    if (!pool) return fail(nullptr, VBX_E_INVALID, "vbx_pool_mark_utterance: null pool");
    VBX_REQUIRE(pool->ctx, stream >= 0 && (size_t)stream < pool->max_streams, "a stream outside [0, max_streams)");
    pool_slot_t &s = pool->slots[(size_t)stream];
    s.utt_frame = vbx_frame_count(s.consumed, pool->frame_len, pool->stride);
    return VBX_SUCCESS;
}

int vbx_pool_reset_stream(vbx_pool *pool, int32_t stream) {
    if (!pool) return fail(nullptr, VBX_E_INVALID, "vbx_pool_reset_stream: null pool");
    VBX_REQUIRE(pool->ctx, stream >= 0 && (size_t)stream < pool->max_streams, "a stream outside [0, max_streams)");
    // (nothing is queued: the next ingest keeps nothing of the tail, and a first push of an utterance stitches from no state)
    pool_slot_t &s = pool->slots[(size_t)stream];
    s.consumed = 0; s.utt_frame = 0; s.frames = 0; s.keep_from = 0;
    return VBX_SUCCESS;
}

int vbx_pool_info(const vbx_pool *pool, int32_t stream, size_t *h_consumed, size_t *h_frames, size_t *h_carried) {
    if (!pool) return fail(nullptr, VBX_E_INVALID, "vbx_pool_info: null pool");
    VBX_REQUIRE(pool->ctx, stream >= 0 && (size_t)stream < pool->max_streams, "a stream outside [0, max_streams)");
    const pool_slot_t &s = pool->slots[(size_t)stream];
    if (h_consumed) *h_consumed = s.consumed;
    if (h_frames) *h_frames = s.frames;
    if (h_carried) *h_carried = s.consumed - s.keep_from;
    return VBX_SUCCESS;
}

void vbx_pool_close(vbx_pool *pool) {
    if (!pool) return;
    hipSetDevice(pool->ctx->device);
    hipStreamSynchronize(pool->ctx->stream);              // the pool's buffers may still be read by queued work
    if (pool->ctx->side) hipStreamSynchronize(pool->ctx->side);
    if (pool->ctx->trk) hipStreamSynchronize(pool->ctx->trk);
    pool_free(pool);
}

// test hook (tests/test_gpu_pool_ingest.py): the ingest kernel on its own, on the context's stream, on caller-supplied tails, blocks,
// plane and carry destinations.  Entry i: its block and old tail (device), the positions of its region's and its new tail's first
// element relative to the block's sample 0, and their lengths; the regions are laid out by the plan's rule -- the next one starts
// ceil(span / stride) hops behind -- and the plane ends where the last region ends; *h_total: its elements.
struct vbx_internal_pool_ingest_entry {
    const void *d_block; size_t n_new; const void *d_old; size_t old_len; void *d_carry;
    int64_t first; size_t span; int64_t carry_first; size_t carry_len;
};
int vbx_internal_pool_ingest(vbx_ctx *ctx, int format, const vbx_internal_pool_ingest_entry *h_entries, size_t n_entries, size_t stride,
                             void *d_plane, size_t *h_total) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_REQUIRE(ctx, sample_format_ok(format), "unknown sample format");
    VBX_REQUIRE(ctx, stride >= 1 && (n_entries == 0 || h_entries), "bad argument");
    const size_t sb = sample_src_bytes(format), ob = sample_out_bytes(format), gpe = 16 / ob;
    std::vector<pool_entry_t> tab(n_entries);
    size_t off = 0, total = 0, groups = 0;
    for (size_t i = 0; i < n_entries; i++) {
        const vbx_internal_pool_ingest_entry &h = h_entries[i];
        VBX_REQUIRE(ctx, h.n_new <= ((size_t)1 << 40) && h.old_len <= ((size_t)1 << 40) && h.span <= ((size_t)1 << 40) && h.carry_len <= ((size_t)1 << 40), "too large");
        VBX_REQUIRE(ctx, (h.n_new == 0 || h.d_block) && (h.old_len == 0 || h.d_old) && (h.carry_len == 0 || h.d_carry), "null argument");
        VBX_REQUIRE(ctx, format == VBX_SAMPLE_PCM24 || (uintptr_t)h.d_block % sb == 0, "a block needs its type's alignment");
        VBX_REQUIRE(ctx, (uintptr_t)h.d_old % ob == 0 && (uintptr_t)h.d_carry % ob == 0, "the tails need their type's alignment");
        // every position read lies in [-old_len, n_new)
        VBX_REQUIRE(ctx, h.span == 0 || (h.first >= -(int64_t)h.old_len && h.first + (int64_t)h.span <= (int64_t)h.n_new), "a region reads outside its sources");
        VBX_REQUIRE(ctx, h.carry_len == 0 || (h.carry_first >= -(int64_t)h.old_len && h.carry_first + (int64_t)h.carry_len <= (int64_t)h.n_new),
                    "a tail reads outside its sources");
        pool_entry_t &e = tab[i];
        e = pool_entry_t{};
        e.src = h.d_block; e.old = h.d_old; e.carry = h.d_carry; e.n_new = h.n_new; e.old_len = h.old_len;
        e.off = off; e.span = h.span; e.first = h.first;
        e.carry_g0 = groups; e.carry_len = h.carry_len; e.carry_first = h.carry_first;
        groups += (h.carry_len + gpe - 1) / gpe;
        if (h.span) { total = off + h.span; off += (h.span / stride + (h.span % stride != 0)) * stride; }
    }
    if (h_total) *h_total = total;
    if (total + groups == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, total == 0 || (d_plane != nullptr && (uintptr_t)d_plane % ob == 0), "the plane needs its type's alignment");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    void *d = nullptr;
    int rc = stage_upload(ctx, 3, vbx_ctx::WS_CLIPS_TAB, tab.data(), tab.size() * sizeof(pool_entry_t), ctx->stream, &d);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, k_pool_ingest_names[sample_name_slot(format)]);
      launch_pool_ingest(ctx->stream, format, static_cast<const pool_entry_t *>(d), n_entries, total, d_plane, groups); }
    return check_launch(ctx, __func__);
}

}  // extern "C"
