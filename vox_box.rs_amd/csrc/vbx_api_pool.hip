// vbx_api_pool.hip -- a session pool: many independent live streams on one context, analysed from one upload and one launch chain
// per tick (vbx_pool_*), and every slot's live pitch contour from one more launch per tick
// (vbx_pool_path_bind; section 5m).  What a tick shares with a session's push is the live core's (vbx_live.hpp).
#include "vbx_live.hpp"

#include <cmath>
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
    uint64_t live = 0;                                    // ... with a block of at least one sample
};

// A bound pool's online paths (vbx_pool_path_bind): slot k's stream allocation -- pp_online_state_t, then the ring of max_pending
// frames, vbx_path_stream_open's layout -- at mem + k * slot_bytes, and where the slots' rows and commits go.  flag[k]: slot k's
// deferred PP_POOL_RESET / PP_POOL_MARK, applied by the next tick's path launch; flagged: the slots with one, each listed once.
struct pool_path_t {
    bool bound = false;
    double peak_ref = 0.0;
    size_t max_pending = 0, slot_rows = 0, path_ld = 0;
    int G = 4;
    void *mem = nullptr;
    size_t slot_bytes = 0, off_row = 0, off_psi = 0, off_idx = 0;
    vbx_pool_path_outputs out{};
    std::vector<uint8_t> flag;
    std::vector<int32_t> flagged;
    std::vector<pp_pool_row_t> tab;                       // a tick's path table (host scratch)
};
static_assert(sizeof(pp_pool_row_t) == 24, "the path table's rows: slot, flags, first list row, frames");

// max_streams slots that share a format, a frame shape and a parameter set.  The pool owns everything a tick writes before the
// caller's arrays: the carry regions (slot k's two regions at elements (2 k + b) * carry_cap), the tick's plane, the two pinned
// staging buffers with their raw device slots (the ring: table first, the gathered blocks behind it) and the core's chunk-local
// buffers of the largest frame-loop call and max_streams state rows.
struct vbx_pool {
    live_core_t core;
    size_t max_streams = 0, max_block = 0, max_tick = 0;
    size_t call_max = 0, plane_cap = 0, carry_cap = 0;
    std::vector<pool_slot_t> slots;
    uint64_t ticks = 0;                                   // vbx_pool_push calls so far (the duplicate check's stamp)
    bool queued = false;                                  // a tick has queued work: too late for a first vbx_pool_path_bind
    pool_path_t path;
    void *carry = nullptr, *plane = nullptr;
    live_ring_t ring;
    // a tick's host scratch, kept between ticks so that none allocates
    std::vector<size_t> h_consumed, h_utt, h_new;
    std::vector<vbx_pool_plan_row> rows;
    std::vector<pool_entry_t> tab;
    std::vector<int64_t> seg;
};

static void pool_free(vbx_pool *q) {
    q->ring.free();
    if (q->path.mem) hipFree(q->path.mem);
    if (q->carry) hipFree(q->carry);
    if (q->plane) hipFree(q->plane);
    live_free(q->core);
    delete q;
}

int vbx_pool_open(vbx_ctx *ctx, const vbx_host_audio *h_fmt, size_t frame_len, size_t stride, const vbx_analysis_params *h_p,
                  const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, size_t max_streams, size_t max_block,
                  size_t max_tick, vbx_pool **out) {
    const char *fn = __func__;
    if (!ctx) return fail(nullptr, VBX_E_INVALID, "vbx_pool_open: null context");
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    *out = nullptr;
    VBX_REQUIRE(ctx, h_fmt != nullptr && h_p != nullptr, "null argument");
    int rc = live_check_audio(ctx, fn, h_fmt, h_fmt->channels == 1 && h_fmt->channel == 0, "a pool's streams are mono: channels must be 1 and channel 0");
    if (rc != VBX_SUCCESS) return rc;
    VBX_REQUIRE(ctx, max_streams >= 1, "max_streams must be >= 1");
    VBX_REQUIRE(ctx, max_block >= 1 && max_tick >= max_block, "need 1 <= max_block_sample_frames <= max_tick_sample_frames");
    VBX_REQUIRE(ctx, frame_len >= 1 && frame_len <= VBX_MAX_FRAME_LEN, "frame_len must be in [1, VBX_MAX_FRAME_LEN]: longer frames take one vbx_session per stream");
    VBX_REQUIRE(ctx, stride >= 1 && stride <= ((size_t)1 << 40), "stride must be in [1, 2^40]");
    VBX_REQUIRE(ctx, max_streams <= 0x7fffffffull && max_tick <= ((size_t)1 << 40), "max_streams or max_tick_sample_frames too large");
    if ((rc = live_check_n_est(ctx, fn, h_p)) != VBX_SUCCESS) return rc;
    const size_t call_max = pool_max_call_frames(frame_len, stride, max_streams, max_tick);
    VBX_REQUIRE(ctx, call_max <= 0x7fffffffull, "too many frames for one launch");
    const live_core_t core = live_make(ctx, h_fmt->format, frame_len, stride, h_p, h_ext, h_track);
    if ((rc = live_check_path(core, fn, call_max)) != VBX_SUCCESS) return rc;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    vbx_pool *q = new vbx_pool();
    q->core = core; q->max_streams = max_streams; q->max_block = max_block; q->max_tick = max_tick;
    q->call_max = call_max;
    q->plane_cap = call_max * stride + frame_len;
    q->carry_cap = (pool_carry_samples(frame_len, stride) + 7) & ~(size_t)7;      // whole 16-byte groups for every element type
    const size_t e_max = max_streams < max_tick ? max_streams : max_tick;         // entries that hold a sample
    // (a tracked pool can be bound: the path table of a tick, a row per slot at most, travels between the entry table and the blocks)
    const size_t path_bytes = core.have_track ? (max_streams * sizeof(pp_pool_row_t) + 15) & ~(size_t)15 : 0;
    const size_t raw_bytes = e_max * sizeof(pool_entry_t) + path_bytes + max_tick * sample_src_bytes(core.fmt) + 16 * e_max;
    q->slots.resize(max_streams);
    q->h_consumed.reserve(max_streams); q->h_utt.reserve(max_streams); q->h_new.reserve(max_streams);
    q->rows.reserve(max_streams); q->tab.reserve(e_max); q->seg.reserve(max_streams);
    const size_t ob = sample_out_bytes(core.fmt);
    LIVE_HIP(ctx, hipMalloc(&q->carry, 2 * max_streams * q->carry_cap * ob), pool_free(q));    // (hipMalloc: 256-byte aligned bases)
    LIVE_HIP(ctx, hipMemsetAsync(q->carry, 0, 2 * max_streams * q->carry_cap * ob, ctx->stream), pool_free(q));
    LIVE_HIP(ctx, hipMalloc(&q->plane, q->plane_cap * ob), pool_free(q));
    LIVE_HIP(ctx, hipMemsetAsync(q->plane, 0, q->plane_cap * ob, ctx->stream), pool_free(q));
    rc = q->ring.alloc(ctx, raw_bytes, raw_bytes);
    if (rc == VBX_SUCCESS) rc = live_alloc(q->core, call_max, max_streams);
    if (rc != VBX_SUCCESS) { pool_free(q); return rc; }
    // the warm-up: the largest shape a tick can ask for, on the zeroed plane, with as many segments as a tick can have entries
    const size_t per = call_max / e_max;
    for (size_t k = 0; k < e_max; k++) q->seg.push_back((int64_t)(k * per));
    rc = live_warm_up(q->core, fn, q->plane, call_max, q->seg.data(), q->seg.size(), [&] { pool_free(q); });
    if (rc != VBX_SUCCESS) return rc;
    q->seg.clear();
    *out = q;
    return VBX_SUCCESS;
}

// The rest of a tick's path table behind its entries' rows (q->path.tab), into the tick's staging buffer: every slot's deferred
// flags go into its row, and a flagged slot without a row -- not listed in the tick, or with an empty block -- gets one of no
// frames.  The flags are taken: the launch the caller queues next applies them.
static void pool_path_table(vbx_pool *q, uint64_t stamp, char *h_dst) {
    pool_path_t &pp = q->path;
    for (pp_pool_row_t &r : pp.tab) r.flags = pp.flag[(size_t)r.slot];
    for (int32_t k : pp.flagged)
        if (stamp == 0 || q->slots[(size_t)k].live != stamp) pp.tab.push_back(pp_pool_row_t{k, pp.flag[(size_t)k], 0, 0});
    for (int32_t k : pp.flagged) pp.flag[(size_t)k] = 0;
    pp.flagged.clear();
    std::memcpy(h_dst, pp.tab.data(), pp.tab.size() * sizeof(pp_pool_row_t));
}

// ONE launch for the n rows of the uploaded table: a lane group per visited slot (k_pitch_path_pool.hip)
static void pool_path_launch(vbx_pool *q, const pp_pool_row_t *d_tab, size_t n, bool have_peak) {
    const live_core_t &c = q->core;
    const pool_path_t &pp = q->path;
    const vbx_pitch_path_params pr = live_path_params(c);
    pp_par_t P{};
    P.cand = reinterpret_cast<const pitch_t *>(c.c_cand); P.count = c.c_count; P.status = c.c_st; P.lpk = have_peak ? c.c_peak : nullptr;
    P.kmax = (int)c.track.kmax; P.use_u = (have_peak && pr.silence_threshold != 0.0) ? 1 : 0;
    const double corr = 0.01 / pr.time_step;                   // the host constants of the definition, in its order (pp_setup)
    P.vt = pr.voicing_threshold; P.oc = pr.octave_cost;
    P.cvu = pr.voiced_unvoiced_cost * corr; P.cj = pr.octave_jump_cost * corr;
    P.Lc = std::log2(pr.ceiling_hz); P.q = pr.silence_threshold / (1.0 + pr.voicing_threshold);
    pp_online_t O{};
    O.cap = (long)pp.max_pending; O.peak = pp.peak_ref; O.ld = (long)pp.path_ld;
    pp_online_pool_t A{};
    A.tab = d_tab;
    A.mem = static_cast<char *>(pp.mem); A.slot_bytes = pp.slot_bytes; A.off_row = pp.off_row; A.off_psi = pp.off_psi; A.off_idx = pp.off_idx;
    A.out_path = reinterpret_cast<pitch_t *>(pp.out.out_path); A.out_index = pp.out.out_index; A.out_forced = pp.out.out_forced;
    A.commit = reinterpret_cast<pp_commit_t *>(pp.out.d_commit); A.slot_rows = (long)pp.slot_rows;
    Prof pf(c.ctx, "pitch_path_online_pool");
    launch_pitch_path_online_pool(c.ctx->stream, P, pp.G, O, A, (long)n);
}

// A tick without a block on a bound pool with flagged slots: the single upload -- the path table alone -- and the single path launch
static int pool_path_tick(vbx_pool *q, const char *fn) {
    vbx_ctx *ctx = q->core.ctx;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    char *stage = nullptr;
    int rc = q->ring.acquire(ctx, &stage);
    if (rc != VBX_SUCCESS) return rc;
    const void *raw = q->ring.raw[q->ring.slot()];
    q->path.tab.clear();
    pool_path_table(q, 0, stage);
    const size_t n = q->path.tab.size();
    if ((rc = q->ring.upload(ctx, n * sizeof(pp_pool_row_t))) != VBX_SUCCESS) return rc;
    q->queued = true;
    pool_path_launch(q, static_cast<const pp_pool_row_t *>(raw), n, false);
    return check_launch(ctx, fn);
}

static int pool_push_impl(vbx_pool *q, const char *fn, const vbx_pool_entry *h_entries, bool on_device, size_t n_entries, double *out_records,
                          size_t record_ld, int32_t *status3, size_t status_ld, const vbx_pitch_track_outputs *h_out, vbx_pool_rows *h_rows,
                          size_t *h_total) {
    if (!q) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null pool");
    const live_core_t &c = q->core;
    vbx_ctx *ctx = c.ctx;
    if (h_total) *h_total = 0;
    if (n_entries == 0) return q->path.flagged.empty() ? VBX_SUCCESS : pool_path_tick(q, fn);
    VBX_REQUIRE_FN(ctx, fn, h_entries != nullptr, "null entries");
    // ---- everything that can be refused, before anything is queued or any slot changes
    const size_t sb = sample_src_bytes(c.fmt), ob = sample_out_bytes(c.fmt), stride = c.stride;
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
        else if (on_device && c.fmt != VBX_SAMPLE_PCM24 && (uintptr_t)e.block % sb != 0) why = "a block needs its type's alignment";
        sum += e.n_sample_frames;
        s.live = stamp;
        n_live++;
    }
    VBX_REQUIRE_FN(ctx, fn, why == nullptr, why);
    q->h_consumed.resize(n_entries); q->h_utt.resize(n_entries); q->h_new.resize(n_entries); q->rows.resize(n_entries);
    for (size_t i = 0; i < n_entries; i++) {
        const pool_slot_t &s = q->slots[(size_t)h_entries[i].stream];
        q->h_consumed[i] = s.consumed; q->h_utt[i] = s.utt_frame; q->h_new[i] = h_entries[i].n_sample_frames;
    }
    size_t total = 0, call_frames = 0;
    if (vbx_pool_plan(q->h_consumed.data(), q->h_utt.data(), q->h_new.data(), n_entries, c.frame_len, stride, q->rows.data(), &total,
                      &call_frames) != VBX_SUCCESS)
        return fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad pool plan");
    VBX_REQUIRE_FN(ctx, fn, call_frames <= q->call_max, "the tick's frame-loop call is larger than the pool was opened for");
    bool want_peak = false;
    if (total) {
        const vbx_channel_outputs o{out_records, status3, h_out};
        int rc = live_check_outputs(c, fn, LIVE_OUT_ALL, "h_outputs", o, record_ld, status_ld, total, "status_ld must be >= the rows the tick delivers", &want_peak);
        if (rc != VBX_SUCCESS) return rc;
    }
    for (size_t i = 0; i < n_entries; i++) if (h_rows) { h_rows[i].row_start = q->rows[i].row_start; h_rows[i].n_rows = q->rows[i].n_rows; }
    if (h_total) *h_total = total;
    if (n_live == 0)                                      // nothing but empty blocks: nothing is queued, but what marks and resets deferred
        return q->path.flagged.empty() ? VBX_SUCCESS : pool_path_tick(q, fn);

    // ---- the table, and in the host form the blocks behind it, in one pinned buffer
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    char *stage = nullptr;
    int rc = q->ring.acquire(ctx, &stage);
    if (rc != VBX_SUCCESS) return rc;
    const char *raw = static_cast<const char *>(q->ring.raw[q->ring.slot()]);
    // a bound pool: the path table's rows, the tick's entries first, behind the entry table
    size_t n_path = 0;
    if (q->path.bound) {
        n_path = n_live;
        for (int32_t k : q->path.flagged) n_path += q->slots[(size_t)k].live != stamp;
    }
    const size_t path_at = n_live * sizeof(pool_entry_t);
    size_t at = path_at + ((n_path * sizeof(pp_pool_row_t) + 15) & ~(size_t)15);       // where the next block goes (16-byte aligned)
    q->tab.clear(); q->seg.clear(); q->path.tab.clear();
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
            e.span = ((size_t)r.frames - 1) * stride + q->core.frame_len;
            e.first = (int64_t)r.plan.read_from - (int64_t)c;
            e.plane_frame = r.plane_frame; e.frames = r.frames; e.warm = (int64_t)r.plan.warm;
            e.off = (size_t)r.plane_frame * stride;
            e.continues_prev = r.plan.continues_prev;
            any_continues = any_continues || r.plan.continues_prev;
            plane_total = e.off + e.span;
            next_off = e.off + (e.span / stride + (e.span % stride != 0)) * stride;
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
        // its slot's lane group scans the rows the entry delivers (none: it reports what is pending)
        if (q->path.bound) q->path.tab.push_back(pp_pool_row_t{he.stream, 0, r.n_rows ? r.plane_frame + (int64_t)r.plan.warm : 0, r.n_rows});
    }
    std::memcpy(stage, q->tab.data(), n_live * sizeof(pool_entry_t));
    const pool_entry_t *d_tab = reinterpret_cast<const pool_entry_t *>(raw);
    if (q->path.bound) pool_path_table(q, stamp, stage + path_at);
    if ((rc = q->ring.upload(ctx, on_device ? path_at + n_path * sizeof(pp_pool_row_t) : at)) != VBX_SUCCESS) return rc;      // ONE upload
    q->queued = true;
    { Prof p(ctx, k_pool_ingest_names[sample_name_slot(c.fmt)]);
      launch_pool_ingest(ctx->stream, c.fmt, d_tab, n_live, plane_total, q->plane, carry_groups); }
    for (size_t i = 0; i < n_entries; i++) {              // the slots' timelines: the tails are where the ingest puts them
        if (h_entries[i].n_sample_frames == 0) continue;
        pool_slot_t &s = q->slots[(size_t)h_entries[i].stream];
        s.cur ^= 1; s.consumed += h_entries[i].n_sample_frames; s.keep_from = q->rows[i].plan.keep_from; s.frames += (size_t)q->rows[i].n_rows;
    }
    if (total) {
        if ((rc = live_analyze(c, fn, q->plane, call_frames, q->seg.data(), q->seg.size(), want_peak)) != VBX_SUCCESS) return rc;
        // the entries that continue an utterance: their trackers go on from the true state, the formant row of the slot's last frame delivered
        if (any_continues && c.p.formant_order) {
            if ((rc = live_take_last_track(c, fn, call_frames)) != VBX_SUCCESS) return rc;
            const auto &lt = ctx->last_track;
            Prof p(ctx, "tracker_stitch_pool");
            launch_tracker_stitch_pool(ctx->stream, lt.res, lt.F, VBX_MAX_RESONANCES, lt.cnt, lt.n_est, lt.st, lt.out, lt.out_ld, d_tab, (long)n_live, c.state);
        }
        pool_deliver_t d{};
        live_deliver_source(d, c, call_frames, want_peak);
        d.tab = d_tab; d.n = n_live; d.rows = total; d.dst = out_records; d.dst_ld = record_ld;
        for (int k = 0; k < 3; k++) d.dst_st[k] = status3 ? status3 + (size_t)k * status_ld : nullptr;
        if (c.have_track) { d.dst_cand = reinterpret_cast<double *>(h_out->cand); d.dst_count = h_out->count; d.dst_peak = h_out->peak; }
        { Prof p(ctx, "pool_deliver"); launch_pool_deliver(ctx->stream, d); }
        live_drop_last_track(ctx);
    }
    // the contours: every visited slot's online path over its own rows of the pool-owned lists, in one launch behind the deliver
    if (q->path.bound) pool_path_launch(q, reinterpret_cast<const pp_pool_row_t *>(raw + path_at), n_path, want_peak);
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

static void pool_path_defer(vbx_pool *q, int32_t stream, int32_t what) {
    pool_path_t &pp = q->path;
    if (!pp.bound) return;
    if (pp.flag[(size_t)stream] == 0) pp.flagged.push_back(stream);
    // a reset drops what a mark before it asked for: there is nothing left to end
    pp.flag[(size_t)stream] = (uint8_t)(what == PP_POOL_RESET ? PP_POOL_RESET : pp.flag[(size_t)stream] | PP_POOL_MARK);
}

int vbx_pool_mark_utterance(vbx_pool *pool, int32_t stream) {
    if (!pool) return fail(nullptr, VBX_E_INVALID, "vbx_pool_mark_utterance: null pool");
    VBX_REQUIRE(pool->core.ctx, stream >= 0 && (size_t)stream < pool->max_streams, "a stream outside [0, max_streams)");
    pool_slot_t &s = pool->slots[(size_t)stream];
    s.utt_frame = vbx_frame_count(s.consumed, pool->core.frame_len, pool->core.stride);
    pool_path_defer(pool, stream, PP_POOL_MARK);          // a bound pool: the next tick's path launch ends the slot's path utterance first
    return VBX_SUCCESS;
}

int vbx_pool_reset_stream(vbx_pool *pool, int32_t stream) {
    if (!pool) return fail(nullptr, VBX_E_INVALID, "vbx_pool_reset_stream: null pool");
    VBX_REQUIRE(pool->core.ctx, stream >= 0 && (size_t)stream < pool->max_streams, "a stream outside [0, max_streams)");
    // (nothing is queued: the next ingest keeps nothing of the tail, and a first push of an utterance stitches from no state)
    pool_slot_t &s = pool->slots[(size_t)stream];
    s.consumed = 0; s.utt_frame = 0; s.frames = 0; s.keep_from = 0;
    pool_path_defer(pool, stream, PP_POOL_RESET);         // a bound pool: ... zeroes the slot's path state before anything else
    return VBX_SUCCESS;
}

int vbx_pool_path_bind(vbx_pool *pool, double peak_ref, size_t max_pending, const vbx_pool_path_outputs *h_out, size_t path_ld, size_t slot_rows) {
    const char *fn = __func__;
    if (!pool) return fail(nullptr, VBX_E_INVALID, "vbx_pool_path_bind: null pool");
    const live_core_t &c = pool->core;
    vbx_ctx *ctx = c.ctx;
    pool_path_t &pp = pool->path;
    VBX_REQUIRE(ctx, c.have_track, "the pool was opened without h_track: it has no candidate lists");
    VBX_REQUIRE(ctx, h_out != nullptr && h_out->out_path != nullptr && h_out->d_commit != nullptr, "null h_out, out_path or d_commit");
    VBX_REQUIRE(ctx, path_ld >= 2, "path_ld must be >= 2");
    VBX_REQUIRE(ctx, max_pending >= 1 && max_pending <= ((size_t)1 << 24), "max_pending must be in [1, 2^24]");
    const size_t need = vbx_pool_path_slot_rows(max_pending, pool->max_block, c.stride);
    VBX_REQUIRE(ctx, slot_rows >= need && slot_rows <= ((size_t)1 << 40), "slot_rows must be >= vbx_pool_path_slot_rows(max_pending, max_block_sample_frames, stride)");
    if (pp.bound) {                                       // between ticks: other destinations, the same paths
        VBX_REQUIRE(ctx, pp.max_pending == max_pending && pp.slot_rows == slot_rows && std::memcmp(&peak_ref, &pp.peak_ref, sizeof(double)) == 0,
                    "a bound pool keeps its peak_ref, max_pending and slot_rows");
        pp.out = *h_out; pp.path_ld = path_ld;
        return VBX_SUCCESS;
    }
    VBX_REQUIRE(ctx, !pool->queued, "bind before the first tick that queues work");
    const vbx_pitch_path_params pr = live_path_params(c);
    int rc = check_pitch_path(ctx, fn, pr, 0, c.track.kmax, true, nullptr, 0);
    if (rc != VBX_SUCCESS) return rc;
    VBX_REQUIRE(ctx, !(pr.silence_threshold > 0.0 && !(std::isfinite(peak_ref) && peak_ref >= 0.0)), "silence_threshold > 0 needs a finite peak_ref >= 0");
    // every slot's stream allocation, as vbx_path_stream_open lays one out, rounded up to 256 bytes
    int G = 4;
    while (G < (int)c.track.kmax + 1) G <<= 1;
    const size_t b_st = (sizeof(pp_online_state_t) + 255) & ~(size_t)255, b_row = max_pending * (size_t)G * sizeof(pitch_t), b_psi = max_pending * (size_t)G;
    const size_t slot_bytes = (b_st + b_row + 2 * b_psi + 255) & ~(size_t)255;
    if (slot_bytes > SIZE_MAX / pool->max_streams) return fail(ctx, VBX_E_RUNTIME, std::string(fn) + ": the slots' rings are too large to allocate");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    void *mem = nullptr;
    hipError_t e = hipMalloc(&mem, slot_bytes * pool->max_streams);
    if (e == hipSuccess) e = hipMemset2DAsync(mem, slot_bytes, 0, b_st, pool->max_streams, ctx->stream);
    if (e != hipSuccess) {
        if (mem) { hipStreamSynchronize(ctx->stream); hipFree(mem); }
        return fail(ctx, VBX_E_RUNTIME, std::string(fn) + ": " + hipGetErrorString(e));
    }
    pp.flag.assign(pool->max_streams, 0);
    pp.flagged.clear(); pp.flagged.reserve(pool->max_streams); pp.tab.reserve(pool->max_streams);
    pp.mem = mem; pp.slot_bytes = slot_bytes; pp.off_row = b_st; pp.off_psi = b_st + b_row; pp.off_idx = b_st + b_row + b_psi;
    pp.G = G; pp.peak_ref = peak_ref; pp.max_pending = max_pending; pp.slot_rows = slot_rows; pp.path_ld = path_ld; pp.out = *h_out;
    pp.bound = true;
    return VBX_SUCCESS;
}

int vbx_pool_info(const vbx_pool *pool, int32_t stream, size_t *h_consumed, size_t *h_frames, size_t *h_carried) {
    if (!pool) return fail(nullptr, VBX_E_INVALID, "vbx_pool_info: null pool");
    VBX_REQUIRE(pool->core.ctx, stream >= 0 && (size_t)stream < pool->max_streams, "a stream outside [0, max_streams)");
    const pool_slot_t &s = pool->slots[(size_t)stream];
    if (h_consumed) *h_consumed = s.consumed;
    if (h_frames) *h_frames = s.frames;
    if (h_carried) *h_carried = s.consumed - s.keep_from;
    return VBX_SUCCESS;
}

void vbx_pool_close(vbx_pool *pool) {
    if (!pool) return;
    live_drain(pool->core.ctx);
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
