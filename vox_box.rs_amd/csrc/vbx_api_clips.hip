// vbx_api_clips.hip -- a batch of variable-length clips in separate device buffers, analysed from one call: vbx_analyze_clips.
#include "vbx_ctx.hpp"

#include <string>
#include <vector>

using namespace vbx;

// ---- a batch of clips (header: "a batch of variable-length clips") ---------------------------------------------

extern "C" {

static const char *const k_pack_names[9] = {"", "clips_pack_pcm16", "clips_pack_pcm24", "clips_pack_pcm32", "clips_pack_f32", "clips_pack_f64",
                                            "clips_pack_u8", "clips_pack_ulaw", "clips_pack_alaw"};      // by sample_name_slot
static_assert(UNPACK_PCM16 == VBX_SAMPLE_PCM16 && UNPACK_F64 == VBX_SAMPLE_F64 && UNPACK_U8 == VBX_SAMPLE_U8 && UNPACK_ULAW == VBX_SAMPLE_ULAW &&
              UNPACK_ALAW == VBX_SAMPLE_ALAW, "the pack kernels take the header's formats");

// a * b + c in size_t, false on overflow
static bool mul_add(size_t a, size_t b, size_t c, size_t *out) {
    size_t p = 0;
    return !__builtin_mul_overflow(a, b, &p) && !__builtin_add_overflow(p, c, out);
}

int vbx_analyze_clips(vbx_ctx *ctx, const void *const *h_clip, const size_t *h_len, size_t n_clips, const vbx_clip_format *h_fmt,
                      size_t frame_len, size_t stride, const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext,
                      const vbx_pitch_track_params *h_track, double *out_records, size_t record_ld, int32_t *status3,
                      const vbx_pitch_track_outputs *h_out) {
    const char *fn = __func__;
    if (!ctx) return fail(nullptr, VBX_E_INVALID, "vbx_analyze_clips: null context");
    VBX_REQUIRE(ctx, h_fmt != nullptr, "null format");
    VBX_REQUIRE(ctx, sample_format_ok(h_fmt->format), "unknown sample format");
    VBX_REQUIRE(ctx, h_fmt->reserved == 0, "reserved must be 0");
    VBX_REQUIRE(ctx, h_fmt->group_frames == 0 || h_fmt->group_frames >= (size_t)VBX_CLIPS_MIN_GROUP_FRAMES,
                "group_frames must be 0 or >= VBX_CLIPS_MIN_GROUP_FRAMES");
    VBX_REQUIRE(ctx, n_clips == 0 || (h_clip != nullptr && h_len != nullptr), "null clip array");
    VBX_REQUIRE(ctx, frame_len >= 1 && frame_len <= VBX_MAX_LONG_FRAME_LEN, "frame_len must be in [1, 67108864]");
    VBX_REQUIRE(ctx, stride >= 1 && stride <= ((size_t)1 << 40), "stride must be in [1, 2^40]");
    std::vector<vbx_clip_row> rows(n_clips);
    size_t total = 0, n_groups = 0;
    VBX_REQUIRE(ctx, vbx_clips_plan(h_len, n_clips, frame_len, stride, h_fmt->group_frames, rows.data(), &total, &n_groups) == VBX_SUCCESS,
                "bad clip plan (more than 0x7fffffff rows)");
    if (total == 0)                                       // the resident call's empty batch: its checks, its state
        return analyze_ex(ctx, fn, frames_t(), 0, frame_len, stride, h_p, h_ext, h_track, nullptr, 0, out_records, record_ld, status3, h_out);
    // what the resident call rejects from its arguments alone, asked first: nothing is packed or written for such a call.  (What
    // only the parts themselves know -- orders, the resampled shape, the MFCC geometry -- is rejected by the first group's call,
    // which has written nothing of the caller's by then: its rows are the context's.)
    VBX_REQUIRE(ctx, h_p != nullptr && out_records != nullptr, "null argument");
    const size_t rec = vbx_record_doubles_ex(h_p, h_ext);
    VBX_REQUIRE(ctx, record_ld >= rec && record_ld % 2 == 0, "record_ld must be even and >= vbx_record_doubles(params)");
    VBX_REQUIRE(ctx, ((uintptr_t)out_records & 15) == 0, "records must be 16-byte aligned");
    VBX_REQUIRE(ctx, !h_p->formant_order || (h_p->n_est >= 1 && h_p->n_est <= VBX_FORMANT_SLOTS), "n_est must be in [1, 6]");
    const int fmt = h_fmt->format;
    const size_t sb = sample_src_bytes(fmt), ob = sample_out_bytes(fmt);
    // the table: one entry per clip with frames; per group its entries, the frames of its call and the elements of its plane
    struct group_t { size_t e0 = 0, e1 = 0, frames = 0, elems = 0; };
    std::vector<clip_entry_t> tab;
    std::vector<int64_t> seg_rows;
    std::vector<group_t> groups(n_groups);
    size_t max_frames = 0, max_elems = 0;
    for (size_t b = 0; b < n_clips; b++) {
        const vbx_clip_row &r = rows[b];
        if (r.n_rows == 0) continue;
        VBX_REQUIRE(ctx, h_clip[b] != nullptr, "null clip pointer");
        VBX_REQUIRE(ctx, fmt == VBX_SAMPLE_PCM24 || (uintptr_t)h_clip[b] % sb == 0, "a clip needs its type's alignment");
        clip_entry_t e{};
        e.src = h_clip[b]; e.len = h_len[b]; e.plane_frame = r.plane_frame; e.row_start = r.row_start; e.n_rows = r.n_rows;
        size_t off = 0, end = 0, bytes = 0;
        VBX_REQUIRE(ctx, mul_add((size_t)r.plane_frame, stride, 0, &off) && mul_add((size_t)r.plane_frame + (size_t)r.n_rows - 1, stride, frame_len, &end) &&
                         mul_add(end, ob, 0, &bytes), "a group's plane is too large");
        e.off = off;
        group_t &g = groups[(size_t)r.group];
        if (g.e1 == 0) g.e0 = tab.size();
        tab.push_back(e);
        seg_rows.push_back(r.row_start);
        g.e1 = tab.size(); g.frames = (size_t)(r.plane_frame + r.n_rows); g.elems = end;
        if (g.frames > max_frames) max_frames = g.frames;
        if (g.elems > max_elems) max_elems = g.elems;
    }
    VBX_REQUIRE(ctx, max_frames <= 0x7fffffffull, "too many frames for one launch");
    vbx_pitch_path_params path{};
    size_t kmax = 0;
    bool need_peak = false;
    if (h_track) {
        kmax = h_track->kmax; path = h_track->path;
        if (path.time_step == 0.0) path.time_step = (double)stride / h_p->sample_rate;        // the batch's own hop
        int rc = check_pitch_path(ctx, fn, path, total, kmax, true, seg_rows.data(), seg_rows.size());
        if (rc != VBX_SUCCESS) return rc;
        need_peak = path.silence_threshold != 0.0 || (h_out && h_out->peak);
    }
    VBX_HIP(ctx, hipSetDevice(ctx->device));

    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    void *plane = nullptr, *w = nullptr;
    int rc = ws_get(ctx, vbx_ctx::WS_CLIPS_PLANE, max_elems * ob, &plane);
    if (rc != VBX_SUCCESS) return rc;
    // a group's staging: what its frame-loop call writes, rows between the clips included
    const size_t ld_c = rec + (rec & 1);
    const size_t b_rec = up(max_frames * ld_c * sizeof(double)), b_st = up(3 * max_frames * sizeof(int32_t));
    const size_t b_cand = h_track ? up(max_frames * kmax * sizeof(vbx_pitch)) : 0, b_count = h_track ? up(max_frames * sizeof(int32_t)) : 0,
                 b_peak = need_peak ? up(max_frames * sizeof(double)) : 0;
    rc = ws_get(ctx, vbx_ctx::WS_CLIPS_ROWS, b_rec + b_st + b_cand + b_count + b_peak, &w);
    if (rc != VBX_SUCCESS) return rc;
    char *q = static_cast<char *>(w);
    double *c_rec = reinterpret_cast<double *>(q); q += b_rec;
    int32_t *c_st = reinterpret_cast<int32_t *>(q); q += b_st;
    vbx_pitch *c_cand = h_track ? reinterpret_cast<vbx_pitch *>(q) : nullptr; q += b_cand;
    int32_t *c_count = h_track ? reinterpret_cast<int32_t *>(q) : nullptr; q += b_count;
    double *c_peak = need_peak ? reinterpret_cast<double *>(q) : nullptr;
    // the tracked form's compacted lists, counts, peaks and pitch status row of ALL rows, which the path reads behind the last
    // group: the caller's arrays, or a part of the context workspace
    vbx_pitch *g_cand = h_out ? h_out->cand : nullptr;
    int32_t *g_count = h_out ? h_out->count : nullptr, *g_st = status3;
    double *g_peak = (h_out && need_peak) ? h_out->peak : nullptr;
    if (h_track) {
        const size_t l_cand = g_cand ? 0 : up(total * kmax * sizeof(vbx_pitch)), l_peak = (need_peak && !g_peak) ? up(total * sizeof(double)) : 0,
                     l_count = g_count ? 0 : up(total * sizeof(int32_t)), l_st = g_st ? 0 : up(total * sizeof(int32_t));
        if (l_cand + l_peak + l_count + l_st) {
            rc = ws_get(ctx, vbx_ctx::WS_CLIPS_LISTS, l_cand + l_peak + l_count + l_st, &w);
            if (rc != VBX_SUCCESS) return rc;
            q = static_cast<char *>(w);
            if (l_cand) { g_cand = reinterpret_cast<vbx_pitch *>(q); q += l_cand; }
            if (l_peak) { g_peak = reinterpret_cast<double *>(q); q += l_peak; }
            if (l_count) { g_count = reinterpret_cast<int32_t *>(q); q += l_count; }
            if (l_st) g_st = reinterpret_cast<int32_t *>(q);
        }
    }
    // ONE upload of the whole table, on the context's stream (the host arrays are not read after this)
    void *d = nullptr;
    rc = stage_upload(ctx, 3, vbx_ctx::WS_CLIPS_TAB, tab.data(), tab.size() * sizeof(clip_entry_t), ctx->stream, &d);
    if (rc != VBX_SUCCESS) return rc;
    const clip_entry_t *d_tab = static_cast<const clip_entry_t *>(d);

    std::vector<int64_t> seg;
    for (const group_t &g : groups) {
        const size_t cnt = g.e1 - g.e0;
        { Prof p(ctx, k_pack_names[sample_name_slot(fmt)]); launch_clips_pack(ctx->stream, fmt, d_tab + g.e0, cnt, g.elems, plane); }
        // every clip a segment of its own: the rows between two clips lie behind the first one's own rows in its segment
        seg.resize(cnt);
        for (size_t i = 0; i < cnt; i++) seg[i] = tab[g.e0 + i].plane_frame;
        vbx_pitch_track_outputs to{};
        to.cand = c_cand; to.count = c_count; to.peak = c_peak;
        rc = analyze_ex(ctx, fn, frames_t(plane, sample_plane_kind(fmt)), g.frames, frame_len, stride, h_p, h_ext, h_track, seg.data(), cnt, c_rec,
                        ld_c, c_st, h_track ? &to : nullptr, true);
        if (rc != VBX_SUCCESS) return rc;
        clips_deliver_t dl{};
        dl.tab = d_tab + g.e0; dl.n = cnt; dl.row0 = (size_t)tab[g.e0].row_start;
        dl.rows = (size_t)(tab[g.e1 - 1].row_start + tab[g.e1 - 1].n_rows) - dl.row0;
        dl.src = c_rec; dl.src_ld = ld_c; dl.c0 = h_track ? 2 : 0; dl.c1 = rec; dl.dst = out_records; dl.dst_ld = record_ld;
        dl.src_st = c_st; dl.src_n = g.frames;
        dl.dst_st[0] = g_st; dl.dst_st[1] = status3 ? status3 + total : nullptr; dl.dst_st[2] = status3 ? status3 + 2 * total : nullptr;
        if (h_track) {
            dl.src_cand = reinterpret_cast<const double *>(c_cand); dl.dst_cand = reinterpret_cast<double *>(g_cand); dl.kmax = kmax;
            dl.src_count = c_count; dl.dst_count = g_count;
            dl.src_peak = c_peak; dl.dst_peak = g_peak;
        }
        { Prof p(ctx, "clips_deliver"); launch_clips_deliver(ctx->stream, dl); }
    }
    rc = check_launch(ctx, fn);
    if (rc != VBX_SUCCESS) return rc;
    // ONE path over the compacted lists, every clip a segment, straight into columns 0-1: the dropped rows cannot reach it
    if (h_track) {
        rc = run_pitch_path(ctx, ctx->stream, g_cand, g_count, g_st, total, kmax, g_peak, seg_rows.data(), seg_rows.size(), path,
                            reinterpret_cast<vbx_pitch *>(out_records), record_ld, h_out ? h_out->index : nullptr, fn);
        if (rc != VBX_SUCCESS) return rc;
    }
    ctx->last_track.res = nullptr;                        // the groups' rows are no track of the caller's: nothing to stitch
    ctx->last_track.n_est = 0;
    return VBX_SUCCESS;
}

// test hook (tests/test_gpu_clips_pack.py): the pack kernel on its own, on the context's stream.  The clips are laid out by the
// plan's rule -- clip b + 1 starts ceil(len_b / stride) hops behind clip b -- and the plane ends where the last clip ends;
// *h_total: its elements.
int vbx_internal_clips_pack(vbx_ctx *ctx, int format, const void *const *h_clip, const size_t *h_len, size_t n_clips, size_t stride,
                            void *d_out, size_t *h_total) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_REQUIRE(ctx, sample_format_ok(format), "unknown sample format");
    VBX_REQUIRE(ctx, stride >= 1 && (n_clips == 0 || (h_clip && h_len)), "bad argument");
    std::vector<clip_entry_t> tab(n_clips);
    size_t off = 0, total = 0;
    for (size_t b = 0; b < n_clips; b++) {
        VBX_REQUIRE(ctx, h_len[b] == 0 || h_clip[b] != nullptr, "null clip pointer");
        VBX_REQUIRE(ctx, format == VBX_SAMPLE_PCM24 || (uintptr_t)h_clip[b] % sample_src_bytes(format) == 0, "a clip needs its type's alignment");
        tab[b].src = h_clip[b]; tab[b].len = h_len[b]; tab[b].off = off;
        total = off + h_len[b];
        off += (h_len[b] / stride + (h_len[b] % stride != 0)) * stride;
    }
    if (h_total) *h_total = total;
    if (total == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, d_out != nullptr && (uintptr_t)d_out % sample_out_bytes(format) == 0, "the plane needs its type's alignment");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    void *d = nullptr;
    int rc = stage_upload(ctx, 3, vbx_ctx::WS_CLIPS_TAB, tab.data(), tab.size() * sizeof(clip_entry_t), ctx->stream, &d);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, k_pack_names[sample_name_slot(format)]); launch_clips_pack(ctx->stream, format, static_cast<const clip_entry_t *>(d), n_clips, total, d_out); }
    return check_launch(ctx, __func__);
}

}  // extern "C"
