// vbx_api_path.hip -- the pitch path (k_pitch_path.hip): over resident lists, across shard cuts, and online while the lists arrive.
#include "vbx_ctx.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace vbx;

// ---- periodic.rs: the pitch path (k_pitch_path.hip) -----------------------------------------

namespace vbx {

// Chunk length C and warm-up W of the speculative scan.  The warm-up is where forgetting has to happen: a chunk whose entry state
// after W frames from a fresh start is not bit for bit the true one is redone (DESIGN.md "Pitch path" has the measured counts).
#ifndef VBX_PP_CHUNK
#define VBX_PP_CHUNK 256
#endif
#ifndef VBX_PP_WARM
#define VBX_PP_WARM 64
#endif
#ifndef VBX_PP_ROUNDS
#define VBX_PP_ROUNDS 3
#endif
#ifndef VBX_PP_ROUNDS_LONG
#define VBX_PP_ROUNDS_LONG 8
#endif

int check_pitch_path(vbx_ctx *ctx, const char *fn, const vbx_pitch_path_params &pr, size_t n_frames, size_t kmax, bool have_peak,
                     const int64_t *h_seg_start, size_t n_segments) {
    VBX_REQUIRE_FN(ctx, fn, kmax >= 1 && kmax <= 63, "kmax must be in [1, 63] (at most 64 states per frame)");
    for (double v : {pr.voicing_threshold, pr.silence_threshold, pr.octave_cost, pr.octave_jump_cost, pr.voiced_unvoiced_cost,
                     pr.ceiling_hz, pr.time_step})
        VBX_REQUIRE_FN(ctx, fn, std::isfinite(v) && v >= 0.0, "every parameter must be finite and >= 0");
    VBX_REQUIRE_FN(ctx, fn, pr.time_step > 0.0 && pr.ceiling_hz > 0.0, "time_step and ceiling_hz must be > 0");
    VBX_REQUIRE_FN(ctx, fn, !(pr.silence_threshold > 0.0 && !have_peak), "silence_threshold > 0 needs local_peak");
    VBX_REQUIRE_FN(ctx, fn, n_frames <= 0x7fffffffull, "too many frames for one launch");
    if (h_seg_start != nullptr && n_segments > 0) {            // the rules of vbx_analyze_frames_f64
        VBX_REQUIRE_FN(ctx, fn, h_seg_start[0] == 0, "seg_start[0] must be 0");
        for (size_t i = 1; i < n_segments; i++)
            VBX_REQUIRE_FN(ctx, fn, h_seg_start[i] >= h_seg_start[i - 1] && (size_t)h_seg_start[i] <= n_frames, "seg_start must ascend within [0, n_frames]");
    }
    return VBX_SUCCESS;
}

// The chunk table, the workspace and the constants of one path call (arguments checked by the caller).  split: a frame at which a
// chunk must begin whatever C is (the shard calls' `first`; 0: none).  Ends what a vbx_pitch_path_shard_begin_f64 left: WS_PATH is reused.
static int pp_setup(vbx_ctx *ctx, hipStream_t st, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                    size_t n_frames, size_t kmax, const double *local_peak, const int64_t *h_seg_start, size_t n_segments,
                    const vbx_pitch_path_params &pr, size_t split, pp_plan_t &S) {
    ctx->shard.live = false;
    const bool segmented = h_seg_start != nullptr && n_segments > 0;
    const long F = (long)n_frames, W = VBX_PP_WARM;
    const size_t nseg = segmented ? n_segments : 1;
    int G = 4;
    while (G < (int)kmax + 1) G <<= 1;
    const long C = (pr.chunk_frames == 0) ? VBX_PP_CHUNK : (long)std::min<size_t>(pr.chunk_frames, n_frames);
    // the chunk table: every segment cut into chunks of C frames (a chunk never spans two segments), then seg_chunk0[nseg + 1]
    std::vector<pp_chunk_t> chunks;
    chunks.reserve((size_t)(F / C + (long)nseg + 1));
    std::vector<int64_t> seg_chunk0(nseg + 1);
    long max_per_seg = 1, n_guessed = 0;
    for (size_t sg = 0; sg < nseg; sg++) {
        const long s0 = segmented ? (long)h_seg_start[sg] : 0, s1 = (segmented && sg + 1 < nseg) ? (long)h_seg_start[sg + 1] : F;
        seg_chunk0[sg] = (int64_t)chunks.size();
        for (long f0 = s0; f0 < s1;) {
            long f1 = (f0 + C < s1) ? f0 + C : s1;
            if (f0 < (long)split && (long)split < f1) f1 = (long)split;
            chunks.push_back(pp_chunk_t{f0, f1, s0, (long)sg, f1 == s1 ? 1 : 0, 0});
            if (f0 - W > s0) n_guessed++;                      // entered from a warm-up guess, not from the segment's start
            f0 = f1;
        }
        max_per_seg = std::max<long>(max_per_seg, (long)chunks.size() - (long)seg_chunk0[sg]);
    }
    seg_chunk0[nseg] = (int64_t)chunks.size();
    const long nch = (long)chunks.size();
    S.c_first = nch; S.c_end = nch;
    for (long c = 0; c < nch; c++)
        if (chunks[c].f0 >= (long)split) { S.c_first = c; S.c_end = (long)seg_chunk0[chunks[c].seg + 1]; break; }
    std::vector<char> tab((size_t)nch * sizeof(pp_chunk_t) + (nseg + 1) * sizeof(int64_t));
    std::memcpy(tab.data(), chunks.data(), (size_t)nch * sizeof(pp_chunk_t));
    std::memcpy(tab.data() + (size_t)nch * sizeof(pp_chunk_t), seg_chunk0.data(), (nseg + 1) * sizeof(int64_t));
    void *dtab = nullptr;
    int rc = stage_upload(ctx, 2, vbx_ctx::WS_PATH_TAB, tab.data(), tab.size(), st, &dtab);
    if (rc != VBX_SUCCESS) return rc;
    S.d_seg_chunk0 = reinterpret_cast<const int64_t *>(static_cast<char *>(dtab) + (size_t)nch * sizeof(pp_chunk_t));
    // workspace: psi [F][G] uint8, per chunk entry / exit / wanted D, flags, maps; per segment leader and peak
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_psi = al((size_t)F * G), b_d = al((size_t)nch * G * sizeof(double)), b_i = al((size_t)nch * sizeof(int32_t)),
                 b_mask = al(((size_t)(nch + 63) / 64 + 1) * sizeof(unsigned long long)), b_lead = al(nseg * sizeof(int32_t)),
                 b_cpk = al((size_t)nch * sizeof(double)), b_spk = al(nseg * sizeof(double)), b_map = al((size_t)nch * G), b_cnt = 256;
    void *w = nullptr;
    rc = ws_get(ctx, vbx_ctx::WS_PATH, b_psi + 3 * b_d + 2 * b_i + b_mask + b_lead + b_cpk + b_spk + 2 * b_map + b_cnt, &w);
    if (rc != VBX_SUCCESS) return rc;
    char *p = static_cast<char *>(w);
    pp_par_t &P = S.P;
    P = pp_par_t{};
    P.psi = reinterpret_cast<uint8_t *>(p); p += b_psi;
    P.entry = reinterpret_cast<double *>(p); p += b_d;
    P.exitd = reinterpret_cast<double *>(p); p += b_d;
    P.want = reinterpret_cast<double *>(p); p += b_d;
    P.exact = reinterpret_cast<int32_t *>(p); p += b_i;
    P.redo = reinterpret_cast<int32_t *>(p); p += b_i;
    P.mask = reinterpret_cast<unsigned long long *>(p); p += b_mask;
    P.lead = reinterpret_cast<int32_t *>(p); p += b_lead;
    S.cpk = reinterpret_cast<double *>(p); p += b_cpk;
    P.spk = reinterpret_cast<double *>(p); p += b_spk;
    S.map_a = reinterpret_cast<uint8_t *>(p); p += b_map;
    S.map_b = reinterpret_cast<uint8_t *>(p); p += b_map;
    P.redone = reinterpret_cast<unsigned long long *>(p);
    P.cand = reinterpret_cast<const pitch_t *>(cand); P.count = count; P.status = status; P.lpk = local_peak;
    P.F = F; P.kmax = (int)kmax; P.use_u = (local_peak != nullptr && pr.silence_threshold != 0.0) ? 1 : 0;
    const double corr = 0.01 / pr.time_step;                   // the host constants of the definition, in its order
    P.vt = pr.voicing_threshold; P.oc = pr.octave_cost;
    P.cvu = pr.voiced_unvoiced_cost * corr; P.cj = pr.octave_jump_cost * corr;
    P.Lc = std::log2(pr.ceiling_hz); P.q = pr.silence_threshold / (1.0 + pr.voicing_threshold);
    P.ch = reinterpret_cast<const pp_chunk_t *>(dtab); P.nch = nch;
    S.G = G; S.nch = nch; S.nseg = nseg; S.max_per_seg = max_per_seg; S.n_guessed = n_guessed;
    return VBX_SUCCESS;
}

// the forward scan: P per segment (seg_peak, when given, in its place), the speculative chunks, the repair rounds and the sweep
static int pp_scan(vbx_ctx *ctx, hipStream_t st, const pp_plan_t &S, const double *seg_peak) {
    const pp_par_t &P = S.P;
    const long W = VBX_PP_WARM;
    VBX_HIP(ctx, hipMemsetAsync(P.redone, 0, sizeof(unsigned long long), st));
    if (P.use_u && seg_peak != nullptr)
        VBX_HIP(ctx, hipMemcpyAsync(const_cast<double *>(P.spk), seg_peak, S.nseg * sizeof(double), hipMemcpyDeviceToDevice, st));
    else if (P.use_u) { Prof pf(ctx, "pitch_path_peak", st); launch_pitch_path_peak(st, P, S.d_seg_chunk0, (long)S.nseg, S.cpk); }
    { Prof pf(ctx, "pitch_path_spec", st); launch_pitch_path_spec(st, P, S.G, W); }
    if (S.n_guessed > 0) {
        const int rounds = (P.F / (long)S.nseg > 8192) ? VBX_PP_ROUNDS_LONG : VBX_PP_ROUNDS;
        for (int r = 0; r < rounds; r++) {
            { Prof pf(ctx, "pitch_path_check", st); launch_pitch_path_check(st, P, S.G); }
            { Prof pf(ctx, "pitch_path_repair", st); launch_pitch_path_repair(st, P, S.G); }
        }
        { Prof pf(ctx, "pitch_path_check", st); launch_pitch_path_check(st, P, S.G); launch_pitch_path_mask(st, P); }
        { Prof pf(ctx, "pitch_path_sweep", st); launch_pitch_path_sweep(st, P, S.G, S.d_seg_chunk0, (long)S.nseg); }
    }
    return VBX_SUCCESS;
}

// the back-maps and their suffix composition: S.map_a then holds, per chunk, the map to its last frame's state from its
// utterance's end state -- constant (the leader's) unless open: then the last chunk's utterance ends on another rank
static void pp_maps(vbx_ctx *ctx, hipStream_t st, pp_plan_t &S, bool open) {
    { Prof pf(ctx, "pitch_path_backtrack", st); launch_pitch_path_map(st, S.P, S.G, S.map_a); }
    if (open) { Prof pf(ctx, "pitch_path_open_map", st); launch_pitch_path_open_map(st, S.map_a, S.nch - 1, S.G); }
    for (long d = 1; d < S.max_per_seg; d <<= 1) {
        { Prof pf(ctx, "pitch_path_compose", st); launch_pitch_path_compose(st, S.nch, S.G, S.map_a, S.map_b, d); }
        std::swap(S.map_a, S.map_b);
    }
}

// the launches (arguments checked by the caller).  out_path rows lie path_ld doubles apart: 2 for the dense rows of vbx_pitch_path_f64,
// record_ld for columns 0-1 of the frame records.  Leaves ctx->lpc_list_armed alone: the tracked frame loop reports its LPC probe.
int run_pitch_path(vbx_ctx *ctx, hipStream_t st, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                   size_t n_frames, size_t kmax, const double *local_peak, const int64_t *h_seg_start, size_t n_segments,
                   const vbx_pitch_path_params &pr, vbx_pitch *out_path, size_t path_ld, int32_t *out_index, const char *fn) {
    pp_plan_t S;
    int rc = pp_setup(ctx, st, cand, count, status, n_frames, kmax, local_peak, h_seg_start, n_segments, pr, 0, S);
    if (rc != VBX_SUCCESS) return rc;
    rc = pp_scan(ctx, st, S, nullptr);
    if (rc != VBX_SUCCESS) return rc;
    pp_maps(ctx, st, S, false);
    { Prof pf(ctx, "pitch_path_write", st); launch_pitch_path_write(st, S.P, S.G, S.map_a, reinterpret_cast<pitch_t *>(out_path), (long)path_ld, out_index); }
    ctx->path_redone = S.P.redone;
    ctx->path_last = true;
    return check_launch(ctx, fn);
}

}  // namespace vbx

extern "C" {

int vbx_frame_peak_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride, double *out_peak) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc == 1) return VBX_SUCCESS;
    if (rc != VBX_SUCCESS) return rc;
    VBX_REQUIRE(ctx, out_peak != nullptr, "null out_peak");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "frame_peak"); launch_frame_peak(ctx->stream, x, (long)n_frames, (long)frame_len, (long)stride, out_peak); }
    return check_launch(ctx, __func__);
}

int vbx_pitch_path_f64(vbx_ctx *ctx, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                       size_t n_frames, size_t kmax, const double *local_peak,
                       const int64_t *h_seg_start, size_t n_segments, const vbx_pitch_path_params *h_params,
                       vbx_pitch *out_path, int32_t *out_index) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    ctx->path_last = false;
    ctx->lpc_list_armed = false;
    ctx->shard.live = false;
    VBX_REQUIRE(ctx, h_params != nullptr, "null params");
    int rc = check_pitch_path(ctx, __func__, *h_params, n_frames, kmax, local_peak != nullptr, h_seg_start, n_segments);
    if (rc != VBX_SUCCESS) return rc;
    if (n_frames == 0) { ctx->path_redone = nullptr; ctx->path_last = true; return VBX_SUCCESS; }
    VBX_REQUIRE(ctx, cand != nullptr && count != nullptr && out_path != nullptr, "null argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    return run_pitch_path(ctx, ctx->stream, cand, count, status, n_frames, kmax, local_peak, h_seg_start, n_segments, *h_params,
                          out_path, 2, out_index, __func__);
}

// ---- the pitch path across shard cuts (header: "The pitch path across a shard cut") ----------

int vbx_pitch_path_segment_peaks_f64(vbx_ctx *ctx, const double *local_peak, size_t n_frames, const int64_t *h_seg_start,
                                     size_t n_segments, double *out_peak) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_REQUIRE(ctx, n_frames <= 0x7fffffffull, "too many frames for one launch");
    const bool segmented = h_seg_start != nullptr && n_segments > 0;
    if (segmented) {
        VBX_REQUIRE(ctx, h_seg_start[0] == 0, "seg_start[0] must be 0");
        for (size_t i = 1; i < n_segments; i++)
            VBX_REQUIRE(ctx, h_seg_start[i] >= h_seg_start[i - 1] && (size_t)h_seg_start[i] <= n_frames, "seg_start must ascend within [0, n_frames]");
    }
    VBX_REQUIRE(ctx, out_peak != nullptr && (local_peak != nullptr || n_frames == 0), "null argument");
    ctx->path_last = false;
    ctx->lpc_list_armed = false;
    ctx->shard.live = false;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nseg = segmented ? n_segments : 1;
    if (n_frames == 0) {                                       // no frames: every segment's max is NaN (all bits set is one)
        VBX_HIP(ctx, hipMemsetAsync(out_peak, 0xff, nseg * sizeof(double), ctx->stream));
        return VBX_SUCCESS;
    }
    vbx_pitch_path_params pr{};                                // only the chunk table is used: the library's chunk length
    pr.time_step = 0.01; pr.ceiling_hz = 600.0;
    pp_plan_t S;
    int rc = pp_setup(ctx, ctx->stream, nullptr, nullptr, nullptr, n_frames, 1, local_peak, h_seg_start, n_segments, pr, 0, S);
    if (rc != VBX_SUCCESS) return rc;
    S.P.spk = out_peak;
    { Prof pf(ctx, "pitch_path_segment_peaks"); launch_pitch_path_peak(ctx->stream, S.P, S.d_seg_chunk0, (long)nseg, S.cpk); }
    return check_launch(ctx, __func__);
}

int vbx_pitch_path_shard_begin_f64(vbx_ctx *ctx, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                                   size_t n_frames, size_t kmax, const double *local_peak, const double *seg_peak,
                                   const int64_t *h_seg_start, size_t n_segments, const vbx_pitch_path_params *h_params,
                                   size_t first, int continues_prev, int continues_next) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    ctx->path_last = false;
    ctx->lpc_list_armed = false;
    ctx->shard.live = false;
    VBX_REQUIRE(ctx, h_params != nullptr, "null params");
    int rc = check_pitch_path(ctx, __func__, *h_params, n_frames, kmax, local_peak != nullptr, h_seg_start, n_segments);
    if (rc != VBX_SUCCESS) return rc;
    const bool segmented = h_seg_start != nullptr && n_segments > 0;
    VBX_REQUIRE(ctx, first <= n_frames, "first must be <= n_frames");
    VBX_REQUIRE(ctx, !continues_prev || first >= 1, "continues_prev needs first >= 1: the frame before the cut must be analysed here too");
    VBX_REQUIRE(ctx, !(continues_prev || continues_next) || n_frames >= 1, "a continued utterance needs n_frames >= 1");
    if (segmented && continues_prev)                           // frames [0, first] are one utterance: the one that is entered
        for (size_t i = 1; i < n_segments; i++)
            VBX_REQUIRE(ctx, h_seg_start[i] == 0 || (size_t)h_seg_start[i] > first, "continues_prev: an utterance starts within [1, first]");
    if (segmented && continues_next)
        VBX_REQUIRE(ctx, (size_t)h_seg_start[n_segments - 1] < n_frames, "continues_next: the last utterance is empty");
    VBX_REQUIRE(ctx, n_frames == 0 || (cand != nullptr && count != nullptr), "null argument");
    auto &sh = ctx->shard;
    sh.S = pp_plan_t{};
    sh.prev = continues_prev ? 1 : 0; sh.next = continues_next ? 1 : 0; sh.entered = false;
    ctx->path_redone = nullptr;
    if (n_frames > 0) {
        VBX_HIP(ctx, hipSetDevice(ctx->device));
        rc = pp_setup(ctx, ctx->stream, cand, count, status, n_frames, kmax, local_peak, h_seg_start, n_segments, *h_params, first, sh.S);
        if (rc != VBX_SUCCESS) return rc;
        rc = pp_scan(ctx, ctx->stream, sh.S, seg_peak);
        if (rc != VBX_SUCCESS) return rc;
        ctx->path_redone = sh.S.P.redone;
        rc = check_launch(ctx, __func__);
        if (rc != VBX_SUCCESS) return rc;
    }
    ctx->path_last = true;
    sh.live = true;
    return VBX_SUCCESS;
}

int vbx_pitch_path_shard_enter_f64(vbx_ctx *ctx, const double *d_state_in, double *d_state_out, int32_t *d_back_map, int32_t *d_changed) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    auto &sh = ctx->shard;
    VBX_REQUIRE(ctx, sh.live, "no vbx_pitch_path_shard_begin_f64 scan to continue (another path or frame-batch call came between)");
    VBX_REQUIRE(ctx, (d_state_in != nullptr) == (sh.prev != 0), "d_state_in must be given exactly when the shard continues its predecessor's utterance");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    pp_plan_t &S = sh.S;
    if (d_changed != nullptr) VBX_HIP(ctx, hipMemsetAsync(d_changed, 0, sizeof(int32_t), st));
    if (sh.prev && S.c_first < S.nch) {
        Prof pf(ctx, "pitch_path_enter", st);
        launch_pitch_path_enter(st, S.P, S.G, S.c_first, S.c_end, d_state_in, d_changed);
    }
    if (S.nch > 0) pp_maps(ctx, st, S, sh.next != 0);          // from psi: calling enter again rebuilds them
    sh.entered = true;
    if (d_state_out != nullptr || d_back_map != nullptr) {
        // the exit state: the last chunk's -- or, with no frame of its own (first == n_frames), the state that came in;
        // the back map: that of the chunk that ends at frame first - 1
        const bool pass = sh.prev && S.c_first == S.nch;
        const double *src = pass ? d_state_in : (S.nch > 0) ? S.P.exitd + (S.nch - 1) * S.G : nullptr;
        const uint8_t *map = (S.nch > 0 && S.c_first >= 1) ? S.map_a + (S.c_first - 1) * S.G : nullptr;
        Prof pf(ctx, "pitch_path_export", st);
        launch_pitch_path_export(st, src, pass ? 64 : S.G, map, S.G, d_state_out, d_back_map);
    }
    return check_launch(ctx, __func__);
}

int vbx_pitch_path_shard_finish_f64(vbx_ctx *ctx, const int32_t *d_end_state, vbx_pitch *out_path, size_t path_ld, int32_t *out_index) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    auto &sh = ctx->shard;
    VBX_REQUIRE(ctx, sh.live, "no vbx_pitch_path_shard_begin_f64 scan to finish (another path or frame-batch call came between)");
    VBX_REQUIRE(ctx, sh.entered, "vbx_pitch_path_shard_enter_f64 has not run");
    VBX_REQUIRE(ctx, (d_end_state != nullptr) == (sh.next != 0), "d_end_state must be given exactly when the last utterance continues on the next shard");
    VBX_REQUIRE(ctx, path_ld >= 2, "path_ld must be >= 2");
    pp_plan_t &S = sh.S;
    if (S.c_first >= S.nch) return VBX_SUCCESS;                // no frame of its own
    VBX_REQUIRE(ctx, out_path != nullptr, "null out_path");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    { Prof pf(ctx, "pitch_path_select", st); launch_pitch_path_select(st, S.map_a, S.c_first, S.nch, S.G, d_end_state, S.map_b); }
    pp_par_t Q = S.P;                                          // the chunks from `first` on: rows [0, first) are not written
    Q.ch += S.c_first; Q.nch -= S.c_first;
    { Prof pf(ctx, "pitch_path_write", st);
      launch_pitch_path_write(st, Q, S.G, S.map_b + S.c_first * S.G, reinterpret_cast<pitch_t *>(out_path), (long)path_ld, out_index); }
    return check_launch(ctx, __func__);
}

int vbx_internal_last_path_chunks_redone(vbx_ctx *ctx, int64_t *h_out) {
    VBX_REQUIRE(ctx, ctx && h_out, "null argument");
    *h_out = -1;
    if (!ctx->path_last) return VBX_SUCCESS;
    *h_out = 0;
    if (!ctx->path_redone) return VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long v = 0;
    VBX_HIP(ctx, hipMemcpy(&v, ctx->path_redone, sizeof(v), hipMemcpyDeviceToHost));
    *h_out = (int64_t)v;
    return VBX_SUCCESS;
}

}  // extern "C"

// ---- the online pitch path (header: "the pitch path while the lists arrive") --------------------

namespace vbx {

int path_stream_open(vbx_ctx *ctx, const char *fn, size_t kmax, const vbx_pitch_path_params &pr, double peak_ref, size_t max_pending,
                     vbx_path_stream **out) {
    int rc = check_pitch_path(ctx, fn, pr, 0, kmax, true, nullptr, 0);
    if (rc != VBX_SUCCESS) return rc;
    if (max_pending < 1 || max_pending > ((size_t)1 << 24)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": max_pending must be in [1, 2^24]");
    if (pr.silence_threshold > 0.0 && !(std::isfinite(peak_ref) && peak_ref >= 0.0))
        return fail(ctx, VBX_E_INVALID, std::string(fn) + ": silence_threshold > 0 needs a finite peak_ref >= 0");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    vbx_path_stream *ps = new vbx_path_stream();
    ps->ctx = ctx; ps->kmax = kmax; ps->max_pending = max_pending; ps->pr = pr; ps->peak_ref = peak_ref;
    while (ps->G < (int)kmax + 1) ps->G <<= 1;
    const size_t G = (size_t)ps->G, b_st = (sizeof(pp_online_state_t) + 255) & ~(size_t)255, b_row = max_pending * G * sizeof(pitch_t),
                 b_psi = max_pending * G;
    hipError_t e = hipMalloc(&ps->mem, b_st + b_row + 2 * b_psi);
    if (e == hipSuccess) e = hipMemsetAsync(ps->mem, 0, b_st, ctx->stream);
    if (e != hipSuccess) {
        if (ps->mem) { hipStreamSynchronize(ctx->stream); hipFree(ps->mem); }
        delete ps;
        return fail(ctx, VBX_E_RUNTIME, std::string(fn) + ": " + hipGetErrorString(e));
    }
    char *p = static_cast<char *>(ps->mem);
    ps->O.st = reinterpret_cast<pp_online_state_t *>(p); p += b_st;
    ps->O.row = reinterpret_cast<pitch_t *>(p); p += b_row;
    ps->O.psi = reinterpret_cast<uint8_t *>(p); p += b_psi;
    ps->O.idx = reinterpret_cast<int8_t *>(p);
    ps->O.cap = (long)max_pending;
    ps->O.peak = peak_ref;
    *out = ps;
    return VBX_SUCCESS;
}

// one launch (arguments checked by the caller): n frames of lists, rows from row 0 of the outputs
int path_stream_launch(vbx_path_stream *ps, const char *fn, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                       const double *local_peak, size_t n, int end_utterance, vbx_pitch *out_path, size_t path_ld, int32_t *out_index,
                       uint8_t *out_forced, vbx_path_commit *d_commit) {
    vbx_ctx *ctx = ps->ctx;
    const vbx_pitch_path_params &pr = ps->pr;
    pp_par_t P{};
    P.cand = reinterpret_cast<const pitch_t *>(cand); P.count = count; P.status = status; P.lpk = local_peak;
    P.F = (long)n; P.kmax = (int)ps->kmax; P.use_u = (local_peak != nullptr && pr.silence_threshold != 0.0) ? 1 : 0;
    const double corr = 0.01 / pr.time_step;                   // the host constants of the definition, in its order (pp_setup)
    P.vt = pr.voicing_threshold; P.oc = pr.octave_cost;
    P.cvu = pr.voiced_unvoiced_cost * corr; P.cj = pr.octave_jump_cost * corr;
    P.Lc = std::log2(pr.ceiling_hz); P.q = pr.silence_threshold / (1.0 + pr.voicing_threshold);
    pp_online_t O = ps->O;
    O.end = end_utterance ? 1 : 0;
    O.out_path = reinterpret_cast<pitch_t *>(out_path); O.ld = (long)path_ld; O.out_index = out_index; O.out_forced = out_forced;
    O.commit = reinterpret_cast<pp_commit_t *>(d_commit);
    { Prof pf(ctx, "pitch_path_online"); launch_pitch_path_online(ctx->stream, P, ps->G, O); }
    return check_launch(ctx, fn);
}

// the same launch for the n_sel streams of a bound multi-channel session (they share kmax, the parameters, peak_ref and max_pending):
// ONE launch, block k scans rows [k * plane_frames, k * plane_frames + n) of the lists from ps[k]'s state into out[k]
int path_stream_launch_all(vbx_path_stream *const *ps, size_t n_sel, const char *fn, const vbx_pitch *cand, const int32_t *count,
                           const int32_t *status, const double *local_peak, size_t plane_frames, size_t n, int end_utterance,
                           const vbx_channel_path_outputs *out, size_t path_ld) {
    vbx_ctx *ctx = ps[0]->ctx;
    const vbx_pitch_path_params &pr = ps[0]->pr;
    pp_par_t P{};
    P.cand = reinterpret_cast<const pitch_t *>(cand); P.count = count; P.status = status; P.lpk = local_peak;
    P.F = (long)n; P.kmax = (int)ps[0]->kmax; P.use_u = (local_peak != nullptr && pr.silence_threshold != 0.0) ? 1 : 0;
    const double corr = 0.01 / pr.time_step;                   // the host constants of the definition, in its order (pp_setup)
    P.vt = pr.voicing_threshold; P.oc = pr.octave_cost;
    P.cvu = pr.voiced_unvoiced_cost * corr; P.cj = pr.octave_jump_cost * corr;
    P.Lc = std::log2(pr.ceiling_hz); P.q = pr.silence_threshold / (1.0 + pr.voicing_threshold);
    pp_online_t O = ps[0]->O;                                  // cap and peak; the pointers are each block's own
    O.end = end_utterance ? 1 : 0;
    O.ld = (long)path_ld;
    pp_online_all_t A{};
    A.plane_frames = (long)plane_frames;
    const char *mem0 = static_cast<const char *>(ps[0]->mem);
    A.off_row = (size_t)(reinterpret_cast<const char *>(ps[0]->O.row) - mem0);
    A.off_psi = (size_t)(reinterpret_cast<const char *>(ps[0]->O.psi) - mem0);
    A.off_idx = (size_t)(reinterpret_cast<const char *>(ps[0]->O.idx) - mem0);
    for (size_t k = 0; k < n_sel; k++) {
        A.ch[k].mem = ps[k]->mem;
        A.ch[k].out_path = reinterpret_cast<pitch_t *>(out[k].out_path); A.ch[k].out_index = out[k].out_index;
        A.ch[k].out_forced = out[k].out_forced; A.ch[k].commit = reinterpret_cast<pp_commit_t *>(out[k].d_commit);
    }
    { Prof pf(ctx, "pitch_path_online_all"); launch_pitch_path_online_all(ctx->stream, P, ps[0]->G, O, A, (int)n_sel); }
    return check_launch(ctx, fn);
}

int path_stream_reset(vbx_path_stream *ps) {
    VBX_HIP(ps->ctx, hipSetDevice(ps->ctx->device));
    VBX_HIP(ps->ctx, hipMemsetAsync(ps->mem, 0, sizeof(pp_online_state_t), ps->ctx->stream));
    return VBX_SUCCESS;
}

void path_stream_free(vbx_path_stream *ps) {
    hipSetDevice(ps->ctx->device);
    hipStreamSynchronize(ps->ctx->stream);                // queued pushes may still use the ring
    if (ps->mem) hipFree(ps->mem);
    delete ps;
}

}  // namespace vbx

extern "C" {

int vbx_path_stream_open(vbx_ctx *ctx, size_t kmax, const vbx_pitch_path_params *h_params, double peak_ref, size_t max_pending,
                         vbx_path_stream **out) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, "vbx_path_stream_open: null context");
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    *out = nullptr;
    VBX_REQUIRE(ctx, h_params != nullptr, "null params");
    return path_stream_open(ctx, __func__, kmax, *h_params, peak_ref, max_pending, out);
}

int vbx_path_stream_push(vbx_path_stream *ps, const vbx_pitch *cand, const int32_t *count, const int32_t *status, const double *local_peak,
                         size_t n_frames, int end_utterance, vbx_pitch *out_path, size_t path_ld, int32_t *out_index, uint8_t *out_forced,
                         vbx_path_commit *d_commit) {
    if (!ps) return fail(nullptr, VBX_E_INVALID, "vbx_path_stream_push: null stream");
    vbx_ctx *ctx = ps->ctx;
    VBX_REQUIRE(ctx, out_path != nullptr && d_commit != nullptr, "null out_path or d_commit");
    VBX_REQUIRE(ctx, path_ld >= 2, "path_ld must be >= 2");
    VBX_REQUIRE(ctx, n_frames == 0 || (cand != nullptr && count != nullptr), "null cand or count");
    VBX_REQUIRE(ctx, !(ps->pr.silence_threshold > 0.0 && n_frames > 0 && local_peak == nullptr), "silence_threshold > 0 needs local_peak");
    VBX_REQUIRE(ctx, n_frames <= ((size_t)1 << 40), "too many frames for one push");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    return path_stream_launch(ps, __func__, cand, count, status, local_peak, n_frames, end_utterance, out_path, path_ld, out_index, out_forced,
                              d_commit);
}

int vbx_path_stream_reset(vbx_path_stream *ps) {
    if (!ps) return fail(nullptr, VBX_E_INVALID, "vbx_path_stream_reset: null stream");
    return path_stream_reset(ps);
}

void vbx_path_stream_close(vbx_path_stream *ps) {
    if (ps) path_stream_free(ps);
}

}  // extern "C"
