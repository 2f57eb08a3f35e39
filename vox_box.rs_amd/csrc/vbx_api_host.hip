// vbx_api_host.hip -- host-resident recordings: unpack, pinned memory, vbx_analyze_host and vbx_analyze_host_channels.
#include "vbx_ctx.hpp"

#include <string>
#include <vector>

using namespace vbx;

// ---- host-resident recordings (header: "host-resident recordings") ---------------------------

namespace vbx {

// the accepted set: 1..5 and the three 8-bit formats (6 and 7 are the WAV tags of A-law and mu-law, NOT formats of this library)
bool sample_format_ok(int f) { return (f >= VBX_SAMPLE_PCM16 && f <= VBX_SAMPLE_F64) || f == VBX_SAMPLE_U8 || f == VBX_SAMPLE_ULAW || f == VBX_SAMPLE_ALAW; }
static bool sample_is_8bit(int f) { return f == VBX_SAMPLE_U8 || f == VBX_SAMPLE_ULAW || f == VBX_SAMPLE_ALAW; }
size_t sample_src_bytes(int f) { return sample_is_8bit(f) ? 1 : f == VBX_SAMPLE_PCM16 ? 2 : f == VBX_SAMPLE_PCM24 ? 3 : f == VBX_SAMPLE_F64 ? 8 : 4; }
// the typed plane the frame loop reads for a VBX_SAMPLE_* format (what launch_unpack writes): PCM24 / PCM32 / F64 / U8 unpack to f64,
// G.711 to the int16 plane of PCM16 (from there on it IS a PCM16 recording: the same kernels, the same dispatch)
sample_kind_t sample_plane_kind(int f) { return (f == VBX_SAMPLE_PCM16 || f == VBX_SAMPLE_ULAW || f == VBX_SAMPLE_ALAW) ? SAMPLE_PCM16 : f == VBX_SAMPLE_F32 ? SAMPLE_F32 : SAMPLE_F64; }
size_t sample_out_bytes(int f) { static const size_t bytes[3] = {8, 2, 4}; return bytes[sample_plane_kind(f)]; }

// the copy stream, the slots' events and the two raw slots of `bytes` each (grown on demand: both streams are drained first)
int ensure_host_slots(vbx_ctx *ctx, size_t bytes) {
    if (!ctx->copy) {
        VBX_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            VBX_HIP(ctx, hipEventCreateWithFlags(&ctx->host_ready[i], hipEventDisableTiming));
            VBX_HIP(ctx, hipEventCreateWithFlags(&ctx->host_freed[i], hipEventDisableTiming));
        }
    }
    if (ctx->host_raw_bytes >= bytes) return VBX_SUCCESS;
    VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VBX_HIP(ctx, hipStreamSynchronize(ctx->copy));
    for (int i = 0; i < 2; i++) if (ctx->host_raw[i]) { VBX_HIP(ctx, hipFree(ctx->host_raw[i])); ctx->host_raw[i] = nullptr; }
    ctx->host_raw_bytes = 0;
    const size_t cap = bytes + bytes / 8;
    for (int i = 0; i < 2; i++) VBX_HIP(ctx, hipMalloc(&ctx->host_raw[i], cap));
    ctx->host_raw_bytes = cap;
    return VBX_SUCCESS;
}

// a selection of channels: 1 <= n_sel <= min(channels, VBX_HOST_MAX_CHANNELS) distinct values in [0, channels)
bool channel_selection_ok(const int32_t *h_channels, size_t n_sel, int channels, unpack_sel_t *sel) {
    if (!h_channels || channels < 1 || n_sel < 1 || n_sel > (size_t)channels || n_sel > (size_t)VBX_HOST_MAX_CHANNELS) return false;
    for (size_t k = 0; k < n_sel; k++) {
        if (h_channels[k] < 0 || h_channels[k] >= channels) return false;
        for (size_t j = 0; j < k; j++) if (h_channels[j] == h_channels[k]) return false;
        sel->ch[k] = h_channels[k];
    }
    return true;
}

}  // namespace vbx

extern "C" {

static const char *const k_unpack_names[9] = {"", "unpack_pcm16", "unpack_pcm24", "unpack_pcm32", "unpack_f32", "unpack_f64",
                                              "unpack_u8", "unpack_ulaw", "unpack_alaw"};      // by sample_name_slot

int vbx_unpack_samples(vbx_ctx *ctx, const void *d_src, size_t n_sample_frames, int format, int channels, int channel, void *d_out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_REQUIRE(ctx, sample_format_ok(format), "unknown sample format");
    VBX_REQUIRE(ctx, channels >= 1 && channel >= 0 && channel < channels, "need channels >= 1 and 0 <= channel < channels");
    if (n_sample_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, d_src && d_out, "null argument");
    VBX_REQUIRE(ctx, format == VBX_SAMPLE_PCM24 || (uintptr_t)d_src % sample_src_bytes(format) == 0, "the source needs its type's alignment");
    VBX_REQUIRE(ctx, (uintptr_t)d_out % sample_out_bytes(format) == 0, "the destination needs its type's alignment");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, k_unpack_names[sample_name_slot(format)]); launch_unpack(ctx->stream, format, d_src, n_sample_frames, (size_t)channels, (size_t)channel, d_out); }
    return check_launch(ctx, __func__);
}

static const char *const k_unpack_all_names[9] = {"", "unpack_all_pcm16", "unpack_all_pcm24", "unpack_all_pcm32", "unpack_all_f32", "unpack_all_f64",
                                                  "unpack_all_u8", "unpack_all_ulaw", "unpack_all_alaw"};
static_assert(UNPACK_MAX_SEL == VBX_HOST_MAX_CHANNELS, "the selection is a kernel argument of VBX_HOST_MAX_CHANNELS entries");

int vbx_unpack_channels(vbx_ctx *ctx, const void *d_src, size_t n_sample_frames, int format, int channels, const int32_t *h_channels,
                        size_t n_sel, void *d_out, size_t plane_ld) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_REQUIRE(ctx, sample_format_ok(format), "unknown sample format");
    VBX_REQUIRE(ctx, channels >= 1, "need channels >= 1");
    unpack_sel_t sel{};
    VBX_REQUIRE(ctx, channel_selection_ok(h_channels, n_sel, channels, &sel),
                "need 1 <= n_sel <= min(channels, VBX_HOST_MAX_CHANNELS) distinct channels in [0, channels)");
    VBX_REQUIRE(ctx, plane_ld >= n_sample_frames, "plane_ld must be >= n_sample_frames");
    if (n_sample_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, d_src && d_out, "null argument");
    VBX_REQUIRE(ctx, format == VBX_SAMPLE_PCM24 || (uintptr_t)d_src % sample_src_bytes(format) == 0, "the source needs its type's alignment");
    VBX_REQUIRE(ctx, (uintptr_t)d_out % sample_out_bytes(format) == 0, "the destination needs its type's alignment");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, k_unpack_all_names[sample_name_slot(format)]);
      launch_unpack_all(ctx->stream, format, d_src, n_sample_frames, (size_t)channels, sel, n_sel, d_out, plane_ld); }
    return check_launch(ctx, __func__);
}

int vbx_malloc_host(vbx_ctx *ctx, void **out, size_t bytes) {
    VBX_REQUIRE(ctx, ctx && out, "null argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    VBX_HIP(ctx, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return VBX_SUCCESS;
}

int vbx_free_host(vbx_ctx *ctx, void *p) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (!p) return VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    VBX_HIP(ctx, hipHostFree(p));
    return VBX_SUCCESS;
}

// One selected channel of a host call: the caller's outputs, and where the tracked form keeps the channel's lists, counts, peaks and
// status rows of the WHOLE recording until the path has run (the caller's arrays, or a part of the context workspace).
struct host_chan_t {
    double *rec = nullptr;
    int32_t *st = nullptr;
    const vbx_pitch_track_outputs *out = nullptr;
    bool need_peak = false;
    vbx_pitch *g_cand = nullptr;
    double *g_peak = nullptr;
    int32_t *g_count = nullptr, *g_st = nullptr;
};

// vbx_analyze_host (sel null: channel h_fmt->channel, the per-channel unpack kernel) and vbx_analyze_host_channels (sel: the n_sel
// selected channels, one unpack_all launch per chunk) behind their own argument checks: chan holds n_sel entries.
static int analyze_host_impl(vbx_ctx *ctx, const char *fn, const void *h_audio, size_t n_sample_frames, const vbx_host_audio *h_fmt,
                             const unpack_sel_t *sel, size_t n_sel, size_t frame_len, size_t stride, const vbx_analysis_params *h_p,
                             const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, const int64_t *h_seg_start,
                             size_t n_segments, host_chan_t *chan, size_t record_ld) {
    VBX_REQUIRE_FN(ctx, fn, h_fmt->reserved == 0, "reserved must be 0");
    VBX_REQUIRE_FN(ctx, fn, h_fmt->chunk_frames == 0 || h_fmt->chunk_frames >= (size_t)VBX_SHARD_WARM_FRAMES, "chunk_frames must be 0 or >= VBX_SHARD_WARM_FRAMES");
    VBX_REQUIRE_FN(ctx, fn, h_p != nullptr, "null argument");
    const size_t F = vbx_frame_count(n_sample_frames, frame_len, stride);
    if (F == 0) {                                         // the resident call's empty batch: its checks, its state
        for (size_t k = 0; k < n_sel; k++) {
            int rc0 = analyze_ex(ctx, fn, frames_t(), 0, frame_len, stride, h_p, h_ext, h_track, h_seg_start, n_segments, chan[k].rec,
                                 record_ld, chan[k].st, chan[k].out);
            if (rc0 != VBX_SUCCESS) return rc0;
        }
        return VBX_SUCCESS;
    }
    // what the resident call rejects from its arguments alone, asked first: nothing is uploaded or written for such a call.  (What
    // only the parts themselves know -- orders, the resampled shape, the MFCC geometry -- is rejected by the first chunk's call,
    // which has written nothing of the caller's by then: its records are chunk-local.)
    VBX_REQUIRE_FN(ctx, fn, h_audio != nullptr, "null audio");
    VBX_REQUIRE_FN(ctx, fn, frame_len <= VBX_MAX_LONG_FRAME_LEN, "frame_len must be in [1, 67108864]");
    VBX_REQUIRE_FN(ctx, fn, F <= 0x7fffffffull, "too many frames for one launch");
    const size_t rec = vbx_record_doubles_ex(h_p, h_ext);
    VBX_REQUIRE_FN(ctx, fn, record_ld >= rec && record_ld % 2 == 0, "record_ld must be even and >= vbx_record_doubles(params)");
    for (size_t k = 0; k < n_sel; k++) {
        VBX_REQUIRE_FN(ctx, fn, chan[k].rec != nullptr, "null argument");
        VBX_REQUIRE_FN(ctx, fn, ((uintptr_t)chan[k].rec & 15) == 0, "records must be 16-byte aligned");
        for (size_t j = 0; j < k; j++) {                  // [F, record_ld] each
            const uintptr_t a = (uintptr_t)chan[j].rec, b = (uintptr_t)chan[k].rec, len = F * record_ld * sizeof(double);
            VBX_REQUIRE_FN(ctx, fn, a + len <= b || b + len <= a, "the channels' records overlap");
        }
    }
    VBX_REQUIRE_FN(ctx, fn, !h_p->formant_order || (h_p->n_est >= 1 && h_p->n_est <= VBX_FORMANT_SLOTS), "n_est must be in [1, 6]");
    const bool segmented = h_seg_start != nullptr && n_segments > 0;
    if (segmented) {
        VBX_REQUIRE_FN(ctx, fn, h_seg_start[0] == 0, "seg_start[0] must be 0");
        for (size_t i = 1; i < n_segments; i++)
            VBX_REQUIRE_FN(ctx, fn, h_seg_start[i] >= h_seg_start[i - 1] && (size_t)h_seg_start[i] <= F, "seg_start must ascend within [0, n_frames]");
    }
    vbx_pitch_path_params path{};
    size_t kmax = 0;
    if (h_track) {
        kmax = h_track->kmax; path = h_track->path;
        if (path.time_step == 0.0) path.time_step = (double)stride / h_p->sample_rate;        // the batch's own hop
        int rc = check_pitch_path(ctx, fn, path, F, kmax, true, h_seg_start, n_segments);
        if (rc != VBX_SUCCESS) return rc;
        for (size_t k = 0; k < n_sel; k++) chan[k].need_peak = path.silence_threshold != 0.0 || (chan[k].out && chan[k].out->peak);
    }
    VBX_HIP(ctx, hipSetDevice(ctx->device));

    const int fmt = h_fmt->format;
    const size_t C = (size_t)h_fmt->channels, ch = (size_t)h_fmt->channel;
    size_t cf = h_fmt->chunk_frames ? h_fmt->chunk_frames : (size_t)VBX_HOST_DEFAULT_CHUNK_FRAMES;
    if (cf > F) cf = F;                                   // one chunk (and no overflow in the sizes below)
    const size_t nc = (F + cf - 1) / cf;
    const size_t nmax = (nc == 1) ? F : (cf + VBX_SHARD_WARM_FRAMES < F ? cf + VBX_SHARD_WARM_FRAMES : F);
    const size_t ns_max = (nmax - 1) * stride + frame_len;                    // sample frames of the largest chunk
    const size_t sf_bytes = C * sample_src_bytes(fmt);                        // one interleaved sample frame
    // mono PCM16 / F32 / F64: the slot holds the frame loop's type already (an 8-bit slot never does: its bytes are always unpacked)
    const bool unpack = !(C == 1 && (fmt == VBX_SAMPLE_PCM16 || fmt == VBX_SAMPLE_F32 || fmt == VBX_SAMPLE_F64));
    int rc = ensure_host_slots(ctx, ns_max * sf_bytes);
    if (rc != VBX_SUCCESS) return rc;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // the typed planes, one per selected channel: a pitch that keeps every plane 256-byte aligned, so that each is read as a
    // resident recording of its own would be (the 1200-sample PCM16 / F32 shapes without a widening copy)
    const size_t plane_bytes = up(ns_max * sample_out_bytes(fmt));
    char *typed = nullptr;
    if (unpack) {
        void *t = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_HOST_TYPED, n_sel * plane_bytes, &t);
        if (rc != VBX_SUCCESS) return rc;
        typed = static_cast<char *>(t);
    }
    // chunk-local records and status rows (shared by the channels: the stream orders them); per channel the tracked form's
    // whole-recording arrays where the caller keeps none
    const size_t ld_c = rec + (rec & 1);
    const size_t b_rec = up(nmax * ld_c * sizeof(double)), b_st = up(3 * nmax * sizeof(int32_t));
    auto b_cand = [&](const host_chan_t &h) { return (h_track && !(h.out && h.out->cand)) ? up(F * kmax * sizeof(vbx_pitch)) : (size_t)0; };
    auto b_peak = [&](const host_chan_t &h) { return (h.need_peak && !(h.out && h.out->peak)) ? up(F * sizeof(double)) : (size_t)0; };
    auto b_count = [&](const host_chan_t &h) { return (h_track && !(h.out && h.out->count)) ? up(F * sizeof(int32_t)) : (size_t)0; };
    auto b_gst = [&](const host_chan_t &h) { return (h_track && !h.st) ? up(3 * F * sizeof(int32_t)) : (size_t)0; };
    size_t b_all = b_rec + b_st;
    for (size_t k = 0; k < n_sel; k++) b_all += b_cand(chan[k]) + b_peak(chan[k]) + b_count(chan[k]) + b_gst(chan[k]);
    void *w = nullptr;
    rc = ws_get(ctx, vbx_ctx::WS_HOST, b_all, &w);
    if (rc != VBX_SUCCESS) return rc;
    char *q = static_cast<char *>(w);
    double *c_rec = reinterpret_cast<double *>(q); q += b_rec;
    int32_t *c_st = reinterpret_cast<int32_t *>(q); q += b_st;
    for (size_t k = 0; k < n_sel; k++) {
        host_chan_t &h = chan[k];
        h.g_cand = h.out ? h.out->cand : nullptr;
        h.g_peak = (h.out && h.need_peak) ? h.out->peak : nullptr;
        h.g_count = h.out ? h.out->count : nullptr;
        h.g_st = h.st;
        if (b_cand(h)) { h.g_cand = reinterpret_cast<vbx_pitch *>(q); q += b_cand(h); }
        if (b_peak(h)) { h.g_peak = reinterpret_cast<double *>(q); q += b_peak(h); }
        if (b_count(h)) { h.g_count = reinterpret_cast<int32_t *>(q); q += b_count(h); }
        if (b_gst(h)) { h.g_st = reinterpret_cast<int32_t *>(q); q += b_gst(h); }
    }

    vbx_shard_plan_t pl{};
    size_t s0 = 0, s1 = 0;
    auto upload = [&](size_t c) -> int {                  // chunk c's bytes into slot c & 1, on the copy stream
        vbx_shard_plan_t p{}; size_t a = 0, b = 0;
        if (vbx_host_chunk_plan(F, cf, c, frame_len, stride, h_seg_start, n_segments, &p, &a, &b) != VBX_SUCCESS)
            return fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad chunk plan");
        const int slot = (int)(c & 1);
        // behind the slot's last reader -- chunk c - 2's, or for the first two chunks the PREVIOUS call's last chunks, whose kernels may
        // still be queued when this call begins (an event that was never recorded is complete)
        VBX_HIP(ctx, hipStreamWaitEvent(ctx->copy, ctx->host_freed[slot], 0));
        VBX_HIP(ctx, hipMemcpyAsync(ctx->host_raw[slot], static_cast<const char *>(h_audio) + a * sf_bytes, (b - a) * sf_bytes,
                                    hipMemcpyHostToDevice, ctx->copy));
        VBX_HIP(ctx, hipEventRecord(ctx->host_ready[slot], ctx->copy));
        return VBX_SUCCESS;
    };
    auto bail = [&](int code) { hipStreamSynchronize(ctx->copy); return code; };      // h_audio is not read after the call returns
    std::vector<int64_t> lseg;
    rc = upload(0);
    if (rc != VBX_SUCCESS) return bail(rc);
    for (size_t c = 0; c < nc; c++) {
        // the next chunk's upload is issued first: this chunk's analysis may block the host on its segment list's upload
        if (c + 1 < nc) { rc = upload(c + 1); if (rc != VBX_SUCCESS) return bail(rc); }
        if (vbx_host_chunk_plan(F, cf, c, frame_len, stride, h_seg_start, n_segments, &pl, &s0, &s1) != VBX_SUCCESS)
            return bail(fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad chunk plan"));
        const int slot = (int)(c & 1);
        const size_t first = pl.lo - pl.warm, n = pl.hi - first, own = pl.hi - pl.lo;
        VBX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->host_ready[slot], 0));
        if (unpack) {
            if (sel) { Prof p(ctx, k_unpack_all_names[sample_name_slot(fmt)]);
                       launch_unpack_all(ctx->stream, fmt, ctx->host_raw[slot], s1 - s0, C, *sel, n_sel, typed, plane_bytes / sample_out_bytes(fmt)); }
            else { Prof p(ctx, k_unpack_names[sample_name_slot(fmt)]); launch_unpack(ctx->stream, fmt, ctx->host_raw[slot], s1 - s0, C, ch, typed); }
            VBX_HIP(ctx, hipEventRecord(ctx->host_freed[slot], ctx->stream));
        }
        const int64_t *seg_c = nullptr; size_t nseg_c = 0;
        if (segmented) {
            size_t need = 0;
            vbx_shard_local_segments(&pl, h_seg_start, n_segments, nullptr, 0, &need);
            lseg.resize(need);
            if (vbx_shard_local_segments(&pl, h_seg_start, n_segments, lseg.data(), need, &need) != VBX_SUCCESS)
                return bail(fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad chunk plan"));
            seg_c = lseg.data(); nseg_c = need;
        }
        // the selected channels one after another: the chunk-local rows are reused, and a channel's stitch directly follows its own
        // frame loop (it reads the resonance rows the context still holds)
        for (size_t k = 0; k < n_sel; k++) {
            const host_chan_t &h = chan[k];
            const void *xs = unpack ? static_cast<const void *>(typed + k * plane_bytes) : ctx->host_raw[slot];
            vbx_pitch_track_outputs to{};
            if (h_track) { to.cand = h.g_cand + first * kmax; to.count = h.g_count + first; to.peak = h.g_peak ? h.g_peak + first : nullptr; }
            rc = analyze_ex(ctx, fn, frames_t(xs, sample_plane_kind(fmt)), n, frame_len, stride, h_p, h_ext, h_track, seg_c, nseg_c, c_rec, ld_c, c_st,
                            h_track ? &to : nullptr, true);
            if (rc != VBX_SUCCESS) return bail(rc);
            if (!unpack) VBX_HIP(ctx, hipEventRecord(ctx->host_freed[slot], ctx->stream));      // (mono: the one channel read the slot itself)
            // a cut inside an utterance: the tracker continues from the true state, the row before the cut (already in place)
            if (pl.continues_prev && h_p->formant_order) {
                rc = vbx_internal_track_stitch(ctx, nullptr, reinterpret_cast<vbx_resonance *>(c_rec + 2), n, ld_c, pl.warm, pl.stop,
                                               h.rec + (pl.lo - 1) * record_ld + 2, nullptr);
                if (rc != VBX_SUCCESS) return bail(rc);
            }
            { Prof p(ctx, "host_rows");
              launch_host_rows(ctx->stream, c_rec, ld_c, pl.warm, own, h_track ? 2 : 0, rec, h.rec + pl.lo * record_ld, record_ld,
                               c_st, n, h.g_st ? h.g_st + pl.lo : nullptr, F); }
        }
    }
    rc = check_launch(ctx, fn);
    if (rc != VBX_SUCCESS) return bail(rc);
    if (h_track) {
        // ONE path per channel over the whole recording's lists, behind the last chunk, straight into columns 0-1
        for (size_t k = 0; k < n_sel; k++) {
            const host_chan_t &h = chan[k];
            rc = run_pitch_path(ctx, ctx->stream, h.g_cand, h.g_count, h.g_st, F, kmax, h.g_peak, h_seg_start, n_segments, path,
                                reinterpret_cast<vbx_pitch *>(h.rec), record_ld, h.out ? h.out->index : nullptr, fn);
            if (rc != VBX_SUCCESS) return bail(rc);
        }
    }
    ctx->last_track.res = nullptr;                        // the chunk-local rows are no track of the caller's: nothing to stitch
    ctx->last_track.n_est = 0;
    VBX_HIP(ctx, hipEventSynchronize(ctx->host_ready[(nc - 1) & 1]));      // the last byte of h_audio has been read
    return VBX_SUCCESS;
}

int vbx_analyze_host(vbx_ctx *ctx, const void *h_audio, size_t n_sample_frames, const vbx_host_audio *h_fmt, size_t frame_len, size_t stride,
                     const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                     const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld, int32_t *status3,
                     const vbx_pitch_track_outputs *h_outputs) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, "vbx_analyze_host: null context");
    VBX_REQUIRE(ctx, h_fmt != nullptr, "null format");
    VBX_REQUIRE(ctx, sample_format_ok(h_fmt->format), "unknown sample format");
    VBX_REQUIRE(ctx, h_fmt->channels >= 1 && h_fmt->channel >= 0 && h_fmt->channel < h_fmt->channels, "need channels >= 1 and 0 <= channel < channels");
    host_chan_t one;
    one.rec = out_records; one.st = status3; one.out = h_outputs;
    return analyze_host_impl(ctx, __func__, h_audio, n_sample_frames, h_fmt, nullptr, 1, frame_len, stride, h_p, h_ext, h_track, h_seg_start,
                             n_segments, &one, record_ld);
}

int vbx_analyze_host_channels(vbx_ctx *ctx, const void *h_audio, size_t n_sample_frames, const vbx_host_audio *h_fmt,
                              const int32_t *h_channels, size_t n_sel, size_t frame_len, size_t stride, const vbx_analysis_params *h_p,
                              const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, const int64_t *h_seg_start,
                              size_t n_segments, const vbx_channel_outputs *h_out, size_t record_ld) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, "vbx_analyze_host_channels: null context");
    VBX_REQUIRE(ctx, h_fmt != nullptr, "null format");
    VBX_REQUIRE(ctx, sample_format_ok(h_fmt->format), "unknown sample format");
    VBX_REQUIRE(ctx, h_fmt->channels >= 1 && h_fmt->channel == 0, "need channels >= 1 and channel == 0 (the selection is h_channels)");
    unpack_sel_t sel{};
    VBX_REQUIRE(ctx, channel_selection_ok(h_channels, n_sel, h_fmt->channels, &sel),
                "need 1 <= n_sel <= min(channels, VBX_HOST_MAX_CHANNELS) distinct channels in [0, channels)");
    VBX_REQUIRE(ctx, h_out != nullptr, "null outputs");
    host_chan_t chan[VBX_HOST_MAX_CHANNELS];
    for (size_t k = 0; k < n_sel; k++) { chan[k].rec = h_out[k].records; chan[k].st = h_out[k].status3; chan[k].out = h_out[k].outputs; }
    return analyze_host_impl(ctx, __func__, h_audio, n_sample_frames, h_fmt, &sel, n_sel, frame_len, stride, h_p, h_ext, h_track, h_seg_start,
                             n_segments, chan, record_ld);
}

}  // extern "C"
