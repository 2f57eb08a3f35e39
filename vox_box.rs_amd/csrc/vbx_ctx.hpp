// vbx_ctx.hpp -- what the host units of libvoxbox_hip.so (vbx_api*.hip, vbx_comm.hip) share: the context, the error and profile
// helpers, and every function one unit calls in another.  Each is defined once, in the unit named beside it.  No kernel unit
// includes this file.
#pragma once

#include "../../include/voxbox_hip.h"
#include "vbx_kernels.hpp"
#include "vbx_host.hpp"
#include "vbx_table_cache.hpp"

#include <hip/hip_runtime.h>

#include <functional>
#include <map>
#include <string>
#include <vector>

namespace vbx {

struct ProfRec { std::string name; hipEvent_t a, b; hipStream_t stream; };

// what one pitch path call works on: the kernels' arguments (pointers into WS_PATH and WS_PATH_TAB) and the chunk table's shape
struct pp_plan_t {
    pp_par_t P{};
    int G = 4;
    long nch = 0, max_per_seg = 1, n_guessed = 0;
    size_t nseg = 1;
    const int64_t *d_seg_chunk0 = nullptr;
    double *cpk = nullptr;                                // [nch] chunk peaks
    uint8_t *map_a = nullptr, *map_b = nullptr;           // [nch][G] each
    long c_first = 0, c_end = 0;                          // shard calls: the chunk that begins at `first` (nch: none), its utterance's end
};

}  // namespace vbx

struct vbx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    std::string last_error;
    size_t curve_failed_bytes = 0;                        // a WS_CURVE size hipMalloc refused (launch_spectral: not retried per call)
    std::string arch;
    int cu_count = 0;
    // workspaces (grown on demand, never shrunk)
    enum { WS_COEFFS, WS_RES, WS_COUNT, WS_STATUS, WS_MISC, WS_SEG, WS_EST, WS_UNSURE, WS_F32_IN, WS_F32_OUT, WS_TRK, WS_BURG_LIST, WS_ROOTS_LIST, WS_LONG, WS_LONG2, WS_CZT, WS_CURVE, WS_LPC_LIST, WS_PATH, WS_PATH_TAB, WS_TRACK, WS_EX, WS_HOST, WS_HOST_TYPED, WS_CLIPS_TAB, WS_CLIPS_PLANE, WS_CLIPS_ROWS, WS_CLIPS_LISTS, WS_RANGE_SEG, WS_N };
    void *ws[WS_N] = {nullptr};
    const int32_t *burg_list_count = nullptr;             // device counter of the last one-pass Burg call (tests)
    const int32_t *roots_list_count = nullptr;            // the same for the resonance kernel of find_formants
    size_t ws_bytes[WS_N] = {0};
    vbx::device_tables_t tables;                          // every host-built device table (vbx_table_cache.hpp)
    bool pitch_whole_curve = false;                       // VBX_PITCH_CURVE_CUT=0: the pow2 kernels keep every lag of the curve in LDS (tests)
    bool mfcc_czt_split = false;                          // VBX_MFCC_CZT_SPLIT=1: the two-block form of the chirp-z kernel wherever it fits (tests)
    int mfcc_czt = -1;                                    // VBX_MFCC_CZT=0 / 1: never / wherever it fits (tests); -1: the measured choice
    int last_mfcc_interp = 0;                             // the last vbx_mfcc_f64 call took the interpolated form (tests)
    int last_spectral_split = 0;                          // the last fused / pitch call ran as two kernels (tests)
    long last_batching[2] = {0, 0};                       // {launches, frames per launch} of the host loop that cut the last call's frames into the most launches (batch_count_t; tests)
    int last_autocorr_long_splits = 0;                    // partial sums per lag of the last long-frame autocorrelation launch, from its scratch size (tests)
    int last_analyze_spec = 0;                            // the instance of the 1200-point fused kernel launch_analyze took: 0 generic, 1 / 2 launch-specialised for f64 / PCM (tests)
    int spectral_spec = 1;                                // VBX_SPECTRAL_SPEC=0: the generic instance of the 1200-point fused kernel everywhere (A/B, tests)
    int last_mfcc_form = 0;                               // which kernel the last vbx_mfcc_f64 call launched: VBX_MFCC_FORM_* below (tests)
    int last_pitch_form = 0;                              // the same for vbx_pitch_f64: 100 * kernel family + candidate list form (tests)
    int mfcc_defer = 1;                                   // VBX_MFCC_DEFER=0: log10 + DCT of the fused call's MFCC rows inside the frame's wavefront (rounds 2-5; A/B)
    int lpc_policy = VBX_LPC_POLICY_EXACT;                // VBX_LPC_POLICY_*; VBX_LPC_EXACT=0 initialises PLAIN (no conditioning probe, no double-double redo:
                                                          //   the rows of rounds 1-5), vbx_ctx_set_lpc_policy overrides
    bool lpc_list_armed = false;                          // the last call that writes LPC rows from frames armed the probe's list (vbx_internal_last_lpc_exact_count)
    int pow2_split = -1;                                  // VBX_POW2_SPLIT=0: the 4096-point plan as ONE kernel (transforms and refinement fused, as before round 5; tests, A/B)
    int mfcc_interp = -1;                                 // VBX_MFCC_INTERP=0: never (the chirp-z kernel beside the fused one, as before round 5; tests, A/B)
    // timing
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool prof = false;
    // VBX_ROCTX=1: every kernel group of an entry point (the names vbx_profile_* reports) is also a roctx range, so that a
    // `rocprofv3 --marker-trace --kernel-trace` timeline shows which call a kernel belongs to
    int (*roctx_push)(const char *) = nullptr;
    int (*roctx_pop)() = nullptr;
    std::vector<vbx::ProfRec> recs;
    std::map<std::string, std::pair<double, long>> prof_acc;
    std::map<std::string, int> prof_stream;               // name -> 0: the context's stream, 1: the side stream, 2: the tracker's
    int boersma_group = 16;                               // lanes per refined entry of vbx_pitch_boersma_f64 from kmax 4 on (VBX_BOERSMA_GROUP=64: one entry per wavefront, A/B)
    bool pitch_force_mfma = false;                        // test hook: VBX_PITCH_MFMA=1 keeps the matrix-core pitch kernel on 1200-sample frames
    bool mfcc_force_goertzel = false;                     // test hooks: VBX_MFCC_GOERTZEL=1 / VBX_MFCC_DFT2=1 keep the
    bool mfcc_force_dft2 = false;                         //   fallback kernels covered on lengths the MFMA kernel takes
    bool mfcc_force_mfma = false;                         //   VBX_MFCC_MFMA=1: no FFT kernel for 1024 / 1200 / 2048 / 4096 (k_spectral*.hip)
    unsigned long long *pitch_work = nullptr;             // [PITCH_WORK_SLOTS][4], counted while profiling
    // second stream of vbx_analyze_frames_f64 (the formant chain runs beside the pitch kernel) + fork/join events
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_peak = nullptr;                         // vbx_analyze_frames_tracked_*: the side stream's frame peaks exist (the path waits for it)
    // the fused frame loop with Burg's lag sums from the analyze kernel (vbx_api_frames.hip): read once, at context creation
    int burg_fused = 1;                                   // VBX_BURG_FUSED=0: burg_lags_kernel beside the analyze kernel, as before (A/B, tests)
    // VBX_BURG_FUSED_MIN_FRAMES: calls of fewer frames keep that path (tests lower it).  The formant chain of the last launches runs behind the
    // analyze kernel with nothing to hide it (~2 ms), where the lag kernel beside the analyze kernel costs the call ~1 ms per million frames
    // more than the fused block does.  Measured at 1200 / 480 against the parent's path (profiles/burg_fused/by_length.txt):
    // 4 % slower at 1.08 M frames, equal at 2.16 M, 2.5 % faster at 4.5 M
    long burg_fused_min_frames = 3145728;
    long analyze_launch_frames = 524288;                  // VBX_ANALYZE_LAUNCH_FRAMES: frames per launch of the fused path (tests lower it)
    hipEvent_t ev_bf_launch[2] = {nullptr, nullptr};      // launch j has left its lag sums in scratch j & 1 (the side stream waits for it)
    hipEvent_t ev_bf_free[2] = {nullptr, nullptr};        // the recursion is through with that scratch (launch j + 2 waits for it)
    hipStream_t trk = nullptr;                            // the tracker's time slices (run_find_formants)
    hipEvent_t ev_slice[8] = {nullptr}, ev_trk = nullptr;
    // pinned staging of the small host arrays (segment starts, initial estimates): the caller's arrays may be
    // freed on return, and an upload whose content has not changed since the last call is skipped
    enum { N_STAGE = 5 };
    void *stage[N_STAGE] = {nullptr};                     // 0: segment starts, 1: initial estimates, 2: the pitch path's chunk table, 3: vbx_analyze_clips' clip table, 4: the fused frame loop's per-launch utterance starts
    size_t stage_cap[N_STAGE] = {0};
    std::vector<char> staged[N_STAGE];                    // content now on the device
    hipEvent_t stage_ev[N_STAGE] = {nullptr};             // completion of the last staged copy
    // what the tracker of the last find_formants / analyze_frames call ran on (vbx_track_stitch_f64 continues that track)
    struct { const vbx::res_t *res = nullptr; const int32_t *cnt = nullptr, *st = nullptr; long F = 0; int n_est = 0;
             vbx::res_t *out = nullptr; long out_ld = 0; } last_track;
    double *stitch_state = nullptr;                       // 2 * VBX_FORMANT_SLOTS doubles: the state a stitch received (vbx_comm.hip)
    // the last vbx_pitch_path_f64 call (vbx_internal_last_path_chunks_redone): its device counter, cleared by every frame-batch call
    const unsigned long long *path_redone = nullptr;
    bool path_last = false;
    // the scan vbx_pitch_path_shard_begin_f64 left in WS_PATH for _enter / _finish; any other path or frame-batch call ends it
    struct { bool live = false, entered = false; vbx::pp_plan_t S; int prev = 0, next = 0; } shard;
    // vbx_analyze_host: the copy stream, the two raw staging slots of a chunk's bytes and their events -- ready: the upload has
    // landed (the context's stream waits for it); freed: the slot's last reader on the context's stream is through (the copy stream
    // waits for it before the next upload into the slot)
    hipStream_t copy = nullptr;
    void *host_raw[2] = {nullptr, nullptr};
    size_t host_raw_bytes = 0;
    hipEvent_t host_ready[2] = {nullptr, nullptr}, host_freed[2] = {nullptr, nullptr};
};

// One contour that grows while its lists arrive.  The stream owns the carried state and the ring of max_pending frames (one
// allocation, made at open); a push is one launch of pp_online_kernel on the context's stream and touches nothing of the context's.
// (Here because a session reads max_pending and peak_ref of the path it owns; everything else about it is vbx_api_path.hip's.)
struct vbx_path_stream {
    vbx_ctx *ctx = nullptr;
    size_t kmax = 0, max_pending = 0;
    int G = 4;
    vbx_pitch_path_params pr{};
    double peak_ref = 0.0;
    void *mem = nullptr;                                  // pp_online_state_t, then the ring: row [cap][G], psi [cap][G], idx [cap][G]
    vbx::pp_online_t O{};
};

// the one hook that is both an exported symbol and called across units (vbx_api.hip; callers: host, session, vbx_comm.hip)
extern "C" int vbx_internal_track_stitch(vbx_ctx *ctx, void *stream, vbx_resonance *formants, size_t n_frames, size_t formants_ld,
                                         size_t first, size_t stop, const double *d_state_in, int32_t *d_changed);

namespace vbx {

// ---- errors (vbx_api.hip) ---------------------------------------------------------------------

// records msg as the thread's and the context's last error and returns code
int fail(vbx_ctx *ctx, int code, const std::string &msg);
int check_launch(vbx_ctx *ctx, const char *what);
// A host loop that cuts a call's frames into launches of `per` counts them as they happen (vbx_internal_last_batching): launched() once per
// trip, the record is made when the loop is left, however it is left.  A call that runs several such loops keeps the one with the most
// launches (the later one of two equals); check_frames clears the record.
inline void note_batching(vbx_ctx *ctx, long launches, long per) {
    if (launches > 0 && launches >= ctx->last_batching[0]) { ctx->last_batching[0] = launches; ctx->last_batching[1] = per; }
}
struct batch_count_t {
    vbx_ctx *ctx; long per, n = 0;
    batch_count_t(vbx_ctx *c, long frames_per_launch) : ctx(c), per(frames_per_launch) {}
    void launched() { n++; }
    ~batch_count_t() { note_batching(ctx, n, per); }
};

#define VBX_HIP(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return vbx::fail(ctx, VBX_E_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// "<fn>: <msg>" -- fn: the entry point's name where a helper checks on its caller's behalf
#define VBX_REQUIRE_FN(ctx, fn, cond, msg) \
    do { if (!(cond)) return vbx::fail(ctx, VBX_E_INVALID, std::string(fn) + ": " + (msg)); } while (0)
#define VBX_REQUIRE(ctx, cond, msg) VBX_REQUIRE_FN(ctx, __func__, cond, msg)

struct Prof {
    vbx_ctx *ctx; const char *name; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    Prof(vbx_ctx *c, const char *n, hipStream_t stream = nullptr) : ctx(c), name(n), st(stream ? stream : c->stream) {
        if (ctx->roctx_push) ctx->roctx_push(name);
        if (ctx->prof) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, st); }
    }
    ~Prof() {
        if (ctx->prof) { hipEventRecord(b, st); ctx->recs.push_back({name, a, b, st}); }
        if (ctx->roctx_pop) ctx->roctx_pop();
    }
};

// ---- workspaces, argument checks, staged uploads (vbx_api.hip) ---------------------------------

int ws_get(vbx_ctx *ctx, int slot, size_t bytes, void **out);
int get_bins_dev(vbx_ctx *ctx, size_t n, size_t k, double lo, double hi, double sr,
                 const int32_t **out, std::vector<int32_t> &host_bins, bool &bad);
int check_frames(vbx_ctx *ctx, const char *fn, const void *x, size_t n_frames, size_t frame_len, size_t stride,
                 size_t max_len = VBX_MAX_FRAME_LEN);
int stage_upload(vbx_ctx *ctx, int which, int ws_slot, const void *h_src, size_t bytes, hipStream_t st, void **d_out);
int upload_segments(vbx_ctx *ctx, hipStream_t st, const int64_t *h_seg, size_t n_seg, size_t n_frames, const int64_t **d_seg, size_t *n_out);
int upload_estimates(vbx_ctx *ctx, hipStream_t st, const vbx_resonance *h_est, size_t n_est, const res_t **d_est);

// ---- the single operations' runners (vbx_api.hip) ----------------------------------------------

struct resample_plan_t { resample_src_t rs; size_t n_src, m; bool direct; };

// launch_spectral in launches of rg->launch_frames frames, each leaving Burg's lag sums of its frames in scratch[j & 1] (spectral_launch_t:
// burg_*); before(j) / after(j, f0, nf) run around launch j's analyze kernel (the formant chain of those frames: find_formants_ranges_*)
struct analyze_ranges_t {
    long launch_frames; double *scratch[2]; const double *burg_window;
    std::function<int(int)> before; std::function<int(int, long, long)> after;
};
int launch_spectral(vbx_ctx *ctx, hipStream_t st, spectral_launch_t &L, const char *prof_name, const analyze_ranges_t *rg = nullptr);
// Would launch_spectral's launch of L take an instance that can leave Burg's lag sums?  (L as the caller hands it to launch_spectral)
bool spectral_burg_fusable_call(vbx_ctx *ctx, const spectral_launch_t &L);
// find_formants on the side stream behind the analyze kernel's launches, a range of frames at a time (vbx_api.hip): _begin takes the
// workspaces (the scratch ring among them), uploads and clears what run_find_formants would; _step runs the recursion, the direct list,
// the resonances and -- chunked scans -- the tracker of frames [f0, f0 + nf) from the lag sums launch j left; _end what is left.
struct formants_ranges_t {
    hipStream_t side; frames_t x; long F, stride; double sample_rate; int p, n_est;
    const double *hann; double *coeffs; res_t *res; int32_t *cnt, *st, *list, *redo; double *scratch[2];
    const res_t *d_est; const int64_t *d_seg; size_t nseg; bool chunked;
    res_t *out; long out_ld; void *trk_ws;
    const int64_t *d_range_seg; std::vector<size_t> off; std::vector<int64_t> stitch;
};
int find_formants_ranges_begin(vbx_ctx *ctx, hipStream_t side, frames_t x, size_t n_frames, size_t stride, double sample_rate, size_t n_coeffs,
                               const int64_t *h_seg_start, size_t n_segments, const vbx_resonance *h_est_init, size_t n_est,
                               vbx_resonance *out_formants, size_t formants_ld, int32_t *status, long launch_frames, formants_ranges_t *R);
int find_formants_ranges_step(vbx_ctx *ctx, formants_ranges_t *R, int j, long f0, long nf);
int find_formants_ranges_end(vbx_ctx *ctx, formants_ranges_t *R);
const char *pitch_shape_error(size_t frame_len, size_t kmax);
int run_pitch(vbx_ctx *ctx, hipStream_t st, const double *x, size_t n_frames, size_t frame_len, size_t stride,
              const double *window, double sample_rate, double threshold, double fmin, double fmax,
              size_t kmax, vbx_pitch *out_cand, size_t cand_ld, int32_t *out_count, int32_t *status);
bool lpc_order_ok(size_t frame_len, size_t n_coeffs);
int run_autocorr_lpc(vbx_ctx *ctx, hipStream_t st, const double *x, size_t n_frames, size_t frame_len,
                     size_t stride, const double *window, size_t n_coeffs, int normalize,
                     double *out_r, double *out_lpc, size_t lpc_ld);
bool burg_order_ok(size_t frame_len, size_t n_coeffs);
int run_burg(vbx_ctx *ctx, hipStream_t stm, frames_t x, long F, int n, long stride, const double *window, int p, double *coeffs,
             int32_t *st, frame_map_t map = frame_map_t{0, 0, 0}, const resample_plan_t *rp = nullptr);
int run_find_formants(vbx_ctx *ctx, hipStream_t stm, frames_t x, size_t n_frames, size_t frame_len,
                      size_t stride, double sample_rate, size_t n_coeffs,
                      const int64_t *h_seg_start, size_t n_segments,
                      const vbx_resonance *h_est_init, size_t n_est,
                      vbx_resonance *out_formants, size_t formants_ld, vbx_resonance *out_res, int32_t *out_res_count,
                      double *out_coeffs, int32_t *status,
                      const resample_plan_t *rp = nullptr /* find_formants on the frames' resampled view (run_burg) */);
int run_mfcc(vbx_ctx *ctx, hipStream_t stm, const double *x, size_t n_frames, size_t frame_len, size_t stride,
             const double *window, size_t num_coeffs, double lo_hz, double hi_hz,
             double sample_rate, double *out, size_t out_ld, int32_t *status);

// ---- the fused frame loop (vbx_api_frames.hip) -------------------------------------------------

int make_resample_plan(vbx_ctx *ctx, const char *fn, double ratio, size_t frame_len, size_t order, resample_plan_t *rp, bool *have);
int analyze_ex(vbx_ctx *ctx, const char *fn, frames_t x, size_t n_frames, size_t frame_len, size_t stride,
               const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
               const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld, int32_t *status3,
               const vbx_pitch_track_outputs *h_out, bool defer_path = false /* vbx_analyze_host's chunks: track_req_t */);

// ---- host-resident recordings (vbx_api_host.hip) -----------------------------------------------

bool sample_format_ok(int f);
// where the per-format tables of profile names keep a format's entry: 1..5 as they are, the 8-bit formats (16, 17, 18) at 6, 7, 8
inline int sample_name_slot(int f) { return f >= VBX_SAMPLE_U8 ? f - VBX_SAMPLE_U8 + 6 : f; }
size_t sample_src_bytes(int f);
sample_kind_t sample_plane_kind(int f);
size_t sample_out_bytes(int f);
int ensure_host_slots(vbx_ctx *ctx, size_t bytes);
// a selection of channels (vbx_unpack_channels' rules), copied into *sel
bool channel_selection_ok(const int32_t *h_channels, size_t n_sel, int channels, unpack_sel_t *sel);

// ---- the pitch path (vbx_api_path.hip) ---------------------------------------------------------

int check_pitch_path(vbx_ctx *ctx, const char *fn, const vbx_pitch_path_params &pr, size_t n_frames, size_t kmax, bool have_peak,
                     const int64_t *h_seg_start, size_t n_segments);
int run_pitch_path(vbx_ctx *ctx, hipStream_t st, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                   size_t n_frames, size_t kmax, const double *local_peak, const int64_t *h_seg_start, size_t n_segments,
                   const vbx_pitch_path_params &pr, vbx_pitch *out_path, size_t path_ld, int32_t *out_index, const char *fn);
int path_stream_open(vbx_ctx *ctx, const char *fn, size_t kmax, const vbx_pitch_path_params &pr, double peak_ref, size_t max_pending,
                     vbx_path_stream **out);
int path_stream_launch(vbx_path_stream *ps, const char *fn, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                       const double *local_peak, size_t n, int end_utterance, vbx_pitch *out_path, size_t path_ld, int32_t *out_index,
                       uint8_t *out_forced, vbx_path_commit *d_commit);
int path_stream_launch_all(vbx_path_stream *const *ps, size_t n_sel, const char *fn, const vbx_pitch *cand, const int32_t *count,
                           const int32_t *status, const double *local_peak, size_t plane_frames, size_t n, int end_utterance,
                           const vbx_channel_path_outputs *out, size_t path_ld);
int path_stream_reset(vbx_path_stream *ps);
void path_stream_free(vbx_path_stream *ps);

}  // namespace vbx
