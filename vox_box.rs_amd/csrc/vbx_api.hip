// vbx_api.hip -- host side of libvoxbox_hip.so: context, workspaces, host-built tables and
// the extern "C" entry points declared in include/voxbox_hip.h.  No CPU fallback: every
// numeric entry point launches gfx950 kernels on the context's stream.
#include "../../include/voxbox_hip.h"
#include "vbx_kernels.hpp"
#include "vbx_host.hpp"
#include "vbx_table_cache.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <string>
#include <vector>

using namespace vbx;

extern "C" const double VBX_MALE_FORMANT_ESTIMATES[4] = {320., 1440., 2760., 3200.};     // src/lib.rs:27
extern "C" const double VBX_FEMALE_FORMANT_ESTIMATES[4] = {480., 1760., 3200., 3520.};   // src/lib.rs:28

namespace {

thread_local std::string g_last_error;

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

}  // namespace

struct vbx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    std::string last_error;
    size_t curve_failed_bytes = 0;                        // a WS_CURVE size hipMalloc refused (launch_spectral: not retried per call)
    std::string arch;
    int cu_count = 0;
    // workspaces (grown on demand, never shrunk)
    enum { WS_COEFFS, WS_RES, WS_COUNT, WS_STATUS, WS_MISC, WS_SEG, WS_EST, WS_UNSURE, WS_F32_IN, WS_F32_OUT, WS_TRK, WS_BURG_LIST, WS_ROOTS_LIST, WS_LONG, WS_LONG2, WS_CZT, WS_CURVE, WS_LPC_LIST, WS_PATH, WS_PATH_TAB, WS_TRACK, WS_EX, WS_HOST, WS_HOST_TYPED, WS_N };
    void *ws[WS_N] = {nullptr};
    const int32_t *burg_list_count = nullptr;             // device counter of the last one-pass Burg call (tests)
    const int32_t *roots_list_count = nullptr;            // the same for the resonance kernel of find_formants
    size_t ws_bytes[WS_N] = {0};
    device_tables_t tables;                               // every host-built device table (vbx_table_cache.hpp)
    bool pitch_whole_curve = false;                       // VBX_PITCH_CURVE_CUT=0: the pow2 kernels keep every lag of the curve in LDS (tests)
    bool mfcc_czt_split = false;                          // VBX_MFCC_CZT_SPLIT=1: the two-block form of the chirp-z kernel wherever it fits (tests)
    int mfcc_czt = -1;                                    // VBX_MFCC_CZT=0 / 1: never / wherever it fits (tests); -1: the measured choice
    int last_mfcc_interp = 0;                             // the last vbx_mfcc_f64 call took the interpolated form (tests)
    int last_spectral_split = 0;                          // the last fused / pitch call ran as two kernels (tests)
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
    std::vector<ProfRec> recs;
    std::map<std::string, std::pair<double, long>> prof_acc;
    std::map<std::string, int> prof_stream;               // name -> 0: the context's stream, 1: the side stream, 2: the tracker's
    bool pitch_force_mfma = false;                        // test hook: VBX_PITCH_MFMA=1 keeps the matrix-core pitch kernel on 1200-sample frames
    bool mfcc_force_goertzel = false;                     // test hooks: VBX_MFCC_GOERTZEL=1 / VBX_MFCC_DFT2=1 keep the
    bool mfcc_force_dft2 = false;                         //   fallback kernels covered on lengths the MFMA kernel takes
    bool mfcc_force_mfma = false;                         //   VBX_MFCC_MFMA=1: no FFT kernel for 1024 / 1200 / 2048 / 4096 (k_spectral*.hip)
    unsigned long long *pitch_work = nullptr;             // [PITCH_WORK_SLOTS][4], counted while profiling
    // second stream of vbx_analyze_frames_f64 (the formant chain runs beside the pitch kernel) + fork/join events
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_peak = nullptr;                         // vbx_analyze_frames_tracked_*: the side stream's frame peaks exist (the path waits for it)
    hipStream_t trk = nullptr;                            // the tracker's time slices (run_find_formants)
    hipEvent_t ev_slice[8] = {nullptr}, ev_trk = nullptr;
    // pinned staging of the small host arrays (segment starts, initial estimates): the caller's arrays may be
    // freed on return, and an upload whose content has not changed since the last call is skipped
    void *stage[3] = {nullptr, nullptr, nullptr};         // 0: segment starts, 1: initial estimates, 2: the pitch path's chunk table
    size_t stage_cap[3] = {0, 0, 0};
    std::vector<char> staged[3];                          // content now on the device
    hipEvent_t stage_ev[3] = {nullptr, nullptr, nullptr}; // completion of the last staged copy
    // what the tracker of the last find_formants / analyze_frames call ran on (vbx_track_stitch_f64 continues that track)
    struct { const res_t *res = nullptr; const int32_t *cnt = nullptr, *st = nullptr; long F = 0; int n_est = 0;
             res_t *out = nullptr; long out_ld = 0; } last_track;
    double *stitch_state = nullptr;                       // 2 * VBX_FORMANT_SLOTS doubles: the state a stitch received (vbx_comm.hip)
    // the last vbx_pitch_path_f64 call (vbx_internal_last_path_chunks_redone): its device counter, cleared by every frame-batch call
    const unsigned long long *path_redone = nullptr;
    bool path_last = false;
    // the scan vbx_pitch_path_shard_begin_f64 left in WS_PATH for _enter / _finish; any other path or frame-batch call ends it
    struct { bool live = false, entered = false; pp_plan_t S; int prev = 0, next = 0; } shard;
    // vbx_analyze_host: the copy stream, the two raw staging slots of a chunk's bytes and their events -- ready: the upload has
    // landed (the context's stream waits for it); freed: the slot's last reader on the context's stream is through (the copy stream
    // waits for it before the next upload into the slot)
    hipStream_t copy = nullptr;
    void *host_raw[2] = {nullptr, nullptr};
    size_t host_raw_bytes = 0;
    hipEvent_t host_ready[2] = {nullptr, nullptr}, host_freed[2] = {nullptr, nullptr};
};

namespace {

int fail(vbx_ctx *ctx, int code, const std::string &msg) {
    g_last_error = msg;
    if (ctx) ctx->last_error = msg;
    return code;
}

#define VBX_HIP(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ctx, VBX_E_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define VBX_REQUIRE(ctx, cond, msg) \
    do { if (!(cond)) return fail(ctx, VBX_E_INVALID, std::string(__func__) + ": " + (msg)); } while (0)

int check_launch(vbx_ctx *ctx, const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, VBX_E_RUNTIME, std::string(what) + " launch: " + hipGetErrorString(e));
    return VBX_SUCCESS;
}

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

int ws_get(vbx_ctx *ctx, int slot, size_t bytes, void **out) {
    if (bytes == 0) bytes = 16;
    if (ctx->ws_bytes[slot] < bytes) {
        if (ctx->ws[slot]) {
            VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (ctx->side) VBX_HIP(ctx, hipStreamSynchronize(ctx->side));
            if (ctx->trk) VBX_HIP(ctx, hipStreamSynchronize(ctx->trk));
            VBX_HIP(ctx, hipFree(ctx->ws[slot]));
            ctx->ws[slot] = nullptr; ctx->ws_bytes[slot] = 0;
        }
        size_t cap = bytes + bytes / 8;
        VBX_HIP(ctx, hipMalloc(&ctx->ws[slot], cap));
        ctx->ws_bytes[slot] = cap;
    }
    *out = ctx->ws[slot];
    return VBX_SUCCESS;
}

// the mel bins: on the host on every call (the callers need them), their device copy from the context's tables
int get_bins_dev(vbx_ctx *ctx, size_t n, size_t k, double lo, double hi, double sr,
                 const int32_t **out, std::vector<int32_t> &host_bins, bool &bad) {
    mel_bins_host(n, k, lo, hi, sr, host_bins, bad);
    for (size_t i = 0; i + 1 < host_bins.size(); i++) if (host_bins[i + 1] < host_bins[i]) bad = true;   // usize underflow panics
    if (host_bins.back() > (int32_t)n) bad = true;                                                    // spectrum[bin] out of bounds
    VBX_HIP(ctx, ctx->tables.bins(n, k, lo, hi, sr, host_bins, out));
    return VBX_SUCCESS;
}

// max_len: VBX_MAX_FRAME_LEN for the entry points whose kernels keep a frame in registers / LDS, VBX_MAX_LONG_FRAME_LEN for
// the ones that also have a tiled form for longer frames (k_long.hip)
int check_frames(vbx_ctx *ctx, const char *fn, const void *x, size_t n_frames, size_t frame_len, size_t stride,
                 size_t max_len = VBX_MAX_FRAME_LEN) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null context");
    ctx->lpc_list_armed = false;   // every frame-batch call: only one that arms the LPC probe's list (below) sets it again
    ctx->path_last = false;        // (and vbx_internal_last_path_chunks_redone answers -1 until the next path call)
    ctx->shard.live = false;       // (and vbx_pitch_path_shard_enter_f64 / _finish_f64 are refused until the next _begin)
    if (n_frames == 0) return 1;   // empty batch: nothing to do
    if (!x) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": null frame pointer");
    if (frame_len < 1 || frame_len > max_len)
        return fail(ctx, VBX_E_INVALID, std::string(fn) + ": frame_len must be in [1, " + std::to_string(max_len) + "]");
    if (stride < 1) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": stride must be >= 1");
    if (n_frames > 0x7fffffffull) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": too many frames for one launch");
    return VBX_SUCCESS;
}

// Small host array -> ctx-owned device buffer through pinned staging.  The caller's array may be freed on return
// (the copy below reads the staging buffer, not the caller's memory), and identical content (the usual case: the same
// segments / estimates every call) is not uploaded again and never waits.  Changed content reuses the one staging buffer:
// the host waits until the PREVIOUS upload of that array has left it -- at once if that upload has long run, behind the
// queued work if it is still queued (two changes in one queue; include/voxbox_hip.h lists it among the calls that block).
int stage_upload(vbx_ctx *ctx, int which, int ws_slot, const void *h_src, size_t bytes, hipStream_t st, void **d_out) {
    void *d = nullptr;
    const bool grown = ctx->ws_bytes[ws_slot] < bytes;
    int rc = ws_get(ctx, ws_slot, bytes, &d);
    if (rc != VBX_SUCCESS) return rc;
    *d_out = d;
    std::vector<char> &have = ctx->staged[which];
    if (!grown && have.size() == bytes && std::memcmp(have.data(), h_src, bytes) == 0) return VBX_SUCCESS;
    if (!ctx->stage_ev[which]) VBX_HIP(ctx, hipEventCreateWithFlags(&ctx->stage_ev[which], hipEventDisableTiming));
    else VBX_HIP(ctx, hipEventSynchronize(ctx->stage_ev[which]));          // the previous copy has left the staging buffer
    if (ctx->stage_cap[which] < bytes) {
        if (ctx->stage[which]) VBX_HIP(ctx, hipHostFree(ctx->stage[which]));
        ctx->stage[which] = nullptr; ctx->stage_cap[which] = 0;
        VBX_HIP(ctx, hipHostMalloc(&ctx->stage[which], bytes + bytes / 2, hipHostMallocDefault));
        ctx->stage_cap[which] = bytes + bytes / 2;
    }
    std::memcpy(ctx->stage[which], h_src, bytes);
    // uploads of either stream are ordered behind everything queued on the main stream that may still read the old content
    VBX_HIP(ctx, hipMemcpyAsync(d, ctx->stage[which], bytes, hipMemcpyHostToDevice, st));
    VBX_HIP(ctx, hipEventRecord(ctx->stage_ev[which], st));
    have.assign((const char *)h_src, (const char *)h_src + bytes);
    return VBX_SUCCESS;
}

int upload_segments(vbx_ctx *ctx, hipStream_t st, const int64_t *h_seg, size_t n_seg, size_t n_frames, const int64_t **d_seg, size_t *n_out) {
    if (h_seg == nullptr || n_seg == 0) { *d_seg = nullptr; *n_out = 1; return VBX_SUCCESS; }
    if (h_seg[0] != 0) return fail(ctx, VBX_E_INVALID, "seg_start[0] must be 0");
    for (size_t i = 1; i < n_seg; i++)
        if (h_seg[i] < h_seg[i - 1] || (size_t)h_seg[i] > n_frames) return fail(ctx, VBX_E_INVALID, "seg_start must ascend within [0, n_frames]");
    void *d = nullptr;
    int rc = stage_upload(ctx, 0, vbx_ctx::WS_SEG, h_seg, n_seg * sizeof(int64_t), st, &d);
    if (rc != VBX_SUCCESS) return rc;
    *d_seg = (const int64_t *)d; *n_out = n_seg;
    return VBX_SUCCESS;
}

int upload_estimates(vbx_ctx *ctx, hipStream_t st, const vbx_resonance *h_est, size_t n_est, const res_t **d_est) {
    void *d = nullptr;
    int rc = stage_upload(ctx, 1, vbx_ctx::WS_EST, h_est, n_est * sizeof(vbx_resonance), st, &d);
    if (rc != VBX_SUCCESS) return rc;
    *d_est = (const res_t *)d;
    return VBX_SUCCESS;
}

}  // namespace

// =============================================================================================
extern "C" {

// hooks for vbx_comm.hip (the context is opaque outside this file)
int vbx_internal_fail(vbx_ctx *ctx, int code, const char *msg) { return fail(ctx, code, msg ? msg : ""); }
void *vbx_internal_stream(vbx_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
int vbx_internal_device(vbx_ctx *ctx) { return ctx ? ctx->device : 0; }

int vbx_abi_version(void) { return VBX_ABI_VERSION; }

int vbx_ctx_set_lpc_policy(vbx_ctx *ctx, int policy) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_REQUIRE(ctx, policy == VBX_LPC_POLICY_EXACT || policy == VBX_LPC_POLICY_PLAIN || policy == VBX_LPC_POLICY_REFERENCE,
                "vbx_ctx_set_lpc_policy: unknown policy");
    ctx->lpc_policy = policy;
    return VBX_SUCCESS;
}

int vbx_ctx_get_lpc_policy(const vbx_ctx *ctx, int *h_policy) {
    if (!ctx || !h_policy) return fail(const_cast<vbx_ctx *>(ctx), VBX_E_INVALID, "vbx_ctx_get_lpc_policy: null argument");
    *h_policy = ctx->lpc_policy;
    return VBX_SUCCESS;
}

int vbx_ctx_create(vbx_ctx **out, int device, void *hip_stream) {
    if (!out) return fail(nullptr, VBX_E_INVALID, "vbx_ctx_create: null out");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, VBX_E_NODEVICE, "vbx_ctx_create: no HIP device (this library has no CPU fallback)");
    if (device < 0 || device >= count) return fail(nullptr, VBX_E_INVALID, "vbx_ctx_create: bad device ordinal");
    VBX_HIP(nullptr, hipSetDevice(device));
    hipDeviceProp_t prop;
    VBX_HIP(nullptr, hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, VBX_E_NODEVICE, std::string("vbx_ctx_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    vbx_ctx *ctx = new vbx_ctx();
    ctx->device = device;
    ctx->arch = prop.gcnArchName;
    ctx->cu_count = prop.multiProcessorCount;
    { const char *e = std::getenv("VBX_MFCC_GOERTZEL"); ctx->mfcc_force_goertzel = e && e[0] == '1'; }
    { const char *e = std::getenv("VBX_MFCC_DFT2"); ctx->mfcc_force_dft2 = e && e[0] == '1'; }
    { const char *e = std::getenv("VBX_MFCC_MFMA"); ctx->mfcc_force_mfma = e && e[0] == '1'; }
    { const char *e = std::getenv("VBX_MFCC_CZT"); ctx->mfcc_czt = e ? (e[0] == '1' ? 1 : 0) : -1; }
    { const char *e = std::getenv("VBX_MFCC_DEFER"); ctx->mfcc_defer = (e && e[0] == '0') ? 0 : 1; }
    { const char *e = std::getenv("VBX_LPC_EXACT"); ctx->lpc_policy = (e && e[0] == '0') ? VBX_LPC_POLICY_PLAIN : VBX_LPC_POLICY_EXACT; }
    { const char *e = std::getenv("VBX_POW2_SPLIT"); ctx->pow2_split = e ? (e[0] == '0' ? 0 : 1) : -1; }
    { const char *e = std::getenv("VBX_MFCC_INTERP"); ctx->mfcc_interp = e ? (e[0] == '0' ? 0 : 1) : -1; }
    { const char *e = std::getenv("VBX_MFCC_CZT_SPLIT"); ctx->mfcc_czt_split = e != nullptr && e[0] == '1'; }
    { const char *e = std::getenv("VBX_PITCH_CURVE_CUT"); ctx->pitch_whole_curve = e != nullptr && e[0] == '0'; }
    if (const char *e = std::getenv("VBX_ROCTX"); e != nullptr && e[0] == '1') {
        void *h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (h == nullptr) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (h != nullptr) {
            ctx->roctx_push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
            ctx->roctx_pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (ctx->roctx_push == nullptr || ctx->roctx_pop == nullptr) { ctx->roctx_push = nullptr; ctx->roctx_pop = nullptr; }
        }
    }
    { const char *e = std::getenv("VBX_PITCH_MFMA"); ctx->pitch_force_mfma = e && e[0] == '1'; }
    if (hip_stream) { ctx->stream = (hipStream_t)hip_stream; ctx->owns_stream = false; }
    else {
        e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete ctx; return fail(nullptr, VBX_E_RUNTIME, "hipStreamCreate failed"); }
        ctx->owns_stream = true;
    }
    hipEventCreate(&ctx->t0);
    hipEventCreate(&ctx->t1);
    *out = ctx;
    return VBX_SUCCESS;
}

void vbx_ctx_destroy(vbx_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < vbx_ctx::WS_N; i++) if (ctx->ws[i]) hipFree(ctx->ws[i]);
    if (ctx->pitch_work) hipFree(ctx->pitch_work);
    if (ctx->stitch_state) hipFree(ctx->stitch_state);
    ctx->tables.clear();
    for (auto &r : ctx->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    if (ctx->side) { hipStreamSynchronize(ctx->side); hipStreamDestroy(ctx->side); }
    if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
    if (ctx->ev_peak) hipEventDestroy(ctx->ev_peak);
    for (auto &e : ctx->ev_slice) if (e) hipEventDestroy(e);
    if (ctx->ev_trk) hipEventDestroy(ctx->ev_trk);
    if (ctx->trk) { hipStreamSynchronize(ctx->trk); hipStreamDestroy(ctx->trk); }
    if (ctx->copy) { hipStreamSynchronize(ctx->copy); hipStreamDestroy(ctx->copy); }
    for (int i = 0; i < 2; i++) {
        if (ctx->host_raw[i]) hipFree(ctx->host_raw[i]);
        if (ctx->host_ready[i]) hipEventDestroy(ctx->host_ready[i]);
        if (ctx->host_freed[i]) hipEventDestroy(ctx->host_freed[i]);
    }
    for (int i = 0; i < 3; i++) { if (ctx->stage[i]) hipHostFree(ctx->stage[i]); if (ctx->stage_ev[i]) hipEventDestroy(ctx->stage_ev[i]); }
    if (ctx->t0) hipEventDestroy(ctx->t0);
    if (ctx->t1) hipEventDestroy(ctx->t1);
    if (ctx->owns_stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

int vbx_sync(vbx_ctx *ctx) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, "vbx_sync: null context");
    VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // every call joins its inner streams into ctx->stream before it returns, so they are idle by now; draining them as well
    // costs nothing and makes "after vbx_sync nothing of this context runs" hold by construction (buffers may be freed)
    if (ctx->side) VBX_HIP(ctx, hipStreamSynchronize(ctx->side));
    if (ctx->trk) VBX_HIP(ctx, hipStreamSynchronize(ctx->trk));
    if (ctx->copy) VBX_HIP(ctx, hipStreamSynchronize(ctx->copy));       // (vbx_analyze_host's uploads: idle once that call has returned)
    return VBX_SUCCESS;
}

const char *vbx_last_error(const vbx_ctx *ctx) { return ctx ? ctx->last_error.c_str() : g_last_error.c_str(); }

int vbx_device_info(const vbx_ctx *ctx, char *h_name, size_t name_cap, int *h_cu_count) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, "vbx_device_info: null context");
    if (h_name && name_cap) { std::strncpy(h_name, ctx->arch.c_str(), name_cap - 1); h_name[name_cap - 1] = 0; }
    if (h_cu_count) *h_cu_count = ctx->cu_count;
    return VBX_SUCCESS;
}

int vbx_malloc(vbx_ctx *ctx, void **out_dptr, size_t bytes) {
    VBX_REQUIRE(ctx, ctx && out_dptr, "null argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    VBX_HIP(ctx, hipMalloc(out_dptr, bytes ? bytes : 16));
    return VBX_SUCCESS;
}
int vbx_free(vbx_ctx *ctx, void *dptr) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (dptr) { VBX_HIP(ctx, hipStreamSynchronize(ctx->stream)); VBX_HIP(ctx, hipFree(dptr)); }
    return VBX_SUCCESS;
}
int vbx_memcpy_h2d(vbx_ctx *ctx, void *dst, const void *h_src, size_t bytes) {
    VBX_REQUIRE(ctx, ctx && (bytes == 0 || (dst && h_src)), "null argument");
    if (bytes == 0) return VBX_SUCCESS;
    VBX_HIP(ctx, hipMemcpyAsync(dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VBX_SUCCESS;
}
int vbx_memcpy_d2h(vbx_ctx *ctx, void *h_dst, const void *src, size_t bytes) {
    VBX_REQUIRE(ctx, ctx && (bytes == 0 || (h_dst && src)), "null argument");
    if (bytes == 0) return VBX_SUCCESS;
    VBX_HIP(ctx, hipMemcpyAsync(h_dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VBX_SUCCESS;
}
int vbx_memset(vbx_ctx *ctx, void *dst, int value, size_t bytes) {
    VBX_REQUIRE(ctx, ctx && (bytes == 0 || dst), "null argument");
    if (bytes == 0) return VBX_SUCCESS;
    VBX_HIP(ctx, hipMemsetAsync(dst, value, bytes, ctx->stream));
    return VBX_SUCCESS;
}

int vbx_timer_begin(vbx_ctx *ctx) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_HIP(ctx, hipEventRecord(ctx->t0, ctx->stream));
    return VBX_SUCCESS;
}
int vbx_timer_end(vbx_ctx *ctx, float *h_ms) {
    VBX_REQUIRE(ctx, ctx && h_ms, "null argument");
    VBX_HIP(ctx, hipEventRecord(ctx->t1, ctx->stream));
    VBX_HIP(ctx, hipEventSynchronize(ctx->t1));
    VBX_HIP(ctx, hipEventElapsedTime(h_ms, ctx->t0, ctx->t1));
    return VBX_SUCCESS;
}

static int prof_flush(vbx_ctx *ctx) {
    if (ctx->recs.empty()) return VBX_SUCCESS;
    VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->side) VBX_HIP(ctx, hipStreamSynchronize(ctx->side));
    if (ctx->trk) VBX_HIP(ctx, hipStreamSynchronize(ctx->trk));
    for (auto &r : ctx->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            auto &acc = ctx->prof_acc[r.name];
            acc.first += ms; acc.second += 1;
            ctx->prof_stream[r.name] = (r.stream == ctx->stream) ? 0 : (r.stream == ctx->side) ? 1 : 2;
        }
        hipEventDestroy(r.a); hipEventDestroy(r.b);
    }
    ctx->recs.clear();
    return VBX_SUCCESS;
}
int vbx_profile_enable(vbx_ctx *ctx, int on) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    int rc = prof_flush(ctx);
    ctx->prof = on != 0;
    return rc;
}
int vbx_profile_reset(vbx_ctx *ctx) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    int rc = prof_flush(ctx);
    ctx->prof_acc.clear();
    ctx->prof_stream.clear();
    if (ctx->pitch_work)
        VBX_HIP(ctx, hipMemsetAsync(ctx->pitch_work, 0, PITCH_WORK_WORDS * sizeof(unsigned long long), ctx->stream));
    return rc;
}
int vbx_profile_pitch_work(vbx_ctx *ctx, uint64_t *h_out4) {
    VBX_REQUIRE(ctx, ctx && h_out4, "null argument");
    for (int i = 0; i < 4; i++) h_out4[i] = 0;
    if (!ctx->pitch_work) return VBX_SUCCESS;
    unsigned long long h[PITCH_WORK_SLOTS * 4];
    VBX_HIP(ctx, hipMemcpyAsync(h, ctx->pitch_work, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < PITCH_WORK_SLOTS; s++) for (int i = 0; i < 4; i++) h_out4[i] += h[4 * s + i];
#ifdef VBX_EXP_PHASES
    {   // experiment build: the phase clock sums, to stderr
        unsigned long long ph[PITCH_WORK_SLOTS * PHASE_SLOTS], tot[PHASE_SLOTS] = {0};
        VBX_HIP(ctx, hipMemcpy(ph, ctx->pitch_work + PITCH_WORK_SLOTS * 4, sizeof ph, hipMemcpyDeviceToHost));
        for (int s = 0; s < PITCH_WORK_SLOTS; s++) for (int k = 0; k < PHASE_SLOTS; k++) tot[k] += ph[s * PHASE_SLOTS + k];
        fprintf(stderr, "VBX_PHASES frames %llu cycles", (unsigned long long)h_out4[0]);
        for (int k = 0; k < PHASE_SLOTS; k++) fprintf(stderr, " %llu", tot[k]);
        fprintf(stderr, "\n");
    }
#endif
    return VBX_SUCCESS;
}
int vbx_profile_get(vbx_ctx *ctx, const char *kernel_name, double *h_total_ms, long *h_launches) {
    VBX_REQUIRE(ctx, ctx && kernel_name, "null argument");
    int rc = prof_flush(ctx);
    if (rc != VBX_SUCCESS) return rc;
    auto it = ctx->prof_acc.find(kernel_name);
    if (h_total_ms) *h_total_ms = (it == ctx->prof_acc.end()) ? 0.0 : it->second.first;
    if (h_launches) *h_launches = (it == ctx->prof_acc.end()) ? 0 : it->second.second;
    return VBX_SUCCESS;
}
int vbx_profile_stream(vbx_ctx *ctx, const char *kernel_name, int *h_stream) {
    VBX_REQUIRE(ctx, ctx && kernel_name && h_stream, "null argument");
    int rc = prof_flush(ctx);
    if (rc != VBX_SUCCESS) return rc;
    auto it = ctx->prof_stream.find(kernel_name);
    *h_stream = (it == ctx->prof_stream.end()) ? -1 : it->second;
    return VBX_SUCCESS;
}
int vbx_profile_names(vbx_ctx *ctx, char *h_buf, size_t cap) {
    VBX_REQUIRE(ctx, ctx && h_buf && cap, "null argument");
    int rc = prof_flush(ctx);
    if (rc != VBX_SUCCESS) return rc;
    std::string s;
    for (auto &kv : ctx->prof_acc) { s += kv.first; s += '\n'; }
    std::strncpy(h_buf, s.c_str(), cap - 1); h_buf[cap - 1] = 0;
    return VBX_SUCCESS;
}

// ---- tables -------------------------------------------------------------------------------

// ---- periodic.rs --------------------------------------------------------------------------

// Autocorrelate::autocorrelate(n_lags) of every frame on stream st: the few-lag register kernel, one FFT of the zero-padded
// frame (many lags of a 512..4096-sample frame), or the matrix-core tiles.
static int run_autocorrelate(vbx_ctx *ctx, hipStream_t st, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                             const double *window, size_t n_lags, double *out) {
    if (frame_len > VBX_MAX_FRAME_LEN) {
        // a frame that no wavefront's LDS image holds: the matrix-core lag tiles over chunked images (k_long.hip)
        void *w = nullptr;
        int rc = ws_get(ctx, vbx_ctx::WS_LONG, autocorr_long_scratch_bytes((long)n_frames, (long)frame_len, (long)n_lags), &w);
        if (rc != VBX_SUCCESS) return rc;
        Prof p(ctx, "autocorr_long", st);
        launch_autocorr_long(st, x, (long)n_frames, (long)frame_len, (long)stride, window, (long)n_lags, out, (double *)w);
        return VBX_SUCCESS;
    }
    if (fewlags_supported((int)frame_len, (int)n_lags, false)) {
        Prof p(ctx, "autocorr_fewlags", st);
        launch_autocorr_fewlags(st, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_lags, 0, out, nullptr);
    } else if (!ctx->pitch_force_mfma && spectral_plan((int)frame_len) != SPECTRAL_PLAN_NONE &&
               (n_lags >= SPECTRAL_AC_MIN_LAGS || frame_len >= 1024)) {
        // every lag sum from one real FFT of the zero-padded frame (k_spectral*.hip) instead of lags x frame_len products;
        // the rounding error, ~1e-16 r[0] per lag, is a thousandth of the tolerance's floor
        const double *tab = nullptr;
        spectral_launch_t L{};
        L.plan = spectral_plan((int)frame_len); L.n = (int)frame_len;
        VBX_HIP(ctx, ctx->tables.spectral(L.plan, &tab));
        L.x = x; L.F = (long)n_frames; L.stride = (long)stride; L.window = window; L.tab = tab;
        L.out_r = out; L.n_lags = (int)n_lags;
        Prof p(ctx, "autocorr_fft", st);
        launch_analyze(st, L);
    } else {
        Prof p(ctx, "autocorr_tiles", st);
        launch_autocorr_tiles(st, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_lags, out);
    }
    return VBX_SUCCESS;
}

int vbx_autocorrelate_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len,
                          size_t stride, const double *window, size_t n_lags, double *out) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, n_lags >= 1 && n_lags <= frame_len, "n_lags must be in [1, frame_len] (the reference panics beyond)");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->lpc_policy == VBX_LPC_POLICY_REFERENCE) {
        // every lag the crate's sequential fold (k_lpc_ref.hip) instead of the FFT / matrix-core / register forms
        VBX_REQUIRE(ctx, frame_len <= 0x7fffffffull, "frame_len too large");
        { Prof p(ctx, "autocorr_ref"); launch_lpc_ref(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_lags, 0, 0,
                                                      out, (long)n_lags, nullptr, 0); }
        return check_launch(ctx, __func__);
    }
    rc = run_autocorrelate(ctx, ctx->stream, x, n_frames, frame_len, stride, window, n_lags, out);
    if (rc != VBX_SUCCESS) return rc;
    return check_launch(ctx, __func__);
}

int vbx_normalize_f64(vbx_ctx *ctx, double *data, size_t n_rows, size_t n) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_rows == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, data && n >= 1 && n <= 0x7fffffff && n_rows <= 0x7fffffff, "bad argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "normalize_rows"); launch_normalize_rows(ctx->stream, data, (long)n_rows, (int)n); }
    return check_launch(ctx, __func__);
}

int vbx_interpolate_sinc_f64(vbx_ctx *ctx, const double *y, size_t ylen, long offset, size_t nx,
                             const double *xs, size_t m, size_t max_depth, double *out, int32_t *status) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (m == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, y && xs && out && ylen >= 1 && ylen <= 0x7fffffff && m <= 0x7fffffff, "bad argument");
    VBX_REQUIRE(ctx, max_depth <= 0x3fffffff && nx <= 0x3fffffff && ylen <= 0x3fffffff &&
                offset > -0x3fffffffL && offset < 0x3fffffffL, "depth / nx / offset / ylen too large");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "sinc_points"); launch_sinc_points(ctx->stream, y, (int)ylen, offset, (long)nx, xs, (long)m, (long)max_depth, out, status); }
    return check_launch(ctx, __func__);
}

int vbx_improve_extremum_ex_f64(vbx_ctx *ctx, const double *y, size_t ylen, long offset, size_t nx,
                                const double *ixmid, size_t m, int interpolation, size_t depth, int is_max,
                                double *out_xy, int32_t *status) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (m == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, y && ixmid && out_xy && ylen >= 1 && ylen <= 0x7fffffff && m <= 0x7fffffff, "bad argument");
    VBX_REQUIRE(ctx, interpolation >= VBX_INTERP_NONE && interpolation <= VBX_INTERP_SINC, "interpolation must be NONE, PARABOLIC or SINC");
    VBX_REQUIRE(ctx, depth <= 0x3fffffff && nx <= 0x3fffffff && ylen <= 0x3fffffff &&
                offset > -0x3fffffffL && offset < 0x3fffffffL, "depth / nx / offset / ylen too large");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "extremum_points"); launch_extremum_points(ctx->stream, y, (int)ylen, offset, (long)nx, ixmid, (long)m, (long)depth, out_xy, status, interpolation, is_max ? 1 : 0); }
    return check_launch(ctx, __func__);
}

int vbx_improve_extremum_f64(vbx_ctx *ctx, const double *y, size_t ylen, long offset, size_t nx,
                             const double *ixmid, size_t m, size_t depth, double *out_xy, int32_t *status) {
    return vbx_improve_extremum_ex_f64(ctx, y, ylen, offset, nx, ixmid, m, VBX_INTERP_SINC, depth, 1, out_xy, status);
}

// The FFT-based kernel (k_spectral.hip) followed by the direct-sum kernel on the frames whose peak decisions lie
// inside the FFT's rounding error (normally none; curves that are exactly zero over a stretch, e.g. a few impulses).
static int launch_spectral(vbx_ctx *ctx, hipStream_t st, spectral_launch_t &L, const char *prof_name) {
    void *w = nullptr;
    int rc = ws_get(ctx, vbx_ctx::WS_UNSURE, ((size_t)L.F + 4) * sizeof(int32_t), &w);
    if (rc != VBX_SUCCESS) return rc;
    L.unsure_count = (int32_t *)w;                       // [0]: count, [4..]: frame indices
    L.unsure_list = (int32_t *)w + 4;
    VBX_HIP(ctx, hipMemsetAsync(L.unsure_count, 0, sizeof(int32_t), st));
    // LPC rows: levinson_rows_kernel_t (k_lpc.hip) lists the frames whose Levinson row a few eps of lag-sum rounding can move by more
    // than 1e-6; lpc_exact_list_kernel redoes those in double-double.  VBX_LPC_EXACT=0: no probe, the rows of rounds 1-5 (A/B, tests).
    L.lpc_list = nullptr; L.lpc_count = nullptr;
    if (L.out_lpc != nullptr && ctx->lpc_policy == VBX_LPC_POLICY_EXACT) {
        void *lw = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_LPC_LIST, ((size_t)L.F + 4) * sizeof(int32_t), &lw);
        if (rc != VBX_SUCCESS) return rc;
        L.lpc_count = (int32_t *)lw; L.lpc_list = (int32_t *)lw + 4;
        VBX_HIP(ctx, hipMemsetAsync(L.lpc_count, 0, sizeof(int32_t), st));
        ctx->lpc_list_armed = true;
    }
    // the 4096-point plan runs as two kernels with the lag curves in a scratch buffer between them (vbx_spectral.hpp, SP_ANALYZE_SPLIT):
    // batches of up to 131,072 frames (~10 KB each)
    L.curve_ws = nullptr; L.curve_ws_bytes = 0;
    const size_t rowb = (ctx->pow2_split != 0 && !L.whole_curve && !L.mfcc_only && L.out_r == nullptr && pitch_full_list_bytes(L.n, L.kmax) == 0)
                            ? spectral_split_row_bytes(L.n, L.sample_rate, L.fmin) : 0;      // (a list region in LDS, kmax > 64: the fused kernel)
    if (rowb) {
        const size_t frames = (size_t)L.F < 131072 ? (size_t)L.F : 131072;
        const size_t need = (frames < 1024 ? 1024 : frames) * rowb + 64;
        void *cw = nullptr;
        // (no memory for it: the fused form.  A size that failed once is not asked for again on every call -- each attempt drains the
        // streams and fails a multi-GB hipMalloc --, and the fallback is not an error of this call: the error string is put back)
        if (ctx->curve_failed_bytes == 0 || need < ctx->curve_failed_bytes) {
            const std::string before = ctx->last_error;
            if (ws_get(ctx, vbx_ctx::WS_CURVE, need, &cw) == VBX_SUCCESS) { L.curve_ws = (double *)cw; L.curve_ws_bytes = need; }
            else { (void)hipGetLastError(); ctx->curve_failed_bytes = need; ctx->last_error = before; g_last_error = before; }
        }
    }
    // MFCC::mfcc's log10 + DCT out of the frame's wavefront (mfcc_tail_q's `defer`): the kernel leaves the filter sums in the row
    // (the 1200-point plan only: in the power-of-two kernels the deferred form changes the register allocation -- thirteen index registers
    // spilled across the second transform, 3 KB of scratch traffic per frame -- for the same ~1 %; they keep the tail)
    L.mfcc_defer = L.out_mfcc != nullptr && !L.mfcc_only && L.num_coeffs >= 1 && L.num_coeffs <= 16 && ctx->mfcc_defer && L.plan == SPECTRAL_PLAN_1200;
    { Prof p(ctx, prof_name, st); ctx->last_spectral_split = launch_analyze(st, L); }
    if (L.mfcc_defer && L.out_lpc == nullptr) { Prof p(ctx, "mfcc_rows", st); launch_mfcc_rows(st, L.out_mfcc, L.F, L.mfcc_ld, L.num_coeffs, L.dct); }
    {
        Prof p(ctx, "pitch_direct_fallback", st);
        // a fixed grid over a count only the device knows (almost always zero).  Every workgroup of this kernel allocates the
        // frame's LDS image + refinement state before it can look at the count: ~70 KB at 3000 samples -- 1024 of them took
        // 4 ms to come and go with nothing to do, beside 13.5 ms of the analysis itself.  One per CU where the state is large.
        const int cus = ctx->cu_count > 0 ? ctx->cu_count : 256;
        const int grid = pitch_lds_bytes(L.n) > 24 * 1024 ? cus : cus * 4;
        launch_pitch_list(st, L.unsure_list, L.unsure_count, grid, L.x, L.n, L.stride, L.window, L.lag_window,
                          L.sample_rate, L.threshold, L.fmin, L.fmax, L.kmax, L.out_cand, L.cand_ld, L.out_count,
                          L.pitch_status, L.work);
    }
    if (L.out_lpc != nullptr) {
        // the fused kernel left r[0..12] in every frame's LPC row: LPC::lpc(12) in place, one row per lane (+ the conditioning probe), then
        // the listed rows again from their frames in double-double
        { Prof p(ctx, "lpc_rows", st);
          launch_levinson_rows_probe(st, L.out_lpc, L.F, L.lpc_ld, SPECTRAL_LPC_ORDER, L.out_lpc, L.lpc_ld, L.lpc_list, L.lpc_count,
                                     L.mfcc_defer ? L.out_mfcc : nullptr, L.mfcc_ld, L.num_coeffs, L.dct); }        // (+ the deferred MFCC tail of the same record)
        if (L.lpc_list != nullptr) {
            Prof p(ctx, "lpc_exact_list", st);
            const int cus = ctx->cu_count > 0 ? ctx->cu_count : 256;
            launch_lpc_exact_list(st, L.lpc_list, L.lpc_count, cus, L.x, L.n, L.stride, L.window, SPECTRAL_LPC_ORDER, L.out_lpc, L.lpc_ld);
        }
        if (ctx->lpc_policy == VBX_LPC_POLICY_REFERENCE) {
            // the crate's rows (k_lpc_ref.hip) over the column, after the kernels above on the same stream: the fused kernel and the
            // Levinson pass run as under every policy (their instantiations, and so every other column, unchanged), only the LPC
            // row is replaced
            Prof p(ctx, "lpc_ref", st);
            launch_lpc_ref(st, L.x, L.F, L.n, L.stride, L.window, SPECTRAL_LPC_ORDER + 1, SPECTRAL_LPC_ORDER, 0, nullptr, 0, L.out_lpc, L.lpc_ld);
        }
    }
    return check_launch(ctx, "launch_spectral");
}

// What run_pitch rejects about (frame_len, kmax), as a message, or nullptr: also asked by the tracked frame loop before its first
// launch.  (kmax <= 63 there, below every cap of this function: only the frame_len rules can bind.)
static const char *pitch_shape_error(size_t frame_len, size_t kmax) {
    const size_t kcap = frame_len > VBX_MAX_FRAME_LEN ? VBX_PITCH_MAX_CANDIDATES(frame_len) : (size_t)VBX_MAX_PITCH_CANDIDATES;
    if (!(kmax >= 1 && kmax <= kcap)) return "kmax must be in [1, VBX_MAX_PITCH_CANDIDATES] (long frames: [1, frame_len / 4 + 2])";
    if (frame_len < 4) return "frame_len must be >= 4";
    if (frame_len > VBX_MAX_FRAME_LEN) return frame_len <= 0x3fffffff ? nullptr : "frame_len too large for the lag curve's 32-bit indices";
    if (pitch_lds_bytes((int)frame_len) + pitch_full_list_bytes((int)frame_len, (int)kmax) + 16 > 160 * 1024) return "frame does not fit the LDS";
    return nullptr;
}

static int run_pitch(vbx_ctx *ctx, hipStream_t st, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                     const double *window, double sample_rate, double threshold, double fmin, double fmax,
                     size_t kmax, vbx_pitch *out_cand, size_t cand_ld, int32_t *out_count, int32_t *status) {
    VBX_REQUIRE(ctx, out_cand != nullptr, "null output");
    if (const char *e = pitch_shape_error(frame_len, kmax)) return fail(ctx, VBX_E_INVALID, std::string(__func__) + ": " + e);
    VBX_REQUIRE(ctx, cand_ld >= 2 * kmax && cand_ld % 2 == 0, "candidate rows must hold kmax entries and their leading dimension must be even");
    const double *lagw = nullptr; bool lag_rcp = false;
    int rc;
    VBX_HIP(ctx, ctx->tables.window(VBX_WINDOW_HANNING_LAG, frame_len, &lagw, &lag_rcp));
    if (frame_len > VBX_MAX_FRAME_LEN) {
        // a frame whose lag curve no LDS holds (k_long.hip): every lag by the chunked matrix-core tiles, the curve as an array in
        // HBM, peak scan -> improve_extremum per candidate -> rank sort; batches of frames so that the scratch stays <= 2 GiB
        size_t per = (size_t(1) << 31) / pitch_long_scratch_bytes(1, (long)frame_len);
        if (per < 1) per = 1;
        if (per > n_frames) per = n_frames;
        void *w2 = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_LONG2, pitch_long_scratch_bytes((long)per, (long)frame_len), &w2);
        if (rc != VBX_SUCCESS) return rc;
        for (size_t f0 = 0; f0 < n_frames; f0 += per) {
            const size_t m = (n_frames - f0 < per) ? n_frames - f0 : per;
            double *r = pitch_long_r(w2);
            rc = run_autocorrelate(ctx, st, x + f0 * stride, m, frame_len, stride, window, frame_len, r);      // :402
            if (rc != VBX_SUCCESS) return rc;
            { Prof p(ctx, "normalize_rows", st); launch_normalize_rows(st, r, (long)m, (int)frame_len); }       // :404
            ctx->last_pitch_form = 100;
            { Prof p(ctx, "pitch_long", st);
              launch_pitch_long(st, (long)m, (long)frame_len, lagw, sample_rate, threshold, fmin, fmax, (int)kmax,
                                (double *)out_cand + f0 * cand_ld, (long)cand_ld, out_count ? out_count + f0 : nullptr,
                                status ? status + f0 : nullptr, w2); }
        }
        return check_launch(ctx, "vbx_pitch_f64");
    }
    if (ctx->prof && !ctx->pitch_work) {
        const size_t wb = PITCH_WORK_WORDS * sizeof(unsigned long long);
        VBX_HIP(ctx, hipMalloc((void **)&ctx->pitch_work, wb));
        VBX_HIP(ctx, hipMemsetAsync(ctx->pitch_work, 0, wb, st));
    }
    if (!ctx->pitch_force_mfma && spectral_supported((int)frame_len, 0, 0, 0, 0)) {
        // autocorrelation by one real FFT of the frame (k_spectral.hip) instead of the O(N^2) lag sums
        const double *tab = nullptr;
        spectral_launch_t L{};
        L.plan = spectral_plan((int)frame_len); L.n = (int)frame_len;
        VBX_HIP(ctx, ctx->tables.spectral(L.plan, &tab));
        L.x = x; L.F = (long)n_frames; L.stride = (long)stride; L.window = window; L.lag_window = lagw; L.tab = tab;
        L.lag_rcp = lag_rcp;
        L.sample_rate = sample_rate; L.threshold = threshold; L.fmin = fmin; L.fmax = fmax; L.kmax = (int)kmax;
        L.whole_curve = ctx->pitch_whole_curve;
        L.out_cand = (pitch_t *)out_cand; L.cand_ld = (long)cand_ld; L.out_count = out_count; L.pitch_status = status;
        L.work = ctx->prof ? ctx->pitch_work : nullptr;
        ctx->last_pitch_form = 100 * (3 + L.plan) + (pitch_full_list_bytes(L.n, L.kmax) == 0 ? 0 : spectral_list_parked(L) ? 2 : 1);
        return launch_spectral(ctx, st, L, "pitch");
    }
    {
        ctx->last_pitch_form = 200 + (pitch_full_list_bytes((int)frame_len, (int)kmax) == 0 ? 0 : 1);
        Prof p(ctx, "pitch", st);
        launch_pitch(st, x, (long)n_frames, (int)frame_len, (long)stride, window, lagw, sample_rate, threshold,
                     fmin, fmax, (int)kmax, (pitch_t *)out_cand, (long)cand_ld, out_count, status,
                     ctx->prof ? ctx->pitch_work : nullptr);
    }
    return check_launch(ctx, "vbx_pitch_f64");
}

int vbx_pitch_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                  const double *window, double sample_rate, double threshold, double fmin, double fmax,
                  size_t kmax, vbx_pitch *out_cand, int32_t *out_count, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    return run_pitch(ctx, ctx->stream, x, n_frames, frame_len, stride, window, sample_rate, threshold, fmin, fmax,
                     kmax, out_cand, 2 * kmax, out_count, status);
}

// ---- spectrum.rs: LPC ---------------------------------------------------------------------

int vbx_lpc_mut_f64(vbx_ctx *ctx, const double *r, size_t n_frames, size_t r_stride, size_t n_coeffs, double *out_ac,
                    double *out_kc) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, r && out_ac, "null argument");
    VBX_REQUIRE(ctx, n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && r_stride >= n_coeffs + 1, "bad order / stride");
    VBX_REQUIRE(ctx, n_frames <= 0x7fffffffull, "too many rows");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->lpc_policy == VBX_LPC_POLICY_REFERENCE) {
        // the recursion with contraction off, operation for operation src/spectrum.rs:63-84 (the default kernel lets the compiler fuse
        // its multiply-adds)
        Prof p(ctx, "levinson_ref_rows");
        launch_levinson_ref_rows(ctx->stream, r, (long)n_frames, (long)r_stride, (int)n_coeffs, out_ac, (long)n_coeffs + 1, out_kc);
        return check_launch(ctx, __func__);
    }
    { Prof p(ctx, "levinson_rows"); launch_levinson_rows(ctx->stream, r, (long)n_frames, (long)r_stride, (int)n_coeffs, out_ac, (long)n_coeffs + 1, out_kc); }
    return check_launch(ctx, __func__);
}

int vbx_lpc_f64(vbx_ctx *ctx, const double *r, size_t n_frames, size_t r_stride, size_t n_coeffs, double *out) {
    return vbx_lpc_mut_f64(ctx, r, n_frames, r_stride, n_coeffs, out, nullptr);
}

static bool lpc_order_ok(size_t frame_len, size_t n_coeffs) {      // run_autocorr_lpc's rule (and the tracked frame loop's pre-check)
    return n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && n_coeffs + 1 <= frame_len;
}

static int run_autocorr_lpc(vbx_ctx *ctx, hipStream_t st, const double *x, size_t n_frames, size_t frame_len,
                            size_t stride, const double *window, size_t n_coeffs, int normalize,
                            double *out_r, double *out_lpc, size_t lpc_ld) {
    VBX_REQUIRE(ctx, out_r || out_lpc, "both outputs null");
    VBX_REQUIRE(ctx, lpc_order_ok(frame_len, n_coeffs), "bad order");
    VBX_REQUIRE(ctx, lpc_ld >= n_coeffs + 1, "LPC rows must hold n_coeffs + 1 entries");
    const int n_lags = (int)n_coeffs + 1;
    int rc;
    if (ctx->lpc_policy == VBX_LPC_POLICY_REFERENCE) {
        // the crate's own arithmetic (k_lpc_ref.hip): fold, [normalize,] recursion, bit for bit; no probe, no redo
        VBX_REQUIRE(ctx, frame_len <= 0x7fffffffull, "frame_len too large");
        { Prof p(ctx, "lpc_ref", st);
          launch_lpc_ref(st, x, (long)n_frames, (int)frame_len, (long)stride, window, n_lags, (int)n_coeffs, normalize, out_r, n_lags,
                         out_lpc, (long)lpc_ld); }
        return check_launch(ctx, "vbx_autocorr_lpc_f64");
    }
    // LPC rows: a conditioning probe lists the frames whose row a few eps of lag-sum rounding can move by more than 1e-6; those are
    // redone from the frame in double-double (k_lpc_exact.hip).  VBX_LPC_EXACT=0: the rows of rounds 1-5.
    int32_t *lpc_list = nullptr, *lpc_count = nullptr;
    if (out_lpc != nullptr && ctx->lpc_policy == VBX_LPC_POLICY_EXACT && lpc_exact_supported((int)frame_len, (int)n_coeffs)) {
        void *lw = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_LPC_LIST, (n_frames + 4) * sizeof(int32_t), &lw);
        if (rc != VBX_SUCCESS) return rc;
        lpc_count = (int32_t *)lw; lpc_list = (int32_t *)lw + 4;
        VBX_HIP(ctx, hipMemsetAsync(lpc_count, 0, sizeof(int32_t), st));
        ctx->lpc_list_armed = true;
    }
    auto redo = [&]() {
        if (lpc_list == nullptr) return;
        Prof p(ctx, "lpc_exact_list", st);
        const int cus = ctx->cu_count > 0 ? ctx->cu_count : 256;
        launch_lpc_exact_list(st, lpc_list, lpc_count, cus, x, (int)frame_len, (long)stride, window, (int)n_coeffs, out_lpc, (long)lpc_ld);
    };
    if (fewlags_supported((int)frame_len, n_lags, out_lpc != nullptr)) {
        { Prof p(ctx, "autocorr_lpc", st);
          launch_autocorr_fewlags(st, x, (long)n_frames, (int)frame_len, (long)stride, window, n_lags, normalize, out_r, out_lpc, (long)lpc_ld,
                                  lpc_list, lpc_count); }
        redo();
        return check_launch(ctx, "vbx_autocorr_lpc_f64");
    }
    // general shapes: autocorrelate -> [normalize] -> Levinson as three launches
    double *r = out_r;
    if (!r) {
        void *w = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_MISC, n_frames * (size_t)n_lags * sizeof(double), &w);
        if (rc != VBX_SUCCESS) return rc;
        r = (double *)w;
    }
    rc = run_autocorrelate(ctx, st, x, n_frames, frame_len, stride, window, (size_t)n_lags, r);
    if (rc != VBX_SUCCESS) return rc;
    if (normalize) { Prof p(ctx, "normalize_rows", st); launch_normalize_rows(st, r, (long)n_frames, n_lags); }
    if (out_lpc) {
        Prof p(ctx, "levinson_rows", st);
        if (lpc_list != nullptr) launch_levinson_rows_probe(st, r, (long)n_frames, n_lags, (int)n_coeffs, out_lpc, (long)lpc_ld, lpc_list, lpc_count);
        else launch_levinson_rows(st, r, (long)n_frames, n_lags, (int)n_coeffs, out_lpc, (long)lpc_ld);
    }
    redo();
    return check_launch(ctx, "vbx_autocorr_lpc_f64");
}

int vbx_autocorr_lpc_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len,
                         size_t stride, const double *window, size_t n_coeffs, int normalize,
                         double *out_r, double *out_lpc) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    return run_autocorr_lpc(ctx, ctx->stream, x, n_frames, frame_len, stride, window, n_coeffs, normalize, out_r, out_lpc, n_coeffs + 1);
}

static bool burg_order_ok(size_t frame_len, size_t n_coeffs) {
    return frame_len >= 2 && n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER;
}

// Burg on a batch: the one-pass form (k_burg_fast.hip) where it exists, the frames its guard turns away and every other
// shape through the direct recursion (k_burg.hip)
// rp (vbx_find_formants_resampled_f64, vbx_analyze_frames_ex_*): x holds the caller's frames of rp->n_src samples and Burg runs on
// their RESAMPLED view -- n is then the resampled length m and window its periodic Hanning window.  The shapes the resampled
// loaders take (k_burg_resampled.hip) never exist as a batch; the others are resampled into a context-owned dense batch, a
// chunk of frames at a time, and take this function's plain form -- the same kernels at the same parameters either way.
struct resample_plan_t { resample_src_t rs; size_t n_src, m; bool direct; };
constexpr size_t EX_DENSE_BYTES = size_t(256) << 20;          // the dense fallback's batch: at most this, or one resampled frame
static const char *const k_kind_names[3] = {"f64", "pcm16", "float32"};      // by sample_kind_t, for messages

static int run_burg(vbx_ctx *ctx, hipStream_t stm, frames_t x, long F, int n, long stride, const double *window, int p, double *coeffs,
                    int32_t *st, frame_map_t map = frame_map_t{0, 0, 0}, const resample_plan_t *rp = nullptr) {
    if (rp && !rp->direct) {
        // the dense fallback (the callers widen PCM / float32 first; no time slices: run_find_formants)
        if (x.kind != SAMPLE_F64) return fail(ctx, VBX_E_RUNTIME, "run_burg: the dense resampled batch is made from f64 frames");
        long per = (long)(EX_DENSE_BYTES / ((size_t)n * sizeof(double)));
        if (per < 1) per = 1;
        if (per > F) per = F;
        void *w = nullptr;
        int rc = ws_get(ctx, vbx_ctx::WS_EX, 16 + (size_t)per * (size_t)n * sizeof(double), &w);
        if (rc != VBX_SUCCESS) return rc;
        int32_t *total = (int32_t *)w;                            // [1]: the guard's count over the whole call
        double *dense = (double *)((char *)w + 16);
        bool counted = false;
        for (long f0 = 0; f0 < F; f0 += per) {
            const long nf = (F - f0 < per) ? F - f0 : per;
            { Prof pr(ctx, "resample", stm); launch_resample(stm, x.f64() + f0 * stride, nf, (int)rp->n_src, stride, rp->rs.li, rp->rs.frac, n, dense); }
            rc = run_burg(ctx, stm, dense, nf, n, (long)n, window, p, coeffs + f0 * (long)p, st + f0);
            if (rc != VBX_SUCCESS) return rc;
            if (ctx->burg_list_count) { launch_count_accumulate(stm, ctx->burg_list_count + 1, total + 1, f0 == 0); counted = true; }
        }
        if (counted) ctx->burg_list_count = total;
        return VBX_SUCCESS;
    }
    if (!rp && n > VBX_MAX_FRAME_LEN) {
        // a frame longer than a wavefront's registers hold (tests/lib.rs:27-41 passes a whole file as one): one workgroup per
        // frame, the error arrays in an L2-resident scratch (k_long.hip); batches of frames so that the scratch stays <= 1 GiB
        if (x.kind != SAMPLE_F64) return fail(ctx, VBX_E_RUNTIME, "run_burg: the long-frame kernel reads f64 frames");
        ctx->burg_list_count = nullptr;
        long per = (long)((size_t(1) << 30) / burg_long_scratch_bytes(1, n));
        if (per < 1) per = 1;
        if (per > F) per = F;
        void *w = nullptr;
        int rc = ws_get(ctx, vbx_ctx::WS_LONG, burg_long_scratch_bytes(per, n), &w);
        if (rc != VBX_SUCCESS) return rc;
        Prof pr(ctx, "burg_long", stm);
        for (long f0 = 0; f0 < F; f0 += per)
            launch_burg_long(stm, x.f64(), f0, (f0 + per < F) ? f0 + per : F, F, n, stride, window, p, coeffs, st, (double *)w);
        return VBX_SUCCESS;
    }
    if (burg_fast_supported(n, p)) {
        const char *const lags_name = rp ? "burg_lags_resampled" : "burg_lags", *const list_name = rp ? "burg_direct_list_resampled" : "burg_direct_list";
        void *w = nullptr;
        int rc = ws_get(ctx, vbx_ctx::WS_BURG_LIST, burg_fast_scratch_bytes(F, p), &w);
        if (rc != VBX_SUCCESS) return rc;
        int32_t *list = burg_fast_list(w, F, p);
        ctx->burg_list_count = list;
        VBX_HIP(ctx, hipMemsetAsync(list, 0, sizeof(int32_t), stm));
        const long items = frame_map_items(map, F), chunk = burg_fast_chunk(F);
        for (long i0 = 0; i0 < items; i0 += chunk) {
            const long m = (items - i0 < chunk) ? items - i0 : chunk;
            { Prof pr(ctx, lags_name, stm);
              const bool ok = rp ? launch_burg_lags_resampled(stm, x, F, n, stride, window, rp->rs, p, map, i0, m, w)
                                 : launch_burg_lags(stm, x, F, n, stride, window, p, map, i0, m, w);
              if (!ok) return fail(ctx, VBX_E_RUNTIME, std::string(lags_name) + ": no " + k_kind_names[x.kind] + " lag kernel at order " + std::to_string(p)); }
            { Prof pr(ctx, "burg_recursion", stm); launch_burg_recursion(stm, F, p, map, i0, m, coeffs, st, w); }
        }
        { Prof pr(ctx, list_name, stm);
          if (rp) launch_burg_resampled_list(stm, x, F, n, stride, window, rp->rs, p, coeffs, st, list + 2, list);
          else launch_burg_list(stm, x, F, n, stride, window, p, coeffs, st, list + 2, list); }
        // the probe (vbx_internal_last_burg_direct_count) reports the whole CALL: list[0] restarts with every time slice of
        // find_formants, list[1] adds the slices up (reset with the call's first slice)
        launch_count_accumulate(stm, list, list + 1, map.seg_len == 0 || map.t0 == 0);
        return VBX_SUCCESS;
    }
    Prof pr(ctx, rp ? "burg_resampled" : "burg", stm);
    ctx->burg_list_count = nullptr;
    if (rp) launch_burg_resampled(stm, x, F, n, stride, window, rp->rs, p, coeffs, st, map);
    else launch_burg(stm, x, F, n, stride, window, p, coeffs, st, map);
    return VBX_SUCCESS;
}

int vbx_lpc_burg_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len,
                     size_t stride, const double *window, size_t n_coeffs, double *out, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, burg_order_ok(frame_len, n_coeffs), "frame_len must be >= 2, order in [1, 62]");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    rc = run_burg(ctx, ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_coeffs, out, status);
    if (rc != VBX_SUCCESS) return rc;
    return check_launch(ctx, __func__);
}

// ---- polynomial.rs ------------------------------------------------------------------------

int vbx_find_roots_c64(vbx_ctx *ctx, vbx_complex *polys, size_t n_polys, size_t len, int32_t *status) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_polys == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, polys != nullptr, "null polynomials");
    VBX_REQUIRE(ctx, len >= 1 && len <= VBX_MAX_POLY_LEN, "len must be in [1, 64]");
    VBX_REQUIRE(ctx, n_polys <= 0x7fffffffull, "too many polynomials");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "find_roots"); launch_find_roots(ctx->stream, (cplx_t *)polys, (long)n_polys, (int)len, status); }
    return check_launch(ctx, __func__);
}

int vbx_laguerre_c64(vbx_ctx *ctx, const vbx_complex *polys, size_t n_polys, size_t len,
                     vbx_complex start, vbx_complex *out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_polys == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, polys && out, "null argument");
    VBX_REQUIRE(ctx, len >= 2 && len <= VBX_MAX_POLY_LEN, "len must be in [2, 64]");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    cplx_t s; s.re = start.re; s.im = start.im;
    { Prof p(ctx, "laguerre"); launch_laguerre(ctx->stream, (const cplx_t *)polys, (long)n_polys, (int)len, s, (cplx_t *)out); }
    return check_launch(ctx, __func__);
}

int vbx_div_polynomial_c64(vbx_ctx *ctx, vbx_complex *polys, const vbx_complex *others, size_t n_polys, size_t len,
                           vbx_complex *rem, int32_t *status) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_polys == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, polys && others && rem, "null argument");
    VBX_REQUIRE(ctx, len >= 1 && len <= VBX_MAX_POLY_LEN, "len must be in [1, 64]");
    VBX_REQUIRE(ctx, n_polys <= 0x7fffffffull, "too many polynomials");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "div_polynomial"); launch_div_polynomial(ctx->stream, (cplx_t *)polys, (const cplx_t *)others, (long)n_polys, (int)len, (cplx_t *)rem, status); }
    return check_launch(ctx, __func__);
}

int vbx_find_roots_c32(vbx_ctx *ctx, vbx_complex32 *polys, size_t n_polys, size_t len, int32_t *status) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_polys == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, polys != nullptr, "null polynomials");
    VBX_REQUIRE(ctx, len >= 1 && len <= VBX_MAX_POLY_LEN, "len must be in [1, 64]");
    VBX_REQUIRE(ctx, n_polys <= 0x7fffffffull, "too many polynomials");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "find_roots_f32"); launch_find_roots_f32(ctx->stream, (cplx32_t *)polys, (long)n_polys, (int)len, status); }
    return check_launch(ctx, __func__);
}

int vbx_laguerre_c32(vbx_ctx *ctx, const vbx_complex32 *polys, size_t n_polys, size_t len,
                     vbx_complex32 start, vbx_complex32 *out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_polys == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, polys && out, "null argument");
    VBX_REQUIRE(ctx, len >= 2 && len <= VBX_MAX_POLY_LEN, "len must be in [2, 64]");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    cplx32_t s; s.re = start.re; s.im = start.im;
    { Prof p(ctx, "laguerre_f32"); launch_laguerre_f32(ctx->stream, (const cplx32_t *)polys, (long)n_polys, (int)len, s, (cplx32_t *)out); }
    return check_launch(ctx, __func__);
}

// ---- spectrum.rs: resonances, tracker -----------------------------------------------------

int vbx_to_resonance_c64(vbx_ctx *ctx, const vbx_complex *roots, size_t n_rows, size_t n_roots,
                         double sample_rate, vbx_resonance *out_res, int32_t *out_count) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_rows == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, roots && out_res && n_roots >= 1 && n_roots <= 0x7fffffff, "bad argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    {
        Prof p(ctx, "to_resonance");
        launch_to_resonance(ctx->stream, (const cplx_t *)roots, (long)n_rows, (int)n_roots, sample_rate, 0,
                            (res_t *)out_res, (int)n_roots, out_count, nullptr);
    }
    return check_launch(ctx, __func__);
}

// Utterances of a few hundred frames or more take the chunked scan (k_tracker.hip: speculative chunks + exact repair, the
// same rows bit for bit, ~1 ms whatever the lengths): one lane per utterance costs ~5.4 us per frame of the LONGEST
// utterance.  VBX_TRACKER_CHUNKED=1 / 0 forces / forbids it (tests, A/B runs).
static bool tracker_wants_chunks(const int64_t *h_seg_start, size_t n_segments, size_t n_frames) {
    const char *env = getenv("VBX_TRACKER_CHUNKED");          // read per call: tests switch it
    const int forced = env ? atoi(env) : -1;
    if (forced >= 0) return forced != 0;
    long longest = 0;
    if (h_seg_start == nullptr || n_segments == 0) longest = (long)n_frames;
    else for (size_t i = 0; i < n_segments; i++) {
        const long end = (i + 1 < n_segments) ? (long)h_seg_start[i + 1] : (long)n_frames;
        if (end - (long)h_seg_start[i] > longest) longest = end - (long)h_seg_start[i];
    }
    // 2 ms of scan on one lane, where the chunked scan takes about 0.6 for any batch; and large batches of SHORT utterances
    // too since round 3: with Burg in one pass and the roots from conjugate pairs nothing is left for the time slices of
    // run_find_formants to hide the sequential scan behind (a million frames in utterances of 64 / 256 / 383 frames: sliced
    // 2.15 / 2.21 / 2.27 ms, chunked 1.84 / 2.15 / 2.13)
    return longest >= 384 || n_frames >= 65536;
}

static int run_tracker(vbx_ctx *ctx, hipStream_t st, bool chunked, const res_t *res, long F, int n_res, const int32_t *res_count,
                       const int64_t *d_seg, long nseg, const res_t *d_est, int n_est, const int32_t *frame_status,
                       res_t *out, long out_ld) {
    if (!chunked) {
        Prof p(ctx, "tracker", st);
        launch_tracker(st, res, F, n_res, res_count, d_seg, nseg, d_est, n_est, frame_status, out, out_ld);
        return VBX_SUCCESS;
    }
    void *w = nullptr;
    int rc = ws_get(ctx, vbx_ctx::WS_TRK, tracker_chunked_workspace_bytes(F), &w);
    if (rc != VBX_SUCCESS) return rc;
    Prof p(ctx, "tracker_chunked", st);
    launch_tracker_chunked(st, res, F, n_res, res_count, d_seg, nseg, d_est, n_est, frame_status, out, out_ld, w);
    return VBX_SUCCESS;
}

int vbx_estimate_formants_f64(vbx_ctx *ctx, const vbx_resonance *res, size_t n_frames, size_t n_res,
                              const int64_t *h_seg_start, size_t n_segments,
                              const vbx_resonance *h_est_init, size_t n_est,
                              const int32_t *frame_status, vbx_resonance *out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, res && h_est_init && out, "null argument");
    VBX_REQUIRE(ctx, n_res >= 1 && n_res <= 0x7fffffff, "n_res must be >= 1 (the reference indexes resonances[0])");
    VBX_REQUIRE(ctx, n_est >= 1 && n_est <= VBX_FORMANT_SLOTS, "n_est must be in [1, 6]");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t *d_seg = nullptr; size_t nseg = 1; const res_t *d_est = nullptr;
    int rc = upload_segments(ctx, ctx->stream, h_seg_start, n_segments, n_frames, &d_seg, &nseg);
    if (rc != VBX_SUCCESS) return rc;
    rc = upload_estimates(ctx, ctx->stream, h_est_init, n_est, &d_est);
    if (rc != VBX_SUCCESS) return rc;
    rc = run_tracker(ctx, ctx->stream, tracker_wants_chunks(h_seg_start, n_segments, n_frames), (const res_t *)res, (long)n_frames,
                     (int)n_res, nullptr, d_seg, (long)nseg, d_est, (int)n_est, frame_status, (res_t *)out, 2 * (long)n_est);
    if (rc != VBX_SUCCESS) return rc;
    return check_launch(ctx, __func__);
}

// internal (tests only; not part of the public header): the same scan with the per-row counts find_formants keeps beside
// its resonance rows (rows of `count` real entries with ascending positive frequencies, then zeros, may take the tracker's
// index form: k_tracker.hip)
int vbx_internal_estimate_formants_counted(vbx_ctx *ctx, const vbx_resonance *res, size_t n_frames, size_t n_res,
                                           const int32_t *res_count, const int64_t *h_seg_start, size_t n_segments,
                                           const vbx_resonance *h_est_init, size_t n_est,
                                           const int32_t *frame_status, vbx_resonance *out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, res && res_count && h_est_init && out, "null argument");
    VBX_REQUIRE(ctx, n_res >= 1 && n_res <= 0x7fffffff && n_est >= 1 && n_est <= VBX_FORMANT_SLOTS, "bad size");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t *d_seg = nullptr; size_t nseg = 1; const res_t *d_est = nullptr;
    int rc = upload_segments(ctx, ctx->stream, h_seg_start, n_segments, n_frames, &d_seg, &nseg);
    if (rc != VBX_SUCCESS) return rc;
    rc = upload_estimates(ctx, ctx->stream, h_est_init, n_est, &d_est);
    if (rc != VBX_SUCCESS) return rc;
    rc = run_tracker(ctx, ctx->stream, tracker_wants_chunks(h_seg_start, n_segments, n_frames), (const res_t *)res, (long)n_frames,
                     (int)n_res, res_count, d_seg, (long)nseg, d_est, (int)n_est, frame_status, (res_t *)out, 2 * (long)n_est);
    if (rc != VBX_SUCCESS) return rc;
    return check_launch(ctx, __func__);
}

// Burg coefficients -> resonance rows: the conjugate-pair form (k_roots_fast.hip) where it exists (it does the frames that
// fail its own check again by the reference's iteration), every other order through the reference's iteration (k_roots.hip)
static int run_formant_resonances(vbx_ctx *ctx, hipStream_t stm, const double *coeffs, long F, int p, double sample_rate,
                                  res_t *res, int32_t *cnt, int32_t *st, frame_map_t map = frame_map_t{0, 0, 0}) {
    if (formant_resonances_fast_supported(p)) {
        void *w = nullptr;
        int rc = ws_get(ctx, vbx_ctx::WS_ROOTS_LIST, 4 * sizeof(int32_t), &w);
        if (rc != VBX_SUCCESS) return rc;
        int32_t *redo = (int32_t *)w;
        ctx->roots_list_count = redo;
        if (map.seg_len == 0 || map.t0 == 0) VBX_HIP(ctx, hipMemsetAsync(redo, 0, sizeof(int32_t), stm));   // once per call
        Prof pr(ctx, "formant_resonances", stm);
        launch_formant_resonances_fast(stm, coeffs, F, p, sample_rate, res, cnt, st, map, redo);
        return VBX_SUCCESS;
    }
    ctx->roots_list_count = nullptr;
    Prof pr(ctx, "formant_resonances", stm);
    launch_formant_resonances(stm, coeffs, F, p, sample_rate, res, cnt, st, map);
    return VBX_SUCCESS;
}

static int run_find_formants(vbx_ctx *ctx, hipStream_t stm, frames_t x, size_t n_frames, size_t frame_len,
                             size_t stride, double sample_rate, size_t n_coeffs,
                             const int64_t *h_seg_start, size_t n_segments,
                             const vbx_resonance *h_est_init, size_t n_est,
                             vbx_resonance *out_formants, size_t formants_ld, vbx_resonance *out_res, int32_t *out_res_count,
                             double *out_coeffs, int32_t *status,
                             const resample_plan_t *rp = nullptr /* find_formants on the frames' resampled view (run_burg) */) {
    VBX_REQUIRE(ctx, h_est_init && out_formants, "null argument");
    if (rp) frame_len = rp->m;                                   // what Burg sees
    VBX_REQUIRE(ctx, burg_order_ok(frame_len, n_coeffs), "frame_len must be >= 2, order in [1, 62]");
    VBX_REQUIRE(ctx, n_est >= 1 && n_est <= VBX_FORMANT_SLOTS, "n_est must be in [1, 6]");
    VBX_REQUIRE(ctx, formants_ld >= 2 * n_est && formants_ld % 2 == 0, "formant rows must be 16-byte aligned and hold n_est entries");
    const long F = (long)n_frames; const int p = (int)n_coeffs;
    int rc;
    void *w = nullptr;
    double *coeffs = out_coeffs;
    if (!coeffs) { rc = ws_get(ctx, vbx_ctx::WS_COEFFS, n_frames * n_coeffs * sizeof(double), &w); if (rc) return rc; coeffs = (double *)w; }
    res_t *res = (res_t *)out_res;
    if (!res) { rc = ws_get(ctx, vbx_ctx::WS_RES, n_frames * VBX_MAX_RESONANCES * sizeof(vbx_resonance), &w); if (rc) return rc; res = (res_t *)w; }
    int32_t *cnt = out_res_count;
    if (!cnt) { rc = ws_get(ctx, vbx_ctx::WS_COUNT, n_frames * sizeof(int32_t), &w); if (rc) return rc; cnt = (int32_t *)w; }
    int32_t *st = status;
    if (!st) { rc = ws_get(ctx, vbx_ctx::WS_STATUS, n_frames * sizeof(int32_t), &w); if (rc) return rc; st = (int32_t *)w; }
    const double *hann = nullptr;
    VBX_HIP(ctx, ctx->tables.window(VBX_WINDOW_HANNING_PERIODIC, frame_len, &hann));   // src/lib.rs:65-70
    const int64_t *d_seg = nullptr; size_t nseg = 1; const res_t *d_est = nullptr;
    rc = upload_segments(ctx, stm, h_seg_start, n_segments, n_frames, &d_seg, &nseg);
    if (rc != VBX_SUCCESS) return rc;
    rc = upload_estimates(ctx, stm, h_est_init, n_est, &d_est);
    if (rc != VBX_SUCCESS) return rc;
    // The tracker is a chain of dependent steps per utterance (~5 us per frame, whatever the batch size).  Utterances long
    // enough for that to matter take the chunked scan after Burg and the root finder (run_tracker).  The alternative kept
    // behind VBX_TRACKER_CHUNKED=0 -- round 2's first answer, for batches of equal-length utterances: the work is cut into
    // time slices, and while the tracker walks frames [t0, t0 + tc) of every utterance on its own stream, Burg and the root
    // finder already produce the next slice (config 4 in round 2: 152 M frames/s against the chunked scan's 156 M).  Since
    // round 3 only VBX_TRACKER_CHUNKED=0 reaches it (tracker_wants_chunks).
    long seg_len = 0;
    const bool chunked = tracker_wants_chunks(h_seg_start, n_segments, n_frames);   // long utterances: the chunked scan instead
    if (!chunked && h_seg_start != nullptr && n_segments >= 64 && F >= 65536 && !(rp && !rp->direct)) {
        seg_len = (n_segments > 1) ? (long)h_seg_start[1] : 0;
        for (size_t i = 0; i < n_segments && seg_len > 0; i++) if (h_seg_start[i] != (int64_t)i * seg_len) seg_len = 0;
        // the slices cover t in [0, seg_len) of every utterance: a LAST utterance longer than the others (its end is
        // n_frames, not a seg_start entry) would keep rows past seg_len that no slice tracks -> the unsliced path
        if (seg_len > 0 && ((long)(n_segments - 1) * seg_len >= F || (long)n_segments * seg_len < F || seg_len < 64)) seg_len = 0;
    }
    // Six slices (VBX_FF_SLICES overrides, 1..8).  With k equal slices the call ends about one slice's scan after the last
    // resonance exists, so more slices shorten the exposed tail -- until a slice no longer fills the GPU: the root finder
    // is a chain of dependent operations per lane and a launch takes one wavefront's run time (0.47 ms at order 12) however
    // few wavefronts it has.  Measured, frames/s at 1 M x 512 for k = 4, 5, 6, 7, 8: 140, 144, 153, 142, 136 M; k = 6 is also
    // the best or within 1 % of it at 0.3, 0.7, 1.3 and 2 M frames and in the 4.5 M-frame pipeline.
    static const int want_slices = [] { const char *e = getenv("VBX_FF_SLICES"); const int v = e ? atoi(e) : 6; return v < 1 ? 1 : (v > 8 ? 8 : v); }();
    const int n_slices = seg_len > 0 ? want_slices : 1;
    const long tc = (seg_len + n_slices - 1) / n_slices;
    ctx->last_track.res = res; ctx->last_track.cnt = cnt; ctx->last_track.st = st; ctx->last_track.F = F;
    ctx->last_track.n_est = (int)n_est; ctx->last_track.out = (res_t *)out_formants; ctx->last_track.out_ld = (long)formants_ld;
    if (n_slices == 1) {
        rc = run_burg(ctx, stm, x, F, (int)frame_len, (long)stride, hann, p, coeffs, st, frame_map_t{0, 0, 0}, rp);                // :75
        if (rc != VBX_SUCCESS) return rc;
        rc = run_formant_resonances(ctx, stm, coeffs, F, p, sample_rate, res, cnt, st);                                            // :80-110
        if (rc != VBX_SUCCESS) return rc;
        rc = run_tracker(ctx, stm, chunked, res, F, VBX_MAX_RESONANCES, cnt, d_seg, (long)nseg, d_est, (int)n_est, st,
                         (res_t *)out_formants, (long)formants_ld);                                                                    // :114
        if (rc != VBX_SUCCESS) return rc;
        return check_launch(ctx, "vbx_find_formants_f64");
    }
    if (!ctx->trk) {
        VBX_HIP(ctx, hipStreamCreateWithFlags(&ctx->trk, hipStreamNonBlocking));
        for (auto &e : ctx->ev_slice) VBX_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        VBX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_trk, hipEventDisableTiming));
    }
    for (int j = 0; j < n_slices && j * tc < seg_len; j++) {
        const frame_map_t map{seg_len, j * tc, (seg_len - j * tc < tc) ? seg_len - j * tc : tc};   // the last slice may be shorter
        rc = run_burg(ctx, stm, x, F, (int)frame_len, (long)stride, hann, p, coeffs, st, map, rp);
        if (rc != VBX_SUCCESS) return rc;
        rc = run_formant_resonances(ctx, stm, coeffs, F, p, sample_rate, res, cnt, st, map);
        if (rc != VBX_SUCCESS) return rc;
        VBX_HIP(ctx, hipEventRecord(ctx->ev_slice[j], stm));
        VBX_HIP(ctx, hipStreamWaitEvent(ctx->trk, ctx->ev_slice[j], 0));
        { Prof pr(ctx, "tracker", ctx->trk); launch_tracker(ctx->trk, res, F, VBX_MAX_RESONANCES, cnt, d_seg, (long)nseg, d_est, (int)n_est, st, (res_t *)out_formants, (long)formants_ld, j * tc, tc); }
    }
    VBX_HIP(ctx, hipEventRecord(ctx->ev_trk, ctx->trk));
    VBX_HIP(ctx, hipStreamWaitEvent(stm, ctx->ev_trk, 0));                // join: the formant tracks are complete on stm
    return check_launch(ctx, "vbx_find_formants_f64");
}

int vbx_find_formants_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len,
                          size_t stride, double sample_rate, size_t n_coeffs,
                          const int64_t *h_seg_start, size_t n_segments,
                          const vbx_resonance *h_est_init, size_t n_est,
                          vbx_resonance *out_formants, vbx_resonance *out_res, int32_t *out_res_count,
                          double *out_coeffs, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    return run_find_formants(ctx, ctx->stream, x, n_frames, frame_len, stride, sample_rate, n_coeffs, h_seg_start, n_segments,
                             h_est_init, n_est, out_formants, 2 * n_est, out_res, out_res_count, out_coeffs, status);
}

// The tracks of the LAST vbx_find_formants_f64 / vbx_analyze_frames_* call on this context, continued from the true state
// before frame `first` (k_tracker.hip, tracker_stitch_kernel); stream: the context's, or the communicator's (vbx_comm.hip)
int vbx_internal_track_stitch(vbx_ctx *ctx, void *stream, vbx_resonance *formants, size_t n_frames, size_t formants_ld,
                              size_t first, size_t stop, const double *d_state_in, int32_t *d_changed) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_REQUIRE(ctx, formants && d_state_in, "null argument");
    const auto &lt = ctx->last_track;
    VBX_REQUIRE(ctx, lt.res != nullptr && lt.out == (res_t *)formants && lt.F == (long)n_frames && lt.out_ld == (long)formants_ld,
                "the formant rows are not the ones the last find_formants / analyze_frames call on this context wrote");
    VBX_REQUIRE(ctx, first <= stop && stop <= n_frames, "need first <= stop <= n_frames");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    { Prof p(ctx, "tracker_stitch", st);
      launch_tracker_stitch(st, lt.res, lt.F, VBX_MAX_RESONANCES, lt.cnt, lt.n_est, lt.st, lt.out, lt.out_ld, (long)first, (long)stop,
                            d_state_in, d_changed); }
    return check_launch(ctx, "vbx_track_stitch_f64");
}

int vbx_track_stitch_f64(vbx_ctx *ctx, vbx_resonance *formants, size_t n_frames, size_t formants_ld, size_t first, size_t stop,
                         const vbx_resonance *d_state_in, int32_t *d_changed) {
    return vbx_internal_track_stitch(ctx, nullptr, formants, n_frames, formants_ld, first, stop, (const double *)d_state_in, d_changed);
}

// 2 * VBX_FORMANT_SLOTS doubles of context-owned device memory (the state a communicator receives from the previous rank)
double *vbx_internal_stitch_state(vbx_ctx *ctx) {
    if (!ctx) return nullptr;
    if (!ctx->stitch_state) {
        if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
        if (hipMalloc((void **)&ctx->stitch_state, (2 * VBX_FORMANT_SLOTS + 2) * sizeof(double)) != hipSuccess) { ctx->stitch_state = nullptr; return nullptr; }
    }
    return ctx->stitch_state;
}
int vbx_internal_last_track_n_est(vbx_ctx *ctx) { return ctx ? ctx->last_track.n_est : 0; }
int vbx_internal_last_spectral_split(vbx_ctx *ctx) { return ctx ? ctx->last_spectral_split : 0; }
int vbx_internal_last_mfcc_interp(vbx_ctx *ctx) { return ctx ? ctx->last_mfcc_interp : 0; }
// Every MFCC kernel is profiled as "mfcc" and every pitch kernel as "pitch": these say which one the context's last call took.
// MFCC: 1 the fused kernels' forward transform, 2 the same with interpolated bins, 3 chirp-z, 4 matrix-core two-stage DFT,
// 5 vector two-stage DFT, 6 Goertzel, 7 the long-frame kernel, 8 every frame panics (rows filled).
// Pitch: 100 * family (1 long frames, 2 the direct lag sums below 512 samples / VBX_PITCH_MFMA, 3 + spectral plan: the FFT kernels)
// + the candidate list (0 lane-resident, 1 LDS-resident, 2 parked in the output row).
int vbx_internal_last_mfcc_form(vbx_ctx *ctx) { return ctx ? ctx->last_mfcc_form : 0; }
int vbx_internal_last_pitch_form(vbx_ctx *ctx) { return ctx ? ctx->last_pitch_form : 0; }
// every host-side condition of a stitch / hand-off on these rows, for callers that must know BEFORE they enqueue anything
// a peer waits for (vbx_comm.hip: an early return between ncclRecv and ncclSend would leave the next rank blocked)
int vbx_internal_track_check(vbx_ctx *ctx, const vbx_resonance *formants, size_t n_frames, size_t formants_ld) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    const auto &lt = ctx->last_track;
    VBX_REQUIRE(ctx, lt.res != nullptr && lt.n_est >= 1, "no tracks on this context: the last call produced none");
    VBX_REQUIRE(ctx, formants && lt.out == (const res_t *)formants && lt.F == (long)n_frames && lt.out_ld == (long)formants_ld,
                "the formant rows are not the ones the last find_formants / analyze_frames call on this context wrote");
    return VBX_SUCCESS;
}

// Host only (no device, no context): the tables of the MFCC bins interpolated inside the fused kernel (mfcc_interp_t) for one shape,
// for tests that hold the interpolation to the frame's exact DFT.  desc[8] = {M, threads per frame, slots, taps, jmin, jmax,
// byte offset of the taps, byte offset of the first-tap indices}; *need = bytes of the table (copied to buf when cap >= *need).
// Returns 1 when the shape has the form, 0 when it has not (its MFCC comes from the chirp-z kernel), < 0 on a bad argument.
int vbx_internal_mfcc_interp_table(size_t frame_len, int b_lo, int nb, int32_t *desc, void *buf, size_t cap, size_t *need) {
    if (!desc || !need || frame_len < 2 || frame_len > VBX_MAX_FRAME_LEN || nb < 1 || nb > 4096) return VBX_E_INVALID;
    const int plan = spectral_plan_mfcc((int)frame_len);                  // (the plan vbx_analyze_frames_f64 picks)
    if (plan == SPECTRAL_PLAN_NONE || (2 * spectral_plan_nc(plan)) % (int)frame_len == 0) return 0;
    const size_t bytes = mfcc_interp_table_bytes(plan, nb);
    *need = bytes;
    std::vector<char> h(bytes, 0);
    mfcc_interp_t d{};
    if (!mfcc_interp_fill(plan, (int)frame_len, b_lo, nb, h.data(), &d)) return 0;
    const int nt = plan == SPECTRAL_PLAN_4096 ? 128 : 64;
    desc[0] = 4 * spectral_plan_nc(plan) / 2; desc[1] = nt; desc[2] = (nb + nt - 1) / nt; desc[3] = d.taps;
    desc[4] = d.jmin; desc[5] = d.jmax; desc[6] = (int32_t)mfcc_interp_coef_offset(plan); desc[7] = (int32_t)mfcc_interp_j0_offset(plan, nb);
    if (buf && cap >= bytes) std::memcpy(buf, h.data(), bytes);
    return 1;
}

// Host only: the plans whose fields the MFCC table builders of vbx_host.cpp take (vbx_internal_host_table; tests): out[0 .. 9) = the
// matrix-core plan {ok, n1, n2, k2, mt, ntd, ntm, src0, src1}, out[9 .. 14) = the two-stage plan {ok, n1, n2, nc, tm}
int vbx_internal_mfcc_table_plans(size_t frame_len, int b_lo, int nb, int32_t *out) {
    if (!out || frame_len < 2 || frame_len > VBX_MAX_FRAME_LEN || b_lo < 0 || nb < 1 || nb > 4096) return VBX_E_INVALID;
    const mfcc_mplan_t m = mfcc_mfma_plan((int)frame_len, b_lo, nb);
    const mfcc_plan_t p = mfcc_plan((int)frame_len, nb);
    const int32_t v[14] = {m.ok, m.n1, m.n2, m.k2, m.mt, m.ntd, m.ntm, m.src0, m.src1, p.ok, p.n1, p.n2, p.nc, p.tm};
    std::memcpy(out, v, sizeof v);
    return VBX_SUCCESS;
}

// ---- spectrum.rs: MFCC --------------------------------------------------------------------

static int run_mfcc(vbx_ctx *ctx, hipStream_t stm, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                    const double *window, size_t num_coeffs, double lo_hz, double hi_hz,
                    double sample_rate, double *out, size_t out_ld, int32_t *status) {
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, num_coeffs >= 1 && num_coeffs <= 64, "num_coeffs must be in [1, 64]");
    VBX_REQUIRE(ctx, out_ld >= num_coeffs, "output rows must hold num_coeffs entries");
    std::vector<int32_t> hb; bool bad = false; const int32_t *d_bins = nullptr;
    ctx->last_mfcc_interp = 0;
    ctx->last_mfcc_form = 0;
    int rc = get_bins_dev(ctx, frame_len, num_coeffs, lo_hz, hi_hz, sample_rate, &d_bins, hb, bad);
    if (rc != VBX_SUCCESS) return rc;
    if (bad) {   // the reference panics on every frame (bins do not depend on the data)
        ctx->last_mfcc_form = 8;
        { Prof p(ctx, "fill_rows", stm); launch_fill_rows(stm, out, (long)n_frames, (int)num_coeffs, (long)out_ld, 0.0, status, VBX_FRAME_ERR_PANIC); }
        return check_launch(ctx, "vbx_mfcc_f64");
    }
    const int nb = hb.back() - hb.front();
    const double *dct = nullptr, *slopes = nullptr;
    VBX_HIP(ctx, ctx->tables.dct(num_coeffs, &dct));
    VBX_HIP(ctx, ctx->tables.slopes(frame_len, num_coeffs, lo_hz, hi_hz, sample_rate, hb, &slopes));
    if (frame_len > VBX_MAX_FRAME_LEN) {          // a long frame: the Goertzel recurrence over HBM, the filter sums' inputs in a scratch (k_long.hip)
        VBX_REQUIRE(ctx, nb >= 1, "no mel bins");
        const double *tw = nullptr;
        VBX_HIP(ctx, ctx->tables.goertzel(frame_len, hb.front(), nb, &tw));
        void *w = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_CZT, mfcc_long_scratch_bytes((long)n_frames, nb), &w); if (rc != VBX_SUCCESS) return rc;
        ctx->last_mfcc_form = 7;
        { Prof p(ctx, "mfcc_long", stm);
          launch_mfcc_long(stm, x, (long)n_frames, (long)frame_len, (long)stride, window, tw, d_bins, slopes, dct, (int)num_coeffs, nb, out,
                           (long)out_ld, status, (double *)w); }
        return check_launch(ctx, "vbx_mfcc_f64");
    }
    // frames that fill one of the FFT kernels' transforms (1024, 1200, 2048, 4096): the forward half of the fused spectral
    // kernel -- one real FFT of the zero-padded frame, whose even bins are the n-point DFT the mel filters read
    {
        int plan = spectral_plan((int)frame_len);
        // 2048 and 4096 samples: the frame as the real sequence of the half-size transform (complex 1024 / 2048), no padding
        if (frame_len == 2048) plan = SPECTRAL_PLAN_1024; else if (frame_len == 4096) plan = SPECTRAL_PLAN_2048;
        if (!ctx->mfcc_force_goertzel && !ctx->mfcc_force_dft2 && !ctx->mfcc_force_mfma && plan != SPECTRAL_PLAN_NONE &&
            ((int)frame_len == spectral_plan_nc(plan) || (int)frame_len == 2 * spectral_plan_nc(plan)) &&
            num_coeffs <= 64 && nb >= 1 && hb.front() >= 0 && hb.front() + nb <= (int)frame_len / 2) {
            const double *tab = nullptr;
            VBX_HIP(ctx, ctx->tables.spectral(plan, &tab));
            spectral_launch_t L{};
            L.plan = plan; L.n = (int)frame_len; L.mfcc_only = true;
            L.x = x; L.F = (long)n_frames; L.stride = (long)stride; L.window = window; L.tab = tab;
            L.out_mfcc = out; L.mfcc_ld = (long)out_ld; L.mfcc_status = status;
            L.bins = d_bins; L.slopes = slopes; L.dct = dct; L.num_coeffs = (int)num_coeffs; L.nb = nb;
            ctx->last_mfcc_form = 1;
            { Prof p(ctx, "mfcc", stm); launch_analyze(stm, L); }
            return check_launch(ctx, "vbx_mfcc_f64");
        }
    }
    // composite frame lengths: two-stage DFT of the needed bins, on the matrix cores when the factorisation fits
    // the MFMA kernel's tiles, else on the vector ALU; otherwise (prime-ish lengths) Goertzel.  Every kernel writes
    // status 0 itself (no separate memset queued behind whatever the stream is running).
    const bool composite_ok = nb > 0 && !ctx->mfcc_force_goertzel;
    const mfcc_mplan_t mp = (composite_ok && !ctx->mfcc_force_dft2 && ctx->mfcc_czt != 1) ? mfcc_mfma_plan((int)frame_len, hb.front(), nb) : mfcc_mplan_t{};
    const mfcc_plan_t pl = (composite_ok && !mp.ok) ? mfcc_plan((int)frame_len, nb) : mfcc_plan_t{false, 0, 0, 0, 0};
    // Round 5: the forward transform of the zero-padded frame that the fused kernels use, the frame's DFT bins interpolated from the
    // transform's (mfcc_interp_t, vbx_kernels.hpp: 24-40 taps per bin, error < 1e-14 of the largest bin) -- one transform instead of the
    // chirp-z kernel's two.  Where the matrix-core kernel has no plan, and from 1400 samples up where it has (measured, M frames/s,
    // before -> interpolated: 1103: 63 -> 110, 2047: 30 -> 54, 3000: 29 -> 34, 4000: 12 -> 26; 1500 / 1600 / 1800: 61 -> 71, 62 -> 73,
    // 48 -> 67; the matrix-core kernel stays at 700 / 882 / 1280: 209 / 161 / 94 against 133 / 123 / 74).
    // VBX_MFCC_INTERP=0 / the force switches: the kernels below, as before.
    if ((!mp.ok || frame_len >= 1400) && ctx->mfcc_interp != 0 && ctx->mfcc_czt != 1 && !ctx->mfcc_force_goertzel && !ctx->mfcc_force_dft2 && !ctx->mfcc_force_mfma &&
        num_coeffs <= 64 && nb >= 1 && nb <= 4096 && hb.front() >= 0 && hb.front() + nb <= (int)frame_len / 2) {
        const int plan = spectral_plan_mfcc((int)frame_len);
        bool ok = false;
        mfcc_interp_t ip{};
        if (plan != SPECTRAL_PLAN_NONE && (2 * spectral_plan_nc(plan)) % (int)frame_len != 0 && (int)frame_len < spectral_plan_nc(plan)) {
            VBX_HIP(ctx, ctx->tables.interp(plan, (int)frame_len, hb.front(), nb, &ip, &ok));
        }
        if (ok) {
            const double *tab = nullptr;
            VBX_HIP(ctx, ctx->tables.spectral(plan, &tab));
            spectral_launch_t L{};
            L.plan = plan; L.n = (int)frame_len; L.mfcc_only = true; L.interp = true; L.ip = ip;
            ctx->last_mfcc_interp = 1;
            ctx->last_mfcc_form = 2;
            L.x = x; L.F = (long)n_frames; L.stride = (long)stride; L.window = window; L.tab = tab;
            L.out_mfcc = out; L.mfcc_ld = (long)out_ld; L.mfcc_status = status;
            L.bins = d_bins; L.slopes = slopes; L.dct = dct; L.num_coeffs = (int)num_coeffs; L.nb = nb;
            { Prof p(ctx, "mfcc", stm); launch_analyze(stm, L); }
            return check_launch(ctx, "vbx_mfcc_f64");
        }
    }
    // no matrix-core factorisation (prime-ish lengths such as 1103 = 25 ms at 44.1 kHz, or too many bins for the two-stage
    // kernel's tiles: 2500, 3000): the needed bins by the chirp-z identity on a power-of-two transform (two complex FFTs per
    // frame, k_mfcc_czt.hip) instead of evaluating them bin by bin on the vector ALU.  Measured, MFCC alone / the whole
    // pipeline, M frames/s: 1103: 28.9 -> 61.9 / 15.2 -> 20.3; 2500: 7.4 -> 15.0 / 3.2 -> 4.0; 3000: 2.8 -> 15.2 / 1.8 -> 3.9.
    // Where the matrix-core kernel has a plan it stays (1000, 1102, 1800: it is the faster one; 1500, 1600: within 5 %).
    const int czt_top = hb.back();
    int czt_plan = (nb >= 1 && hb.front() >= 0 && num_coeffs <= 64) ? mfcc_czt_plan((int)frame_len, czt_top) : SPECTRAL_PLAN_NONE;
    // too long for one transform (frame_len + top - 1 > 4096: 3,431..4,095 samples at these settings), or VBX_MFCC_CZT_SPLIT=1
    // (tests): the frame in two halves, each with its own chirp segment, the complex results summed (vbx_mfcc_czt.hpp) -- four
    // 4096-point transforms per frame instead of frame_len x bins products (pipeline at 4000 / 2000: 1.4 -> 5.7 M frames/s)
    int czt_n1 = 0;
    if (nb >= 1 && hb.front() >= 0 && num_coeffs <= 64 && (czt_plan == SPECTRAL_PLAN_NONE || ctx->mfcc_czt_split)) {
        int n1 = 0;
        const int p2 = mfcc_czt_split_plan((int)frame_len, czt_top, &n1);
        if (p2 != SPECTRAL_PLAN_NONE) { czt_plan = p2; czt_n1 = n1; }
    }
    // ... and from 1400 samples up to what the 2048-point transform holds, where the matrix-core kernel HAS a plan: inside the
    // pipeline its 512-thread workgroups with ~100 KB of LDS keep the analyze kernel's wavefronts out, the chirp-z kernel's
    // one-wavefront workgroups interleave with them (pipeline at 1500 / 1600 samples: 15.6 -> 16.2, 15.1 -> 16.8 M frames/s;
    // below 1400 and on the 4096-point transform the matrix-core kernel wins: 1280: 19.6 against 17.6, 1800: 14.8 against 12.5)
    const bool czt_over_mfma = mp.ok && czt_plan == SPECTRAL_PLAN_2048 && czt_n1 == 0 && frame_len >= 1400 && ctx->mfcc_czt == -1 &&
                               !(ctx->mfcc_force_goertzel || ctx->mfcc_force_dft2 || ctx->mfcc_force_mfma);
    if (!mp.ok || czt_over_mfma) {
        const int top = czt_top;
        const int cplan = czt_plan;
        const bool forced = ctx->mfcc_force_goertzel || ctx->mfcc_force_dft2 || ctx->mfcc_force_mfma;
        // (below ~600 samples the Goertzel kernel's n * nb products cost less than two 1024-point transforms)
        const bool want = ctx->mfcc_czt == 1 || czt_over_mfma || (ctx->mfcc_czt == -1 && !forced && frame_len >= 600);
        if (cplan != SPECTRAL_PLAN_NONE && want) {
            const double *tab = nullptr, *chirp = nullptr, *bhat = nullptr;
            VBX_HIP(ctx, ctx->tables.spectral(cplan, &tab));
            VBX_HIP(ctx, ctx->tables.czt(frame_len, top, spectral_plan_nc(cplan), czt_n1, &chirp, &bhat));
            void *cw = nullptr;
            rc = ws_get(ctx, vbx_ctx::WS_CZT, (czt_n1 ? 4 : 2) * (size_t)spectral_plan_nc(cplan) * sizeof(double), &cw); if (rc != VBX_SUCCESS) return rc;
            ctx->last_mfcc_form = 3;
            { Prof p(ctx, "mfcc", stm);
              launch_mfcc_czt(stm, cplan, x, (long)n_frames, (int)frame_len, czt_n1, (long)stride, window, tab, chirp, bhat, d_bins, slopes, dct,
                              (int)num_coeffs, nb, out, (long)out_ld, status, (double *)cw); }
            return check_launch(ctx, "vbx_mfcc_f64");
        }
    }
    if (mp.ok) {
        const double *ctab = nullptr, *twd = nullptr, *twm = nullptr, *wm = nullptr;
        VBX_HIP(ctx, ctx->tables.mfma(frame_len, mp, &ctab, &twd, &twm, &wm));
        ctx->last_mfcc_form = 4;
        Prof p(ctx, "mfcc", stm);
        launch_mfcc_mfma(stm, x, (long)n_frames, (int)frame_len, (long)stride, window, mp, ctab, twd, twm, wm, d_bins,
                         slopes, dct, (int)num_coeffs, out, (long)out_ld, status, nb, ctx->cu_count);
    } else if (pl.ok) {
        const double *ctab = nullptr, *twid = nullptr;
        VBX_HIP(ctx, ctx->tables.dft2(frame_len, pl, &ctab, &twid));
        ctx->last_mfcc_form = 5;
        Prof p(ctx, "mfcc", stm);
        launch_mfcc_dft2(stm, x, (long)n_frames, (int)frame_len, (long)stride, window, pl, ctab, twid, d_bins,
                         slopes, dct, (int)num_coeffs, out, (long)out_ld, status, nb, ctx->cu_count);
    } else {
        VBX_REQUIRE(ctx, mfcc_fits((int)frame_len, nb), "frame / bin range does not fit the LDS");
        const double *tw = nullptr;
        VBX_HIP(ctx, ctx->tables.goertzel(frame_len, hb.front(), nb, &tw));
        ctx->last_mfcc_form = 6;
        Prof p(ctx, "mfcc", stm);
        launch_mfcc(stm, x, (long)n_frames, (int)frame_len, (long)stride, window, tw, d_bins, slopes, dct, (int)num_coeffs, out, (long)out_ld, status, nb);
    }
    return check_launch(ctx, "vbx_mfcc_f64");
}

int vbx_mfcc_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                 const double *window, size_t num_coeffs, double lo_hz, double hi_hz,
                 double sample_rate, double *out, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    return run_mfcc(ctx, ctx->stream, x, n_frames, frame_len, stride, window, num_coeffs, lo_hz, hi_hz, sample_rate,
                    out, num_coeffs, status);
}

int vbx_dct_f64(vbx_ctx *ctx, const double *in, size_t n_rows, size_t n, double *out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_rows == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, in && out && n >= 1 && n <= 4096 && n_rows <= 0x7fffffffull, "bad argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const double *dct = nullptr;
    VBX_HIP(ctx, ctx->tables.dct(n, &dct));
    { Prof p(ctx, "dct_rows"); launch_dct_rows(ctx->stream, in, (long)n_rows, (int)n, dct, out); }
    return check_launch(ctx, __func__);
}

// ---- front end (N2, N3) ---------------------------------------------------------------------

int vbx_pcm16_to_f64(vbx_ctx *ctx, const int16_t *pcm, size_t n_samples, double *out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_samples == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, pcm && out, "null argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "pcm16"); launch_pcm16(ctx->stream, pcm, n_samples, 32767.0, out); }
    return check_launch(ctx, __func__);
}

int vbx_f32_to_f64(vbx_ctx *ctx, const float *x, size_t n_samples, double *out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_samples == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, x && out, "null argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "f32_to_f64"); launch_f32_to_f64(ctx->stream, x, n_samples, out); }
    return check_launch(ctx, __func__);
}

int vbx_rms_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                const double *window, double *out) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "rms"); launch_rms(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, out); }
    return check_launch(ctx, __func__);
}

int vbx_preemphasis_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                        double factor, double *out) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, out != x || stride == frame_len, "in-place filtering needs a dense batch (stride == frame_len)");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    if (frame_len > VBX_MAX_FRAME_LEN) {          // a whole signal (src/waves.rs:86 takes any slice): tiles + a carry pass (k_long.hip)
        void *w = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_LONG, preemphasis_long_scratch_bytes((long)n_frames, (long)frame_len), &w);
        if (rc != VBX_SUCCESS) return rc;
        { Prof p(ctx, "preemphasis_long"); launch_preemphasis_long(ctx->stream, x, (long)n_frames, (long)frame_len, (long)stride, 2.0 * M_PI * factor, out, (double *)w); }
        return check_launch(ctx, __func__);
    }
    { Prof p(ctx, "preemphasis"); launch_preemphasis(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, 2.0 * M_PI * factor, out); }
    return check_launch(ctx, __func__);
}

int vbx_ring_frames_f64(vbx_ctx *ctx, const double *ring, size_t capacity, size_t head, size_t n_frames,
                        size_t frame_len, size_t stride, double *out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, ring && out, "null argument");
    VBX_REQUIRE(ctx, capacity >= 1 && head < capacity, "head must lie inside the ring");
    VBX_REQUIRE(ctx, frame_len >= 1 && frame_len <= VBX_MAX_LONG_FRAME_LEN && stride >= 1, "bad frame geometry");
    VBX_REQUIRE(ctx, (n_frames - 1) * stride + frame_len <= capacity, "the view is longer than the deque can be");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "ring_frames"); launch_ring_frames(ctx->stream, ring, (long)capacity, (long)head, (long)n_frames, (int)frame_len, (long)stride, out); }
    return check_launch(ctx, __func__);
}

int vbx_resample_linear_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                            double resample_ratio, double *out) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, resample_ratio > 0.0 && resample_ratio <= 64.0, "resample_ratio must be in (0, 64]");
    const size_t m = vbx_resampled_len(frame_len, resample_ratio);
    VBX_REQUIRE(ctx, m >= 1 && m <= 0x3fffffff, "bad resampled length");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const int32_t *index = nullptr; const double *frac = nullptr;
    VBX_HIP(ctx, ctx->tables.resample(frame_len, resample_ratio, m, &index, &frac));
    { Prof p(ctx, "resample"); launch_resample(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, index, frac, (int)m, out); }
    return check_launch(ctx, __func__);
}

// ---- the user's frame loop, batched and fused ------------------------------------------------------------------

static int ensure_side_stream(vbx_ctx *ctx) {
    if (ctx->side) return VBX_SUCCESS;
    VBX_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    VBX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    VBX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    VBX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_peak, hipEventDisableTiming));
    return VBX_SUCCESS;
}

// the pitch path (defined with vbx_pitch_path_f64, further down): the argument checks and the launches that entry point shares
// with the tracked frame loop
static int check_pitch_path(vbx_ctx *ctx, const char *fn, const vbx_pitch_path_params &pr, size_t n_frames, size_t kmax, bool have_peak,
                            const int64_t *h_seg_start, size_t n_segments);
static int run_pitch_path(vbx_ctx *ctx, hipStream_t st, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                          size_t n_frames, size_t kmax, const double *local_peak, const int64_t *h_seg_start, size_t n_segments,
                          const vbx_pitch_path_params &pr, vbx_pitch *out_path, size_t path_ld, int32_t *out_index, const char *fn);

// vbx_analyze_frames_tracked_*: columns 0-1 of the records are the pitch path over the call's own kmax-entry lists
// (defer_path: the lists, counts and peaks only -- vbx_analyze_host runs ONE path over the whole recording behind its last chunk)
struct track_req_t { size_t kmax; vbx_pitch_path_params path; vbx_pitch_track_outputs out; bool defer_path; };
// vbx_analyze_frames_ex_*: find_formants on the frames' resampled view (rp non-null) at formant_rate, and the RMS column
struct ex_req_t { const resample_plan_t *rp; double formant_rate; bool rms; };

// own: the caller's frames, as f64, 16-bit PCM or float32 samples.  PCM and float32 are read directly where EVERY kernel that goes over
// the samples has a form for them (full 1200-sample frames through the fused spectral kernel with nothing beside it but Burg, which
// has one at every length); every other shape takes one widening pass into a context-owned f64 copy of the view and the f64 path.
static int analyze_frames_impl(vbx_ctx *ctx, const char *fn, frames_t own, size_t n_frames, size_t frame_len,
                               size_t stride, const vbx_analysis_params *h_p, const int64_t *h_seg_start, size_t n_segments,
                               double *out_records, size_t record_ld, int32_t *status3, const track_req_t *tk = nullptr,
                               const ex_req_t *ex = nullptr) {
    int rc = check_frames(ctx, fn, own.p, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc == 1 && tk) { ctx->path_redone = nullptr; ctx->path_last = true; }      // an empty batch: an empty path
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, h_p && out_records, "null argument");
    const size_t c_rms = vbx_record_doubles(h_p), rec = c_rms + ((ex && ex->rms) ? 1 : 0);     // RMS: the record's last column
    VBX_REQUIRE(ctx, record_ld >= rec && record_ld % 2 == 0, "record_ld must be even and >= vbx_record_doubles(params)");
    VBX_REQUIRE(ctx, ((uintptr_t)out_records & 15) == 0, "records must be 16-byte aligned");
    VBX_REQUIRE(ctx, !h_p->formant_order || (h_p->n_est >= 1 && h_p->n_est <= VBX_FORMANT_SLOTS), "n_est must be in [1, 6]");
    if (tk || ex) {
        // The tracked form writes its peaks before the parts below look at their own arguments: what they would reject is asked first,
        // through the predicates those parts use themselves.  (The unfused MFCC kernels choose their form from the geometry: the tracked
        // form queues them FIRST on the side stream, below, so that their rejection also precedes every write.)
        if (const char *e = pitch_shape_error(frame_len, tk ? tk->kmax : 1)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": " + e);
        VBX_REQUIRE(ctx, !h_p->formant_order || burg_order_ok((ex && ex->rp) ? ex->rp->m : frame_len, h_p->formant_order), "frame_len must be >= 2, order in [1, 62]");
        VBX_REQUIRE(ctx, !h_p->lpc_order || lpc_order_ok(frame_len, h_p->lpc_order), "bad order");
    }
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    rc = ensure_side_stream(ctx);
    if (rc != VBX_SUCCESS) return rc;
    // One spectral pass for pitch + LPC + MFCC when the shape has a fused kernel (k_spectral.hip); otherwise the LPC
    // and MFCC kernels run on the side stream and the pitch kernel alone on the main one.
    std::vector<int32_t> hb; bool bad_bins = false; const int32_t *d_bins = nullptr;
    const double *dct = nullptr, *slopes = nullptr;
    int nb = 0;
    if (h_p->mfcc_coeffs) {
        VBX_REQUIRE(ctx, h_p->mfcc_coeffs <= 64, "mfcc_coeffs must be in [0, 64]");
        rc = get_bins_dev(ctx, frame_len, h_p->mfcc_coeffs, h_p->mfcc_lo_hz, h_p->mfcc_hi_hz, h_p->sample_rate, &d_bins, hb, bad_bins);
        if (rc != VBX_SUCCESS) return rc;
        nb = hb.back() - hb.front();
    }
    // (MFCC joins the fused kernel when the frame's length divides the transform's: n = 512, 600, 800, 1024, 1200, 2048, 4096 -- and, since
    // round 5, at every other length by interpolated bins, below; LPC only at the order the kernel's register Levinson is built for -- what
    // cannot join runs from its own kernel on the side stream)
    const bool fused = !ctx->pitch_force_mfma && spectral_supported((int)frame_len, 0, 0, 0, 0);
    const bool fused_lpc = fused && h_p->lpc_order == SPECTRAL_LPC_ORDER;
    // the transform: the one its length asks for, or -- if MFCC can join only there -- the one whose length the frame divides
    int plan = fused ? spectral_plan((int)frame_len) : SPECTRAL_PLAN_NONE;
    if (fused && !bad_bins && h_p->mfcc_coeffs) {
        const int pm = spectral_plan_mfcc((int)frame_len);
        if (spectral_supported_plan(pm, (int)frame_len, 0, nb, hb.front(), (int)h_p->mfcc_coeffs)) plan = pm;
    }
    bool fused_mfcc = fused && !bad_bins && h_p->mfcc_coeffs &&
                      spectral_supported_plan(plan, (int)frame_len, 0, nb, hb.front(), (int)h_p->mfcc_coeffs);
    // ... and at the other lengths by interpolating the frame's DFT bins from the transform's (mfcc_interp_t)
    bool interp_mfcc = false;
    mfcc_interp_t ip{};
    if (fused && !fused_mfcc && !bad_bins && h_p->mfcc_coeffs && ctx->mfcc_interp != 0 && plan != SPECTRAL_PLAN_NONE && nb >= 1 && nb <= 4096 && hb.front() >= 0) {
        VBX_HIP(ctx, ctx->tables.interp(plan, (int)frame_len, hb.front(), nb, &ip, &interp_mfcc));
        fused_mfcc = interp_mfcc;
    }
    // x: what the kernels read -- the caller's own samples, or their widened copy (the RMS and peak kernels read `own` either way)
    frames_t x = own;
    const bool native = fused && frame_len == (size_t)SPECTRAL_N && (!h_p->lpc_order || fused_lpc) && (!h_p->mfcc_coeffs || fused_mfcc) &&
                        !(ex && ex->rp && !ex->rp->direct);                // (the dense fallback resamples f64 frames)
    if (own.kind != SAMPLE_F64 && !native) {
        const size_t ns = (n_frames - 1) * stride + frame_len;
        void *w = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_F32_IN, ns * sizeof(double), &w);
        if (rc != VBX_SUCCESS) return rc;
        if (own.kind == SAMPLE_PCM16) { Prof p(ctx, "pcm16"); launch_pcm16(ctx->stream, own.pcm16(), ns, 32767.0, (double *)w); }
        else { Prof p(ctx, "f32_to_f64"); launch_f32_to_f64(ctx->stream, own.f32in(), ns, (double *)w); }
        x = (const double *)w;
    }
    const double *hann = nullptr;
    VBX_HIP(ctx, ctx->tables.window(VBX_WINDOW_HANNING, frame_len, &hann));        // Windower::hanning frames (examples/pitch_detection.rs:23)
    // record columns
    const size_t c_form = 2, c_mfcc = c_form + (h_p->formant_order ? 2 * h_p->n_est : 0),
                 c_lpc = c_mfcc + h_p->mfcc_coeffs;
    int32_t *st_pitch = nullptr, *st_form = nullptr, *st_mfcc = nullptr;
    if (status3) { st_pitch = status3; st_form = status3 + n_frames; st_mfcc = status3 + 2 * n_frames; }
    // the tracked form: the lists, counts and peaks the path reads -- the caller's arrays, or context-owned ones
    vbx_pitch *tk_cand = nullptr; int32_t *tk_count = nullptr; double *tk_peak = nullptr;
    if (tk) {
        tk_cand = tk->out.cand; tk_count = tk->out.count;
        const bool need_peak = tk->path.silence_threshold != 0.0 || tk->out.peak != nullptr;
        tk_peak = need_peak ? tk->out.peak : nullptr;
        const size_t b_cand = tk_cand ? 0 : n_frames * tk->kmax * sizeof(vbx_pitch), b_peak = (need_peak && !tk_peak) ? n_frames * sizeof(double) : 0,
                     b_count = tk_count ? 0 : n_frames * sizeof(int32_t), b_st = st_pitch ? 0 : n_frames * sizeof(int32_t);
        if (b_cand + b_peak + b_count + b_st) {
            void *w = nullptr;
            rc = ws_get(ctx, vbx_ctx::WS_TRACK, b_cand + b_peak + b_count + b_st, &w);
            if (rc != VBX_SUCCESS) return rc;
            char *q = static_cast<char *>(w);
            if (b_cand) { tk_cand = reinterpret_cast<vbx_pitch *>(q); q += b_cand; }
            if (b_peak) { tk_peak = reinterpret_cast<double *>(q); q += b_peak; }
            if (b_count) { tk_count = reinterpret_cast<int32_t *>(q); q += b_count; }
            if (b_st) st_pitch = reinterpret_cast<int32_t *>(q);              // (the path must see the frames the pitch kernel gave up on)
        }
    }
    // fork: the formant chain (Burg -> roots -> the latency-bound tracker scan) and the MFCC run on the side stream,
    // beside the FP64-bound pitch kernel
    VBX_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    // (frames longer than VBX_MAX_FRAME_LEN: everything in order on the context's stream -- the long-frame kernels share one scratch)
    hipStream_t side = frame_len > VBX_MAX_FRAME_LEN ? ctx->stream : ctx->side;
    VBX_HIP(ctx, hipStreamWaitEvent(side, ctx->ev_fork, 0));
    const bool mfcc_beside = h_p->mfcc_coeffs && !fused_mfcc;              // MFCC from its own kernel on the side stream
    if (tk && mfcc_beside) {                                               // (tracked: first, see above; its columns are nobody else's)
        rc = run_mfcc(ctx, side, x.f64(), n_frames, frame_len, stride, hann, h_p->mfcc_coeffs, h_p->mfcc_lo_hz, h_p->mfcc_hi_hz,
                      h_p->sample_rate, out_records + c_mfcc, record_ld, st_mfcc);
        if (rc != VBX_SUCCESS) return rc;
    }
    // RMS::rms of the rectangular frame (examples/formant_extraction/src/main.rs:84), from the caller's own samples -- a PCM
    // recording is never widened for it.  A tracked call that needs the frame peaks takes both from one read, here; otherwise
    // the RMS kernel is the side stream's LAST launch, behind everything that may still reject the call.
    const bool want_rms = ex && ex->rms;
    if (tk_peak && want_rms) {
        { Prof p(ctx, "frame_rms_peak", side);
          launch_frame_rms(side, own, (long)n_frames, (int)frame_len, (long)stride, out_records + c_rms, (long)record_ld, tk_peak); }
        VBX_HIP(ctx, hipEventRecord(ctx->ev_peak, side));
    } else if (tk_peak) {
        // max |x| per frame, first on the side stream: HBM-bound, beside the FP64-bound kernel; the path waits for ev_peak
        static const char *const k_peak_names[3] = {"frame_peak", "frame_peak_pcm16", "frame_peak_f32in"};      // by sample_kind_t
        { Prof p(ctx, k_peak_names[own.kind], side); launch_frame_peak(side, own, (long)n_frames, (long)frame_len, (long)stride, tk_peak); }
        VBX_HIP(ctx, hipEventRecord(ctx->ev_peak, side));
    }
    if (h_p->formant_order) {
        vbx_resonance est[VBX_FORMANT_SLOTS];
        for (size_t e = 0; e < h_p->n_est; e++) est[e] = h_p->est_init[e];
        rc = run_find_formants(ctx, side, x, n_frames, frame_len, stride, ex ? ex->formant_rate : h_p->sample_rate, h_p->formant_order,
                               h_seg_start, n_segments, est, h_p->n_est, (vbx_resonance *)(out_records + c_form), record_ld,
                               nullptr, nullptr, nullptr, st_form, ex ? ex->rp : nullptr);
        if (rc != VBX_SUCCESS) return rc;
    } else {
        ctx->last_track.res = nullptr;                        // no tracks in these records: nothing for vbx_track_stitch_f64 to continue
        ctx->last_track.n_est = 0;                            // ... and no row for a communicator to send on
        if (st_form) VBX_HIP(ctx, hipMemsetAsync(st_form, 0, n_frames * sizeof(int32_t), side));
    }
    // (what runs beside the spectral kernel reads f64: `native` is false wherever one of these runs)
    if (h_p->lpc_order && !fused_lpc) {
        rc = run_autocorr_lpc(ctx, side, x.f64(), n_frames, frame_len, stride, hann, h_p->lpc_order, 0, nullptr,
                              out_records + c_lpc, record_ld);
        if (rc != VBX_SUCCESS) return rc;
    }
    if (mfcc_beside && !tk) {
        rc = run_mfcc(ctx, side, x.f64(), n_frames, frame_len, stride, hann, h_p->mfcc_coeffs, h_p->mfcc_lo_hz, h_p->mfcc_hi_hz,
                      h_p->sample_rate, out_records + c_mfcc, record_ld, st_mfcc);
        if (rc != VBX_SUCCESS) return rc;
    }
    if (!h_p->mfcc_coeffs && st_mfcc) VBX_HIP(ctx, hipMemsetAsync(st_mfcc, 0, n_frames * sizeof(int32_t), side));
    if (want_rms && !tk_peak) {
        Prof p(ctx, "frame_rms", side);
        launch_frame_rms(side, own, (long)n_frames, (int)frame_len, (long)stride, out_records + c_rms, (long)record_ld, nullptr);
    }
    VBX_HIP(ctx, hipEventRecord(ctx->ev_join, side));
    if (fused) {
        const double *lagw = nullptr, *tab = nullptr; bool lag_rcp = false;
        VBX_HIP(ctx, ctx->tables.window(VBX_WINDOW_HANNING_LAG, frame_len, &lagw, &lag_rcp));
        VBX_HIP(ctx, ctx->tables.spectral(plan, &tab));
        if (fused_mfcc) {
            VBX_HIP(ctx, ctx->tables.dct(h_p->mfcc_coeffs, &dct));
            VBX_HIP(ctx, ctx->tables.slopes(frame_len, h_p->mfcc_coeffs, h_p->mfcc_lo_hz, h_p->mfcc_hi_hz, h_p->sample_rate, hb, &slopes));
        }
        if (ctx->prof && !ctx->pitch_work) {
            const size_t wb = PITCH_WORK_WORDS * sizeof(unsigned long long);
            VBX_HIP(ctx, hipMalloc((void **)&ctx->pitch_work, wb));
            VBX_HIP(ctx, hipMemsetAsync(ctx->pitch_work, 0, wb, ctx->stream));
        }
        spectral_launch_t L{};
        L.plan = plan; L.n = (int)frame_len;
        L.x = x; L.F = (long)n_frames; L.stride = (long)stride; L.window = hann; L.lag_window = lagw; L.tab = tab;
        L.lag_rcp = lag_rcp;
        L.sample_rate = h_p->sample_rate; L.threshold = h_p->pitch_threshold; L.fmin = h_p->pitch_fmin; L.fmax = h_p->pitch_fmax;
        L.kmax = 1;
        L.whole_curve = ctx->pitch_whole_curve;
        L.out_cand = (pitch_t *)out_records; L.cand_ld = (long)record_ld; L.out_count = nullptr; L.pitch_status = st_pitch;
        if (tk) { L.kmax = (int)tk->kmax; L.out_cand = (pitch_t *)tk_cand; L.cand_ld = 2 * (long)tk->kmax; L.out_count = tk_count; }
        L.work = ctx->prof ? ctx->pitch_work : nullptr;
        if (fused_lpc) { L.out_lpc = out_records + c_lpc; L.lpc_ld = (long)record_ld; }
        if (fused_mfcc) {
            L.out_mfcc = out_records + c_mfcc; L.mfcc_ld = (long)record_ld; L.mfcc_status = st_mfcc;
            L.bins = d_bins; L.slopes = slopes; L.dct = dct; L.num_coeffs = (int)h_p->mfcc_coeffs; L.nb = nb;
            L.interp = interp_mfcc; L.ip = ip;
        }
        rc = launch_spectral(ctx, ctx->stream, L, "analyze");
    } else if (tk) {
        rc = run_pitch(ctx, ctx->stream, x.f64(), n_frames, frame_len, stride, hann, h_p->sample_rate, h_p->pitch_threshold,
                       h_p->pitch_fmin, h_p->pitch_fmax, tk->kmax, tk_cand, 2 * tk->kmax, tk_count, st_pitch);
    } else {
        rc = run_pitch(ctx, ctx->stream, x.f64(), n_frames, frame_len, stride, hann, h_p->sample_rate, h_p->pitch_threshold,
                       h_p->pitch_fmin, h_p->pitch_fmax, 1, (vbx_pitch *)out_records, record_ld, nullptr, st_pitch);
    }
    if (rc != VBX_SUCCESS) return rc;
    if (tk && !tk->defer_path) {
        // the path over those lists, on the context's stream behind the kernel that wrote them: its rows are columns 0-1 of the records
        if (tk_peak) VBX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_peak, 0));
        rc = run_pitch_path(ctx, ctx->stream, tk_cand, tk_count, st_pitch, n_frames, tk->kmax, tk_peak, h_seg_start, n_segments, tk->path,
                            (vbx_pitch *)out_records, record_ld, tk->out.index, fn);
        if (rc != VBX_SUCCESS) return rc;
    }
    VBX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));       // join: the records are complete on ctx's stream
    return VBX_SUCCESS;
}

int vbx_analyze_frames_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                           const vbx_analysis_params *h_p, const int64_t *h_seg_start, size_t n_segments,
                           double *out_records, size_t record_ld, int32_t *status3) {
    return analyze_frames_impl(ctx, __func__, x, n_frames, frame_len, stride, h_p, h_seg_start, n_segments, out_records, record_ld, status3);
}

int vbx_analyze_frames_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                             const vbx_analysis_params *h_p, const int64_t *h_seg_start, size_t n_segments,
                             double *out_records, size_t record_ld, int32_t *status3) {
    if (n_frames != 0 && ctx && !pcm) return fail(ctx, VBX_E_INVALID, "vbx_analyze_frames_pcm16: null frame pointer");
    return analyze_frames_impl(ctx, __func__, pcm, n_frames, frame_len, stride, h_p, h_seg_start, n_segments, out_records, record_ld, status3);
}

// find_formants' resample_ratio (src/lib.rs:40-64) as a plan: the checks every entry point that takes a ratio shares, the
// resampled length, the context's (li, frac) table and whether the resampled loaders take the shape.  *have = false: no
// resampling (ratio 0 or 1.0: src/lib.rs:57 compares with 1.0).
static int make_resample_plan(vbx_ctx *ctx, const char *fn, double ratio, size_t frame_len, size_t order, resample_plan_t *rp, bool *have) {
    *have = false;
    if (!(ratio >= 0.0) || !std::isfinite(ratio)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": resample_ratio must be finite and >= 0");
    if (ratio == 0.0 || ratio == 1.0) return VBX_SUCCESS;
    if (ratio > 64.0) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": resample_ratio must be in (0, 64]");
    if (order == 0) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": a resample_ratio needs a formant order");
    const size_t m = vbx_resampled_len(frame_len, ratio);
    if (m > 0x3fffffff) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad resampled length");
    if (!burg_order_ok(m, order)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": the resampled frame must have >= 2 samples, order in [1, 62]");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    rp->n_src = frame_len; rp->m = m; rp->rs.n_src = (int)frame_len;
    VBX_HIP(ctx, ctx->tables.resample(frame_len, ratio, m, &rp->rs.li, &rp->rs.frac));
    rp->direct = frame_len <= VBX_MAX_FRAME_LEN && burg_resampled_supported((int)frame_len, (int)m, (int)order);
    *have = true;
    return VBX_SUCCESS;
}

// The frame loop of examples/formant_extraction/src/main.rs:72-88: find_formants at a resample_ratio, the frame's RMS as the
// record's last column.  Everything is checked before anything is launched; an h_ext that asks for nothing is the plain /
// tracked call itself.
static int analyze_ex(vbx_ctx *ctx, const char *fn, frames_t x, size_t n_frames, size_t frame_len, size_t stride,
                      const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                      const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld, int32_t *status3,
                      const vbx_pitch_track_outputs *h_out, bool defer_path = false /* vbx_analyze_host's chunks: track_req_t */) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null context");
    if (!h_p) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": null argument");
    resample_plan_t rp{}; ex_req_t ex{nullptr, h_p->sample_rate, false};
    const ex_req_t *exp = nullptr;
    if (h_ext) {
        const double ratio = h_ext->formant_resample_ratio, rate = h_ext->formant_sample_rate;
        if (!(rate >= 0.0) || !std::isfinite(rate)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": formant_sample_rate must be finite and >= 0");
        bool have = false;
        if (n_frames != 0 && frame_len >= 1 && frame_len <= VBX_MAX_LONG_FRAME_LEN) {      // (any other frame_len is rejected below)
            int rc = make_resample_plan(ctx, fn, ratio, frame_len, h_p->formant_order, &rp, &have);
            if (rc != VBX_SUCCESS) return rc;
        } else if (!(ratio >= 0.0) || !std::isfinite(ratio) || ratio > 64.0) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": resample_ratio must be in [0, 64]");
        ex.rp = have ? &rp : nullptr;
        ex.formant_rate = rate != 0.0 ? rate : (have ? h_p->sample_rate * ratio : h_p->sample_rate);
        ex.rms = h_ext->rms != 0;
        if (have || ex.rms || rate != 0.0) exp = &ex;
    }
    if (!h_track) return analyze_frames_impl(ctx, fn, x, n_frames, frame_len, stride, h_p, h_seg_start, n_segments, out_records, record_ld,
                                             status3, nullptr, exp);
    track_req_t tk{};
    tk.kmax = h_track->kmax; tk.path = h_track->path;
    if (h_out) tk.out = *h_out;
    tk.defer_path = defer_path;
    if (tk.path.time_step == 0.0) tk.path.time_step = (double)stride / h_p->sample_rate;      // the batch's own hop
    int rc = check_pitch_path(ctx, fn, tk.path, n_frames, tk.kmax, true, h_seg_start, n_segments);
    if (rc != VBX_SUCCESS) return rc;
    return analyze_frames_impl(ctx, fn, x, n_frames, frame_len, stride, h_p, h_seg_start, n_segments, out_records, record_ld, status3, &tk, exp);
}

// The frame loop with the TRACKED contour in columns 0-1 (the fused kernel at the caller's kmax into list buffers, the frame peaks
// beside it, the pitch path behind it): analyze_ex with no extension, behind the two checks that come first here.
int vbx_analyze_frames_tracked_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                                   const vbx_analysis_params *h_p, const vbx_pitch_track_params *h_track,
                                   const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld,
                                   int32_t *status3, const vbx_pitch_track_outputs *h_outputs) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, std::string(__func__) + ": null context");
    if (!h_track) return fail(ctx, VBX_E_INVALID, std::string(__func__) + ": null track parameters");
    return analyze_ex(ctx, __func__, x, n_frames, frame_len, stride, h_p, nullptr, h_track, h_seg_start, n_segments, out_records,
                      record_ld, status3, h_outputs);
}

int vbx_analyze_frames_tracked_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                                     const vbx_analysis_params *h_p, const vbx_pitch_track_params *h_track,
                                     const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld,
                                     int32_t *status3, const vbx_pitch_track_outputs *h_outputs) {
    if (n_frames != 0 && ctx && !pcm) return fail(ctx, VBX_E_INVALID, "vbx_analyze_frames_tracked_pcm16: null frame pointer");
    if (!ctx) return fail(nullptr, VBX_E_INVALID, std::string(__func__) + ": null context");
    if (!h_track) return fail(ctx, VBX_E_INVALID, std::string(__func__) + ": null track parameters");
    return analyze_ex(ctx, __func__, pcm, n_frames, frame_len, stride, h_p, nullptr, h_track, h_seg_start, n_segments, out_records,
                      record_ld, status3, h_outputs);
}

int vbx_analyze_frames_ex_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                              const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                              const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld,
                              int32_t *status3, const vbx_pitch_track_outputs *h_outputs) {
    return analyze_ex(ctx, __func__, x, n_frames, frame_len, stride, h_p, h_ext, h_track, h_seg_start, n_segments, out_records,
                      record_ld, status3, h_outputs);
}

int vbx_analyze_frames_ex_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                                const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                                const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld,
                                int32_t *status3, const vbx_pitch_track_outputs *h_outputs) {
    if (n_frames != 0 && ctx && !pcm) return fail(ctx, VBX_E_INVALID, "vbx_analyze_frames_ex_pcm16: null frame pointer");
    return analyze_ex(ctx, __func__, pcm, n_frames, frame_len, stride, h_p, h_ext, h_track, h_seg_start, n_segments, out_records,
                      record_ld, status3, h_outputs);
}

int vbx_analyze_frames_ex_f32in(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                                const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                                const int64_t *h_seg_start, size_t n_segments, double *out_records, size_t record_ld,
                                int32_t *status3, const vbx_pitch_track_outputs *h_outputs) {
    if (n_frames != 0 && ctx && !x) return fail(ctx, VBX_E_INVALID, "vbx_analyze_frames_ex_f32in: null frame pointer");
    return analyze_ex(ctx, __func__, x, n_frames, frame_len, stride, h_p, h_ext, h_track, h_seg_start, n_segments, out_records,
                      record_ld, status3, h_outputs);
}

// ---- host-resident recordings (header: "host-resident recordings") ---------------------------

static const char *const k_unpack_names[6] = {"", "unpack_pcm16", "unpack_pcm24", "unpack_pcm32", "unpack_f32", "unpack_f64"};
static bool sample_format_ok(int f) { return f >= VBX_SAMPLE_PCM16 && f <= VBX_SAMPLE_F64; }
static size_t sample_src_bytes(int f) { return f == VBX_SAMPLE_PCM16 ? 2 : f == VBX_SAMPLE_PCM24 ? 3 : f == VBX_SAMPLE_F64 ? 8 : 4; }
// the typed plane the frame loop reads for a VBX_SAMPLE_* format (what launch_unpack writes): PCM24 / PCM32 / F64 unpack to f64
static sample_kind_t sample_plane_kind(int f) { return f == VBX_SAMPLE_PCM16 ? SAMPLE_PCM16 : f == VBX_SAMPLE_F32 ? SAMPLE_F32 : SAMPLE_F64; }
static size_t sample_out_bytes(int f) { static const size_t bytes[3] = {8, 2, 4}; return bytes[sample_plane_kind(f)]; }

int vbx_unpack_samples(vbx_ctx *ctx, const void *d_src, size_t n_sample_frames, int format, int channels, int channel, void *d_out) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    VBX_REQUIRE(ctx, sample_format_ok(format), "unknown sample format");
    VBX_REQUIRE(ctx, channels >= 1 && channel >= 0 && channel < channels, "need channels >= 1 and 0 <= channel < channels");
    if (n_sample_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, d_src && d_out, "null argument");
    VBX_REQUIRE(ctx, format == VBX_SAMPLE_PCM24 || (uintptr_t)d_src % sample_src_bytes(format) == 0, "the source needs its type's alignment");
    VBX_REQUIRE(ctx, (uintptr_t)d_out % sample_out_bytes(format) == 0, "the destination needs its type's alignment");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, k_unpack_names[format]); launch_unpack(ctx->stream, format, d_src, n_sample_frames, (size_t)channels, (size_t)channel, d_out); }
    return check_launch(ctx, __func__);
}

static const char *const k_unpack_all_names[6] = {"", "unpack_all_pcm16", "unpack_all_pcm24", "unpack_all_pcm32", "unpack_all_f32", "unpack_all_f64"};
static_assert(UNPACK_MAX_SEL == VBX_HOST_MAX_CHANNELS, "the selection is a kernel argument of VBX_HOST_MAX_CHANNELS entries");

// a selection of channels: 1 <= n_sel <= min(channels, VBX_HOST_MAX_CHANNELS) distinct values in [0, channels)
static bool channel_selection_ok(const int32_t *h_channels, size_t n_sel, int channels, unpack_sel_t *sel) {
    if (!h_channels || channels < 1 || n_sel < 1 || n_sel > (size_t)channels || n_sel > (size_t)VBX_HOST_MAX_CHANNELS) return false;
    for (size_t k = 0; k < n_sel; k++) {
        if (h_channels[k] < 0 || h_channels[k] >= channels) return false;
        for (size_t j = 0; j < k; j++) if (h_channels[j] == h_channels[k]) return false;
        sel->ch[k] = h_channels[k];
    }
    return true;
}

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
    { Prof p(ctx, k_unpack_all_names[format]);
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

// the copy stream, the slots' events and the two raw slots of `bytes` each (grown on demand: both streams are drained first)
static int ensure_host_slots(vbx_ctx *ctx, size_t bytes) {
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
#define HOST_REQUIRE(cond, msg) do { if (!(cond)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": " + (msg)); } while (0)
    HOST_REQUIRE(h_fmt->reserved == 0, "reserved must be 0");
    HOST_REQUIRE(h_fmt->chunk_frames == 0 || h_fmt->chunk_frames >= (size_t)VBX_SHARD_WARM_FRAMES, "chunk_frames must be 0 or >= VBX_SHARD_WARM_FRAMES");
    HOST_REQUIRE(h_p != nullptr, "null argument");
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
    HOST_REQUIRE(h_audio != nullptr, "null audio");
    HOST_REQUIRE(frame_len <= VBX_MAX_LONG_FRAME_LEN, "frame_len must be in [1, 67108864]");
    HOST_REQUIRE(F <= 0x7fffffffull, "too many frames for one launch");
    const size_t rec = vbx_record_doubles_ex(h_p, h_ext);
    HOST_REQUIRE(record_ld >= rec && record_ld % 2 == 0, "record_ld must be even and >= vbx_record_doubles(params)");
    for (size_t k = 0; k < n_sel; k++) {
        HOST_REQUIRE(chan[k].rec != nullptr, "null argument");
        HOST_REQUIRE(((uintptr_t)chan[k].rec & 15) == 0, "records must be 16-byte aligned");
        for (size_t j = 0; j < k; j++) {                  // [F, record_ld] each
            const uintptr_t a = (uintptr_t)chan[j].rec, b = (uintptr_t)chan[k].rec, len = F * record_ld * sizeof(double);
            HOST_REQUIRE(a + len <= b || b + len <= a, "the channels' records overlap");
        }
    }
    HOST_REQUIRE(!h_p->formant_order || (h_p->n_est >= 1 && h_p->n_est <= VBX_FORMANT_SLOTS), "n_est must be in [1, 6]");
    const bool segmented = h_seg_start != nullptr && n_segments > 0;
    if (segmented) {
        HOST_REQUIRE(h_seg_start[0] == 0, "seg_start[0] must be 0");
        for (size_t i = 1; i < n_segments; i++)
            HOST_REQUIRE(h_seg_start[i] >= h_seg_start[i - 1] && (size_t)h_seg_start[i] <= F, "seg_start must ascend within [0, n_frames]");
    }
#undef HOST_REQUIRE
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
    // mono PCM16 / F32 / F64: the slot holds the frame loop's type already
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
            if (sel) { Prof p(ctx, k_unpack_all_names[fmt]);
                       launch_unpack_all(ctx->stream, fmt, ctx->host_raw[slot], s1 - s0, C, *sel, n_sel, typed, plane_bytes / sample_out_bytes(fmt)); }
            else { Prof p(ctx, k_unpack_names[fmt]); launch_unpack(ctx->stream, fmt, ctx->host_raw[slot], s1 - s0, C, ch, typed); }
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

// ---- the online pitch path (header: "the pitch path while the lists arrive") --------------------

// One contour that grows while its lists arrive.  The stream owns the carried state and the ring of max_pending frames (one
// allocation, made at open); a push is one launch of pp_online_kernel on the context's stream and touches nothing of the context's.
struct vbx_path_stream {
    vbx_ctx *ctx = nullptr;
    size_t kmax = 0, max_pending = 0;
    int G = 4;
    vbx_pitch_path_params pr{};
    double peak_ref = 0.0;
    void *mem = nullptr;                                  // pp_online_state_t, then the ring: row [cap][G], psi [cap][G], idx [cap][G]
    pp_online_t O{};
};

static int path_stream_open(vbx_ctx *ctx, const char *fn, size_t kmax, const vbx_pitch_path_params &pr, double peak_ref, size_t max_pending,
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
static int path_stream_launch(vbx_path_stream *ps, const char *fn, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
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

static int path_stream_reset(vbx_path_stream *ps) {
    VBX_HIP(ps->ctx, hipSetDevice(ps->ctx->device));
    VBX_HIP(ps->ctx, hipMemsetAsync(ps->mem, 0, sizeof(pp_online_state_t), ps->ctx->stream));
    return VBX_SUCCESS;
}

static void path_stream_free(vbx_path_stream *ps) {
    hipSetDevice(ps->ctx->device);
    hipStreamSynchronize(ps->ctx->stream);                // queued pushes may still use the ring
    if (ps->mem) hipFree(ps->mem);
    delete ps;
}

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

// ---- live sessions (header: "live sessions") --------------------------------------------------

// blocks of up to this many bytes are staged through the session's pinned buffers and uploaded on the context's own stream: a host
// copy of about 10 us at this size, which is what the copy stream's event round trip was measured to add to a push (DESIGN.md
// section 5g); larger blocks take the copy stream, where their upload runs beside the previous block's analysis
#define VBX_SESSION_STAGE_BYTES 131072
static const char *const k_ingest_names[6] = {"", "session_ingest_pcm16", "session_ingest_pcm24", "session_ingest_pcm32", "session_ingest_f32",
                                              "session_ingest_f64"};

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
    delete s;
}

// the frame loop on frames [0, n) of the session's current carry buffer into the chunk-local buffers
static int session_analyze(vbx_session *s, const char *fn, size_t n, bool want_peak) {
    vbx_pitch_track_outputs to{};
    to.cand = s->c_cand; to.count = s->c_count; to.peak = want_peak ? s->c_peak : nullptr;
    return analyze_ex(s->ctx, fn, frames_t(s->carry[s->cur], sample_plane_kind(s->fmt)), n, s->frame_len, s->stride, &s->p,
                      s->have_ext ? &s->ext : nullptr, s->have_track ? &s->track : nullptr, nullptr, 0, s->c_rec, s->ld_c, s->c_st,
                      s->have_track ? &to : nullptr, true);
}

int vbx_session_open(vbx_ctx *ctx, const vbx_host_audio *h_fmt, size_t frame_len, size_t stride, const vbx_analysis_params *h_p,
                     const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, size_t max_block, vbx_session **out) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, "vbx_session_open: null context");
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    *out = nullptr;
    VBX_REQUIRE(ctx, h_fmt != nullptr && h_p != nullptr, "null argument");
    VBX_REQUIRE(ctx, sample_format_ok(h_fmt->format), "unknown sample format");
    VBX_REQUIRE(ctx, h_fmt->channels >= 1 && h_fmt->channel >= 0 && h_fmt->channel < h_fmt->channels, "need channels >= 1 and 0 <= channel < channels");
    VBX_REQUIRE(ctx, h_fmt->reserved == 0 && h_fmt->chunk_frames == 0, "reserved and chunk_frames must be 0");
    VBX_REQUIRE(ctx, max_block >= 1, "max_block_sample_frames must be >= 1");
    VBX_REQUIRE(ctx, frame_len >= 1 && frame_len <= VBX_MAX_LONG_FRAME_LEN, "frame_len must be in [1, 67108864]");
    VBX_REQUIRE(ctx, stride >= 1, "stride must be >= 1");
    VBX_REQUIRE(ctx, max_block <= ((size_t)1 << 40) && stride <= ((size_t)1 << 40), "max_block_sample_frames or stride too large");
    VBX_REQUIRE(ctx, !h_p->formant_order || (h_p->n_est >= 1 && h_p->n_est <= VBX_FORMANT_SLOTS), "n_est must be in [1, 6]");
    const size_t nmax = session_max_frames(stride, max_block);
    VBX_REQUIRE(ctx, nmax <= 0x7fffffffull, "too many frames for one launch");
    if (h_track) {
        vbx_pitch_path_params path = h_track->path;
        if (path.time_step == 0.0) path.time_step = (double)stride / h_p->sample_rate;
        int rc = check_pitch_path(ctx, __func__, path, nmax, h_track->kmax, true, nullptr, 0);
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
    const size_t cap = session_carry_samples(frame_len, stride, max_block), ob = sample_out_bytes(s->fmt);
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
    SESSION_HIP(hipMalloc((void **)&s->c_rec, nmax * s->ld_c * sizeof(double)));
    SESSION_HIP(hipMalloc((void **)&s->c_st, 3 * nmax * sizeof(int32_t)));
    if (h_track) {
        SESSION_HIP(hipMalloc((void **)&s->c_cand, nmax * kmax * sizeof(vbx_pitch)));
        SESSION_HIP(hipMalloc((void **)&s->c_count, nmax * sizeof(int32_t)));
        SESSION_HIP(hipMalloc((void **)&s->c_peak, nmax * sizeof(double)));
    }
    SESSION_HIP(hipMalloc((void **)&s->state, 2 * VBX_FORMANT_SLOTS * sizeof(double)));
    SESSION_HIP(hipMemsetAsync(s->state, 0, 2 * VBX_FORMANT_SLOTS * sizeof(double), ctx->stream));
#undef SESSION_HIP
    // the largest shape a push can ask for, on the zeroed carry: the context's workspaces and tables are as large as they will ever
    // have to be, and what only the frame loop's parts know is rejected here
    rc = session_analyze(s, __func__, nmax, true);
    if (rc == VBX_SUCCESS) rc = check_launch(ctx, __func__);
    ctx->last_track.res = nullptr;                        // the chunk-local rows are no track of the caller's
    ctx->last_track.n_est = 0;
    if (rc != VBX_SUCCESS) { const std::string why = ctx->last_error; hipStreamSynchronize(ctx->stream); vbx_sync(ctx); session_free(s); return fail(ctx, rc, why); }
    *out = s;
    return VBX_SUCCESS;
}

static int session_push_impl(vbx_session *s, const char *fn, const void *block, bool on_device, size_t n, double *out_records,
                             size_t record_ld, int32_t *status3, size_t status_ld, const vbx_pitch_track_outputs *h_out, size_t *h_n) {
    if (!s) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null session");
    vbx_ctx *ctx = s->ctx;
#define PUSH_REQUIRE(cond, msg) do { if (!(cond)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": " + (msg)); } while (0)
    if (h_n) *h_n = 0;
    if (n == 0) return VBX_SUCCESS;
    PUSH_REQUIRE(block != nullptr, "null block");
    PUSH_REQUIRE(n <= s->max_block, "the block is larger than the session's max_block_sample_frames");
    PUSH_REQUIRE(!on_device || s->fmt == VBX_SAMPLE_PCM24 || (uintptr_t)block % sample_src_bytes(s->fmt) == 0, "the block needs its type's alignment");
    vbx_session_plan_t pl{};
    if (vbx_session_plan(s->consumed, s->utt_frame, n, s->frame_len, s->stride, &pl) != VBX_SUCCESS)
        return fail(ctx, VBX_E_INVALID, std::string(fn) + ": bad session plan");
    const size_t nf = pl.hi - pl.lo;
    bool want_peak = false;
    if (nf) {
        PUSH_REQUIRE(out_records != nullptr, "null argument");
        PUSH_REQUIRE(((uintptr_t)out_records & 15) == 0, "records must be 16-byte aligned");
        PUSH_REQUIRE(record_ld >= s->rec && record_ld % 2 == 0, "record_ld must be even and >= vbx_record_doubles(params)");
        PUSH_REQUIRE(status3 == nullptr || status_ld >= nf, "status_ld must be >= the frames the push delivers");
        if (s->have_track) {
            PUSH_REQUIRE(h_out != nullptr && h_out->cand != nullptr && h_out->count != nullptr, "the tracked form needs h_outputs->cand and ->count");
            PUSH_REQUIRE(s->track.path.silence_threshold == 0.0 || h_out->peak != nullptr, "a silence_threshold needs h_outputs->peak");
            PUSH_REQUIRE(h_out->index == nullptr, "h_outputs->index must be NULL: the caller runs the path (vbx_pitch_path_f64)");
            want_peak = h_out->peak != nullptr;
        }
    }
#undef PUSH_REQUIRE
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const size_t sf_bytes = s->channels * sample_src_bytes(s->fmt);
    const void *raw = block;
    int slot = -1;
    bool wait_ready = false;
    if (!on_device) {                                     // the block into raw slot `slot`
        slot = (int)(s->uploads & 1);
        const size_t bytes = n * sf_bytes;
        if (bytes <= s->stage_bytes) {
            // through pinned staging, on the context's stream: behind the slot's last reader by stream order; the caller's block has
            // been read when the host copy returns (the staging buffer's previous upload, two pushes ago, has long left it)
            VBX_HIP(ctx, hipEventSynchronize(s->staged[slot]));
            std::memcpy(s->stage[slot], block, bytes);
            VBX_HIP(ctx, hipMemcpyAsync(s->raw[slot], s->stage[slot], bytes, hipMemcpyHostToDevice, ctx->stream));
            VBX_HIP(ctx, hipEventRecord(s->staged[slot], ctx->stream));
        } else {                                          // on the copy stream, behind the slot's last reader
            VBX_HIP(ctx, hipStreamWaitEvent(ctx->copy, s->freed[slot], 0));
            VBX_HIP(ctx, hipMemcpyAsync(s->raw[slot], block, bytes, hipMemcpyHostToDevice, ctx->copy));
            VBX_HIP(ctx, hipEventRecord(s->ready[slot], ctx->copy));
            VBX_HIP(ctx, hipStreamWaitEvent(ctx->stream, s->ready[slot], 0));
            wait_ready = true;
        }
        raw = s->raw[slot];
        s->uploads++;
    }
    // the other carry buffer: from sample frame nb on -- what this push's analysis reads first, or, when it completes no frame, what
    // a later one may.  (stride > frame_len: nb may lie beyond the carried samples, inside the block; the gap's samples are dropped)
    const size_t c = s->consumed, nb = nf ? pl.read_from : pl.keep_from;
    const size_t from_old = nb < c ? nb : c, skip = nb > c ? nb - c : 0;
    { Prof p(ctx, k_ingest_names[s->fmt]);
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

int vbx_session_reset(vbx_session *s) {
    if (!s) return fail(nullptr, VBX_E_INVALID, "vbx_session_reset: null session");
    // (nothing is queued: the next ingest keeps nothing of the carry, and a first push of an utterance stitches from no state)
    s->consumed = 0; s->utt_frame = 0; s->frames = 0; s->base = 0; s->keep_from = 0;
    if (s->path) {                                        // the path's state goes, and the binding with it
        s->bound = false;
        return path_stream_reset(s->path);
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
    { Prof p(ctx, k_ingest_names[format]);
      launch_session_ingest(ctx->stream, format, d_old, drop, keep, d_raw, n_new, (size_t)channels, (size_t)channel, d_out); }
    return check_launch(ctx, __func__);
}

int vbx_find_formants_resampled_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                                    double sample_rate, double resample_ratio, size_t n_coeffs,
                                    const int64_t *h_seg_start, size_t n_segments, const vbx_resonance *h_est_init, size_t n_est,
                                    vbx_resonance *out_formants, vbx_resonance *out_res, int32_t *out_res_count,
                                    double *out_coeffs, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, n_coeffs >= 1, "frame_len must be >= 2, order in [1, 62]");
    resample_plan_t rp{}; bool have = false;
    rc = make_resample_plan(ctx, __func__, resample_ratio, frame_len, n_coeffs, &rp, &have);
    if (rc != VBX_SUCCESS) return rc;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    return run_find_formants(ctx, ctx->stream, x, n_frames, frame_len, stride, sample_rate, n_coeffs, h_seg_start, n_segments,
                             h_est_init, n_est, out_formants, 2 * n_est, out_res, out_res_count, out_coeffs, status,
                             have ? &rp : nullptr);
}

// ---- Sample = f32, the WIDE forms --------------------------------------------
// The traits are generic over the Sample type (src/periodic.rs:276-289 `T: Sample`, src/spectrum.rs:56 `T: Float`,
// :401-409).  The *_f32_wide entry points take float frames and return float results; samples are widened on load, the
// arithmetic runs in f64 and every result is rounded to f32 once -- more accurate than the reference's own f32 folds and as
// fast as the f64 kernels, but NOT the bits the crate returns at f32.  The reference-faithful forms (every fold in f32, in
// the reference's order) carry the plain *_f32 names, further down; MFCC has only the wide form (its f32 arithmetic lives
// in the un-vendored rustfft).

int vbx_autocorrelate_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                          size_t stride, const float *window, size_t n_lags, float *out) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, n_lags >= 1 && n_lags <= frame_len, "n_lags must be in [1, frame_len] (the reference panics beyond)");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    if (!fewlags_supported((int)frame_len, (int)n_lags, false) && !ctx->pitch_force_mfma &&
        spectral_plan((int)frame_len) != SPECTRAL_PLAN_NONE && (n_lags >= SPECTRAL_AC_MIN_LAGS || frame_len >= 1024)) {
        // many lags: widen (the windowed product rounded to f32 first), the f64 FFT path, one rounding to f32
        void *wi = nullptr, *wo = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_F32_IN, n_frames * frame_len * sizeof(double), &wi);
        if (rc != VBX_SUCCESS) return rc;
        rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * n_lags * sizeof(double), &wo);
        if (rc != VBX_SUCCESS) return rc;
        { Prof p(ctx, "widen_frames"); launch_widen_frames(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (double *)wi); }
        rc = vbx_autocorrelate_f64(ctx, (const double *)wi, n_frames, frame_len, frame_len, nullptr, n_lags, (double *)wo);
        if (rc != VBX_SUCCESS) return rc;
        { Prof p(ctx, "narrow"); launch_narrow(ctx->stream, (const double *)wo, (long)(n_frames * n_lags), out); }
        return check_launch(ctx, __func__);
    }
    if (fewlags_supported((int)frame_len, (int)n_lags, false)) {
        Prof p(ctx, "autocorr_fewlags_f32");
        launch_autocorr_fewlags_f32(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_lags, 0, out, nullptr);
    } else {
        Prof p(ctx, "autocorr_tiles_f32");
        launch_autocorr_tiles_f32(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_lags, out);
    }
    return check_launch(ctx, __func__);
}

int vbx_normalize_f32(vbx_ctx *ctx, float *data, size_t n_rows, size_t n) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_rows == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, data && n >= 1 && n <= 0x7fffffff && n_rows <= 0x7fffffff, "bad argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "normalize_rows_f32"); launch_normalize_rows_f32(ctx->stream, data, (long)n_rows, (int)n); }
    return check_launch(ctx, __func__);
}

int vbx_lpc_mut_f32_wide(vbx_ctx *ctx, const float *r, size_t n_frames, size_t r_stride, size_t n_coeffs, float *out_ac,
                    float *out_kc) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, r && out_ac, "null argument");
    VBX_REQUIRE(ctx, n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && r_stride >= n_coeffs + 1, "bad order / stride");
    VBX_REQUIRE(ctx, n_frames <= 0x7fffffffull, "too many rows");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "levinson_rows_f32"); launch_levinson_rows_f32(ctx->stream, r, (long)n_frames, (long)r_stride, (int)n_coeffs, out_ac, (long)n_coeffs + 1, out_kc); }
    return check_launch(ctx, __func__);
}

int vbx_autocorr_lpc_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                         size_t stride, const float *window, size_t n_coeffs, int normalize,
                         float *out_r, float *out_lpc) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out_r || out_lpc, "both outputs null");
    VBX_REQUIRE(ctx, n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && n_coeffs + 1 <= frame_len, "bad order");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const int n_lags = (int)n_coeffs + 1;
    hipStream_t st = ctx->stream;
    if (fewlags_supported((int)frame_len, n_lags, out_lpc != nullptr)) {
        Prof p(ctx, "autocorr_lpc_f32", st);
        launch_autocorr_fewlags_f32(st, x, (long)n_frames, (int)frame_len, (long)stride, window, n_lags, normalize, out_r, out_lpc, (long)n_lags);
        return check_launch(ctx, __func__);
    }
    float *r = out_r;
    if (!r) {
        void *w = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * (size_t)n_lags * sizeof(float), &w);
        if (rc != VBX_SUCCESS) return rc;
        r = (float *)w;
    }
    if (fewlags_supported((int)frame_len, n_lags, false)) {
        Prof p(ctx, "autocorr_fewlags_f32", st);
        launch_autocorr_fewlags_f32(st, x, (long)n_frames, (int)frame_len, (long)stride, window, n_lags, 0, r, nullptr);
    } else {
        Prof p(ctx, "autocorr_tiles_f32", st);
        launch_autocorr_tiles_f32(st, x, (long)n_frames, (int)frame_len, (long)stride, window, n_lags, r);
    }
    if (normalize) { Prof p(ctx, "normalize_rows_f32", st); launch_normalize_rows_f32(st, r, (long)n_frames, n_lags); }
    if (out_lpc) { Prof p(ctx, "levinson_rows_f32", st); launch_levinson_rows_f32(st, r, (long)n_frames, n_lags, (int)n_coeffs, out_lpc, (long)n_lags); }
    return check_launch(ctx, __func__);
}

int vbx_lpc_burg_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                     size_t stride, const float *window, size_t n_coeffs, float *out, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, burg_supported((int)frame_len, (int)n_coeffs), "frame_len must be in [2, 4096], order in [1, 62]");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "burg_f32"); launch_burg_f32(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_coeffs, out, status); }
    return check_launch(ctx, __func__);
}

// MFCC is bound by its transforms, not by HBM: the f32 frames are widened into a dense f64 batch (windowed product
// rounded to f32 first) and take the f64 kernels; the coefficients are rounded to f32 on the way out.
int vbx_mfcc_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                 const float *window, size_t num_coeffs, double lo_hz, double hi_hz,
                 double sample_rate, float *out, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr && num_coeffs >= 1, "bad argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    void *wi = nullptr, *wo = nullptr;
    rc = ws_get(ctx, vbx_ctx::WS_F32_IN, n_frames * frame_len * sizeof(double), &wi);
    if (rc != VBX_SUCCESS) return rc;
    rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * num_coeffs * sizeof(double), &wo);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, "widen_frames"); launch_widen_frames(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (double *)wi); }
    rc = run_mfcc(ctx, ctx->stream, (const double *)wi, n_frames, frame_len, frame_len, nullptr, num_coeffs, lo_hz, hi_hz,
                  sample_rate, (double *)wo, num_coeffs, status);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, "narrow"); launch_narrow(ctx->stream, (const double *)wo, (long)(n_frames * num_coeffs), out); }
    return check_launch(ctx, __func__);
}

// Pitched::pitch at S = T = f32 (src/periodic.rs:396-455 is generic over the Sample): the frames are widened (windowed
// product rounded to f32 first), the candidates come from the f64 path and are rounded to f32 once.
int vbx_pitch_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                  const float *window, float sample_rate, float threshold, float fmin, float fmax,
                  size_t kmax, vbx_pitch32 *out_cand, int32_t *out_count, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out_cand != nullptr, "null output");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    void *wi = nullptr, *wo = nullptr;
    rc = ws_get(ctx, vbx_ctx::WS_F32_IN, n_frames * frame_len * sizeof(double), &wi);
    if (rc != VBX_SUCCESS) return rc;
    rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * (kmax ? kmax : 1) * sizeof(vbx_pitch), &wo);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, "widen_frames"); launch_widen_frames(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (double *)wi); }
    rc = run_pitch(ctx, ctx->stream, (const double *)wi, n_frames, frame_len, frame_len, nullptr, (double)sample_rate,
                   (double)threshold, (double)fmin, (double)fmax, kmax, (vbx_pitch *)wo, 2 * kmax, out_count, status);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, "narrow"); launch_narrow(ctx->stream, (const double *)wo, (long)(n_frames * kmax * 2), (float *)out_cand); }
    return check_launch(ctx, __func__);
}


// ---- Sample = f32, reference-faithful (k_f32.hip): every fold in f32 in the reference's order ------------------------

int vbx_autocorrelate_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                          size_t stride, const float *window, size_t n_lags, float *out) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, n_lags >= 1 && n_lags <= frame_len, "n_lags must be in [1, frame_len] (the reference panics beyond)");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "autocorr_f32_exact"); launch_autocorr_f32_exact(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_lags, out); }
    return check_launch(ctx, __func__);
}

int vbx_lpc_mut_f32(vbx_ctx *ctx, const float *r, size_t n_frames, size_t r_stride, size_t n_coeffs, float *out_ac,
                    float *out_kc) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_frames == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, r && out_ac, "null argument");
    VBX_REQUIRE(ctx, n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && r_stride >= n_coeffs + 1, "bad order / stride");
    VBX_REQUIRE(ctx, n_frames <= 0x7fffffffull, "too many rows");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "levinson_f32_exact"); launch_levinson_f32_exact(ctx->stream, r, (long)n_frames, (long)r_stride, (int)n_coeffs, out_ac, (long)n_coeffs + 1, out_kc); }
    return check_launch(ctx, __func__);
}

int vbx_autocorr_lpc_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                         size_t stride, const float *window, size_t n_coeffs, int normalize,
                         float *out_r, float *out_lpc) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out_r || out_lpc, "both outputs null");
    VBX_REQUIRE(ctx, n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && n_coeffs + 1 <= frame_len, "bad order");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const int n_lags = (int)n_coeffs + 1;
    hipStream_t st = ctx->stream;
    float *r = out_r;
    if (!r) {
        void *w = nullptr;
        rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * (size_t)n_lags * sizeof(float), &w);
        if (rc != VBX_SUCCESS) return rc;
        r = (float *)w;
    }
    { Prof p(ctx, "autocorr_f32_exact", st); launch_autocorr_f32_exact(st, x, (long)n_frames, (int)frame_len, (long)stride, window, n_lags, r); }
    if (normalize) { Prof p(ctx, "normalize_rows_f32", st); launch_normalize_rows_f32(st, r, (long)n_frames, n_lags); }
    if (out_lpc) { Prof p(ctx, "levinson_f32_exact", st); launch_levinson_f32_exact(st, r, (long)n_frames, n_lags, (int)n_coeffs, out_lpc, (long)n_lags, nullptr); }
    return check_launch(ctx, __func__);
}

int vbx_lpc_burg_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                     size_t stride, const float *window, size_t n_coeffs, float *out, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr, "null output");
    VBX_REQUIRE(ctx, burg_supported((int)frame_len, (int)n_coeffs), "frame_len must be in [2, 4096], order in [1, 62]");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    // one lane per frame, b1 / b2 in a context-owned scratch: launches of at most `chunk` frames keep it under 256 MB
    long chunk = (long)((256ull << 20) / (8ull * frame_len)) & ~63L;
    if (chunk < 64) chunk = 64;
    if ((size_t)chunk > n_frames) chunk = (long)((n_frames + 63) & ~(size_t)63);
    void *w = nullptr;
    rc = ws_get(ctx, vbx_ctx::WS_F32_IN, burg_f32_exact_scratch_bytes(chunk, (int)frame_len), &w);
    if (rc != VBX_SUCCESS) return rc;
    for (long f0 = 0; f0 < (long)n_frames; f0 += chunk) {
        const long f1 = (f0 + chunk < (long)n_frames) ? f0 + chunk : (long)n_frames;
        Prof p(ctx, "burg_f32_exact");
        launch_burg_f32_exact(ctx->stream, x, f0, f1, (long)n_frames, (int)frame_len, (long)stride, window, (int)n_coeffs, out, status, (float *)w);
    }
    return check_launch(ctx, __func__);
}

int vbx_pitch_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                  const float *window, float sample_rate, float threshold, float fmin, float fmax,
                  size_t kmax, vbx_pitch32 *out_cand, int32_t *out_count, int32_t *status) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_REQUIRE(ctx, out_cand != nullptr, "null output");
    VBX_REQUIRE(ctx, kmax >= 1 && kmax <= VBX_MAX_PITCH_CANDIDATES, "kmax must be in [1, VBX_MAX_PITCH_CANDIDATES]");
    VBX_REQUIRE(ctx, frame_len >= 4, "frame_len must be >= 4");
    VBX_REQUIRE(ctx, pitch_f32_exact_lds_bytes((int)frame_len, (int)kmax) + 16 <= 160 * 1024, "frame does not fit the LDS");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    const float *lagw32 = nullptr;
    VBX_HIP(ctx, ctx->tables.lag_window_f32(frame_len, &lagw32));
    void *wo = nullptr;
    rc = ws_get(ctx, vbx_ctx::WS_F32_OUT, n_frames * kmax * sizeof(vbx_pitch), &wo);
    if (rc != VBX_SUCCESS) return rc;
    { Prof p(ctx, "pitch_f32_exact");
      launch_pitch_f32_exact(ctx->stream, x, (long)n_frames, (int)frame_len, (long)stride, window, lagw32, (double)sample_rate,
                             (double)threshold, (double)fmin, (double)fmax, (int)kmax, (pitch_t *)wo, 2 * (long)kmax, out_count, status); }
    { Prof p(ctx, "narrow"); launch_narrow(ctx->stream, (const double *)wo, (long)(n_frames * kmax * 2), (float *)out_cand); }
    return check_launch(ctx, __func__);
}

// ---- periodic.rs: the pitch path (k_pitch_path.hip) -----------------------------------------

int vbx_frame_peak_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride, double *out_peak) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc == 1) return VBX_SUCCESS;
    if (rc != VBX_SUCCESS) return rc;
    VBX_REQUIRE(ctx, out_peak != nullptr, "null out_peak");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "frame_peak"); launch_frame_peak(ctx->stream, x, (long)n_frames, (long)frame_len, (long)stride, out_peak); }
    return check_launch(ctx, __func__);
}

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

#define VBX_PP_REQUIRE(cond, msg) \
    do { if (!(cond)) return fail(ctx, VBX_E_INVALID, std::string(fn) + ": " + (msg)); } while (0)

static int check_pitch_path(vbx_ctx *ctx, const char *fn, const vbx_pitch_path_params &pr, size_t n_frames, size_t kmax, bool have_peak,
                            const int64_t *h_seg_start, size_t n_segments) {
    VBX_PP_REQUIRE(kmax >= 1 && kmax <= 63, "kmax must be in [1, 63] (at most 64 states per frame)");
    for (double v : {pr.voicing_threshold, pr.silence_threshold, pr.octave_cost, pr.octave_jump_cost, pr.voiced_unvoiced_cost,
                     pr.ceiling_hz, pr.time_step})
        VBX_PP_REQUIRE(std::isfinite(v) && v >= 0.0, "every parameter must be finite and >= 0");
    VBX_PP_REQUIRE(pr.time_step > 0.0 && pr.ceiling_hz > 0.0, "time_step and ceiling_hz must be > 0");
    VBX_PP_REQUIRE(!(pr.silence_threshold > 0.0 && !have_peak), "silence_threshold > 0 needs local_peak");
    VBX_PP_REQUIRE(n_frames <= 0x7fffffffull, "too many frames for one launch");
    if (h_seg_start != nullptr && n_segments > 0) {            // the rules of vbx_analyze_frames_f64
        VBX_PP_REQUIRE(h_seg_start[0] == 0, "seg_start[0] must be 0");
        for (size_t i = 1; i < n_segments; i++)
            VBX_PP_REQUIRE(h_seg_start[i] >= h_seg_start[i - 1] && (size_t)h_seg_start[i] <= n_frames, "seg_start must ascend within [0, n_frames]");
    }
    return VBX_SUCCESS;
}
#undef VBX_PP_REQUIRE

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
static int run_pitch_path(vbx_ctx *ctx, hipStream_t st, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
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

// ---- bench utility ------------------------------------------------------------------------

int vbx_synth_speech_f64(vbx_ctx *ctx, double *out, size_t n_samples, uint64_t sample_offset,
                         double sample_rate, uint64_t seed) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (n_samples == 0) return VBX_SUCCESS;
    VBX_REQUIRE(ctx, out != nullptr && sample_rate > 0.0, "bad argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    { Prof p(ctx, "synth"); launch_synth(ctx->stream, out, n_samples, sample_offset, sample_rate, seed); }
    return check_launch(ctx, __func__);
}

// internal (tests only; not part of the public header): how many frames of the last FFT-path pitch / analyze call were
// handed to the direct-sum kernel because a peak decision lay inside the transforms' rounding error
int vbx_internal_last_unsure_count(vbx_ctx *ctx, int32_t *h_count) {
    VBX_REQUIRE(ctx, ctx && h_count, "null argument");
    *h_count = 0;
    if (!ctx->ws[vbx_ctx::WS_UNSURE]) return VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VBX_HIP(ctx, hipMemcpy(h_count, ctx->ws[vbx_ctx::WS_UNSURE], sizeof(int32_t), hipMemcpyDeviceToHost));
    return VBX_SUCCESS;
}

// internal (tests, bench): how many frames of the last fused analyze call the Levinson probe handed to the double-double
// recursion (k_lpc_exact.hip); -1 if the last frame-batch call (every entry point that takes frames: check_frames clears the
// flag) armed no probe list -- no LPC rows, an unsupported shape, or a policy other than VBX_LPC_POLICY_EXACT
int vbx_internal_last_lpc_exact_count(vbx_ctx *ctx, int32_t *h_count) {
    VBX_REQUIRE(ctx, ctx && h_count, "null argument");
    *h_count = -1;
    if (!ctx->ws[vbx_ctx::WS_LPC_LIST] || !ctx->lpc_list_armed) return VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    VBX_HIP(ctx, hipDeviceSynchronize());
    VBX_HIP(ctx, hipMemcpy(h_count, ctx->ws[vbx_ctx::WS_LPC_LIST], sizeof(int32_t), hipMemcpyDeviceToHost));
    return VBX_SUCCESS;
}

// internal (tests only): how many frames of the last Burg / find_formants call the one-pass form's guard handed to the
// direct recursion (k_burg_fast.hip); -1 if the last such call did not take the one-pass form
int vbx_internal_last_burg_direct_count(vbx_ctx *ctx, int32_t *h_count) {
    VBX_REQUIRE(ctx, ctx && h_count, "null argument");
    *h_count = -1;
    if (!ctx->burg_list_count) return VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    VBX_HIP(ctx, hipDeviceSynchronize());
    VBX_HIP(ctx, hipMemcpy(h_count, ctx->burg_list_count + 1, sizeof(int32_t), hipMemcpyDeviceToHost));
    return VBX_SUCCESS;
}

// internal (tests only): the same count for the resonance kernel of the last find_formants call (k_roots_fast.hip)
int vbx_internal_last_roots_direct_count(vbx_ctx *ctx, int32_t *h_count) {
    VBX_REQUIRE(ctx, ctx && h_count, "null argument");
    *h_count = -1;
    if (!ctx->roots_list_count) return VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    VBX_HIP(ctx, hipDeviceSynchronize());
    VBX_HIP(ctx, hipMemcpy(h_count, ctx->roots_list_count, sizeof(int32_t), hipMemcpyDeviceToHost));
    return VBX_SUCCESS;
}

// internal: cross-lane helper self-test (tests only; not part of the public header)
int vbx_selftest_lanes(vbx_ctx *ctx, double *h_out512) {   // h_out512: 1024 doubles
    VBX_REQUIRE(ctx, ctx && h_out512, "null argument");
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    void *d = nullptr;
    int rc = ws_get(ctx, vbx_ctx::WS_MISC, 1024 * sizeof(double), &d);
    if (rc != VBX_SUCCESS) return rc;
    launch_selftest(ctx->stream, (double *)d);
    rc = check_launch(ctx, __func__);
    if (rc != VBX_SUCCESS) return rc;
    VBX_HIP(ctx, hipMemcpyAsync(h_out512, d, 1024 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VBX_SUCCESS;
}

}  // extern "C"
