// vbx_api.hip -- host side of libvoxbox_hip.so: the context's life, memory, timer and profile, the helpers every other host
// unit shares (vbx_ctx.hpp), and the single operations of include/voxbox_hip.h with their runners.  The frame loop, host-resident
// recordings, the pitch path, live sessions and the f32 families are the vbx_api_*.hip units beside this one.  No CPU fallback:
// every numeric entry point launches gfx950 kernels on the context's stream.
#include "vbx_ctx.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

using namespace vbx;

extern "C" const double VBX_MALE_FORMANT_ESTIMATES[4] = {320., 1440., 2760., 3200.};     // src/lib.rs:27
extern "C" const double VBX_FEMALE_FORMANT_ESTIMATES[4] = {480., 1760., 3200., 3520.};   // src/lib.rs:28

namespace {

thread_local std::string g_last_error;

}  // namespace

namespace vbx {

int fail(vbx_ctx *ctx, int code, const std::string &msg) {
    g_last_error = msg;
    if (ctx) ctx->last_error = msg;
    return code;
}

int check_launch(vbx_ctx *ctx, const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, VBX_E_RUNTIME, std::string(what) + " launch: " + hipGetErrorString(e));
    return VBX_SUCCESS;
}

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
                 size_t max_len) {
    if (!ctx) return fail(nullptr, VBX_E_INVALID, std::string(fn) + ": null context");
    ctx->last_batching[0] = ctx->last_batching[1] = 0;      // (vbx_internal_last_batching: the loops of this call, batch_count_t)
    ctx->last_autocorr_long_splits = 0;                     // (set by the call's last long-frame autocorrelation launch)
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

}  // namespace vbx

// =============================================================================================
extern "C" {

// hooks for code that does not see the context: vbx_host.cpp (plain C++, also built alone under the sanitizers) and the Python tools
int vbx_internal_fail(vbx_ctx *ctx, int code, const char *msg) { return fail(ctx, code, msg ? msg : ""); }
void *vbx_internal_stream(vbx_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

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
    { const char *e = std::getenv("VBX_SPECTRAL_SPEC"); ctx->spectral_spec = (e && e[0] == '0') ? 0 : 1; }
    { const char *e = std::getenv("VBX_BURG_FUSED"); ctx->burg_fused = (e && e[0] == '0') ? 0 : 1; }
    { const char *e = std::getenv("VBX_BURG_FUSED_MIN_FRAMES"); if (e && atol(e) >= 1) ctx->burg_fused_min_frames = atol(e); }
    { const char *e = std::getenv("VBX_ANALYZE_LAUNCH_FRAMES"); if (e && atol(e) >= 1) ctx->analyze_launch_frames = atol(e); }
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
    { const char *e = std::getenv("VBX_BOERSMA_GROUP"); ctx->boersma_group = (e && std::strcmp(e, "64") == 0) ? 64 : 16; }
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
    for (auto &e : ctx->ev_bf_launch) if (e) hipEventDestroy(e);
    for (auto &e : ctx->ev_bf_free) if (e) hipEventDestroy(e);
    if (ctx->trk) { hipStreamSynchronize(ctx->trk); hipStreamDestroy(ctx->trk); }
    if (ctx->copy) { hipStreamSynchronize(ctx->copy); hipStreamDestroy(ctx->copy); }
    for (int i = 0; i < 2; i++) {
        if (ctx->host_raw[i]) hipFree(ctx->host_raw[i]);
        if (ctx->host_ready[i]) hipEventDestroy(ctx->host_ready[i]);
        if (ctx->host_freed[i]) hipEventDestroy(ctx->host_freed[i]);
    }
    for (int i = 0; i < vbx_ctx::N_STAGE; i++) { if (ctx->stage[i]) hipHostFree(ctx->stage[i]); if (ctx->stage_ev[i]) hipEventDestroy(ctx->stage_ev[i]); }
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
        // (the scratch holds one partial sum per split, lag and frame: its size says into how many the launch cuts a lag's sum)
        ctx->last_autocorr_long_splits = (int)(autocorr_long_scratch_bytes((long)n_frames, (long)frame_len, (long)n_lags) / (n_frames * n_lags * sizeof(double)));
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

}  // extern "C"

namespace vbx {

// The FFT-based kernel (k_spectral.hip) followed by the direct-sum kernel on the frames whose peak decisions lie
// inside the FFT's rounding error (normally none; curves that are exactly zero over a stretch, e.g. a few impulses).
// (what launch_spectral decides about the launch from the context, before launch_analyze sees it)
static void spectral_launch_choices(const vbx_ctx *ctx, spectral_launch_t &L) {
    // MFCC::mfcc's log10 + DCT out of the frame's wavefront (mfcc_tail_q's `defer`): the kernel leaves the filter sums in the row
    // (the 1200-point plan only: in the power-of-two kernels the deferred form changes the register allocation -- thirteen index registers
    // spilled across the second transform, 3 KB of scratch traffic per frame -- for the same ~1 %; they keep the tail)
    L.mfcc_defer = L.out_mfcc != nullptr && !L.mfcc_only && L.num_coeffs >= 1 && L.num_coeffs <= 16 && ctx->mfcc_defer && L.plan == SPECTRAL_PLAN_1200;
    L.allow_spec = ctx->spectral_spec != 0;
}
bool spectral_burg_fusable_call(vbx_ctx *ctx, const spectral_launch_t &L0) {
    spectral_launch_t L = L0;
    spectral_launch_choices(ctx, L);
    return spectral_burg_fusable(L);
}

int launch_spectral(vbx_ctx *ctx, hipStream_t st, spectral_launch_t &L, const char *prof_name, const analyze_ranges_t *rg) {
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
    spectral_launch_choices(ctx, L);
    // the 4096-point plan runs as two kernels with the lag curves in a scratch buffer between them (vbx_spectral.hpp, SP_ANALYZE_SPLIT), in
    // batches of a little over SPECTRAL_SPLIT_FRAMES frames (~10 KB each; the choice's bytes per frame grant 16 more than it divides the scratch by: 131,193 at 4096 samples).
    // Whether the shape splits at all, and its bytes per frame, are the choice's own answer (a list region in LDS, kmax > 64: the fused kernel).
    L.curve_ws = nullptr; L.curve_ws_bytes = 0;
    const size_t rowb = ctx->pow2_split != 0 ? choose_analyze(L).split_row_bytes : 0;
    if (rowb) {
        const size_t frames = L.F < SPECTRAL_SPLIT_FRAMES ? (size_t)L.F : (size_t)SPECTRAL_SPLIT_FRAMES;
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
    analyze_choice_t acted{};
    int launches = 0;
    // what the launch did, for the probes (vbx_internal_last_*; vbx_pitch_f64's last_pitch_form: run_pitch, from the same choice)
    auto record = [&] {
        const bool split = !acted.refused && acted.per_launch > 0;       // (SP_ANALYZE_SPLIT / _INTERP_SPLIT: the only forms with batches)
        ctx->last_spectral_split = split ? 1 : 0;
        ctx->last_analyze_spec = acted.refused ? 0 : acted.spec;
        note_batching(ctx, split ? launches : 0, acted.per_launch);
    };
    if (rg == nullptr) { Prof p(ctx, prof_name, st); launches = launch_analyze(st, L, &acted); }
    else {
        // the same kernel in launches of rg->launch_frames frames, each leaving Burg's lag sums of its frames for the side stream
        int j = 0;
        for (long f0 = 0; f0 < L.F; f0 += rg->launch_frames, j++) {
            const long nf = (L.F - f0 < rg->launch_frames) ? L.F - f0 : rg->launch_frames;
            rc = rg->before(j);
            if (rc != VBX_SUCCESS) return rc;
            L.burg_scratch = rg->scratch[j & 1]; L.burg_window = rg->burg_window; L.burg_f0 = f0; L.burg_nf = nf;
            { Prof p(ctx, prof_name, st); launch_analyze(st, L, &acted); }
            L.burg_scratch = nullptr;
            if (acted.refused) { record(); return fail(ctx, VBX_E_RUNTIME, "launch_spectral: no instance of the fused kernel leaves Burg's lag sums for this launch"); }
            rc = rg->after(j, f0, nf);
            if (rc != VBX_SUCCESS) return rc;
        }
    }
    record();
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
const char *pitch_shape_error(size_t frame_len, size_t kmax) {
    const size_t kcap = frame_len > VBX_MAX_FRAME_LEN ? VBX_PITCH_MAX_CANDIDATES(frame_len) : (size_t)VBX_MAX_PITCH_CANDIDATES;
    if (!(kmax >= 1 && kmax <= kcap)) return "kmax must be in [1, VBX_MAX_PITCH_CANDIDATES] (long frames: [1, frame_len / 4 + 2])";
    if (frame_len < 4) return "frame_len must be >= 4";
    if (frame_len > VBX_MAX_FRAME_LEN) return frame_len <= 0x3fffffff ? nullptr : "frame_len too large for the lag curve's 32-bit indices";
    if (pitch_lds_bytes((int)frame_len) + pitch_full_list_bytes((int)frame_len, (int)kmax) + 16 > 160 * 1024) return "frame does not fit the LDS";
    return nullptr;
}

int run_pitch(vbx_ctx *ctx, hipStream_t st, const double *x, size_t n_frames, size_t frame_len, size_t stride,
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
        batch_count_t batches(ctx, (long)per);
        for (size_t f0 = 0; f0 < n_frames; f0 += per) {
            batches.launched();
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
        ctx->last_pitch_form = 100 * (3 + L.plan) + choose_analyze(L).list;      // (SP_LIST_*: 0 the lanes, 1 LDS, 2 the output row)
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

}  // namespace vbx

extern "C" {

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

}  // extern "C"

namespace vbx {

bool lpc_order_ok(size_t frame_len, size_t n_coeffs) {      // run_autocorr_lpc's rule (and the tracked frame loop's pre-check)
    return n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER && n_coeffs + 1 <= frame_len;
}

int run_autocorr_lpc(vbx_ctx *ctx, hipStream_t st, const double *x, size_t n_frames, size_t frame_len,
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

}  // namespace vbx

extern "C" {

int vbx_autocorr_lpc_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len,
                         size_t stride, const double *window, size_t n_coeffs, int normalize,
                         double *out_r, double *out_lpc) {
    int rc = check_frames(ctx, __func__, x, n_frames, frame_len, stride, VBX_MAX_LONG_FRAME_LEN);
    if (rc != VBX_SUCCESS) return rc < 0 ? rc : VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    return run_autocorr_lpc(ctx, ctx->stream, x, n_frames, frame_len, stride, window, n_coeffs, normalize, out_r, out_lpc, n_coeffs + 1);
}

}  // extern "C"

namespace vbx {

bool burg_order_ok(size_t frame_len, size_t n_coeffs) {
    return frame_len >= 2 && n_coeffs >= 1 && n_coeffs <= VBX_MAX_LPC_ORDER;
}

// Burg on a batch: the one-pass form (k_burg_fast.hip) where it exists, the frames its guard turns away and every other
// shape through the direct recursion (k_burg.hip)
// rp (vbx_find_formants_resampled_f64, vbx_analyze_frames_ex_*): x holds the caller's frames of rp->n_src samples and Burg runs on
// their RESAMPLED view -- n is then the resampled length m and window its periodic Hanning window.  The shapes the resampled
// loaders take (k_burg_resampled.hip) never exist as a batch; the others are resampled into a context-owned dense batch, a
// chunk of frames at a time, and take this function's plain form -- the same kernels at the same parameters either way.
// experiment builds (-DVBX_EXP_BURG_LAGS_ONLY, tools/experiments/burg_gate.py, profiles/burg_fused/gate.txt): the formant chain stops behind the lag kernel
#ifdef VBX_EXP_BURG_LAGS_ONLY
constexpr bool BURG_LAGS_ONLY = true;
#else
constexpr bool BURG_LAGS_ONLY = false;
#endif
constexpr size_t EX_DENSE_BYTES = size_t(256) << 20;          // the dense fallback's batch: at most this, or one resampled frame
static const char *const k_kind_names[3] = {"f64", "pcm16", "float32"};      // by sample_kind_t, for messages

int run_burg(vbx_ctx *ctx, hipStream_t stm, frames_t x, long F, int n, long stride, const double *window, int p, double *coeffs,
             int32_t *st, frame_map_t map, const resample_plan_t *rp) {
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
        batch_count_t batches(ctx, per);
        for (long f0 = 0; f0 < F; f0 += per) {
            batches.launched();
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
        batch_count_t batches(ctx, per);
        Prof pr(ctx, "burg_long", stm);
        for (long f0 = 0; f0 < F; f0 += per) {
            batches.launched();
            launch_burg_long(stm, x.f64(), f0, (f0 + per < F) ? f0 + per : F, F, n, stride, window, p, coeffs, st, (double *)w);
        }
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
            if (!BURG_LAGS_ONLY) { Prof pr(ctx, "burg_recursion", stm); launch_burg_recursion(stm, F, p, map, i0, m, coeffs, st, w); }
        }
        if (BURG_LAGS_ONLY) return VBX_SUCCESS;
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

}  // namespace vbx

extern "C" {

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

}  // extern "C"

namespace vbx {

int run_find_formants(vbx_ctx *ctx, hipStream_t stm, frames_t x, size_t n_frames, size_t frame_len,
                      size_t stride, double sample_rate, size_t n_coeffs,
                      const int64_t *h_seg_start, size_t n_segments,
                      const vbx_resonance *h_est_init, size_t n_est,
                      vbx_resonance *out_formants, size_t formants_ld, vbx_resonance *out_res, int32_t *out_res_count,
                      double *out_coeffs, int32_t *status,
                      const resample_plan_t *rp /* find_formants on the frames' resampled view (run_burg) */) {
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
#ifdef VBX_EXP_BURG_LAGS_ONLY
        return check_launch(ctx, "vbx_find_formants_f64");          // (nothing behind Burg's lag kernel: the records' formant columns are not written)
#endif
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

// ---- find_formants behind the fused frame loop's launches (vbx_api_frames.hip): Burg's lag sums come from the analyze kernel ----
// The chain of run_find_formants' unsliced path, a range of frames at a time and without its lag kernel: what the records hold is the
// same bit for bit (the recursion reads the same scratch; the resonance rows are per frame; the scan by ranges + stitch is the
// chunked scan's own repair step with the previous range in the role of the previous chunk).
static size_t fr_scratch_doubles(long launch_frames, int p) { return (size_t)(3 * (p + 1)) * (size_t)((launch_frames + 63) & ~63L); }

int find_formants_ranges_begin(vbx_ctx *ctx, hipStream_t side, frames_t x, size_t n_frames, size_t stride, double sample_rate, size_t n_coeffs,
                               const int64_t *h_seg_start, size_t n_segments, const vbx_resonance *h_est_init, size_t n_est,
                               vbx_resonance *out_formants, size_t formants_ld, int32_t *status, long launch_frames, formants_ranges_t *R) {
    VBX_REQUIRE(ctx, h_est_init && out_formants, "null argument");
    VBX_REQUIRE(ctx, (int)n_coeffs == SPECTRAL_BURG_ORDER && launch_frames >= 1, "the fused lag sums are order 12");
    VBX_REQUIRE(ctx, n_est >= 1 && n_est <= VBX_FORMANT_SLOTS, "n_est must be in [1, 6]");
    VBX_REQUIRE(ctx, formants_ld >= 2 * n_est && formants_ld % 2 == 0, "formant rows must be 16-byte aligned and hold n_est entries");
    const long F = (long)n_frames; const int p = (int)n_coeffs;
    if (launch_frames > F) launch_frames = F;
    int rc; void *w = nullptr;
    R->side = side; R->x = x; R->F = F; R->stride = (long)stride; R->sample_rate = sample_rate; R->p = p; R->n_est = (int)n_est;
    rc = ws_get(ctx, vbx_ctx::WS_COEFFS, n_frames * n_coeffs * sizeof(double), &w); if (rc) return rc; R->coeffs = (double *)w;
    rc = ws_get(ctx, vbx_ctx::WS_RES, n_frames * VBX_MAX_RESONANCES * sizeof(vbx_resonance), &w); if (rc) return rc; R->res = (res_t *)w;
    rc = ws_get(ctx, vbx_ctx::WS_COUNT, n_frames * sizeof(int32_t), &w); if (rc) return rc; R->cnt = (int32_t *)w;
    R->st = status;
    if (!R->st) { rc = ws_get(ctx, vbx_ctx::WS_STATUS, n_frames * sizeof(int32_t), &w); if (rc) return rc; R->st = (int32_t *)w; }
    // the ring of two launch-sized scratch buffers, then the direct list: count, the call's total, indices [F]
    const size_t sd = fr_scratch_doubles(launch_frames, p);
    rc = ws_get(ctx, vbx_ctx::WS_BURG_LIST, 2 * sd * sizeof(double) + ((size_t)F + 2) * sizeof(int32_t), &w); if (rc) return rc;
    R->scratch[0] = (double *)w; R->scratch[1] = (double *)w + sd; R->list = (int32_t *)((double *)w + 2 * sd);
    rc = ws_get(ctx, vbx_ctx::WS_ROOTS_LIST, 4 * sizeof(int32_t), &w); if (rc) return rc; R->redo = (int32_t *)w;
    R->chunked = tracker_wants_chunks(h_seg_start, n_segments, n_frames);
    R->trk_ws = nullptr;
    if (R->chunked) { rc = ws_get(ctx, vbx_ctx::WS_TRK, tracker_chunked_workspace_bytes(launch_frames), &R->trk_ws); if (rc) return rc; }
    VBX_HIP(ctx, ctx->tables.window(VBX_WINDOW_HANNING_PERIODIC, SPECTRAL_N, &R->hann));   // src/lib.rs:65-70
    rc = upload_segments(ctx, side, h_seg_start, n_segments, n_frames, &R->d_seg, &R->nseg);
    if (rc != VBX_SUCCESS) return rc;
    rc = upload_estimates(ctx, side, h_est_init, n_est, &R->d_est);
    if (rc != VBX_SUCCESS) return rc;
    R->d_range_seg = nullptr;
    if (R->chunked) {
        std::vector<int64_t> seg;
        launch_ranges_host(R->d_seg ? h_seg_start : nullptr, n_segments, n_frames, (size_t)launch_frames, seg, R->off, R->stitch);
        void *d = nullptr;
        rc = stage_upload(ctx, 4, vbx_ctx::WS_RANGE_SEG, seg.data(), seg.size() * sizeof(int64_t), side, &d);
        if (rc != VBX_SUCCESS) return rc;
        R->d_range_seg = (const int64_t *)d;
    }
    ctx->burg_list_count = R->list;
    ctx->roots_list_count = R->redo;
    VBX_HIP(ctx, hipMemsetAsync(R->list, 0, sizeof(int32_t), side));
    VBX_HIP(ctx, hipMemsetAsync(R->redo, 0, sizeof(int32_t), side));
    R->out = (res_t *)out_formants; R->out_ld = (long)formants_ld;
    ctx->last_track.res = R->res; ctx->last_track.cnt = R->cnt; ctx->last_track.st = R->st; ctx->last_track.F = F;
    ctx->last_track.n_est = (int)n_est; ctx->last_track.out = R->out; ctx->last_track.out_ld = R->out_ld;
    return VBX_SUCCESS;
}

int find_formants_ranges_step(vbx_ctx *ctx, formants_ranges_t *R, int j, long f0, long nf) {
    hipStream_t stm = R->side;
    const int p = R->p;
    { Prof pr(ctx, "burg_recursion", stm); launch_burg_recursion_at(stm, R->scratch[j & 1], R->list, R->F, p, f0, nf, R->coeffs, R->st); }
    VBX_HIP(ctx, hipEventRecord(ctx->ev_bf_free[j & 1], stm));                      // the scratch may be written again
    { Prof pr(ctx, "burg_direct_list", stm); launch_burg_list(stm, R->x, R->F, SPECTRAL_N, R->stride, R->hann, p, R->coeffs, R->st, R->list + 2, R->list); }
    launch_count_accumulate(stm, R->list, R->list + 1, j == 0);                     // list[1]: the call's total (vbx_internal_last_burg_direct_count)
    VBX_HIP(ctx, hipMemsetAsync(R->list, 0, sizeof(int32_t), stm));                 // the next launch's list starts empty
    { Prof pr(ctx, "formant_resonances", stm);
      launch_formant_resonances_fast(stm, R->coeffs + f0 * (long)p, nf, p, R->sample_rate, R->res + f0 * (long)VBX_MAX_RESONANCES, R->cnt + f0, R->st + f0,
                                     frame_map_t{0, 0, 0}, R->redo); }
    if (R->chunked) {
        // the chunked scan of this range alone, then -- a range that begins inside an utterance -- its first rows again from the row before it
        // (tracker_stitch_kernel on the range's own view, first = 0: it always redoes, the row before the range IS the true state)
        Prof pr(ctx, "tracker_chunked", stm);
        res_t *out = reinterpret_cast<res_t *>(reinterpret_cast<double *>(R->out) + f0 * R->out_ld);
        launch_tracker_chunked(stm, R->res + f0 * (long)VBX_MAX_RESONANCES, nf, VBX_MAX_RESONANCES, R->cnt + f0, R->d_range_seg + R->off[j],
                               (long)(R->off[j + 1] - R->off[j]), R->d_est, R->n_est, R->st + f0, out, R->out_ld, R->trk_ws);
        if (R->stitch[j] > 0)
            launch_tracker_stitch(stm, R->res + f0 * (long)VBX_MAX_RESONANCES, nf, VBX_MAX_RESONANCES, R->cnt + f0, R->n_est, R->st + f0, out, R->out_ld,
                                  0, (long)R->stitch[j], reinterpret_cast<const double *>(R->out) + (f0 - 1) * R->out_ld, nullptr);
    }
    return VBX_SUCCESS;
}

int find_formants_ranges_end(vbx_ctx *ctx, formants_ranges_t *R) {
    if (!R->chunked) {                                      // short utterances in a small call: one lane per utterance, once, behind the last range
        Prof p(ctx, "tracker", R->side);
        launch_tracker(R->side, R->res, R->F, VBX_MAX_RESONANCES, R->cnt, R->d_seg, (long)R->nseg, R->d_est, R->n_est, R->st, R->out, R->out_ld);
    }
    return check_launch(ctx, "vbx_find_formants_f64");
}

}  // namespace vbx

extern "C" {

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

int vbx_internal_last_spectral_split(vbx_ctx *ctx) { return ctx ? ctx->last_spectral_split : 0; }
int vbx_internal_last_autocorr_long_splits(vbx_ctx *ctx) { return ctx ? ctx->last_autocorr_long_splits : 0; }
// {launches made, frames per launch} of the host loop that cut the last frame-batch call's frames into the most launches (batch_count_t); 0, 0: it ran none
int vbx_internal_last_batching(vbx_ctx *ctx, long *h_batches, long *h_frames_per_batch) {
    VBX_REQUIRE(ctx, ctx != nullptr, "null context");
    if (h_batches) *h_batches = ctx->last_batching[0];
    if (h_frames_per_batch) *h_frames_per_batch = ctx->last_batching[1];
    return VBX_SUCCESS;
}
int vbx_internal_last_analyze_spec(vbx_ctx *ctx) { return ctx ? ctx->last_analyze_spec : 0; }
int vbx_internal_last_mfcc_interp(vbx_ctx *ctx) { return ctx ? ctx->last_mfcc_interp : 0; }
// Every MFCC kernel is profiled as "mfcc" and every pitch kernel as "pitch": these say which one the context's last call took.
// MFCC: 1 the fused kernels' forward transform, 2 the same with interpolated bins, 3 chirp-z, 4 matrix-core two-stage DFT,
// 5 vector two-stage DFT, 6 Goertzel, 7 the long-frame kernel, 8 every frame panics (rows filled).
// Pitch: 100 * family (1 long frames, 2 the direct lag sums below 512 samples / VBX_PITCH_MFMA, 3 + spectral plan: the FFT kernels)
// + the candidate list (0 lane-resident, 1 LDS-resident, 2 parked in the output row).
int vbx_internal_last_mfcc_form(vbx_ctx *ctx) { return ctx ? ctx->last_mfcc_form : 0; }
int vbx_internal_last_pitch_form(vbx_ctx *ctx) { return ctx ? ctx->last_pitch_form : 0; }

// Host only (no device, no context): what choose_analyze answers for a launch described in plain numbers (tests).
// ip[18] = {n, sample kind (SAMPLE_*), kmax, LPC on, MFCC coefficients, nb, b_lo, interp, mfcc_defer, allow_spec, lag_rcp, whole_curve,
// candidate base 16-byte aligned, cand_ld odd, mode (0 the analysis, 1 MFCC alone, 2 autocorrelation alone), n_lags, curve_ws_bytes,
// BURG requested}; dp[2] = {sample rate, fmin}.  The plan is the one the callers take (spectral_plan_mfcc where MFCC joins or is
// interpolated, spectral_plan otherwise; MFCC alone of 2048 / 2400 / 4096 samples: the half-size transform).  out[24] = {refused, family, plan,
// lpc, mf, full, mode, waves, sample, spec, burg, list, full_off, lds, lds_scan, lds_refine, ncurve, reach, cand_cap, row_doubles,
// list_ints, per_launch, split_row_bytes, spectral_burg_fusable(L)}.
int vbx_internal_analyze_choice(const int64_t *ip, const double *dp, int64_t *out) {
    if (!ip || !dp || !out || ip[0] < 2 || ip[0] > 0x3fffffff || ip[1] < 0 || ip[1] > SAMPLE_F32) return VBX_E_INVALID;
    alignas(16) static double somewhere[4];                  // (addresses the choice compares with NULL or takes the low bits of: it reads no memory)
    spectral_launch_t L{};
    L.n = (int)ip[0]; L.x = frames_t(somewhere, (sample_kind_t)ip[1]); L.kmax = (int)ip[2]; L.num_coeffs = (int)ip[4]; L.nb = (int)ip[5];
    const int mode = (int)ip[14];
    L.interp = ip[7] != 0; L.mfcc_defer = ip[8] != 0; L.allow_spec = ip[9] != 0; L.lag_rcp = ip[10] != 0; L.whole_curve = ip[11] != 0;
    L.mfcc_only = mode == 1;
    L.plan = spectral_plan(L.n);
    if (L.mfcc_only && !L.interp && (L.n == 2048 || L.n == 2400 || L.n == 4096)) L.plan = L.n == 2048 ? SPECTRAL_PLAN_1024 : L.n == 2400 ? SPECTRAL_PLAN_1200 : SPECTRAL_PLAN_2048;
    else if (L.num_coeffs != 0 && (L.interp || spectral_supported_plan(spectral_plan_mfcc(L.n), L.n, 0, L.nb, (int)ip[6], L.num_coeffs))) L.plan = spectral_plan_mfcc(L.n);
    if (L.plan == SPECTRAL_PLAN_NONE) {                      // (no transform serves the length: the callers never reach launch_analyze)
        std::memset(out, 0, 24 * sizeof(int64_t));
        out[0] = 1;
        return VBX_SUCCESS;
    }
    if (L.interp) {
        std::vector<char> h(mfcc_interp_table_bytes(L.plan, L.nb), 0);
        if (!mfcc_interp_fill(L.plan, L.n, (int)ip[6], L.nb, h.data(), &L.ip)) return VBX_E_INVALID;
    }
    L.F = 1; L.sample_rate = dp[0]; L.fmin = dp[1];
    L.out_cand = reinterpret_cast<pitch_t *>(reinterpret_cast<char *>(somewhere) + (ip[12] ? 0 : 8)); L.cand_ld = 2 * (long)L.kmax + (ip[13] ? 1 : 0);
    if (mode == 0 && ip[3]) L.out_lpc = somewhere;
    if (mode != 2 && L.num_coeffs != 0) L.out_mfcc = somewhere;
    if (mode == 2) { L.out_r = somewhere; L.n_lags = (int)ip[15]; }
    if (ip[16] > 0) { L.curve_ws = somewhere; L.curve_ws_bytes = (size_t)ip[16]; }
    const bool fusable = spectral_burg_fusable(L);
    if (ip[17]) { L.burg_scratch = somewhere; L.burg_window = somewhere; L.burg_nf = 1; }
    const analyze_choice_t c = choose_analyze(L);
    const int64_t v[24] = {c.refused, c.family, c.plan, c.lpc, c.mf, c.full, c.mode, c.waves, c.sample, c.spec, c.burg, c.list, c.full_off,
                           (int64_t)c.lds, (int64_t)c.lds_scan, (int64_t)c.lds_refine, c.ncurve, c.reach, c.cand_cap, (int64_t)c.row_doubles,
                           (int64_t)c.list_ints, c.per_launch, (int64_t)c.split_row_bytes, fusable};
    std::memcpy(out, v, sizeof v);
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

}  // extern "C"

namespace vbx {

int run_mfcc(vbx_ctx *ctx, hipStream_t stm, const double *x, size_t n_frames, size_t frame_len, size_t stride,
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

}  // namespace vbx

extern "C" {

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

// the getters below (internal: tests and bench; not part of the public header) report a device counter of the context's last call:
// *h_count = the word at d_count once the work that writes it is through (device_sync: whatever stream it ran on; otherwise the
// context's stream), or dflt where the last call left no counter (d_count null)
static int read_count(vbx_ctx *ctx, const int32_t *d_count, int32_t dflt, bool device_sync, int32_t *h_count) {
    *h_count = dflt;
    if (!d_count) return VBX_SUCCESS;
    VBX_HIP(ctx, hipSetDevice(ctx->device));
    if (device_sync) VBX_HIP(ctx, hipDeviceSynchronize());
    else VBX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VBX_HIP(ctx, hipMemcpy(h_count, d_count, sizeof(int32_t), hipMemcpyDeviceToHost));
    return VBX_SUCCESS;
}

// how many frames of the last FFT-path pitch / analyze call were handed to the direct-sum kernel because a peak decision lay
// inside the transforms' rounding error
int vbx_internal_last_unsure_count(vbx_ctx *ctx, int32_t *h_count) {
    VBX_REQUIRE(ctx, ctx && h_count, "null argument");
    return read_count(ctx, (const int32_t *)ctx->ws[vbx_ctx::WS_UNSURE], 0, false, h_count);
}

// how many frames of the last fused analyze call the Levinson probe handed to the double-double recursion (k_lpc_exact.hip);
// -1 if the last frame-batch call (every entry point that takes frames: check_frames clears the flag) armed no probe list --
// no LPC rows, an unsupported shape, or a policy other than VBX_LPC_POLICY_EXACT
int vbx_internal_last_lpc_exact_count(vbx_ctx *ctx, int32_t *h_count) {
    VBX_REQUIRE(ctx, ctx && h_count, "null argument");
    return read_count(ctx, ctx->lpc_list_armed ? (const int32_t *)ctx->ws[vbx_ctx::WS_LPC_LIST] : nullptr, -1, true, h_count);
}

// how many frames of the last Burg / find_formants call the one-pass form's guard handed to the direct recursion
// (k_burg_fast.hip); -1 if the last such call did not take the one-pass form
int vbx_internal_last_burg_direct_count(vbx_ctx *ctx, int32_t *h_count) {
    VBX_REQUIRE(ctx, ctx && h_count, "null argument");
    return read_count(ctx, ctx->burg_list_count ? ctx->burg_list_count + 1 : nullptr, -1, true, h_count);
}

// the same count for the resonance kernel of the last find_formants call (k_roots_fast.hip)
int vbx_internal_last_roots_direct_count(vbx_ctx *ctx, int32_t *h_count) {
    VBX_REQUIRE(ctx, ctx && h_count, "null argument");
    return read_count(ctx, ctx->roots_list_count, -1, true, h_count);
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
