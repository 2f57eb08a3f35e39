// voxbox.hpp -- header-only C++17 mirror of the vox_box 0.3.0 trait surface over the C ABI
// (include/voxbox_hip.h).  The reference is compiled code (Rust), so the host side above the
// ABI is C++: the same names, argument meaning and error behaviour as the crate's traits, with
// one difference of kind -- every call takes a BATCH of frames (the user's frame loop,
// examples/pitch_detection.rs:23-30, tests/lib.rs:71-83) instead of one slice.
//
//   reference (per frame)                              here (per batch)
//   frame.autocorrelate(n)            periodic.rs:265  Autocorrelate::autocorrelate(ctx, frames, n)
//   r.normalize()                     waves.rs:60      Normalize::normalize(ctx, rows, F, n)
//   r.lpc(p)                          spectrum.rs:86   LPC::lpc(ctx, r, F, r_stride, p)
//   frame.lpc_praat(p)                spectrum.rs:94   LPC::lpc_praat(ctx, frames, p, status)
//   frame.pitch::<Hanning>(..)        periodic.rs:356  Pitched::pitch(ctx, frames, sr, thr, min, max, kmax, ..)
//   poly.find_roots_mut(work)         polynomial.rs:92 Polynomial::find_roots_mut(ctx, polys, F, len, status)
//   roots.to_resonance(sr)            spectrum.rs:204  ToResonance::to_resonance(ctx, roots, F, n, sr, ..)
//   est.estimate_formants(res)        spectrum.rs:232  EstimateFormants::estimate_formants(ctx, ..) (= FormantExtractor)
//   PitchExtractor's third pass       periodic.rs:320  PitchExtractor::pitch_path(ctx, cand, count, status, F, kmax, peak, ..)
//   frame.mfcc(k, (lo, hi), sr)       spectrum.rs:410  MFCC::mfcc(ctx, frames, k, lo, hi, sr, ..)
//   vox_box::find_formants(..)        lib.rs:40        find_formants(ctx, frames, sr, p, segments, est, ..)
//
// VoxBoxResult<()> / panics of a frame become a per-frame status code (Status), API misuse and
// runtime failures throw voxbox::Error.  There is no CPU fallback.
#pragma once

#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "voxbox_hip.h"

namespace voxbox {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// VoxBoxError (src/error.rs:4-16) + the panics of the path, per frame
enum class Status : int32_t { Ok = 0, LPC = 1, Polynomial = 2, NaN = 3, Panic = 4 };

using Resonance = vbx_resonance;   // #[repr(C)] Resonance<f64>, spectrum.rs:149-154
using Pitch = vbx_pitch;           // Pitch<f64>, periodic.rs:306-310
using Complex = vbx_complex;       // num::Complex<f64>

constexpr size_t MAX_RESONANCES = VBX_MAX_RESONANCES;                       // lib.rs:26
inline const double *male_formant_estimates() { return VBX_MALE_FORMANT_ESTIMATES; }     // lib.rs:27
inline const double *female_formant_estimates() { return VBX_FEMALE_FORMANT_ESTIMATES; } // lib.rs:28

// which LPC rows a context computes from frames (vbx_ctx_set_lpc_policy): Reference = the crate's own f64 rows, bit for bit
enum class LpcPolicy : int { Exact = VBX_LPC_POLICY_EXACT, Plain = VBX_LPC_POLICY_PLAIN, Reference = VBX_LPC_POLICY_REFERENCE };

class Context {
public:
    explicit Context(int device = 0, void *hip_stream = nullptr) {
        int rc = vbx_ctx_create(&ctx_, device, hip_stream);
        if (rc != VBX_SUCCESS) throw Error(rc, vbx_last_error(nullptr));
    }
    ~Context() { vbx_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    vbx_ctx *get() const { return ctx_; }
    void check(int rc) const { if (rc != VBX_SUCCESS) throw Error(rc, vbx_last_error(ctx_)); }
    void sync() const { check(vbx_sync(ctx_)); }
    void set_lpc_policy(LpcPolicy p) const { check(vbx_ctx_set_lpc_policy(ctx_, static_cast<int>(p))); }
    LpcPolicy lpc_policy() const {
        int p = 0;
        check(vbx_ctx_get_lpc_policy(ctx_, &p));
        return static_cast<LpcPolicy>(p);
    }
private:
    vbx_ctx *ctx_ = nullptr;
};

// device allocation owned by the caller (the crate's `Vec` returning variants allocate; the
// `_mut` variants below take caller-owned device memory and never allocate)
template <typename T>
class DeviceVec {
public:
    DeviceVec(Context &c, size_t n) : c_(&c), n_(n) { c.check(vbx_malloc(c.get(), &p_, n * sizeof(T))); }
    DeviceVec(Context &c, const std::vector<T> &h) : DeviceVec(c, h.size()) {
        c.check(vbx_memcpy_h2d(c.get(), p_, h.data(), h.size() * sizeof(T)));
    }
    DeviceVec(DeviceVec &&o) noexcept : c_(o.c_), p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
    DeviceVec(const DeviceVec &) = delete;
    ~DeviceVec() { if (p_) vbx_free(c_->get(), p_); }
    T *data() const { return static_cast<T *>(p_); }
    size_t size() const { return n_; }
    std::vector<T> to_host() const {
        std::vector<T> h(n_);
        c_->check(vbx_memcpy_d2h(c_->get(), h.data(), p_, n_ * sizeof(T)));
        return h;
    }
private:
    Context *c_;
    void *p_ = nullptr;
    size_t n_;
};

// sample::window tables on the host (sample 0.10 recurrences), upload with DeviceVec
enum class Window : int { Hanning = VBX_WINDOW_HANNING, HanningLag = VBX_WINDOW_HANNING_LAG,
                          HanningPeriodic = VBX_WINDOW_HANNING_PERIODIC, Rectangle = VBX_WINDOW_RECTANGLE };
inline std::vector<double> window_table(Window w, size_t n) {
    std::vector<double> t(n);
    if (vbx_window_table_f64(static_cast<int>(w), n, t.data()) != VBX_SUCCESS) throw Error(VBX_E_INVALID, "window_table");
    return t;
}

// A batch of frames in device memory: Windower::{hanning,rectangle}(samples, bin, hop) as a view
// (stride = hop) or a dense [F, N] array (stride = N).  `window` is the Windower's multiplier table.
struct Frames {
    const double *x = nullptr;
    size_t n_frames = 0, frame_len = 0, stride = 0;
    const double *window = nullptr;
    static Frames windower(const double *samples, size_t n_samples, size_t bin, size_t hop, const double *window) {
        return Frames{samples, vbx_frame_count(n_samples, bin, hop), bin, hop, window};
    }
    static Frames dense(const double *x, size_t n_frames, size_t frame_len, const double *window = nullptr) {
        return Frames{x, n_frames, frame_len, frame_len, window};
    }
};

struct Autocorrelate {   // periodic.rs:265-274
    static void autocorrelate_mut(Context &c, const Frames &f, size_t n_coeffs, double *coeffs /* [F, n_coeffs] */) {
        c.check(vbx_autocorrelate_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, f.window, n_coeffs, coeffs));
    }
    static DeviceVec<double> autocorrelate(Context &c, const Frames &f, size_t n_coeffs) {
        DeviceVec<double> out(c, f.n_frames * n_coeffs);
        autocorrelate_mut(c, f, n_coeffs, out.data());
        return out;
    }
    // impl Autocorrelate for VecDeque (periodic.rs:291-304): the Windower view over a ring buffer as a dense batch
    static DeviceVec<double> ring_frames(Context &c, const double *ring, size_t capacity, size_t head, size_t n_frames,
                                         size_t frame_len, size_t stride) {
        DeviceVec<double> out(c, n_frames * frame_len);
        c.check(vbx_ring_frames_f64(c.get(), ring, capacity, head, n_frames, frame_len, stride, out.data()));
        return out;
    }
};

struct RMS {             // waves.rs:10-23
    static void rms(Context &c, const Frames &f, double *out /* [F] */) {
        c.check(vbx_rms_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, f.window, out));
    }
};

struct Filter {          // waves.rs:82-96 (result in a dense [F, N] batch: strided frames overlap)
    static void preemphasis(Context &c, const Frames &f, double factor, double *out) {
        c.check(vbx_preemphasis_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, factor, out));
    }
};

// hound-style ingestion of 16-bit PCM (tests/lib.rs:17-19): sample / 32767
inline void pcm16_to_f64(Context &c, const int16_t *pcm, size_t n, double *out) { c.check(vbx_pcm16_to_f64(c.get(), pcm, n, out)); }
// float32 samples -> f64, exactly (every float is a double)
inline void f32_to_f64(Context &c, const float *x, size_t n, double *out) { c.check(vbx_f32_to_f64(c.get(), x, n, out)); }

struct Normalize {       // waves.rs:60-76
    static void normalize(Context &c, double *rows, size_t n_rows, size_t n) { c.check(vbx_normalize_f64(c.get(), rows, n_rows, n)); }
};

struct LPC {             // spectrum.rs:50-55
    static void lpc_mut(Context &c, const double *r, size_t n_frames, size_t r_stride, size_t n_coeffs, double *ac) {
        c.check(vbx_lpc_f64(c.get(), r, n_frames, r_stride, n_coeffs, ac));
    }
    static DeviceVec<double> lpc(Context &c, const double *r, size_t n_frames, size_t r_stride, size_t n_coeffs) {
        DeviceVec<double> out(c, n_frames * (n_coeffs + 1));
        lpc_mut(c, r, n_frames, r_stride, n_coeffs, out.data());
        return out;
    }
    // LPCSolver usage (spectrum.rs:40-42): autocorrelate(p+1) [-> normalize] -> lpc(p), one pass over the samples
    static void solve(Context &c, const Frames &f, size_t n_coeffs, bool normalize, double *r_out, double *lpc_out) {
        c.check(vbx_autocorr_lpc_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, f.window, n_coeffs, normalize ? 1 : 0, r_out, lpc_out));
    }
    static void lpc_praat_mut(Context &c, const Frames &f, size_t n_coeffs, double *coeffs, int32_t *status) {
        c.check(vbx_lpc_burg_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, f.window, n_coeffs, coeffs, status));
    }
    static DeviceVec<double> lpc_praat(Context &c, const Frames &f, size_t n_coeffs, int32_t *status = nullptr) {
        DeviceVec<double> out(c, f.n_frames * n_coeffs);
        lpc_praat_mut(c, f, n_coeffs, out.data(), status);
        return out;
    }
};

struct Pitched {         // periodic.rs:356-358; local_peak / global_peak are unused by the reference and omitted
    static void pitch(Context &c, const Frames &f, double sample_rate, double threshold, double min, double max,
                      size_t kmax, Pitch *candidates /* [F, kmax] */, int32_t *count, int32_t *status) {
        c.check(vbx_pitch_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, f.window, sample_rate, threshold, min, max,
                              kmax, candidates, count, status));
    }
    // Boersma's candidates with an unquantised lag (vbx_pitch_boersma_f64: Q5 / Q6 / Q8 undone): the lists of the pitch path.
    // 1 <= kmax <= 63, 16 <= frame_len <= 4096; the crate's rows stay with pitch().
    static void pitch_boersma(Context &c, const Frames &f, double sample_rate, double threshold, double min, double max,
                              size_t kmax, Pitch *candidates /* [F, kmax] */, int32_t *count, int32_t *status) {
        c.check(vbx_pitch_boersma_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, f.window, sample_rate, threshold, min, max,
                                      kmax, candidates, count, status));
    }
};

struct Polynomial {      // polynomial.rs:10-21
    static void find_roots_mut(Context &c, Complex *polys, size_t n_polys, size_t len, int32_t *status) {
        c.check(vbx_find_roots_c64(c.get(), polys, n_polys, len, status));
    }
    static void laguerre(Context &c, const Complex *polys, size_t n_polys, size_t len, Complex start, Complex *out) {
        c.check(vbx_laguerre_c64(c.get(), polys, n_polys, len, start, out));
    }
    static size_t find_roots_work_size(size_t len) { return len * 6 + 4; }   // polynomial.rs:75-77 (unused: the library owns its scratch)
    // self / (x + other): quotient left in polys, remainder in rem (polynomial.rs:155-195)
    static void div_polynomial_mut(Context &c, Complex *polys, const Complex *others, size_t n_polys, size_t len,
                                   Complex *rem, int32_t *status) {
        c.check(vbx_div_polynomial_c64(c.get(), polys, others, n_polys, len, rem, status));
    }
    static size_t degree(const Complex *h_poly, size_t len) { return vbx_degree_c64(h_poly, len); }     // polynomial.rs:26
    static size_t off_low(const Complex *h_poly, size_t len) { return vbx_off_low_c64(h_poly, len); }   // polynomial.rs:30
    // the Complex<f32> instantiation (polynomial.rs:336-386)
    static void find_roots_mut(Context &c, vbx_complex32 *polys, size_t n_polys, size_t len, int32_t *status) {
        c.check(vbx_find_roots_c32(c.get(), polys, n_polys, len, status));
    }
    static void laguerre(Context &c, const vbx_complex32 *polys, size_t n_polys, size_t len, vbx_complex32 start,
                         vbx_complex32 *out) {
        c.check(vbx_laguerre_c32(c.get(), polys, n_polys, len, start, out));
    }
};

struct ToResonance {     // spectrum.rs:195-210
    static void to_resonance(Context &c, const Complex *roots, size_t n_rows, size_t n_roots, double sample_rate,
                             Resonance *out, int32_t *count) {
        c.check(vbx_to_resonance_c64(c.get(), roots, n_rows, n_roots, sample_rate, out, count));
    }
};

// utterance boundaries for the one stateful step of the path
struct Segments {
    const int64_t *h_seg_start = nullptr;   // host, ascending, [0] == 0
    size_t n = 0;
};

struct EstimateFormants {   // spectrum.rs:216-219, iterated as FormantExtractor (:357-369)
    static void estimate_formants(Context &c, const Resonance *res, size_t n_frames, size_t n_res, Segments seg,
                                  const std::vector<Resonance> &starting_estimates, const int32_t *frame_status,
                                  Resonance *out /* [F, n_est] */) {
        c.check(vbx_estimate_formants_f64(c.get(), res, n_frames, n_res, seg.h_seg_start, seg.n, starting_estimates.data(),
                                          starting_estimates.size(), frame_status, out));
    }
};

// The pitch path: the third pass PitchExtractor (periodic.rs:320-354,394-395) takes the parameters of but never runs.
// pitch_path_params(): Praat's "To Pitch (ac)" values; PitchExtractor::new(candidates, voiced_unvoiced_cost, voicing_threshold)
// sets the two fields of the same names (its iterator, candidates[t][0], is Pitched::pitch's column 0).
using PitchPathParams = vbx_pitch_path_params;
inline PitchPathParams pitch_path_params(double time_step = 0.01, double voiced_unvoiced_cost = 0.14, double voicing_threshold = 0.45) {
    PitchPathParams p{};
    p.voicing_threshold = voicing_threshold; p.silence_threshold = 0.03; p.octave_cost = 0.01; p.octave_jump_cost = 0.35;
    p.voiced_unvoiced_cost = voiced_unvoiced_cost; p.ceiling_hz = 600.0; p.time_step = time_step; p.chunk_frames = 0;
    return p;
}

struct PitchExtractor {
    // max |x| per frame (no window, NaN samples ignored): the path's local_peak
    static void frame_peak(Context &c, const Frames &f, double *out_peak /* [F] */) {
        c.check(vbx_frame_peak_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, out_peak));
    }
    // the path over Pitched::pitch's lists (same kmax); status / local_peak / out_index may be null
    static void pitch_path(Context &c, const Pitch *candidates, const int32_t *count, const int32_t *status, size_t n_frames,
                           size_t kmax, const double *local_peak, Segments seg, const PitchPathParams &p, Pitch *out_path,
                           int32_t *out_index) {
        c.check(vbx_pitch_path_f64(c.get(), candidates, count, status, n_frames, kmax, local_peak, seg.h_seg_start, seg.n, &p,
                                   out_path, out_index));
    }
    // pitch -> frame peak -> path in one call (f.window: the Hanning table pitch expects); status: device [F] (the pitch status)
    // or null
    static void pitch_track(Context &c, const Frames &f, double sample_rate, double threshold, double min, double max,
                            size_t kmax, Segments seg, const PitchPathParams &p, Pitch *out_path, int32_t *out_index,
                            int32_t *status = nullptr) {
        DeviceVec<Pitch> cand(c, f.n_frames * kmax);
        DeviceVec<int32_t> count(c, f.n_frames), st(c, status ? 1 : f.n_frames);
        DeviceVec<double> peak(c, f.n_frames);
        int32_t *pst = status ? status : st.data();
        Pitched::pitch(c, f, sample_rate, threshold, min, max, kmax, cand.data(), count.data(), pst);
        frame_peak(c, f, peak.data());
        pitch_path(c, cand.data(), count.data(), pst, f.n_frames, kmax, peak.data(), seg, p, out_path, out_index);
        c.sync();   // the scratch above is freed on return
    }
};

struct MFCC {            // spectrum.rs:371-373
    static void mfcc(Context &c, const Frames &f, size_t num_coeffs, std::pair<double, double> freq_bounds,
                     double sample_rate, double *out, int32_t *status) {
        c.check(vbx_mfcc_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, f.window, num_coeffs, freq_bounds.first,
                             freq_bounds.second, sample_rate, out, status));
    }
    static double hz_to_mel(double hz) { return vbx_hz_to_mel(hz); }     // spectrum.rs:375
    static double mel_to_hz(double mel) { return vbx_mel_to_hz(mel); }   // spectrum.rs:379
    static void dct_mut(Context &c, const double *signal, size_t n_rows, size_t n, double *coeffs) {
        c.check(vbx_dct_f64(c.get(), signal, n_rows, n, coeffs));
    }
};

inline size_t find_formants_real_work_size(size_t buf_len, size_t n_coeffs) { return vbx_find_formants_real_work_size(buf_len, n_coeffs); }
inline size_t find_formants_complex_work_size(size_t n_coeffs) { return vbx_find_formants_complex_work_size(n_coeffs); }

// vox_box::find_formants (lib.rs:40) over a batch.  `formants` receives the
// estimates after every frame ([F, n_est]); frames whose status != Ok leave the state untouched.
inline void find_formants(Context &c, const Frames &f, double sample_rate, size_t n_coeffs, Segments seg,
                          const std::vector<Resonance> &starting_estimates, Resonance *formants,
                          Resonance *resonances = nullptr, int32_t *res_count = nullptr, double *lpc_coeffs = nullptr,
                          int32_t *status = nullptr, double resample_ratio = 1.0) {
    if (f.window != nullptr) throw Error(VBX_E_INVALID, "find_formants applies its own periodic Hanning (lib.rs:65-70): pass rectangular frames");
    if (resample_ratio != 1.0) {   // lib.rs:57-61 (sample-crate arithmetic: parity unpinned): resampled inside Burg's kernels, the
                                   // bits of vbx_resample_linear_f64 into a dense batch + the same chain on it, without the batch
        c.check(vbx_find_formants_resampled_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, sample_rate, resample_ratio, n_coeffs,
                                                seg.h_seg_start, seg.n, starting_estimates.data(), starting_estimates.size(), formants,
                                                resonances, res_count, lpc_coeffs, status));
        return;
    }
    c.check(vbx_find_formants_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, sample_rate, n_coeffs, seg.h_seg_start,
                                  seg.n, starting_estimates.data(), starting_estimates.size(), formants, resonances,
                                  res_count, lpc_coeffs, status));
}

// The user's whole frame loop in one call (examples/pitch_detection.rs:23-30, tests/lib.rs:71-83): per frame
// pitch(..)[0], autocorrelate(p + 1) -> lpc(p), find_formants(..) with the state carried per utterance, mfcc(..), written as
// one record of record_doubles(params) doubles per frame.  `records` [F, record_ld], `status3` [3, F] (optional).
using AnalysisParams = vbx_analysis_params;
inline AnalysisParams analysis_params(double sample_rate, size_t lpc_order = 12, size_t formant_order = 12, size_t mfcc_coeffs = 13) {
    AnalysisParams p{};
    p.sample_rate = sample_rate; p.pitch_threshold = 0.2; p.pitch_fmin = 75.0; p.pitch_fmax = 600.0;
    p.lpc_order = lpc_order; p.formant_order = formant_order; p.n_est = formant_order ? 4 : 0;
    for (size_t e = 0; e < 4; e++) { p.est_init[e].frequency = VBX_MALE_FORMANT_ESTIMATES[e]; p.est_init[e].bandwidth = 1.0; }
    p.mfcc_coeffs = mfcc_coeffs; p.mfcc_lo_hz = 100.0; p.mfcc_hi_hz = 8000.0;
    return p;
}
inline size_t record_doubles(const AnalysisParams &p) { return vbx_record_doubles(&p); }
inline void analyze_frames(Context &c, const Frames &f, const AnalysisParams &p, Segments seg, double *records, size_t record_ld,
                           int32_t *status3 = nullptr) {
    if (f.window != nullptr) throw Error(VBX_E_INVALID, "analyze_frames applies the windows itself: pass rectangular frames");
    c.check(vbx_analyze_frames_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, &p, seg.h_seg_start, seg.n, records, record_ld, status3));
}
// the same on the WAV reader's 16-bit PCM (tests/lib.rs:17-19 before the `/ 32767`): bit-identical records, a quarter of the bytes
inline void analyze_frames_pcm16(Context &c, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride, const AnalysisParams &p,
                                 Segments seg, double *records, size_t record_ld, int32_t *status3 = nullptr) {
    c.check(vbx_analyze_frames_pcm16(c.get(), pcm, n_frames, frame_len, stride, &p, seg.h_seg_start, seg.n, records, record_ld, status3));
}
// The frame loop with PitchExtractor's third pass run: columns 0-1 of the records hold the pitch path over the call's own kmax-entry
// lists instead of candidates[0].  path.time_step == 0 (the helper's default) means stride / sample_rate.  outputs (optional device
// arrays, any member null): the lists, counts, peaks and path indices, for another Pitched::pitch_path with other costs.
using PitchTrackParams = vbx_pitch_track_params;
using PitchTrackOutputs = vbx_pitch_track_outputs;
inline PitchTrackParams pitch_track_params(size_t kmax = 15, const PitchPathParams &path = pitch_path_params(0.0)) {
    PitchTrackParams t{};
    t.kmax = kmax; t.path = path;
    return t;
}
inline void analyze_frames_tracked(Context &c, const Frames &f, const AnalysisParams &p, const PitchTrackParams &track, Segments seg,
                                   double *records, size_t record_ld, int32_t *status3 = nullptr,
                                   const PitchTrackOutputs *outputs = nullptr) {
    if (f.window != nullptr) throw Error(VBX_E_INVALID, "analyze_frames_tracked applies the windows itself: pass rectangular frames");
    c.check(vbx_analyze_frames_tracked_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, &p, &track, seg.h_seg_start, seg.n, records,
                                           record_ld, status3, outputs));
}
inline void analyze_frames_tracked_pcm16(Context &c, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                                         const AnalysisParams &p, const PitchTrackParams &track, Segments seg, double *records,
                                         size_t record_ld, int32_t *status3 = nullptr, const PitchTrackOutputs *outputs = nullptr) {
    c.check(vbx_analyze_frames_tracked_pcm16(c.get(), pcm, n_frames, frame_len, stride, &p, &track, seg.h_seg_start, seg.n, records,
                                             record_ld, status3, outputs));
}
// The frame loop of examples/formant_extraction/src/main.rs:72-88: find_formants at ext.formant_resample_ratio (given
// ext.formant_sample_rate; 0: sample_rate * ratio) and, with ext.rms, the frame's RMS as the LAST column of the record
// (record_doubles(params, ext) doubles).  track null: columns 0-1 = candidates[0] (analyze_frames); non-null: the pitch path
// (analyze_frames_tracked).  An ext that asks for nothing is that call itself, bit for bit.
using AnalysisExt = vbx_analysis_ext;
inline AnalysisExt analysis_ext(double formant_resample_ratio = 0.0, bool rms = false, double formant_sample_rate = 0.0) {
    AnalysisExt e{};
    e.formant_resample_ratio = formant_resample_ratio; e.formant_sample_rate = formant_sample_rate; e.rms = rms ? 1 : 0;
    return e;
}
inline size_t record_doubles(const AnalysisParams &p, const AnalysisExt &ext) { return vbx_record_doubles_ex(&p, &ext); }
inline void analyze_frames_ex(Context &c, const Frames &f, const AnalysisParams &p, const AnalysisExt &ext, const PitchTrackParams *track,
                              Segments seg, double *records, size_t record_ld, int32_t *status3 = nullptr,
                              const PitchTrackOutputs *outputs = nullptr) {
    if (f.window != nullptr) throw Error(VBX_E_INVALID, "analyze_frames_ex applies the windows itself: pass rectangular frames");
    c.check(vbx_analyze_frames_ex_f64(c.get(), f.x, f.n_frames, f.frame_len, f.stride, &p, &ext, track, seg.h_seg_start, seg.n, records,
                                      record_ld, status3, outputs));
}
inline void analyze_frames_ex_pcm16(Context &c, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                                    const AnalysisParams &p, const AnalysisExt &ext, const PitchTrackParams *track, Segments seg,
                                    double *records, size_t record_ld, int32_t *status3 = nullptr,
                                    const PitchTrackOutputs *outputs = nullptr) {
    c.check(vbx_analyze_frames_ex_pcm16(c.get(), pcm, n_frames, frame_len, stride, &p, &ext, track, seg.h_seg_start, seg.n, records,
                                        record_ld, status3, outputs));
}
// The same on float32 samples (only the input is float: records and everything else written are analyze_frames_ex's on the exactly
// widened samples, bit for bit; full 1200-sample frames are read without an f64 copy).  ext null: the plain / tracked call.
inline void analyze_frames_ex_f32in(Context &c, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                                    const AnalysisParams &p, const AnalysisExt *ext, const PitchTrackParams *track, Segments seg,
                                    double *records, size_t record_ld, int32_t *status3 = nullptr,
                                    const PitchTrackOutputs *outputs = nullptr) {
    c.check(vbx_analyze_frames_ex_f32in(c.get(), x, n_frames, frame_len, stride, &p, ext, track, seg.h_seg_start, seg.n, records,
                                        record_ld, status3, outputs));
}
// The frame loop on a recording in HOST memory, of any length (vbx_analyze_host): h_audio holds n_sample_frames interleaved sample
// frames in fmt.format, uploaded chunk by chunk beside the analysis; records / status3 / outputs are device memory and hold what the
// resident call on the whole selected channel writes, bit for bit.  host_audio(): mono, the library's default chunk.
using HostAudio = vbx_host_audio;
inline HostAudio host_audio(int format, int channels = 1, int channel = 0, size_t chunk_frames = 0) {
    HostAudio a{};
    a.format = format; a.channels = channels; a.channel = channel; a.chunk_frames = chunk_frames;
    return a;
}
inline void analyze_host(Context &c, const void *h_audio, size_t n_sample_frames, const HostAudio &fmt, size_t frame_len, size_t stride,
                         const AnalysisParams &p, const AnalysisExt *ext, const PitchTrackParams *track, Segments seg,
                         double *records, size_t record_ld, int32_t *status3 = nullptr, const PitchTrackOutputs *outputs = nullptr) {
    c.check(vbx_analyze_host(c.get(), h_audio, n_sample_frames, &fmt, frame_len, stride, &p, ext, track, seg.h_seg_start, seg.n, records,
                             record_ld, status3, outputs));
}
// one channel of interleaved sample frames on the device, as the type the frame loop reads (vbx_unpack_samples)
inline void unpack_samples(Context &c, const void *d_src, size_t n_sample_frames, int format, int channels, int channel, void *d_out) {
    c.check(vbx_unpack_samples(c.get(), d_src, n_sample_frames, format, channels, channel, d_out));
}
// the selected channels in one pass (vbx_unpack_channels): plane k = channel h_channels[k], from element k * plane_ld of d_out
inline void unpack_channels(Context &c, const void *d_src, size_t n_sample_frames, int format, int channels, const int32_t *h_channels,
                            size_t n_sel, void *d_out, size_t plane_ld) {
    c.check(vbx_unpack_channels(c.get(), d_src, n_sample_frames, format, channels, h_channels, n_sel, d_out, plane_ld));
}
// analyze_host for n_sel channels of one recording from ONE upload per chunk (vbx_analyze_host_channels): fmt.channel stays 0, the
// selection is h_channels; out[k] holds the device outputs of channel h_channels[k], each what analyze_host writes for that channel,
// bit for bit.  One parameter set, one segment list and one record_ld for all channels; n_sel <= VBX_HOST_MAX_CHANNELS.
using ChannelOutputs = vbx_channel_outputs;
inline void analyze_host_channels(Context &c, const void *h_audio, size_t n_sample_frames, const HostAudio &fmt, const int32_t *h_channels,
                                  size_t n_sel, size_t frame_len, size_t stride, const AnalysisParams &p, const AnalysisExt *ext,
                                  const PitchTrackParams *track, Segments seg, const ChannelOutputs *out, size_t record_ld) {
    c.check(vbx_analyze_host_channels(c.get(), h_audio, n_sample_frames, &fmt, h_channels, n_sel, frame_len, stride, &p, ext, track,
                                      seg.h_seg_start, seg.n, out, record_ld));
}
// A batch of variable-length clips in separate device buffers from ONE call (vbx_analyze_clips): h_clip holds n_clips device
// pointers (a host array), h_len their lengths in samples; clip b's rows are rows [row_start_b, row_start_b + n_rows_b) of every
// output (clips_plan gives them), bit for bit what the resident call writes on that clip alone.  clip_format(): the default groups.
// (8-bit clips -- VBX_SAMPLE_U8 / VBX_SAMPLE_ULAW / VBX_SAMPLE_ALAW, one byte per sample -- are named in clip_format like any other.)
using ClipFormat = vbx_clip_format;
using ClipRow = vbx_clip_row;
inline ClipFormat clip_format(int format, size_t group_frames = 0) {
    ClipFormat f{};
    f.format = format; f.group_frames = group_frames;
    return f;
}
// The 256 16-bit linear values of a G.711 law (VBX_SAMPLE_ULAW or VBX_SAMPLE_ALAW), by the function the reader kernels run; host only.
inline std::array<int16_t, 256> g711_table(int format) {
    std::array<int16_t, 256> t{};
    if (vbx_g711_table(format, t.data()) != VBX_SUCCESS) throw Error(VBX_E_INVALID, "g711_table: format must be VBX_SAMPLE_ULAW or VBX_SAMPLE_ALAW");
    return t;
}
struct ClipsPlan { std::vector<ClipRow> rows; size_t total_rows = 0, n_groups = 0; };
inline ClipsPlan clips_plan(const size_t *h_len, size_t n_clips, size_t frame_len, size_t stride, size_t group_frames = 0) {
    ClipsPlan p;
    p.rows.resize(n_clips);
    if (vbx_clips_plan(h_len, n_clips, frame_len, stride, group_frames, p.rows.data(), &p.total_rows, &p.n_groups) != VBX_SUCCESS)
        throw Error(VBX_E_INVALID, "clips_plan: bad argument");
    return p;
}
inline void analyze_clips(Context &c, const void *const *h_clip, const size_t *h_len, size_t n_clips, const ClipFormat &fmt, size_t frame_len,
                          size_t stride, const AnalysisParams &p, const AnalysisExt *ext, const PitchTrackParams *track, double *records,
                          size_t record_ld, int32_t *status3 = nullptr, const PitchTrackOutputs *outputs = nullptr) {
    c.check(vbx_analyze_clips(c.get(), h_clip, h_len, n_clips, &fmt, frame_len, stride, &p, ext, track, records, record_ld, status3, outputs));
}
// pinned host memory for analyze_host's h_audio (vbx_malloc_host / vbx_free_host)
inline void *malloc_host(Context &c, size_t bytes) { void *p = nullptr; c.check(vbx_malloc_host(c.get(), &p, bytes)); return p; }
inline void free_host(Context &c, void *p) { c.check(vbx_free_host(c.get(), p)); }

// A live session (vbx_session_*): ONE channel of a stream of audio that arrives block by block; every push delivers the records of the
// frames its block completes, and all the rows pushed equal, bit for bit, what the resident frame loop writes on the concatenated
// blocks, for every way of cutting the stream into blocks of at most max_block sample frames.  records / status3 / outputs are device
// memory; push returns the number of rows written (session_plan tells it beforehand).  Tracked form: cand and count (and peak, with a
// silence threshold) are required, index must be null, columns 0-1 are the caller's path to fill (pitch_path over an utterance's rows).
using SessionPlan = vbx_session_plan_t;
inline SessionPlan session_plan(size_t consumed, size_t utt_frame, size_t n_new, size_t frame_len, size_t stride) {
    SessionPlan p{};
    if (vbx_session_plan(consumed, utt_frame, n_new, frame_len, stride, &p) != VBX_SUCCESS) throw Error(VBX_E_INVALID, "session_plan: bad argument");
    return p;
}
class session {
public:
    session(Context &c, const HostAudio &fmt, size_t frame_len, size_t stride, const AnalysisParams &p, const AnalysisExt *ext,
            const PitchTrackParams *track, size_t max_block) : c_(c) {
        c.check(vbx_session_open(c.get(), &fmt, frame_len, stride, &p, ext, track, max_block, &s_));
    }
    ~session() { vbx_session_close(s_); }
    session(const session &) = delete;
    session &operator=(const session &) = delete;
    size_t push(const void *h_block, size_t n_sample_frames, double *records, size_t record_ld, int32_t *status3 = nullptr,
                size_t status_ld = 0, const PitchTrackOutputs *outputs = nullptr) {
        size_t n = 0;
        c_.check(vbx_session_push(s_, h_block, n_sample_frames, records, record_ld, status3, status_ld, outputs, &n));
        return n;
    }
    size_t push_device(const void *d_block, size_t n_sample_frames, double *records, size_t record_ld, int32_t *status3 = nullptr,
                       size_t status_ld = 0, const PitchTrackOutputs *outputs = nullptr) {
        size_t n = 0;
        c_.check(vbx_session_push_device(s_, d_block, n_sample_frames, records, record_ld, status3, status_ld, outputs, &n));
        return n;
    }
    void mark_utterance() { c_.check(vbx_session_mark_utterance(s_)); }
    void reset() { c_.check(vbx_session_reset(s_)); }
    // the contour from a tracked session (vbx_session_path_bind): every push also commits the decided rows of the pitch path into the
    // bound device arrays from row 0 (max_pending + the largest push's frames rows each) and one PathCommit into d_commit
    void bind_path(double peak_ref, size_t max_pending, vbx_pitch *out_path, size_t path_ld, int32_t *out_index, uint8_t *out_forced,
                   vbx_path_commit *d_commit) {
        c_.check(vbx_session_path_bind(s_, peak_ref, max_pending, out_path, path_ld, out_index, out_forced, d_commit));
    }
    struct Info { size_t consumed, frames, carried; };
    Info info() const {
        Info i{};
        c_.check(vbx_session_info(s_, &i.consumed, &i.frames, &i.carried));
        return i;
    }
    vbx_session *get() const { return s_; }
private:
    Context &c_;
    vbx_session *s_ = nullptr;
};

// A pool of independent live streams (vbx_pool_*): max_streams slots on one context that share a sample format (mono), a frame shape
// and a parameter set, each with its own timeline.  One tick -- push -- takes (slot, block) entries of any sizes, any subset of the
// slots, in any order, and delivers every entry's rows into ONE set of device arrays, entry after entry (rows[i] tells where), from
// one upload and a fixed number of launches.  Per slot the rows of all ticks equal, bit for bit, a one-channel session's for the same
// blocks, marks and resets.  Frames of at most VBX_MAX_FRAME_LEN samples; a tracked pool's live pitch contours come from bind_path.
using PoolEntry = vbx_pool_entry;
using PoolRows = vbx_pool_rows;
using PoolPlanRow = vbx_pool_plan_row;
using PoolPathOutputs = vbx_pool_path_outputs;
// the rows one slot's area of a bound pool's contour arrays needs at least: max_pending + ceil(max_block / stride)
inline size_t pool_path_slot_rows(size_t max_pending, size_t max_block, size_t stride) { return vbx_pool_path_slot_rows(max_pending, max_block, stride); }
struct PoolPlan { std::vector<PoolPlanRow> rows; size_t total_rows = 0, call_frames = 0; };
inline PoolPlan pool_plan(const size_t *h_consumed, const size_t *h_utt_frame, const size_t *h_n_new, size_t n_entries, size_t frame_len,
                          size_t stride) {
    PoolPlan p;
    p.rows.resize(n_entries);
    if (vbx_pool_plan(h_consumed, h_utt_frame, h_n_new, n_entries, frame_len, stride, p.rows.data(), &p.total_rows, &p.call_frames) != VBX_SUCCESS)
        throw Error(VBX_E_INVALID, "pool_plan: bad argument");
    return p;
}
class pool {
public:
    pool(Context &c, const HostAudio &fmt, size_t frame_len, size_t stride, const AnalysisParams &p, const AnalysisExt *ext,
         const PitchTrackParams *track, size_t max_streams, size_t max_block, size_t max_tick) : c_(c) {
        c.check(vbx_pool_open(c.get(), &fmt, frame_len, stride, &p, ext, track, max_streams, max_block, max_tick, &p_));
    }
    ~pool() { vbx_pool_close(p_); }
    pool(const pool &) = delete;
    pool &operator=(const pool &) = delete;
    // returns the tick's total rows; h_rows (optional): n_entries entries
    size_t push(const PoolEntry *h_entries, size_t n_entries, double *records, size_t record_ld, int32_t *status3 = nullptr,
                size_t status_ld = 0, const PitchTrackOutputs *outputs = nullptr, PoolRows *h_rows = nullptr) {
        size_t n = 0;
        c_.check(vbx_pool_push(p_, h_entries, n_entries, records, record_ld, status3, status_ld, outputs, h_rows, &n));
        return n;
    }
    size_t push_device(const PoolEntry *h_entries, size_t n_entries, double *records, size_t record_ld, int32_t *status3 = nullptr,
                       size_t status_ld = 0, const PitchTrackOutputs *outputs = nullptr, PoolRows *h_rows = nullptr) {
        size_t n = 0;
        c_.check(vbx_pool_push_device(p_, h_entries, n_entries, records, record_ld, status3, status_ld, outputs, h_rows, &n));
        return n;
    }
    void mark_utterance(int32_t stream) { c_.check(vbx_pool_mark_utterance(p_, stream)); }
    void reset_stream(int32_t stream) { c_.check(vbx_pool_reset_stream(p_, stream)); }
    // every slot's contour from a tracked pool (vbx_pool_path_bind): every tick also commits, in ONE more launch, the decided rows of
    // each visited slot's pitch path into rows [s * slot_rows, ...) of the bound device arrays and its PathCommit into d_commit[s];
    // marks and resets are deferred to the next tick's launch, and an empty tick fetches a marked slot's tail
    void bind_path(double peak_ref, size_t max_pending, const PoolPathOutputs &out, size_t path_ld, size_t slot_rows) {
        c_.check(vbx_pool_path_bind(p_, peak_ref, max_pending, &out, path_ld, slot_rows));
    }
    struct Info { size_t consumed, frames, carried; };
    Info info(int32_t stream) const {
        Info i{};
        c_.check(vbx_pool_info(p_, stream, &i.consumed, &i.frames, &i.carried));
        return i;
    }
    vbx_pool *get() const { return p_; }
private:
    Context &c_;
    vbx_pool *p_ = nullptr;
};

// A live session over several channels (vbx_session_open_channels / vbx_session_push_channels): ONE session, one upload and one
// frame-loop call per push for every selected channel of a stream -- a stereo interface, a microphone array.  select: n_sel distinct
// channels in any order; out: n_sel entries (a host array), entry k the device outputs of channel select[k] for this push's rows.
// Per channel the rows equal, bit for bit, a one-channel session's on that channel.  One parameter set and one list of marks for all.
using SessionChannelsPlan = vbx_session_channels_plan_t;
inline SessionChannelsPlan session_channels_plan(size_t consumed, size_t utt_frame, size_t n_new, size_t frame_len, size_t stride,
                                                 size_t elem_bytes, size_t n_sel, int64_t *h_seg_start = nullptr) {
    SessionChannelsPlan p{};
    if (vbx_session_channels_plan(consumed, utt_frame, n_new, frame_len, stride, elem_bytes, n_sel, &p, h_seg_start) != VBX_SUCCESS)
        throw Error(VBX_E_INVALID, "session_channels_plan: bad argument");
    return p;
}
class session_channels {
public:
    session_channels(Context &c, const HostAudio &fmt /* channel 0 */, const int32_t *select, size_t n_sel, size_t frame_len, size_t stride,
                     const AnalysisParams &p, const AnalysisExt *ext, const PitchTrackParams *track, size_t max_block) : c_(c) {
        c.check(vbx_session_open_channels(c.get(), &fmt, select, n_sel, frame_len, stride, &p, ext, track, max_block, &s_));
    }
    ~session_channels() { vbx_session_close(s_); }
    session_channels(const session_channels &) = delete;
    session_channels &operator=(const session_channels &) = delete;
    size_t push(const void *h_block, size_t n_sample_frames, const ChannelOutputs *out, size_t record_ld, size_t status_ld = 0) {
        size_t n = 0;
        c_.check(vbx_session_push_channels(s_, h_block, n_sample_frames, out, record_ld, status_ld, &n));
        return n;
    }
    size_t push_device(const void *d_block, size_t n_sample_frames, const ChannelOutputs *out, size_t record_ld, size_t status_ld = 0) {
        size_t n = 0;
        c_.check(vbx_session_push_channels_device(s_, d_block, n_sample_frames, out, record_ld, status_ld, &n));
        return n;
    }
    // every channel's contour from a tracked session (vbx_session_path_bind_channels): out holds n_sel entries of device pointers
    void bind_path(double peak_ref, size_t max_pending, const vbx_channel_path_outputs *out, size_t path_ld = 2) {
        c_.check(vbx_session_path_bind_channels(s_, peak_ref, max_pending, out, path_ld));
    }
    void mark_utterance() { c_.check(vbx_session_mark_utterance(s_)); }      // (a mark applies to every channel)
    void reset() { c_.check(vbx_session_reset(s_)); }
    session::Info info() const {
        session::Info i{};
        c_.check(vbx_session_info(s_, &i.consumed, &i.frames, &i.carried));
        return i;
    }
    vbx_session *get() const { return s_; }
private:
    Context &c_;
    vbx_session *s_ = nullptr;
};

// The pitch path committed while the candidate lists arrive (vbx_path_stream_*): pitch_path's contour over lists pushed as they come.
// Every row a push commits without a forced flag is the whole utterance's path, bit for bit, whatever follows; at most max_pending
// frames are held.  All pointers are device memory; a push is one launch on the context's stream and d_commit is written in stream
// order (read it behind a sync).  The output arrays hold max_pending + n_frames rows and are written from row 0.
using PathCommit = vbx_path_commit;
class path_stream {
public:
    path_stream(Context &c, size_t kmax, const vbx_pitch_path_params &params, double peak_ref, size_t max_pending) : c_(c) {
        c.check(vbx_path_stream_open(c.get(), kmax, &params, peak_ref, max_pending, &s_));
    }
    ~path_stream() { vbx_path_stream_close(s_); }
    path_stream(const path_stream &) = delete;
    path_stream &operator=(const path_stream &) = delete;
    void push(const vbx_pitch *cand, const int32_t *count, const int32_t *status, const double *local_peak, size_t n_frames,
              bool end_utterance, vbx_pitch *out_path, size_t path_ld, int32_t *out_index, uint8_t *out_forced, PathCommit *d_commit) {
        c_.check(vbx_path_stream_push(s_, cand, count, status, local_peak, n_frames, end_utterance ? 1 : 0, out_path, path_ld, out_index,
                                      out_forced, d_commit));
    }
    void reset() { c_.check(vbx_path_stream_reset(s_)); }
    vbx_path_stream *get() const { return s_; }
private:
    Context &c_;
    vbx_path_stream *s_ = nullptr;
};

// Frame-range sharding of one recording over the GPUs of a node (no counterpart in the reference) and the gather of the
// per-frame records to one rank: grouped ncclSend / ncclRecv inside the library, one communicator per process.
struct Shard { size_t lo, hi, s0, s1; };
inline Shard shard(size_t n_frames, int world, int rank, Segments seg, size_t frame_len, size_t hop) {
    Shard r{};
    if (vbx_shard_range(n_frames, world, rank, seg.h_seg_start, seg.n, &r.lo, &r.hi) != VBX_SUCCESS ||
        vbx_shard_samples(r.lo, r.hi, frame_len, hop, &r.s0, &r.s1) != VBX_SUCCESS)
        throw Error(VBX_E_INVALID, "shard: bad argument");
    return r;
}
// One rank's part of a recording whose utterances the frame split may cut (vbx_shard_plan): its frames, the tracker's warm-up
// frames before them, the utterance starts re-based to the shard, and whether the track continues from / into a neighbour.
struct ShardPlan {
    vbx_shard_plan_t plan{};
    std::vector<int64_t> local_seg_start;
    size_t first() const { return plan.lo - plan.warm; }              // first frame the rank analyses
    size_t n_frames() const { return plan.hi - plan.lo + plan.warm; }  // frames it analyses
};
inline ShardPlan shard_plan(size_t n_frames, int world, int rank, Segments seg) {
    ShardPlan p;
    size_t n = 0;
    if (vbx_shard_plan(n_frames, world, rank, seg.h_seg_start, seg.n, &p.plan) != VBX_SUCCESS ||
        vbx_shard_local_segments(&p.plan, seg.h_seg_start, seg.n, nullptr, 0, &n) != VBX_SUCCESS)
        throw Error(VBX_E_INVALID, "shard_plan: bad argument");
    p.local_seg_start.resize(n);
    if (vbx_shard_local_segments(&p.plan, seg.h_seg_start, seg.n, p.local_seg_start.data(), n, &n) != VBX_SUCCESS)
        throw Error(VBX_E_INVALID, "shard_plan: bad argument");
    return p;
}
// the one-device form of Comm::stitch_tracks (vbx_track_stitch_f64)
inline void track_stitch(Context &c, vbx_resonance *formants, size_t n_frames, size_t formants_ld, size_t first, size_t stop,
                         const vbx_resonance *d_state_in, int32_t *d_changed = nullptr) {
    c.check(vbx_track_stitch_f64(c.get(), formants, n_frames, formants_ld, first, stop, d_state_in, d_changed));
}
// The pitch path across shard cuts (vbx_pitch_path_shard_*_f64; the protocol is in voxbox_hip.h, "The pitch path across a shard
// cut"): begin on every rank, enter in rank order (each passing its state on), path_end_states on the host, finish on every rank.
// Every pointer is a device pointer; state arrays hold VBX_PITCH_PATH_STATES entries.
struct PitchPathShard {
    static void segment_peaks(Context &c, const double *local_peak, size_t n_frames, Segments seg, double *out_peak) {
        c.check(vbx_pitch_path_segment_peaks_f64(c.get(), local_peak, n_frames, seg.h_seg_start, seg.n, out_peak));
    }
    static void begin(Context &c, const Pitch *candidates, const int32_t *count, const int32_t *status, size_t kmax,
                      const double *local_peak, const double *seg_peak, const ShardPlan &p, const PitchPathParams &params) {
        c.check(vbx_pitch_path_shard_begin_f64(c.get(), candidates, count, status, p.n_frames(), kmax, local_peak, seg_peak,
                                               p.local_seg_start.data(), p.local_seg_start.size(), &params, p.plan.warm,
                                               p.plan.continues_prev, p.plan.continues_next));
    }
    static void enter(Context &c, const double *d_state_in, double *d_state_out, int32_t *d_back_map, int32_t *d_changed = nullptr) {
        c.check(vbx_pitch_path_shard_enter_f64(c.get(), d_state_in, d_state_out, d_back_map, d_changed));
    }
    static void finish(Context &c, const int32_t *d_end_state, Pitch *out_path, size_t path_ld = 2, int32_t *out_index = nullptr) {
        c.check(vbx_pitch_path_shard_finish_f64(c.get(), d_end_state, out_path, path_ld, out_index));
    }
    // end[r] = back_map[r + 1][end[r + 1]] from the last rank backwards; -1: rank r's last utterance ends at its own leader
    // (pass NULL to finish).  back_maps[r]: rank r's back map on the host (unused where rank r does not continue r - 1).
    static std::vector<int32_t> end_states(const std::vector<std::vector<int32_t>> &back_maps, const std::vector<ShardPlan> &plans) {
        std::vector<int32_t> end(plans.size(), -1);
        for (size_t r = plans.size(); r-- > 1;)
            if (plans[r - 1].plan.continues_next) end[r - 1] = back_maps[r][end[r] < 0 ? 0 : end[r]];
        return end;
    }
};

class Comm {
public:
    static std::vector<unsigned char> unique_id() {
        std::vector<unsigned char> id(VBX_UNIQUE_ID_BYTES);
        if (vbx_comm_unique_id(id.data()) != VBX_SUCCESS) throw Error(VBX_E_RUNTIME, vbx_last_error(nullptr));
        return id;
    }
    Comm(Context &c, const std::vector<unsigned char> &id, int world, int rank) : ctx_(c), world_(world), rank_(rank) {
        if (id.size() != VBX_UNIQUE_ID_BYTES) throw Error(VBX_E_INVALID, "Comm: the id must hold VBX_UNIQUE_ID_BYTES bytes");
        c.check(vbx_comm_create(c.get(), id.data(), world, rank, &h_));
    }
    ~Comm() { vbx_comm_destroy(h_); }
    Comm(const Comm &) = delete;
    Comm &operator=(const Comm &) = delete;
    // local: rows[rank] rows of row_doubles doubles; out (dst only): out_doubles doubles, at least what the gather writes
    // (checked here against its transfer list, vbx_gather_plan: the library cannot know the size of a raw device pointer)
    void gather_records(const double *local, const std::vector<int64_t> &rows, size_t row_doubles, int dst, double *out,
                        size_t out_doubles, int slot = 0) {
        if ((int)rows.size() != world_ || dst < 0 || dst >= world_) throw Error(VBX_E_INVALID, "gather_records: one row count per rank, dst a rank");
        std::vector<int64_t> off(rows.size()), cnt(rows.size());
        ctx_.check(vbx_gather_plan(rows.data(), world_, rank_, dst, row_doubles, off.data(), cnt.data(), nullptr));
        if (rank_ == dst && (!out || out_doubles < (size_t)(off.back() + cnt.back())))
            throw Error(VBX_E_INVALID, "gather_records: the gathered buffer is smaller than the rows the ranks send");
        ctx_.check(vbx_gather_records_f64(ctx_.get(), h_, local, rows.data(), row_doubles, dst, out, slot));
    }
    // formants: the formant column of the records the LAST analyze / find_formants call wrote for the plan's frames
    void stitch_tracks(vbx_resonance *formants, size_t formants_ld, const ShardPlan &p, int32_t *d_changed = nullptr, int slot = 0) {
        ctx_.check(vbx_comm_stitch_tracks_f64(ctx_.get(), h_, formants, p.n_frames(), formants_ld, &p.plan, d_changed, slot));
    }
    void wait(int slot) { ctx_.check(vbx_comm_wait(ctx_.get(), h_, slot)); }
    void sync() { ctx_.check(vbx_comm_sync(h_)); }
private:
    Context &ctx_;
    vbx_comm *h_ = nullptr;
    int world_ = 1, rank_ = 0;
};

}  // namespace voxbox
