// vbx_kernels.hpp -- host-side launcher declarations (one per kernel family).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define VBX_MAX_LPC_ORDER_K 62   // == VBX_MAX_LPC_ORDER (include/voxbox_hip.h)
#define VBX_MAX_FRAME_LEN_K 4096
#define VBX_MAX_RESONANCES_K 32
#define VBX_FORMANT_SLOTS_K 6

namespace vbx {

// A launch over a TIME SLICE of equal-length segments: item i is frame (i / tc) * seg_len + t0 + i % tc (skipped when
// it falls outside its segment or the batch).  seg_len == 0: the identity (item i is frame i).  Lets the sequential
// tracker start on the first frames of every utterance while the resonances of the later frames are still computed.
struct frame_map_t { long seg_len, t0, tc; };
__host__ __device__ inline long frame_map(const frame_map_t &m, long i, long n_frames) {
    if (m.seg_len == 0) return (i < n_frames) ? i : -1;
    const long t = m.t0 + i % m.tc, f = (i / m.tc) * m.seg_len + t;
    return (t < m.seg_len && t < m.t0 + m.tc && f < n_frames) ? f : -1;
}
inline long frame_map_items(const frame_map_t &m, long n_frames) {
    return m.seg_len == 0 ? n_frames : ((n_frames + m.seg_len - 1) / m.seg_len) * m.tc;
}


struct res_t { double frequency, bandwidth; };
struct pitch_t { double frequency, strength; };
struct cplx_t { double re, im; };
struct cplx32_t { float re, im; };

// The frames a launcher reads, with the type of their samples: f64, 16-bit PCM (a kernel widens a sample in registers: s / 32767) or
// float32 (widened exactly where it is loaded).  A typed pointer converts to the view of its own kind, so pointer and kind cannot
// disagree; the kind is that of the typed plane a kernel reads, not a VBX_SAMPLE_* format (PCM24 / PCM32 / F64 all unpack to f64).
enum sample_kind_t { SAMPLE_F64, SAMPLE_PCM16, SAMPLE_F32 };
struct frames_t {
    const void *p; sample_kind_t kind;
    frames_t(const double *x = nullptr) : p(x), kind(SAMPLE_F64) {}
    frames_t(const int16_t *x) : p(x), kind(SAMPLE_PCM16) {}
    frames_t(const float *x) : p(x), kind(SAMPLE_F32) {}
    frames_t(const void *x, sample_kind_t k) : p(x), kind(k) {}
    // the samples at their own type; null through an accessor of another kind
    const double *f64() const { return kind == SAMPLE_F64 ? static_cast<const double *>(p) : nullptr; }
    const int16_t *pcm16() const { return kind == SAMPLE_PCM16 ? static_cast<const int16_t *>(p) : nullptr; }
    const float *f32in() const { return kind == SAMPLE_F32 ? static_cast<const float *>(p) : nullptr; }
};

// k_lpc.hip
bool fewlags_supported(int n, int n_lags, bool want_lpc);
void launch_autocorr_fewlags(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                             int n_lags, int normalize, double *out_r, double *out_lpc, long lpc_ld = 0 /* 0: n_lags */,
                             int32_t *lpc_list = nullptr, int32_t *lpc_count = nullptr /* the conditioning probe's list (below) */);
void launch_autocorr_tiles(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                           int n_lags, double *out);
void launch_normalize_rows(hipStream_t s, double *data, long rows, int n);
void launch_levinson_rows(hipStream_t s, const double *r, long rows, long r_stride, int p, double *out, long out_ld,
                          double *out_kc = nullptr /* [rows, p] reflection coefficients */);
// The conditioning probe of the Levinson rows computed from FRAMES (round 6; reasoning at levinson_probe, vbx_spectral.hpp): the
// recursion is repeated on lag sums moved by +-LPC_PROBE_EPS of r[0]; a row that moves by more than LPC_PROBE_TOL in the parity metric
// (|a - b| / max(|b|, 1e-6 max |b|)) is listed and redone from the frame in double-double (k_lpc_exact.hip).
constexpr double LPC_PROBE_EPS = 16.0 * 2.220446049250313e-16;
#ifndef VBX_EXP_LPC_PROBE_TOL
#define VBX_EXP_LPC_PROBE_TOL 1e-6
#endif
constexpr double LPC_PROBE_TOL = VBX_EXP_LPC_PROBE_TOL;
void launch_levinson_rows_probe(hipStream_t s, const double *r, long rows, long r_stride, int p, double *out, long out_ld,
                                int32_t *lpc_list, int32_t *lpc_count, double *mfcc_rows = nullptr, long mfcc_ld = 0, int num_coeffs = 0,
                                const double *dct = nullptr /* p == 12: the same lane finishes the row's deferred MFCC tail */);

// k_burg.hip
bool burg_supported(int n, int p);
// (f64 coefficients whatever the samples' type; PCM samples are widened in registers: s / 32767)
void launch_burg(hipStream_t s, frames_t x, long F, int n, long stride, const double *window, int p, double *out, int32_t *status,
                 frame_map_t map);
void launch_burg_list(hipStream_t s, frames_t x, long F, int n, long stride, const double *window, int p, double *out, int32_t *status,
                      const int32_t *list, const int32_t *count);

// k_burg_fast.hip: the same coefficients from the frame's lag sums and edge samples (one pass over the frame), in chunks
// of burg_fast_chunk(F) items: launch_burg_lags, then launch_burg_recursion, per chunk; the frames its guard turns away
// are appended to burg_fast_list(ws, F, p) ([0] = count, indices from [2]) for launch_burg_list.
// ws: burg_fast_scratch_bytes(F, p) bytes; the caller zeroes the list's count before the first chunk.
bool burg_fast_supported(int n, int p);
long burg_fast_chunk(long F);
size_t burg_fast_scratch_bytes(long F, int p);
int32_t *burg_fast_list(void *ws, long F, int p);
// false: the order has no lag kernel -- NOTHING was launched, and the recursion behind would read scratch that no kernel wrote (the
// caller fails the call)
bool launch_burg_lags(hipStream_t s, frames_t x, long F, int n, long stride, const double *window, int p, frame_map_t map, long i0,
                      long m, void *ws);
void launch_burg_recursion(hipStream_t s, long F, int p, frame_map_t map, long i0, long m, double *out, int32_t *status, void *ws);
// the recursion on a scratch somebody else filled (the fused frame loop's launches: analyze_kernel<.., BURG>): frames [i0, i0 + m) of the batch,
// tile t of `scratch` holding frames [i0 + 64 t, i0 + 64 t + 64); list: [0] count, indices from [2]
void launch_burg_recursion_at(hipStream_t s, const double *scratch, int32_t *list, long F, int p, long i0, long m, double *out, int32_t *status);

void launch_count_accumulate(hipStream_t s, const int32_t *count, int32_t *total, bool reset);   // total = (reset ? 0 : total) + count

// k_burg_resampled.hip: launch_burg / launch_burg_list / launch_burg_lags on the RESAMPLED view of the frames (find_formants with a
// resample_ratio): x holds the caller's frames of rs.n_src samples; m: the resampled length; window: the
// periodic Hanning window of length m; rs: the (li, frac) table of vbx_resample_linear_f64.  Bit for bit the dense launchers on
// the [F, m] batch that entry point writes.  launch_burg_recursion runs behind launch_burg_lags_resampled unchanged.
struct resample_src_t { const int32_t *li; const double *frac; int n_src; };
bool burg_resampled_supported(int n_src, int m, int p);
void launch_burg_resampled(hipStream_t s, frames_t x, long F, int m, long stride, const double *window, resample_src_t rs, int p,
                           double *out, int32_t *status, frame_map_t map);
void launch_burg_resampled_list(hipStream_t s, frames_t x, long F, int m, long stride, const double *window, resample_src_t rs, int p,
                                double *out, int32_t *status, const int32_t *list, const int32_t *count);
bool launch_burg_lags_resampled(hipStream_t s, frames_t x, long F, int m, long stride, const double *window, resample_src_t rs, int p,
                                frame_map_t map, long i0, long n_items, void *ws);      // false: as launch_burg_lags

// k_roots.hip
void launch_find_roots(hipStream_t s, cplx_t *polys, long F, int len, int32_t *status);
void launch_laguerre(hipStream_t s, const cplx_t *polys, long F, int len, cplx_t start, cplx_t *out);
void launch_div_polynomial(hipStream_t s, cplx_t *polys, const cplx_t *others, long F, int len, cplx_t *rem, int32_t *status);
void launch_find_roots_f32(hipStream_t s, cplx32_t *polys, long F, int len, int32_t *status);
void launch_laguerre_f32(hipStream_t s, const cplx32_t *polys, long F, int len, cplx32_t start, cplx32_t *out);
void launch_to_resonance(hipStream_t s, const cplx_t *roots, long F, int n_roots, double sample_rate,
                         int strict_im, res_t *out, int out_stride, int32_t *out_count, const int32_t *status);
// Burg coefficients [F,p] -> reversed complex polynomial -> roots -> resonances [F,32] (find_formants core)
void launch_formant_resonances(hipStream_t s, const double *coeffs, long F, int p, double sample_rate,
                               res_t *out_res, int32_t *out_count, int32_t *status, frame_map_t map = frame_map_t{0, 0, 0});
// k_roots_fast.hip: the same rows from the real polynomial's conjugate pairs (converged Laguerre solves, quadratic
// deflation, a polish step that doubles as the check); a frame that fails the check is done again inside the kernel by
// the reference's iteration.  redo_count: optional device counter of those frames.
bool formant_resonances_fast_supported(int p);
void launch_formant_resonances_fast(hipStream_t s, const double *coeffs, long F, int p, double sample_rate,
                                    res_t *out_res, int32_t *out_count, int32_t *status, frame_map_t map, int32_t *redo_count);

// k_tracker.hip
void launch_tracker(hipStream_t s, const res_t *res, long F, int n_res, const int32_t *res_count,
                    const int64_t *seg_start, long n_seg, const res_t *est_init, int n_est,
                    const int32_t *frame_status, res_t *out, long out_ld /* doubles per output row, >= 2*n_est */,
                    long t0 = 0 /* first frame of every segment's slice */, long tc = 0x7fffffffffffffffL /* frames per slice */);

// the same scan for batches with long utterances: speculative chunks + exact repair (k_tracker.hip)
size_t tracker_chunked_workspace_bytes(long F);
void launch_tracker_chunked(hipStream_t s, const res_t *res, long F, int n_res, const int32_t *res_count,
                            const int64_t *seg_start, long n_seg, const res_t *est_init, int n_est,
                            const int32_t *frame_status, res_t *out, long out_ld, void *ws);

// a shard's track continued from the row the previous shard ends with (k_tracker.hip, tracker_stitch_kernel)
void launch_tracker_stitch(hipStream_t s, const res_t *res, long F, int n_res, const int32_t *res_count, int n_est,
                           const int32_t *frame_status, res_t *out, long out_ld, long first, long stop,
                           const double *state_in /* 2 n_est doubles */, int32_t *changed /* rows rewritten, or NULL */);

// k_pitch.hip
size_t pitch_lds_bytes(int n);
// the sorted candidate list lives one entry per lane up to this many entries; a larger kmax parks the whole
// candidate Vec in an extra LDS region of pitch_full_list_bytes(n, kmax) and rank-sorts it (nothing is pruned)
constexpr int PITCH_LIST_LANES = 64;
size_t pitch_full_list_bytes(int n, int kmax);
// profiling counters of the refine kernel: [PITCH_WORK_SLOTS][4] = frames, candidates, sinc evaluations, sinc terms
constexpr int PITCH_WORK_SLOTS = 64;
// experiment builds (-DVBX_EXP_PHASES, tools/experiments/phases.sh): behind the counters, [PITCH_WORK_SLOTS][PHASE_SLOTS] sums of
// shader-clock cycles a wavefront spent in each phase of the fused kernel (s_memtime at the phase boundaries, after a
// wait for everything outstanding).  A CU holds a fixed number of frames (LDS), so frames/s = frames in flight / a frame's
// time in the kernel: the phase that holds a wavefront longest is the one to shorten, whatever its instruction count.
constexpr int PHASE_SLOTS = 16;
constexpr int PITCH_WORK_WORDS = PITCH_WORK_SLOTS * 4 + PITCH_WORK_SLOTS * PHASE_SLOTS;
#ifdef VBX_EXP_PHASES
#define VBX_PHASE_INIT() unsigned long long _tp = __builtin_readcyclecounter()
#define VBX_PHASE(work_, f_, k_)                                                                                   \
    do {                                                                                                            \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                 \
        const unsigned long long _t = __builtin_readcyclecounter();                                                 \
        if ((work_) != nullptr && lane_id() == 0)                                                                   \
            atomicAdd((work_) + PITCH_WORK_SLOTS * 4 + ((f_) & (PITCH_WORK_SLOTS - 1)) * PHASE_SLOTS + (k_), _t - _tp); \
        _tp = _t;                                                                                                   \
    } while (0)
#else
#define VBX_PHASE_INIT() do { } while (0)
#define VBX_PHASE(work_, f_, k_) do { } while (0)
#endif
void launch_pitch(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                  const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                  int kmax, pitch_t *out_cand, long cand_ld /* doubles per output row, >= 2*kmax, even */,
                  int32_t *out_count, int32_t *status, unsigned long long *work);
// the same kernel over a device-resident list of frame indices (fallback of k_spectral.hip), fixed grid
void launch_pitch_list(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int grid, frames_t x, int n, long stride,
                       const double *window, const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                       int kmax, pitch_t *out_cand, long cand_ld, int32_t *out_count, int32_t *status, unsigned long long *work);
void launch_sinc_points(hipStream_t s, const double *y, int ylen, long offset, long nx, const double *xs, long m,
                        long depth, double *out, int32_t *status);
void launch_extremum_points(hipStream_t s, const double *y, int ylen, long offset, long nx, const double *ix, long m,
                            long depth, double *out_xy, int32_t *status, int interp = 2 /* 0 None, 1 Parabolic, 2 Sinc */,
                            int is_max = 1);

// k_spectral.hip, k_spectral_pow2.hip: pitch + LPC + MFCC from one real FFT of the zero-padded frame.  Three transform
// sizes ("plans"), named by the complex FFT length Nc (the real transform has 2 Nc points, the frame at most Nc samples):
// 1200 (25 ms at 48 kHz, and 1025..1199, e.g. 25 ms at 44.1 kHz), 1024 (512..1024), 2048 (1201..2048) and 4096 (2049..4096):
// the reference's own test and example shapes (tests/lib.rs:56, examples/pitch_detection.rs:23) and everything between.
constexpr int SPECTRAL_N = 1200;
constexpr int SPECTRAL_LPC_ORDER = 12;
constexpr int SPECTRAL_BURG_ORDER = 12;                        // the Burg order whose lag sums the 1200-point fused kernel can leave beside its own work (spectral_launch_t: burg_*)
constexpr int SPECTRAL_TAB_COMPLEX = 60 * 20 + 3 * 20 + 601;    // W_1200^(n' ka) | W_60^(c kb) | W_2400^m
enum { SPECTRAL_PLAN_NONE = 0, SPECTRAL_PLAN_1200 = 1, SPECTRAL_PLAN_1024 = 2, SPECTRAL_PLAN_2048 = 3, SPECTRAL_PLAN_4096 = 4,
       SPECTRAL_PLANS = 5 };
constexpr int SPECTRAL_AC_MIN_LAGS = 64;                        // vbx_autocorrelate_f64 below 1024 samples: fewer lags -> the direct kernel
                                                                // (from 1024 samples on the FFT wins wherever the few-lag kernel does not apply)
constexpr int SPECTRAL_MIN_N = 512;                             // shorter frames: the direct lag sums are as fast (measured)
int spectral_plan(int n);                                       // the plan that serves frame length n, or SPECTRAL_PLAN_NONE
int spectral_plan_mfcc(int n);                                  // the same when MFCC should join the fused kernel (k_spectral.hip)
bool spectral_supported_plan(int plan, int n, int lpc_order, int mfcc_nb, int mfcc_b_lo, int num_coeffs);
int spectral_plan_nc(int plan);                                 // its complex FFT length
int spectral_tab_complex(int plan);                             // complex entries of its twiddle table
void spectral_fill_tab(int plan, double *h_out);                // the table, host side: [2 * spectral_tab_complex(plan)]
int spectral_pow2_tab_complex(int plan);
void spectral_pow2_fill_tab(int plan, double *h_out);
// MFCC::mfcc inside the fused kernel at a frame length n that does not divide the transform's M (src/spectrum.rs:401-441 wants
// the n-point DFT: bin k is the frame's DTFT at k / n, between the transform's bins).  The frame occupies n of the transform's M >= 2 n
// samples, so its DTFT is a band-limited function of the bin index sampled at more than twice its rate: with c = (n - 1) / 2
//     X(k / n) e^{i w c} = sum_j  Z[j] K0(k M / n - j),      Z[j] = X_M[j] e^{2 pi i j c / M},
// exactly, for any real K0 whose transform is 1 on |t| <= n / 2M and 0 on |t - m| <= n / 2M, m != 0.  K0 = sinc * (the transform of a
// Kaiser-Bessel bump of half-width 1/2 - n / 2M) cut to 24 / 32 / 40 taps by M / n: the cut's error is < 1e-14 of the largest |X| of
// the transform at every M / n >= 2 (tests/test_mfcc_interp_table.py holds the tables to the exact DFT on the CPU) -- MFCC values
// within 1e-10 of the chirp-z kernel's on speech.  The phase factor drops out of |X|^2.  ~600 vector instructions per frame instead of a chirp-z kernel of two more
// transforms.  Host tables: rot[j] = e^{2 pi i j c / M} (j <= M / 4), per bin its first tap's index and its taps.
constexpr int MFCC_INTERP_MAX_TAPS = 40;                        // 24, 32 or 40 taps per bin (mfcc_interp_taps: by M / n)
struct mfcc_interp_t {
    const double *rot;                                          // complex [M / 4 + 1]
    const double *coef;                                         // double2 [slots][TAPS / 2][NT]: taps 2 t, 2 t + 1 of bin NT u + thread (NT threads per frame,
                                                                // slots = ceil(nb / NT))
    const int32_t *j0;                                          // [slots][NT]: index of the bin's first tap MINUS jmin
    int jmin, jmax;                                             // the transform's bins the taps read: Z[jmin .. jmax] (jmin may be < 0)
    int taps;                                                   // per bin (a multiple of 8)
    int pu_off;                                                 // doubles from the exchange buffer's start to the filter products
    int lds_bytes;                                              // Z + products + mel sums
};
int mfcc_interp_taps(int plan, int n);
size_t mfcc_interp_table_bytes(int plan, int nb);
size_t mfcc_interp_coef_offset(int plan);                      // byte offsets of coef and j0 in the table (rot at 0)
size_t mfcc_interp_j0_offset(int plan, int nb);
// false: the shape has no interpolated form (bins beyond M / 4, LDS that would cost a frame per CU)
bool mfcc_interp_fill(int plan, int n, int b_lo, int nb, void *h_table, mfcc_interp_t *h_desc /* offsets in the pointer fields */);

struct spectral_launch_t {
    int plan; int n;                                             // spectral_plan(n), frame length
    frames_t x;                                                  // PCM / float32 samples: full 1200-sample frames only (k_spectral.hip, k_spectral_f32in.hip)
    long F; long stride; const double *window; const double *lag_window; const double *tab;
    bool allow_spec;                                             // the launch may take a launch-specialised instance (the context's VBX_SPECTRAL_SPEC switch; the fused frame loop sets it)
    bool mfcc_defer;                                             // the MFCC rows leave the kernel as filter sums; launch_mfcc_rows finishes them (num_coeffs <= 16)
    bool lag_rcp;                                                // lag_window[((n + 1) & ~1) + i] = RN(1 / lag_window[i]) (quotient_by_table, vbx_spectral.hpp)
    double sample_rate, threshold, fmin, fmax; int kmax;
    pitch_t *out_cand; long cand_ld; int32_t *out_count; int32_t *pitch_status; unsigned long long *work;
    double *out_lpc; long lpc_ld;                                // NULL: no LPC
    double *out_mfcc; long mfcc_ld; int32_t *mfcc_status;        // NULL: no MFCC
    const int32_t *bins; const double *slopes; const double *dct; int num_coeffs; int nb;
    int32_t *unsure_list; int32_t *unsure_count;                 // frames handed to launch_pitch_list
    int32_t *lpc_list; int32_t *lpc_count;                       // frames handed to launch_lpc_exact_list (ill-conditioned LPC rows); NULL: no probe
    bool mfcc_only;                                              // MFCC::mfcc alone (n == the plan's Nc): no pitch, no LPC
    double *out_r; int n_lags;                                   // non-NULL: Autocorrelate::autocorrelate(n_lags) alone, [F, n_lags]
    bool whole_curve;                                            // keep every lag of the curve in LDS (VBX_PITCH_CURVE_CUT=0; tests)
    bool interp; mfcc_interp_t ip;                               // MFCC by interpolation of the transform's bins (device pointers)
    double *curve_ws; size_t curve_ws_bytes;                     // scratch for the split form of the 4096-point plan (lag curves between its two kernels); NULL: fused
    // non-NULL: ONE launch over frames [burg_f0, burg_f0 + burg_nf) of the batch that also leaves Burg's order-12 lag sums and edge samples of those
    // frames (under burg_window, find_formants' periodic Hanning window) in burg_scratch, tiled as burg_recursion_kernel reads it (launch-local frame
    // index).  Only where spectral_burg_fusable(L) holds.
    double *burg_scratch; const double *burg_window; long burg_f0, burg_nf;
};
// What launch_analyze launches for L, decided in ONE place (choose_analyze: k_spectral.hip for the 1200-point kernel and its float32
// unit, vbx_spectral_pow2.hpp for the power-of-two kernels) and read by everything that needs to know: the launch itself, the
// scratch launch_spectral sizes, spectral_burg_fusable, the probes (vbx_internal_last_*, vbx_internal_analyze_choice).
enum { SP_FAMILY_1200 = 0, SP_FAMILY_F32IN = 1, SP_FAMILY_POW2 = 2 };
enum { SP_LIST_LANES = 0, SP_LIST_LDS = 1, SP_LIST_PARKED = 2 };   // the candidates stay in the lanes (no whole-Vec list) / the list's own LDS region / the frame's output row
constexpr long SPECTRAL_SPLIT_FRAMES = 131072;                  // frames per launch launch_spectral sizes the split form's scratch for
struct analyze_choice_t {
    bool refused;                                                // no instance serves L: nothing is launched
    int family, plan;                                            // SP_FAMILY_*, SPECTRAL_PLAN_*
    bool lpc, mf, full; int mode;                                // the instance's LPC, MFCC, FULL and MODE (SP_ANALYZE, .., vbx_spectral.hpp)
    int waves;                                                   // wavefronts per SIMD it is compiled for
    int sample, spec; bool burg;                                 // SAMPLE_*, SP_SPEC_*, and whether it also leaves Burg's lag sums
    int list, full_off;                                          // SP_LIST_*, pitch_params_t::full_off
    size_t lds, lds_scan, lds_refine;                            // dynamic LDS of the (first) kernel; split form: of refine_far_kernel and refine_list_kernel
    int ncurve;                                                  // lags of the curve the refinement keeps (0: all)
    int reach, cand_cap; size_t row_doubles, list_ints; long per_launch;      // split form: the scratch row, the candidate list, frames per launch
    size_t split_row_bytes;                                      // scratch bytes per frame with which the shape WOULD split (0: never; launch_spectral sizes WS_CURVE)
};
analyze_choice_t choose_analyze(const spectral_launch_t &L);       // reads L alone: no HIP call, no context
bool spectral_burg_fusable(const spectral_launch_t &L);             // choose_analyze with a BURG request: some instance leaves Burg's lag sums for L
bool spectral_supported(int n, int lpc_order, int mfcc_nb, int mfcc_b_lo, int num_coeffs);
// choose, fill the argument block, launch: returns the launches of the (first) kernel it made -- 0: refused -- and, in *acted, the choice it acted on
int launch_analyze(hipStream_t s, const spectral_launch_t &L, analyze_choice_t *acted = nullptr);
// k_lpc_exact.hip: LPC::lpc(p) of the listed frames from double-double lag sums and a double-double recursion (the exact
// answer rounded once), over a list only the device knows the length of
// k_mfcc.hip: log10 (clamped at 1e-10) + DCT of rows of mel filter sums, in place, a lane per row (the deferred tail of MFCC::mfcc, vbx_mfcc_tail.hpp)
void launch_mfcc_rows(hipStream_t s, double *rows, long F, long ld, int num_coeffs, const double *dct);
bool lpc_exact_supported(int n, int p);                               // frames of 2..4096 samples, orders 1..31
void launch_lpc_exact_list(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int cus, frames_t x, int n, long stride,
                           const double *window, int p, double *out_lpc, long lpc_ld);

// k_lpc_ref.hip (VBX_LPC_POLICY_REFERENCE): the crate's own f64 arithmetic, bit for bit -- lag sums as the sequential fold of
// src/periodic.rs:276-289, [normalize,] the recursion of src/spectrum.rs:63-84, no contraction.  p == 0: lag sums only
// (n_lags <= n, out_r: [F, r_ld]); p >= 1: n_lags = p + 1, out_r (optional) and out_lpc [F, lpc_ld].
void launch_lpc_ref(hipStream_t s, frames_t x, long F, int n, long stride, const double *window, int n_lags, int p, int normalize,
                    double *out_r, long r_ld, double *out_lpc, long lpc_ld);
void launch_levinson_ref_rows(hipStream_t s, const double *r, long rows, long r_stride, int p, double *out, long out_ld, double *out_kc);

// the f32 instantiation (Sample = f32): the same kernels with float frames and float outputs
void launch_autocorr_fewlags_f32(hipStream_t s, const float *x, long F, int n, long stride, const float *window,
                                 int n_lags, int normalize, float *out_r, float *out_lpc, long lpc_ld = 0);
void launch_autocorr_tiles_f32(hipStream_t s, const float *x, long F, int n, long stride, const float *window,
                               int n_lags, float *out);
void launch_normalize_rows_f32(hipStream_t s, float *data, long rows, int n);
void launch_levinson_rows_f32(hipStream_t s, const float *r, long rows, long r_stride, int p, float *out, long out_ld,
                              float *out_kc = nullptr);
void launch_burg_f32(hipStream_t s, const float *x, long F, int n, long stride, const float *window,
                     int p, float *out, int32_t *status);
void launch_widen_frames(hipStream_t s, const float *x, long F, int n, long stride, const float *window, double *out);
// k_f32.hip: the reference-faithful f32 forms (every fold in f32, in source order; bit-identical to the f32 restatement the tests hold them to)
void launch_autocorr_f32_exact(hipStream_t s, const float *x, long F, int n, long stride, const float *window, int n_lags, float *out);
size_t pitch_f32_exact_lds_bytes(int n, int kmax);
void launch_pitch_f32_exact(hipStream_t s, const float *x, long F, int n, long stride, const float *window, const float *lag_window32,
                            double sample_rate, double threshold, double fmin, double fmax, int kmax, pitch_t *out_cand, long cand_ld,
                            int32_t *out_count, int32_t *status);
void launch_levinson_f32_exact(hipStream_t s, const float *r, long rows, long r_stride, int p, float *out, long out_ld, float *out_kc);
size_t burg_f32_exact_scratch_bytes(long frames, int n);
void launch_burg_f32_exact(hipStream_t s, const float *x, long f0, long f1, long F, int n, long stride, const float *window, int p,
                           float *out, int32_t *status, float *scratch);
void launch_narrow(hipStream_t s, const double *in, long count, float *out);

// k_mfcc.hip
bool mfcc_fits(int n, int nb);
struct mfcc_plan_t { bool ok; int n1, n2, nc, tm; };     // two-stage DFT geometry: n = n1*n2, nc = padded stage-1 columns
mfcc_plan_t mfcc_plan(int n, int nb);
void launch_mfcc_dft2(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                      const mfcc_plan_t &pl, const double *ctab /* [n1][nc] */, const double *twid /* [n][2] */,
                      const int32_t *bins_dev, const double *slopes, const double *dct_table, int num_coeffs, double *out,
                      long out_ld /* doubles per output row */, int32_t *status /* set to 0 per frame, or NULL */, int nb, int cu_count);
// k_mfcc_mfma.hip: both DFT stages on the matrix cores
struct mfcc_mplan_t { bool ok; int n1, n2, k2, mt, ntd, ntm, src0, src1; };
mfcc_mplan_t mfcc_mfma_plan(int n, int b_lo, int nb);
void launch_mfcc_mfma(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                      const mfcc_mplan_t &pl, const double *ctab, const double *twd, const double *twm, const double *wm,
                      const int32_t *bins_dev, const double *slopes, const double *dct_table, int num_coeffs, double *out,
                      long out_ld /* doubles per output row */, int32_t *status /* set to 0 per frame, or NULL */, int nb, int cu_count);
void launch_mfcc(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                 const double *kappa_sigma /* [nb][2] Goertzel-Reinsch constants */, const int32_t *bins /* K+2 */,
                 const double *slopes /* [nb][2] */, const double *dct_table /* [K][K] */,
                 int num_coeffs, double *out, long out_ld, int32_t *status, int nb /* bins[K+1]-bins[0] */);
// k_mfcc_czt.hip: the needed bins of the n-point DFT by the chirp-z identity on the power-of-two FFT (any n with
// n + top - 1 <= 4096: frame lengths that are not a transform's and do not divide one; longer ones up to 4096 samples split
// into two blocks of n1 samples whose complex results add up, n1 + top - 1 <= 4096)
int mfcc_czt_plan(int n, int top /* b_lo + nb */);              // SPECTRAL_PLAN_1024 / _2048 / _4096, or SPECTRAL_PLAN_NONE
int mfcc_czt_split_plan(int n, int top, int *n1);               // the same for a frame split in two (n1 = samples per block)
// n1 <= 0 or >= n: one block, h_bhat [2 L]; else ceil(n / n1) blocks, h_bhat [blocks][2 L]
void mfcc_czt_fill_tabs(int n, int top, int L, int n1, double *h_chirp /* [2 n] */, double *h_bhat);
void launch_mfcc_czt(hipStream_t s, int plan, const double *x, long F, int n, int n1, long stride, const double *window,
                     const double *tab /* the plan's twiddles */, const double *chirp, const double *bhat, const int32_t *bins,
                     const double *slopes, const double *dct, int num_coeffs, int nb, double *out, long out_ld, int32_t *status,
                     double *cw_scratch /* [blocks][2 L] */);
void launch_fill_rows(hipStream_t s, double *out, long rows, int n, long ld, double value, int32_t *status, int32_t code);
void launch_dct_rows(hipStream_t s, const double *in, long rows, int n, const double *dct_table, double *out);

// k_front.hip
void launch_resample(hipStream_t s, const double *x, long F, int n, long stride, const int32_t *tab_idx,
                     const double *tab_frac, int m, double *out);
void launch_ring_frames(hipStream_t s, const double *ring, long capacity, long head, long F, int n, long stride, double *out);
void launch_pcm16(hipStream_t s, const int16_t *pcm, size_t n, double denom, double *out);
// max |x| per frame of any sample type: the f64 launch_frame_peak (k_pitch_path.hip) on the widened samples, bit for bit (PCM: an
// integer max widened once by s / 32767; float32: taken in float and widened once, NaNs ignored as there)
void launch_frame_peak(hipStream_t s, frames_t x, long F, long n, long stride, double *out);
void launch_rms(hipStream_t s, const double *x, long F, int n, long stride, const double *window, double *out);
void launch_preemphasis(hipStream_t s, const double *x, long F, int n, long stride, double c, double *out);

// k_reader.hip: channel `channel` of n interleaved sample frames of `channels` samples each, as the type the frame loop reads natively
// (format = VBX_SAMPLE_* of the C header: out is int16 for PCM16, float for F32, double for PCM24 / PCM32 / F64; PCM24 / PCM32 are
// divided by 8388607 / 2147483647 with IEEE division).  A PCM24 source may sit at any byte address, the others need their type's.
// One byte per sample (any byte address): U8 -> double, (b - 128) / 127 with IEEE division; ULAW / ALAW -> int16, the G.711 expansion
// (vbx_sample8.hpp), which the PCM16 kernels then read as any 16-bit sample.
enum { UNPACK_PCM16 = 1, UNPACK_PCM24 = 2, UNPACK_PCM32 = 3, UNPACK_F32 = 4, UNPACK_F64 = 5, UNPACK_U8 = 16, UNPACK_ULAW = 17, UNPACK_ALAW = 18 };
void launch_unpack(hipStream_t s, int format, const void *src, size_t n, size_t channels, size_t channel, void *out);
// the same for n_sel selected channels in ONE pass over the interleaved frames (vbx_unpack_channels): plane k = channel sel.ch[k], n
// elements from element k * plane_ld of out, bit for bit what launch_unpack writes for that channel.  The selection travels as a
// kernel argument (UNPACK_MAX_SEL == VBX_HOST_MAX_CHANNELS).  channels == 1 is launch_unpack itself.
#define UNPACK_MAX_SEL 64
struct unpack_sel_t { int32_t ch[UNPACK_MAX_SEL]; };
void launch_unpack_all(hipStream_t s, int format, const void *src, size_t n, size_t channels, const unpack_sel_t &sel, size_t n_sel,
                       void *out, size_t plane_ld);
// vbx_analyze_host: rows [row0, row0 + rows) x columns [c0, c1) of a chunk's records and of its [3, src_n] status rows into the caller's
// (dst, dst_st point at the chunk's first own row / column; dst_st may be null)
void launch_host_rows(hipStream_t s, const double *src, size_t src_ld, size_t row0, size_t rows, size_t c0, size_t c1, double *dst,
                      size_t dst_ld, const int32_t *src_st, size_t src_n, int32_t *dst_st, size_t dst_n);

// k_session.hip: the two launches a live session's push puts around the frame loop (vbx_session_push).
// ingest: out[0, keep) = old[drop, drop + keep) (the format's output type), out[keep, keep + n_new) = what launch_unpack writes for
// channel `channel` of the n_new interleaved sample frames at raw, bit for bit.  old and out must not overlap.
void launch_session_ingest(hipStream_t s, int format, const void *old, size_t drop, size_t keep, const void *raw, size_t n_new,
                           size_t channels, size_t channel, void *out);
// deliver: rows [row0, row0 + rows) of the chunk-local buffers into the caller's rows [0, rows) -- the records' columns [c0, c1),
// the [3, src_n] status rows to dst_st + k * dst_st_ld, the tracked form's lists (kmax entries a row), counts and peaks -- and the
// n_state formant doubles (columns 2 ...) of the last of those rows into state.  Null destinations are skipped; rows >= 1.
struct session_deliver_t {
    const double *src; size_t src_ld, row0, rows, c0, c1; double *dst; size_t dst_ld;
    const int32_t *src_st; size_t src_n; int32_t *dst_st; size_t dst_st_ld;
    const double *src_cand; double *dst_cand; size_t kmax;
    const int32_t *src_count; int32_t *dst_count;
    const double *src_peak; double *dst_peak;
    double *state; size_t n_state;
};
void launch_session_deliver(hipStream_t s, const session_deliver_t &d);

// k_session_channels.hip: the same two launches for EVERY selected channel of a multi-channel session (vbx_session_push_channels).
// ingest_all: plane p of out (out_ld elements apart) = old plane p (old_ld apart) from element drop, keep elements, then channel
// sel.ch[p] of the n_new interleaved sample frames at raw -- per plane, bit for bit, what launch_session_ingest writes.  The block is
// read from memory once (tiles of whole sample frames through LDS); keep + n_new <= out_ld; old and out must not overlap.
void launch_session_ingest_all(hipStream_t s, int format, const void *old, size_t old_ld, size_t drop, size_t keep, const void *raw,
                               size_t n_new, size_t channels, const unpack_sel_t &sel, size_t n_sel, void *out, size_t out_ld);
// deliver_all: channel k's rows [k * plane_frames + row0, ... + rows) of the chunk-local buffers into ch[k]'s arrays, and the formant
// columns of its last row into state + k * 2 * VBX_FORMANT_SLOTS_K.  The destinations travel as kernel arguments.
struct session_deliver_all_t {
    const double *src; size_t src_ld, plane_frames, row0, rows, c0, c1, dst_ld;
    const int32_t *src_st; size_t src_n, dst_st_ld;
    const double *src_cand; size_t kmax;
    const int32_t *src_count;
    const double *src_peak;
    double *state; size_t n_state;
    struct { double *rec; int32_t *st; double *cand; int32_t *count; double *peak; } ch[UNPACK_MAX_SEL];
};
void launch_session_deliver_all(hipStream_t s, const session_deliver_all_t &d, size_t n_sel);
// k_clips.hip: the two launches vbx_analyze_clips puts around a group's frame-loop call.  One table entry per clip WITH frames, in
// order: off (= plane_frame * stride) and row_start ascend.
struct clip_entry_t {
    const void *src;                                      // the clip's samples (device), its format's alignment
    uint64_t len, off;                                    // samples; the plane element its sample 0 goes to
    int64_t plane_frame, row_start, n_rows;               // its first frame in the plane; its rows in the caller's arrays
};
// pack: plane[0, total) (the format's output type, launch_unpack's bits) = every clip's samples at its off, zeros between a clip's
// end and the next clip's off; tab[0].off == 0, total > tab[n - 1].off, and the last clip has at least total - off samples.  Every
// element is written once; no sample past a clip's len is read.
void launch_clips_pack(hipStream_t s, int format, const clip_entry_t *tab, size_t n, size_t total, void *plane);
// k_sample8.hip: the 8-bit formats (U8 / ULAW / ALAW) of the two kernel templates that k_session_channels.hip and k_clips.hip
// instantiate for the other five (vbx_session_ingest_all.hpp, vbx_clips_pack.hpp); launch_session_ingest_all and launch_clips_pack
// hand these formats on to them, so callers see one launcher each.
void launch_session_ingest_all8(hipStream_t s, int format, const void *old, size_t old_ld, size_t drop, size_t keep, const void *raw,
                                size_t n_new, size_t channels, const unpack_sel_t &sel, size_t n_sel, void *out, size_t out_ld);
void launch_clips_pack8(hipStream_t s, int format, const clip_entry_t *tab, size_t n, size_t total, void *plane);
// deliver: rows [plane_frame_b, + n_rows_b) of the group's staging into rows [row_start_b, ...) of the destinations (which point at
// row 0 of the caller's arrays): the records' columns [c0, c1), the three status rows (src: [3, src_n]; dst_st[q] may be null), the
// lists (kmax entries a row), counts and peaks where the destination is non-null.  rows = the group's delivered rows, from row0 on.
struct clips_deliver_t {
    const clip_entry_t *tab; size_t n, row0, rows;
    const double *src; size_t src_ld, c0, c1; double *dst; size_t dst_ld;
    const int32_t *src_st; size_t src_n; int32_t *dst_st[3];
    const double *src_cand; double *dst_cand; size_t kmax;
    const int32_t *src_count; int32_t *dst_count;
    const double *src_peak; double *dst_peak;
};
void launch_clips_deliver(hipStream_t s, const clips_deliver_t &d);

// k_tracker.hip: launch_tracker_stitch for n_sel channels in ONE launch (a block per channel): channel k's rows
// [k * plane_frames + first, k * plane_frames + stop) continued from state + k * 2 * VBX_FORMANT_SLOTS_K
void launch_tracker_stitch_all(hipStream_t s, const res_t *res, long F, int n_res, const int32_t *res_count, int n_est,
                               const int32_t *frame_status, res_t *out, long out_ld, long plane_frames, long first, long stop,
                               const double *state, long n_sel);

// k_pool.hip: the launches a session pool's tick (vbx_pool_push) puts around its one frame-loop call.  One table entry per pushed
// block of at least one sample, in the tick's order: off, row_start and carry_g0 ascend.  A sample of the slot's stream is named
// by its position relative to `consumed`, the first sample of the block: negative positions lie in the old tail.
struct pool_entry_t {
    const void *src;                                      // the block (device), its format's alignment: n_new samples
    const void *old;                                      // the slot's carried tail (the plane's type): old_len elements, the last one at position -1
    void *carry;                                          // the slot's OTHER carry buffer: the new tail goes here
    uint64_t n_new, old_len;
    uint64_t off, span;                                   // the entry's plane region: elements [off, off + span); span 0: no frame (off: the next region's)
    int64_t first;                                        // position of the region's element 0 (read_from - consumed)
    uint64_t carry_g0, carry_len;                         // the new tail: carry_len elements, its first 16-byte group in the launch's carry space
    int64_t carry_first;                                  // position of the new tail's element 0 (keep_from - consumed)
    int64_t plane_frame, frames, warm;                    // the entry's segment: frames [plane_frame, plane_frame + frames), the first `warm` not delivered
    int64_t row_start, n_rows;                            // its rows in the caller's arrays (n_rows = frames - warm; 0: none)
    int32_t slot, continues_prev;                         // the stream slot (its state row); the tracker continues from that row
    uint64_t pad;                                         // (144 bytes: the blocks uploaded behind the table start on a 16-byte boundary)
};
// ingest: plane[0, total) (the format's output type, launch_unpack's bits) = every entry's region, zeros between a region's end and
// the next entry's off; and every entry's new tail into its carry.  carry_groups: the 16-byte groups of all the tails.  Every
// element is written once; nothing before an old tail's element 0, past its old_len or past a block's n_new is read.
void launch_pool_ingest(hipStream_t s, int format, const pool_entry_t *tab, size_t n, size_t total, void *plane, size_t carry_groups);
// deliver: clips_deliver's scheme from the pool's table -- rows [plane_frame + warm, + n_rows) of the call's staging into rows
// [row_start, ...) of the destinations -- and the n_state formant doubles (columns 2 ...) of every delivering entry's last row into
// state + slot * 2 * VBX_FORMANT_SLOTS_K.  dst_st: the three status rows' bases (null: none).
struct pool_deliver_t {
    const pool_entry_t *tab; size_t n, rows;
    const double *src; size_t src_ld, c0, c1; double *dst; size_t dst_ld;
    const int32_t *src_st; size_t src_n; int32_t *dst_st[3];
    const double *src_cand; double *dst_cand; size_t kmax;
    const int32_t *src_count; int32_t *dst_count;
    const double *src_peak; double *dst_peak;
    double *state; size_t n_state;
};
void launch_pool_deliver(hipStream_t s, const pool_deliver_t &d);
// k_tracker.hip: launch_tracker_stitch for every entry of a pool's tick in ONE launch, a lane per entry: an entry with
// continues_prev has its rows [plane_frame + warm, plane_frame + frames) continued from state + slot * 2 * VBX_FORMANT_SLOTS_K
void launch_tracker_stitch_pool(hipStream_t s, const res_t *res, long F, int n_res, const int32_t *res_count, int n_est,
                                const int32_t *frame_status, res_t *out, long out_ld, const pool_entry_t *tab, long n_entries,
                                const double *state);

// k_front_ex.hip: RMS::rms of the rectangular frame (launch_rms with a null window, bit for bit) of any sample type, written at
// out_rms + f * rms_ld; out_peak non-null: launch_frame_peak from the same read
void launch_frame_rms(hipStream_t s, frames_t x, long F, int n, long stride, double *out_rms, long rms_ld, double *out_peak);

// k_front_f32in.hip: the widening pass of float32 samples (launch_pcm16's counterpart)
void launch_f32_to_f64(hipStream_t s, const float *x, size_t n, double *out);

// ---- the seam between translation units: the forms of ONE sample type of the launchers above that take a frames_t --------------
// ONLY those launchers call these.  Each frames_t launcher switches on x.kind -- nobody else does -- and is defined beside the float32
// instantiations (k_burg_f32in.hip, k_burg_lags_f32in.hip, k_front_f32in.hip, k_lists_f32in.hip); every instantiation stays in the
// unit of its kernel.  (launch_frame_peak on const double *, k_pitch_path.hip, is also vbx_frame_peak_f64 itself.)
// k_burg.hip, k_burg_fast.hip, k_burg_resampled.hip, k_front.hip, k_front_ex.hip, k_pitch.hip, k_lpc_exact.hip, k_lpc_ref.hip: the f64 and PCM forms
void launch_burg(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                 int p, double *out, int32_t *status, frame_map_t map = frame_map_t{0, 0, 0});
void launch_burg_pcm16(hipStream_t s, const int16_t *x, long F, int n, long stride, const double *window,
                       int p, double *out, int32_t *status, frame_map_t map = frame_map_t{0, 0, 0});
void launch_burg_list(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                      int p, double *out, int32_t *status, const int32_t *list, const int32_t *count);
void launch_burg_pcm16_list(hipStream_t s, const int16_t *x, long F, int n, long stride, const double *window,
                            int p, double *out, int32_t *status, const int32_t *list, const int32_t *count);
void launch_burg_lags(hipStream_t s, const double *x, long F, int n, long stride, const double *window, int p,
                      frame_map_t map, long i0, long m, void *ws);
void launch_burg_lags_pcm16(hipStream_t s, const int16_t *x, long F, int n, long stride, const double *window, int p,
                            frame_map_t map, long i0, long m, void *ws);
// (x, or pcm if non-null)
void launch_burg_resampled(hipStream_t s, const double *x, const int16_t *pcm, long F, int m, long stride, const double *window,
                           resample_src_t rs, int p, double *out, int32_t *status, frame_map_t map);
void launch_burg_resampled_list(hipStream_t s, const double *x, const int16_t *pcm, long F, int m, long stride, const double *window,
                                resample_src_t rs, int p, double *out, int32_t *status, const int32_t *list, const int32_t *count);
void launch_burg_lags_resampled(hipStream_t s, const double *x, const int16_t *pcm, long F, int m, long stride, const double *window,
                                resample_src_t rs, int p, frame_map_t map, long i0, long n_items, void *ws);
void launch_pitch_list(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int grid,
                       const double *x, int n, long stride, const double *window,
                       const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                       int kmax, pitch_t *out_cand, long cand_ld, int32_t *out_count, int32_t *status,
                       unsigned long long *work, bool pcm /* x points to int16 PCM samples */);
void launch_lpc_exact_list(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int cus, const double *x, int n,
                           long stride, const double *window, bool pcm /* x points to int16 PCM samples */, int p, double *out_lpc, long lpc_ld);
void launch_lpc_ref(hipStream_t s, const void *x, bool pcm /* x is 16-bit PCM */, long F, int n, long stride, const double *window, int n_lags,
                    int p, int normalize, double *out_r, long r_ld, double *out_lpc, long lpc_ld);
void launch_frame_peak_pcm16(hipStream_t s, const int16_t *pcm, long F, long n, long stride, double *out);
void launch_frame_rms(hipStream_t s, const double *x, const int16_t *pcm /* instead of x, if non-null */, long F, int n, long stride,
                      double *out_rms, long rms_ld, double *out_peak);
// k_front_f32in.hip, k_burg_f32in.hip, k_burg_lags_f32in*.hip, k_lists_f32in.hip (and k_spectral_f32in.hip, declared in vbx_spectral.hpp):
// the kernels above that read a frame's samples, on FLOAT32 samples (vbx_analyze_frames_ex_f32in).  Each widens a sample in registers
// before its first use -- every float is a double, so the frame is the one launch_f32_to_f64 would have written and every result
// is the f64 launcher's on that copy, bit for bit; windows, tables and results stay f64.
// max |x| per frame taken in float and widened once: launch_frame_peak on the widened samples (NaNs ignored, as there)
void launch_frame_peak_f32in(hipStream_t s, const float *x, long F, long n, long stride, double *out);
void launch_frame_rms_f32in(hipStream_t s, const float *x, long F, int n, long stride, double *out_rms, long rms_ld, double *out_peak);
void launch_pitch_list_f32in(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int grid,
                             const float *x, int n, long stride, const double *window,
                             const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                             int kmax, pitch_t *out_cand, long cand_ld, int32_t *out_count, int32_t *status,
                             unsigned long long *work);
void launch_lpc_exact_list_f32in(hipStream_t s, const int32_t *frame_list, const int32_t *list_count, int cus, const float *x, int n,
                                 long stride, const double *window, int p, double *out_lpc, long lpc_ld);
void launch_lpc_ref_f32in(hipStream_t s, const float *x, long F, int n, long stride, const double *window, int n_lags, int p,
                          int normalize, double *out_r, long r_ld, double *out_lpc, long lpc_ld);
void launch_burg_f32in(hipStream_t s, const float *x, long F, int n, long stride, const double *window,
                       int p, double *out, int32_t *status, frame_map_t map = frame_map_t{0, 0, 0});
void launch_burg_f32in_list(hipStream_t s, const float *x, long F, int n, long stride, const double *window,
                            int p, double *out, int32_t *status, const int32_t *list, const int32_t *count);
// the two lag launchers: false when the order has no float instantiation (nothing launched)
bool launch_burg_lags_f32in(hipStream_t s, const float *x, long F, int n, long stride, const double *window, int p,
                            frame_map_t map, long i0, long m, void *ws);
void launch_burg_resampled_f32in(hipStream_t s, const float *x, long F, int m, long stride, const double *window,
                                 resample_src_t rs, int p, double *out, int32_t *status, frame_map_t map);
void launch_burg_resampled_f32in_list(hipStream_t s, const float *x, long F, int m, long stride, const double *window,
                                      resample_src_t rs, int p, double *out, int32_t *status, const int32_t *list, const int32_t *count);
bool launch_burg_lags_resampled_f32in(hipStream_t s, const float *x, long F, int m, long stride, const double *window,
                                      resample_src_t rs, int p, frame_map_t map, long i0, long n_items, void *ws);

// k_long.hip: frames of more than VBX_MAX_FRAME_LEN_K samples (tiles out of HBM / L2 instead of registers / LDS)
size_t burg_long_scratch_bytes(long frames, long n);
void launch_burg_long(hipStream_t s, const double *x, long f0, long f1, long F, long n, long stride, const double *window,
                      int p, double *out, int32_t *status, double *ws /* burg_long_scratch_bytes(f1 - f0, n) */);
size_t autocorr_long_scratch_bytes(long F, long n, long n_lags);
void launch_autocorr_long(hipStream_t s, const double *x, long F, long n, long stride, const double *window, long n_lags,
                          double *out, double *ws);
size_t pitch_long_scratch_bytes(long F, long n);
double *pitch_long_r(void *ws);                                  // [F][n]: the caller fills it with the NORMALISED lag sums of every frame
void launch_pitch_long(hipStream_t s, long F, long n, const double *lag_window, double sample_rate, double threshold, double fmin,
                       double fmax, int kmax, double *out_cand, long cand_ld, int32_t *out_count, int32_t *status, void *ws);
size_t mfcc_long_scratch_bytes(long F, int nb);
void launch_mfcc_long(hipStream_t s, const double *x, long F, long n, long stride, const double *window, const double *kappa_sigma,
                      const int32_t *bins, const double *slopes, const double *dct, int num_coeffs, int nb, double *out, long out_ld,
                      int32_t *status, double *ws);
size_t preemphasis_long_scratch_bytes(long F, long n);
void launch_preemphasis_long(hipStream_t s, const double *x, long F, long n, long stride, double c, double *out, double *ws);

// k_synth.hip
void launch_synth(hipStream_t s, double *out, size_t n_samples, uint64_t sample_offset, double sample_rate, uint64_t seed);

// k_selftest.hip
void launch_selftest(hipStream_t s, double *out /* 64*8 */);

// k_pitch_path.hip: max |x| per frame, and the pitch path over vbx_pitch_f64's candidate lists (speculative chunks + exact repair)
void launch_frame_peak(hipStream_t s, const double *x, long F, long n, long stride, double *out);
struct pp_chunk_t { long f0, f1, s0, seg; int32_t last, pad; };   // frames [f0, f1) of segment seg (which starts at s0); host-built
struct pp_par_t {
    const pitch_t *cand; const int32_t *count; const int32_t *status; const double *lpk; const double *spk;
    long F; int kmax; int use_u;                                  // use_u: u_t reads local_peak / P (else u_t = voicing_threshold)
    double vt, oc, cj, cvu, Lc, q;                                // the host constants of the definition
    const pp_chunk_t *ch; long nch;
    uint8_t *psi;                                                 // [F][G]
    double *entry, *exitd, *want;                                 // [nch][G]
    int32_t *exact, *redo;                                        // [nch]
    unsigned long long *mask;                                     // [ceil(nch / 64)]
    int32_t *lead;                                                // [n_segments]: the leader of each segment's last frame
    unsigned long long *redone;                                   // chunks redone by the repair rounds and the sweep
};
void launch_pitch_path_peak(hipStream_t s, const pp_par_t &P, const int64_t *seg_chunk0, long nseg, double *cpk);
void launch_pitch_path_spec(hipStream_t s, const pp_par_t &P, int G, long W);
void launch_pitch_path_check(hipStream_t s, const pp_par_t &P, int G);
void launch_pitch_path_repair(hipStream_t s, const pp_par_t &P, int G);
void launch_pitch_path_mask(hipStream_t s, const pp_par_t &P);
void launch_pitch_path_sweep(hipStream_t s, const pp_par_t &P, int G, const int64_t *seg_chunk0, long nseg);
void launch_pitch_path_map(hipStream_t s, const pp_par_t &P, int G, uint8_t *map);
void launch_pitch_path_compose(hipStream_t s, long nch, int G, const uint8_t *in, uint8_t *out, long d);
void launch_pitch_path_write(hipStream_t s, const pp_par_t &P, int G, const uint8_t *map, pitch_t *out_path,
                             long ld /* doubles from one out_path row to the next: 2 = dense */, int32_t *out_index);
// the shard hand-off (vbx_pitch_path_shard_*): chunks [c0, c1) are the rest of the utterance that is entered at chunk c0
void launch_pitch_path_enter(hipStream_t s, const pp_par_t &P, int G, long c0, long c1, const double *state_in /* 64 */, int32_t *changed);
void launch_pitch_path_open_map(hipStream_t s, uint8_t *map, long c, int G);
void launch_pitch_path_export(hipStream_t s, const double *src /* ns or NULL */, int ns, const uint8_t *map /* G or NULL */, int G,
                              double *state_out /* 64 or NULL */, int32_t *back_map /* 64 or NULL */);
void launch_pitch_path_select(hipStream_t s, const uint8_t *map, long c0, long nch, int G, const int32_t *end_state, uint8_t *sel);

// the online path (vbx_path_stream_*): what one stream carries from push to push, and its ring of max_pending frames.  Frame g
// (counted since open / reset) lives in slot g % cap while it is pending; a slot holds, per state, psi and the row and index a
// commit of that state writes -- the caller's lists are not read again behind the push that scanned them.
struct pp_online_state_t {
    double D[64], lf[64];                                         // {D, log2 f} of the last frame scanned
    unsigned long long vmask;                                     // ... its voiced states
    int32_t n, pad;                                               // ... and how many states it has
    int64_t scanned, committed, utt;                              // frames since open / reset: scanned, committed; utt: 0 = the next frame starts an utterance
};
struct pp_commit_t { int64_t first, n, n_forced, pending; };      // vbx_path_commit
struct pp_online_t {
    pp_online_state_t *st;
    uint8_t *psi; pitch_t *row; int8_t *idx;                      // the ring: [cap][G] each
    long cap;                                                     // max_pending (<= 2^24)
    int end;                                                      // end_utterance
    double peak;                                                  // P = peak_ref of the silence term
    pitch_t *out_path; long ld; int32_t *out_index; uint8_t *out_forced;
    pp_commit_t *commit;
};
// P: cand / count / status / lpk of the push's F frames, kmax, use_u and the constants; nothing else is read (spk: O.peak)
void launch_pitch_path_online(hipStream_t s, const pp_par_t &P, int G, const pp_online_t &O);
// k_pitch_path_channels.hip: the same scan for the n_sel channels of a bound multi-channel session in ONE launch, a block per
// channel.  P: the lists of channel 0's first frame (channel k's rows lie k * plane_frames rows further on), F frames per channel;
// O: cap, end, peak and ld (its pointers are not read); ch[k]: channel k's stream allocation (pp_online_state_t, then the ring at
// off_row / off_psi / off_idx bytes) and where its rows and its commit go.  (64 channels: UNPACK_MAX_SEL, defined above.)
struct pp_online_ch_t { void *mem; pitch_t *out_path; int32_t *out_index; uint8_t *out_forced; pp_commit_t *commit; };
struct pp_online_all_t { long plane_frames; size_t off_row, off_psi, off_idx; pp_online_ch_t ch[64]; };
void launch_pitch_path_online_all(hipStream_t s, const pp_par_t &P, int G, const pp_online_t &O, const pp_online_all_t &A, int n_sel);
// k_pitch_path_pool.hip: the same scan for every visited slot of a bound session pool's tick in ONE launch, a block per row of the
// tick's path table (any number of rows: the table is device memory, uploaded with the tick's entry table).  Row k: the slot, its
// frames' rows [row0, row0 + frames) of the lists P names (row 0 of the tick's frame-loop call; frames 0: none are read), and the
// slot's deferred flags: RESET zeroes the slot's state first; MARK then ends the slot's utterance (a push of no frames with
// end_utterance) before the frames are scanned as a new one, the rows of both following each other and the commits merged.
// O: cap, peak and ld (its pointers and end are not read); slot s's allocation (pp_online_state_t, then the ring at off_row / off_psi
// / off_idx bytes, vbx_path_stream_open's layout) lies at mem + s * slot_bytes, its rows at row s * slot_rows of out_path (ld doubles
// apart), out_index and out_forced (either may be null), its merged commit at commit[s].
enum : int32_t { PP_POOL_RESET = 1, PP_POOL_MARK = 2 };
struct pp_pool_row_t { int32_t slot, flags; int64_t row0, frames; };
struct pp_online_pool_t {
    const pp_pool_row_t *tab;
    char *mem; size_t slot_bytes, off_row, off_psi, off_idx;
    pitch_t *out_path; int32_t *out_index; uint8_t *out_forced; pp_commit_t *commit; long slot_rows;
};
void launch_pitch_path_online_pool(hipStream_t s, const pp_par_t &P, int G, const pp_online_t &O, const pp_online_pool_t &A, long n_rows);

}  // namespace vbx
