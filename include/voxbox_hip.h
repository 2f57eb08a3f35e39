/*
 * voxbox_hip.h -- C ABI of libvoxbox_hip.so: batched, MI355X-native (gfx950)
 * replacement for the per-frame DSP hot path of the Rust crate vox_box 0.3.0.
 *
 * The reference exposes this path as extension traits on slices, called once
 * per frame from a user loop (examples/pitch_detection.rs:23-30,
 * tests/lib.rs:71-83).  It has no FFI of its own, so these
 * entry points ARE what a Rust/cgo/ctypes binding of the path would bind:
 * one call = the user's whole frame loop (F frames).  Each declaration cites
 * the reference interface it replaces (file:line under /root/reference).
 *
 * Conventions
 *  - plain pointers and sizes only; every data pointer is a DEVICE pointer
 *    unless the parameter name starts with `h_` (host).  vbx_malloc/vbx_memcpy_*
 *    are provided so a caller needs no HIP binding of its own; pointers from
 *    hipMalloc / torch tensors (.data_ptr()) are equally valid.
 *  - a frame batch is (x, n_frames, frame_len, stride, window): frame t is
 *    x[t*stride .. t*stride+frame_len) -- stride == frame_len is the dense
 *    [F, N] batch, stride == hop is the Windower view into contiguous audio
 *    (sample 0.10 Windower: frame t exists while frame_len <= remaining).
 *    `window` (device, frame_len doubles, or NULL) is multiplied onto the
 *    samples on load: the batched form of window::Windower::hanning, whose
 *    frames the reference's traits receive already windowed.
 *  - all arithmetic is f64 ("Sample = f64" instantiation of the traits).  The f32 instantiation (vbx_*_f32: float
 *    frames in, float results out; vbx_*_c32: Complex<f32> Polynomial) widens on load, computes in f64 and rounds
 *    each result to f32 once -- except the Complex<f32> root finder, which follows the reference's f32 arithmetic
 *    step by step because its iteration counts and root ORDER depend on it.
 *  - calls are asynchronous on the context's HIP stream; vbx_sync() waits.  Stream order is the whole contract: a call reads
 *    its device inputs and writes its device outputs in the order of the context's stream, so a producer queued on that stream
 *    before the call and a consumer queued on it after the call need no host wait (the streams and events the library uses
 *    inside are joined into the context's stream before the call returns; tests/test_gpu_stream_order.py).  HOST arrays
 *    (h_ parameters) are read before the call returns.  The host is blocked only by: the first call of a shape (its tables are
 *    built and its workspaces grown, which drains the context's streams); a call whose h_seg_start, h_est_init or pitch path
 *    chunk table differs from the previous call's WHILE that previous call's upload of it is still queued (it waits until the
 *    upload has left the pinned staging buffer, i.e. for the work queued ahead of it -- a first change behind idle uploads and
 *    identical content do not wait; tests/test_gpu_stream_order.py test_host_blocks_only_as_documented); vbx_analyze_host, until
 *    the last byte of its h_audio has been read (its uploads wait for the chunks queued ahead of them); and the calls that
 *    return a value to the host: vbx_sync, vbx_memcpy_h2d / _d2h, vbx_free, vbx_timer_end, vbx_profile_enable / _reset / _get /
 *    _stream / _names / _pitch_work, vbx_internal_last_*_count, vbx_internal_last_path_chunks_redone.
 *  - a context (stream, cached tables, scratch) is not internally synchronised: one host thread per context at
 *    a time.  Contexts are independent of each other and cheap; use one per thread / stream.
 *  - return value: 0 ok, <0 API misuse / runtime failure (vbx_last_error()).
 *    Per-frame conditions that make the reference return Err or panic are
 *    reported in an int32 status[F] array (codes below) so one bad frame never
 *    aborts a batch; outputs of such a frame are zero-filled and tracker state
 *    passes through unchanged (src/lib.rs:75 `?`).
 *  - there is NO CPU fallback: without a HIP device vbx_ctx_create fails.
 */
#ifndef VOXBOX_HIP_H
#define VOXBOX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBX_ABI_VERSION 5

/* API return codes */
#define VBX_SUCCESS 0
#define VBX_E_INVALID (-1)      /* null pointer / bad size / unsupported shape */
#define VBX_E_RUNTIME (-2)      /* HIP runtime error */
#define VBX_E_NODEVICE (-3)     /* no usable gfx950 device */

/* per-frame status codes (VoxBoxError, src/error.rs:4-16, and the panics of the path) */
#define VBX_FRAME_OK 0
#define VBX_FRAME_ERR_LPC 1         /* Err(LPC("Denum was <= 0.0")), src/spectrum.rs:123-125 */
#define VBX_FRAME_ERR_POLYNOMIAL 2  /* Err(Polynomial(..)), src/polynomial.rs:95,123 */
#define VBX_FRAME_ERR_NAN 3         /* partial_cmp().unwrap() on NaN, src/periodic.rs:453 */
#define VBX_FRAME_ERR_PANIC 4       /* any other panic of the reference (index out of bounds, assert) */

#define VBX_MAX_RESONANCES 32       /* MAX_RESONANCES, src/lib.rs:26 */
#define VBX_FORMANT_SLOTS 6         /* FormantSlots, src/spectrum.rs:228 */
#define VBX_MAX_LPC_ORDER 62        /* order of lpc / lpc_praat / find_formants: its at most order / 2 resonances fit the reference's
                                       MAX_RESONANCES, its polynomial (order + 1 coefficients) the root finder's VBX_MAX_POLY_LEN */
#define VBX_MAX_POLY_LEN 64         /* coefficients of a polynomial of vbx_find_roots_* / vbx_laguerre_* / vbx_div_polynomial_* */
#define VBX_MAX_FRAME_LEN 4096      /* frames up to here live in registers / LDS (the fast kernels); the f32 instantiation
                                       (vbx_*_f32, vbx_*_f32_wide) takes no longer ones */
#define VBX_MAX_LONG_FRAME_LEN 67108864 /* 2^26: every f64 frame-batch entry point takes frames up to this length -- the reference's
                                       slices have no cap (tests/lib.rs:27-41 passes a 31,232-sample file as ONE frame of
                                       find_formants).  Beyond VBX_MAX_FRAME_LEN the kernels walk the frame in tiles out of HBM
                                       (k_long.hip): exact, but built for a whole recording per frame, not for millions of them;
                                       vbx_pitch_f64 keeps the frame's 2 * frame_len lag curve in HBM and needs frame_len < 2^30,
                                       and takes kmax up to VBX_PITCH_MAX_CANDIDATES(frame_len) there */
#define VBX_MAX_PITCH_CANDIDATES 1026 /* kmax upper bound of vbx_pitch_f64: frame_len/4 strict local maxima in
                                        [0, frame_len/2) + the unvoiced candidate, at VBX_MAX_FRAME_LEN */
/* the whole Vec of a frame never has more than this many entries (out_count <= vbx_pitch_max_candidates) */
#define VBX_PITCH_MAX_CANDIDATES(frame_len) ((frame_len) / 4 + 2)

typedef struct vbx_ctx vbx_ctx;

/* #[repr(C)] Resonance<f64>, src/spectrum.rs:149-154 */
typedef struct { double frequency; double bandwidth; } vbx_resonance;
/* Pitch<f64>, src/periodic.rs:306-310 */
typedef struct { double frequency; double strength; } vbx_pitch;
/* num::Complex<f64> (repr(C): re, im) */
typedef struct { double re; double im; } vbx_complex;

/* MALE/FEMALE_FORMANT_ESTIMATES, src/lib.rs:27-28 */
extern const double VBX_MALE_FORMANT_ESTIMATES[4];
extern const double VBX_FEMALE_FORMANT_ESTIMATES[4];

/* ------------------------------------------------------------------ context */

int vbx_abi_version(void);
/* device: HIP device ordinal.  hip_stream: a hipStream_t to launch on (e.g. a torch.cuda.Stream's handle), or NULL to let
 * the context create and own one.  NULL ALWAYS means "own stream" (non-blocking: not ordered with the null stream either) --
 * it never means the runtime's default stream.  Any non-NULL handle is used as given, the runtime's special handles
 * (hipStreamLegacy, hipStreamPerThread; hip_runtime_api.h) included -- but those are the runtime's business: on ROCm 7.2 a
 * process whose context ran on hipStreamLegacy died with a segmentation fault, so pass a stream the caller created.  PyTorch
 * reports its default stream's handle as 0, so `torch.cuda.current_stream().cuda_stream` must not be passed on blindly:
 * VoxBox.from_torch (vox_box.rs_amd/voxbox.py) refuses it with an error that asks for a torch.cuda.Stream to be made current
 * (INTEGRATION.md section 3). */
int vbx_ctx_create(vbx_ctx **out, int device, void *hip_stream);
void vbx_ctx_destroy(vbx_ctx *ctx);
int vbx_sync(vbx_ctx *ctx);
const char *vbx_last_error(const vbx_ctx *ctx); /* ctx may be NULL: last global error */
/* device name (e.g. "gfx950:sramecc+:xnack-"), CU count; any pointer may be NULL */
int vbx_device_info(const vbx_ctx *ctx, char *h_name, size_t name_cap, int *h_cu_count);

/* device memory helpers (synchronous w.r.t. the host for memcpy) */
int vbx_malloc(vbx_ctx *ctx, void **out_dptr, size_t bytes);
int vbx_free(vbx_ctx *ctx, void *dptr);
int vbx_memcpy_h2d(vbx_ctx *ctx, void *dst, const void *h_src, size_t bytes);
int vbx_memcpy_d2h(vbx_ctx *ctx, void *h_dst, const void *src, size_t bytes);
int vbx_memset(vbx_ctx *ctx, void *dst, int value, size_t bytes);

/* HIP-event timing on the context's stream (bench.py's roofline leg).
 * vbx_timer_begin/end bracket a region; *h_ms is valid after the call returns. */
int vbx_timer_begin(vbx_ctx *ctx);
int vbx_timer_end(vbx_ctx *ctx, float *h_ms);
/* Per-kernel event profile: when enabled every kernel launch is bracketed by
 * events; vbx_profile_get sums them by kernel name (synchronises the stream). */
int vbx_profile_enable(vbx_ctx *ctx, int on);
int vbx_profile_reset(vbx_ctx *ctx);
int vbx_profile_get(vbx_ctx *ctx, const char *kernel_name, double *h_total_ms, long *h_launches);
/* ABI 5.  The stream the kernel's last profiled launch ran on: 0 = the context's stream (the critical path of a call),
 * 1 = the side stream of the fused frame loop (the formant chain / an unfused MFCC beside the spectral kernel),
 * 2 = the tracker's time-slice stream; -1 = not profiled.  Event times of kernels on streams 1 and 2 include the time
 * they spend co-resident with the context stream's kernel: a bench must not call them "dominant" by that number. */
int vbx_profile_stream(vbx_ctx *ctx, const char *kernel_name, int *h_stream);
/* Work the pitch refine kernel executed while profiling was enabled (since the last
 * vbx_profile_reset): h_out4 = { frames, candidates found, sinc evaluations, sinc terms }.
 * Feeds bench.py's FP64 roofline with the work actually done, not the reference's. */
int vbx_profile_pitch_work(vbx_ctx *ctx, uint64_t *h_out4);
/* names of profiled kernels, '\n'-separated, into h_buf */
int vbx_profile_names(vbx_ctx *ctx, char *h_buf, size_t cap);

/* ------------------------------------------------------------------ tables (host) */

/* sample 0.10 window tables, built on the host with the reference's recurrences.
 *  VBX_WINDOW_HANNING          Window::<Hanning>::new(n): phase accumulated by 1/(n-1), % 1.0
 *                              (Windower::hanning, examples/pitch_detection.rs:23)
 *  VBX_WINDOW_HANNING_LAG      HanningLag::at_phase over the same phases (src/periodic.rs:236-248,:400)
 *  VBX_WINDOW_HANNING_PERIODIC Hanning::at_phase(idx/len) (src/lib.rs:66-70)
 *  VBX_WINDOW_RECTANGLE        all ones (Windower::rectangle, tests/lib.rs:71) */
#define VBX_WINDOW_HANNING 0
#define VBX_WINDOW_HANNING_LAG 1
#define VBX_WINDOW_HANNING_PERIODIC 2
#define VBX_WINDOW_RECTANGLE 3
int vbx_window_table_f64(int kind, size_t n, double *h_out);
/* number of Windower frames: (n_samples - frame_len)/hop + 1 while frame_len <= remaining */
size_t vbx_frame_count(size_t n_samples, size_t frame_len, size_t hop);

/* hz_to_mel / mel_to_hz, src/spectrum.rs:375-381 (host scalars) */
double vbx_hz_to_mel(double hz);
double vbx_mel_to_hz(double mel);
/* find_formants_real_work_size / _complex_work_size, src/lib.rs:30-36.  The library owns
 * its workspaces; these exist so ported callers that size buffers keep compiling. */
size_t vbx_find_formants_real_work_size(size_t buf_len, size_t n_coeffs);
size_t vbx_find_formants_complex_work_size(size_t n_coeffs);

/* ------------------------------------------------------------------ periodic.rs */

/* Autocorrelate::autocorrelate(n_lags) per frame (src/periodic.rs:265-289), including the
 * fold seed quirk r[lag] = x[0] + sum_{i>=1} x[i]*x[i+lag].  out: [F, n_lags]. */
int vbx_autocorrelate_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len,
                          size_t stride, const double *window, size_t n_lags, double *out);

/* Normalize::normalize on each row (src/waves.rs:60-76): row *= 1/max|row|.  data: [F, n] in place. */
int vbx_normalize_f64(vbx_ctx *ctx, double *data, size_t n_rows, size_t n);

/* interpolate_sinc (src/periodic.rs:29-87) of one lag curve y[ylen] at M query points.
 * status[M] (optional) receives VBX_FRAME_ERR_PANIC where the reference would index out of bounds. */
int vbx_interpolate_sinc_f64(vbx_ctx *ctx, const double *y, size_t ylen, long offset, size_t nx,
                             const double *xs, size_t m, size_t max_depth, double *out, int32_t *status);

/* improve_extremum(.., Interpolation::Sinc(depth), is_max = true) (src/periodic.rs:192-229)
 * at M starting points; out_xy: [M, 2] = (xmid, ymid). */
int vbx_improve_extremum_f64(vbx_ctx *ctx, const double *y, size_t ylen, long offset, size_t nx,
                             const double *ixmid, size_t m, size_t depth, double *out_xy, int32_t *status);
/* improve_extremum with every arm of `Interpolation` (src/periodic.rs:89-93,192-229) and the is_max flag: NONE returns
 * (0, y[0]) (:197-199), PARABOLIC the three-point fit around floor(ixmid) (:200-207; status PANIC where the reference indexes
 * out of bounds), SINC(depth) the Brent search of the interpolant -- negated by the closure when is_max == 0 (:219-222).
 * Only SINC with is_max != 0 is on the pitch path; the rest is the crate's public surface. */
#define VBX_INTERP_NONE 0
#define VBX_INTERP_PARABOLIC 1
#define VBX_INTERP_SINC 2
int vbx_improve_extremum_ex_f64(vbx_ctx *ctx, const double *y, size_t ylen, long offset, size_t nx,
                                const double *ixmid, size_t m, int interpolation, size_t depth, int is_max,
                                double *out_xy, int32_t *status);

/* Pitched::pitch::<Hanning>(sample_rate, threshold, _, _, min, max) per frame
 * (src/periodic.rs:356-358,396-455; local_peak/global_peak are unused by the reference).
 * out_cand: [F, kmax] candidates, stable-sorted by descending strength exactly as the
 * reference's Vec (entries past count are zero); out_count[F] = full candidate count
 * (may exceed kmax).  PitchExtractor (src/periodic.rs:337-353) output = out_cand[f*kmax + 0].
 * Only the kmax entries that are returned are guaranteed to have been refined: a candidate whose strength
 * is provably below the kmax-th best is skipped (exact -- the returned entries, the count and the status
 * are the reference's; DESIGN.md "exact top-k pruning").  kmax = 1 is the fast path.
 * The WHOLE Vec of every frame (src/periodic.rs:452-454 returns all of it) is retrievable: either
 * kmax = VBX_PITCH_MAX_CANDIDATES(frame_len), which no frame can exceed, or the two-call protocol -- a first call
 * with kmax = 1 yields out_count[F], a second call with kmax = max(out_count) returns every entry.  kmax > 64
 * switches the kernel from its lane-resident list to an LDS-resident one (nothing is pruned, every candidate is
 * refined as in the reference; slower).
 * Bit identity across kmax: the lists returned for kmax in {1, 2, 3} are bit for bit the head of one another, and so are
 * the lists for every kmax >= 4 (from 4 on, few-candidate frames refine four candidates at a time, which changes the last
 * bits of a candidate's sinc sums); between the two classes a candidate agrees to ~1e-7 relative in Hz.
 * Which shapes are fast (one MI355X, kmax = 1, frames/s; the table in DESIGN.md section 4 is kept current): 512..1024 samples
 * 44-56 M, 1025..1200 39-42 M, 1201..2048 29 M, 2049..4096 16-17 M (that range runs its refinement in kernels of its
 * own, with the lag curves in a context-owned scratch buffer between them: <= 2.3 GB, 4.4 GB at an odd length),
 * below 512 samples the direct lag sums on the matrix cores 50-70 M.  kmax 2 / 8 / 64 / whole Vec at 1200: 13.5 / 6.5 / 3.25 / 2.7 M.
 * Alignment: x, window and out_cand need 8 bytes (what C gives an array of double / vbx_pitch), out_count and status 4; 16-byte
 * aligned frames and windows take the kernels' 16-byte loads, anything else their element-wise ones, with the same results bit for
 * bit (tests/test_gpu_layouts.py).  That holds for every frame-batch entry point of this header unless its comment says otherwise. */
int vbx_pitch_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                  const double *window, double sample_rate, double threshold, double fmin, double fmax,
                  size_t kmax, vbx_pitch *out_cand, int32_t *out_count, int32_t *status);

/* Boersma's (1993) pitch candidates with an UNQUANTISED lag (ABI 5, added): the algorithm the crate's comment describes
 * (src/periodic.rs:382-395: "Second pass maximizes the function more accurately using ... sinc interpolation and the Brent ...
 * maximization") and its code misses -- SURVEY Appendix A, Q5 (a sign slip in the parabola), Q6 (interpolate_sinc's left and right
 * sample indices swapped) and Q8 (brent_maximize minimises, the closure does not negate) together put every refined candidate of
 * vbx_pitch_f64 on the INTEGER lag next to the peak: up to half a lag, 1.1e-3 .. 1.5e-3 relative in the speech range.  This call
 * undoes the three and nothing else; vbx_pitch_f64 still returns the crate's rows.  Arguments, layouts, alignment rules and the
 * asynchronous stream contract are vbx_pitch_f64's; out_cand [F, kmax], out_count [F] and status [F] (may be NULL) are what
 * vbx_pitch_path_f64 and vbx_path_stream_push take.
 * Definition (the contract; IEEE binary64; N = frame_len, H = floor(N / 2); tests/pitch_boersma_model.py is its executable form):
 *   1 curve      y[0 .. N) is Pitched::pitch's curve, unchanged (src/periodic.rs:400-411): the autocorrelation with the Q1 seed,
 *                normalised by the largest |r| over all lags (Q2), divided by the accumulated-phase lag window (Q3).
 *   2 peaks      strict local maxima y[k-1] < y[k] > y[k+1], 1 <= k < H - 1, in ascending k (Q4, unchanged).
 *   3 lag        dr = 0.5 (y[k+1] - y[k-1]), d2r = 2 y[k] - y[k-1] - y[k+1], x0 = k + dr / d2r, f0 = sample_rate / x0; the peak is
 *                kept iff fmin < f0 < fmax.  (d2r > 0 and |dr / d2r| < 0.5 at a strict maximum; a peak whose computed
 *                |dr / d2r| exceeds 1 -- cancellation in d2r between neighbours an ulp apart -- is dropped.)
 *   4 S_depth(x) plain lag coordinates.  x < 0 gives y[0] (:40).  nl = floor(x), nr = nl + 1, phil = x - nl, phir = 1 - phil;
 *                |x - nl| < 1e-10 gives y[nl], |x - nr| < 1e-10 gives y[nr] (:41-42); otherwise, with D = min(depth, nl),
 *                  S = sum_{n=0..D-1} y[nl - n] sinc(pi (phil + n)) (0.5 + 0.5 cos(pi (phil + n) / (phil + D)))
 *                    + sum_{n=0..D-1} y[nr + n] sinc(pi (phir + n)) (0.5 + 0.5 cos(pi (phir + n) / (phir + D))),  sinc(a) = sin(a) / a:
 *                the reference's sum with each side reading its own samples.  The reference's term n = D of either side has the
 *                taper 0.5 + 0.5 cos(pi) = 0 and is left out, so that the curve's last lag -- whose lag window is 0 or a rounding
 *                residue, y[N-1] = 0/0 or x[0]/1e-17 -- cannot turn a sum into NaN.  No index is below 0 or above 2 nl <= N.
 *   5 first pass s1 = S_30(x0), reflected: s1 > 1 becomes 1 / s1 (the reference's dead :433-435, live).  The unvoiced entry
 *                (0, threshold) has s1 = threshold.
 *   6 selection  Praat's rule.  L = the kept peaks in ascending k, then the unvoiced entry; out_count = len(L); m = min(kmax,
 *                out_count); the m entries of L with the largest s1 are kept (a tie goes to the earlier position; a NaN s1 ranks
 *                above every number), in L-order.
 *   7 refinement for each kept voiced entry, brent_maximize's iteration (src/periodic.rs:103-188: the same golden constant, tol =
 *                1e-10, sqrt(EPSILON) term, at most 60 iterations) on -S_1200 over [x0 - 1, x0 + 1] gives xmid;
 *                frequency = sample_rate / xmid, strength = S_1200(xmid), reflected if it exceeds 1.
 *   8 order      stable sort of the kept entries by descending strength (:453); entries past m are zero.
 *   9 kmax       for kmax >= out_count the row is the frame's whole list and does not change with kmax (bit for bit among kmax
 *                1..3 and among kmax >= 4; from 4 on four entries are refined at a time, 16 lanes each, which changes the last
 *                bits of the sums: between the two classes an entry agrees to ~1e-7 relative in Hz).  For a smaller kmax the
 *                rows are NOT prefixes of one another: selection is by the first-pass s1, the order by the refined strength.
 *  10 status     VBX_FRAME_ERR_NAN with a zero row and count 0 only where a selected entry's s1 or final strength is NaN.  A
 *                frame in which no comparison succeeds -- all zeros (the curve is NaN throughout), a NaN or Inf sample -- returns the
 *                unvoiced entry alone with VBX_FRAME_OK and count 1, and so does any frame without a peak in range.
 *                vbx_pitch_f64 reports the same status and count for such frames (tests/test_gpu_pitch_boersma.py).
 * 16 <= frame_len <= 4096 and 1 <= kmax <= 63 (the path's cap).  VBX_E_INVALID, before a byte is written: anything else, a
 * non-finite or non-positive sample_rate, fmin >= fmax (or either NaN), NULL x, out_cand or out_count, stride 0.  n_frames == 0
 * succeeds.  The results carry the kernel's rounding, not the model's: frequencies agree with the model to ~1e-7 relative and
 * strengths to ~1e-12 (Brent stops within 2 tol_act ~ 1e-5 lags of a stationary point, where S is flat); two runs are bit-identical.
 * The fused frame loops (vbx_analyze_frames* and everything built on them), PCM / float input, frames beyond 4096 samples and an
 * f32 instantiation are not covered: a caller composes these lists with vbx_frame_peak_f64 and vbx_pitch_path_f64
 * (examples/pitch_boersma.c).  Cost: DESIGN.md section 5n. */
int vbx_pitch_boersma_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                          const double *window, double sample_rate, double threshold, double fmin, double fmax,
                          size_t kmax, vbx_pitch *out_cand, int32_t *out_count, int32_t *status);

/* The pitch PATH (added in ABI 5): the "third pass" of src/periodic.rs:394-395 -- "a path through these candidates that maximizes
 * both the smoothness of the pitch contour and the strength of the pitches" -- which PitchExtractor::new(candidates,
 * voiced_unvoiced_cost, voicing_threshold) (src/periodic.rs:320-354) takes the parameters of but never runs (its iterator
 * returns candidates[t][0]).  Boersma's (1993) path cost over the lists vbx_pitch_f64 writes, one path per segment.
 * Definition (the contract; IEEE binary64, round to nearest, in exactly this order, no fused multiply-add):
 *   host constants  corr = 0.01 / time_step, cvu = voiced_unvoiced_cost * corr, cj = octave_jump_cost * corr,
 *                   Lc = log2(ceiling_hz), q = silence_threshold / (1 + voicing_threshold)
 *   states of t     the first m_t = min(count[t], kmax) entries of the frame's row, in list order; if none of them has
 *                   frequency 0, one unvoiced state is appended (reported as index -1).  A frame whose status is not
 *                   VBX_FRAME_OK has only that unvoiced state.  A state is voiced iff its frequency is > 0.
 *   lambda_t(s)     voiced (f, a): a - octave_cost * (Lc - log2 f);  unvoiced: u_t = voicing_threshold + max(0, 2 - rho_t / q),
 *                   rho_t = local_peak[t] / P (P = the largest local_peak of the frame's segment; rho = 0 when P == 0) -- the use
 *                   the crate's unused local_peak / global_peak arguments of Pitched::pitch (src/periodic.rs:356-358) point at;
 *                   u_t = voicing_threshold when local_peak is NULL or silence_threshold == 0
 *   c(p -> s)       both unvoiced 0; exactly one voiced cvu; both voiced cj * |log2 f_p - log2 f_s|
 *   recursion       e_0 = lambda_0, D_0 = e_0 - max e_0; for t >= 1: a(s) = max_p (D_{t-1}(p) - c(p -> s)), psi_t(s) = the first
 *                   p in state order attaining it, e_t(s) = a(s) + lambda_t(s), D_t(s) = e_t(s) - max_s' e_t(s')
 *   path            ends in the first state with D_{T-1} = 0, traced back through psi.
 * out_path[t] = the chosen list entry for a voiced state, {0.0, u_t} for an unvoiced one; out_index[t] (optional) = the chosen
 * state's list position, -1 for the appended unvoiced state.  cand / count / status are what vbx_pitch_f64 writes with the same
 * kmax (1 <= kmax <= 63: at most 64 states); status may be NULL (every frame OK); h_seg_start / n_segments follow
 * vbx_analyze_frames_f64 (NULL = one utterance).  The scan runs in speculative chunks with exact repair: the result is the
 * sequential scan's, bit for bit, for any chunk_frames (DESIGN.md "Pitch path").  Asynchronous on the context's stream.
 * VBX_E_INVALID: kmax 0 or > 63, a negative or non-finite parameter, time_step <= 0, ceiling_hz <= 0, silence_threshold > 0
 * with a NULL local_peak, a bad segment list.
 * PitchExtractor::new's arguments map onto voiced_unvoiced_cost and voicing_threshold; the rest default to Praat's "To Pitch (ac)"
 * values: silence 0.03, voicing 0.45, octave 0.01, octave-jump 0.35, voiced/unvoiced 0.14, ceiling 600 Hz. */
typedef struct {
    double voicing_threshold, silence_threshold, octave_cost, octave_jump_cost, voiced_unvoiced_cost;
    double ceiling_hz, time_step;   /* time_step = hop / sample_rate, seconds */
    size_t chunk_frames;            /* 0: the library's choice; >= n_frames: one sequential scan per segment */
} vbx_pitch_path_params;
/* max |x| per frame of the batch (no window), NaN samples ignored (an all-NaN frame gives NaN): the local_peak of the path.
 * out_peak: [F]. */
int vbx_frame_peak_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                       double *out_peak);
int vbx_pitch_path_f64(vbx_ctx *ctx, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                       size_t n_frames, size_t kmax, const double *local_peak,
                       const int64_t *h_seg_start, size_t n_segments, const vbx_pitch_path_params *h_params,
                       vbx_pitch *out_path, int32_t *out_index);
/* chunks the repair rounds and the final sweep of the last vbx_pitch_path_f64 call redid (synchronises the stream); -1 if the
 * context's last frame-batch or path call was not a path call */
int vbx_internal_last_path_chunks_redone(vbx_ctx *ctx, int64_t *h_out);

/* ------------------------------------------------------------------ spectrum.rs: LPC */

/* LPC::lpc(n_coeffs) on autocorrelation rows (Levinson-Durbin, src/spectrum.rs:63-92).
 * r: [F, r_stride] with r_stride >= n_coeffs+1; out: [F, n_coeffs+1] = [1, a1..ap].  The recursion runs in the source's order;
 * only under VBX_LPC_POLICY_REFERENCE (below) is it the crate's operation for operation (otherwise multiply-adds may be fused). */
int vbx_lpc_f64(vbx_ctx *ctx, const double *r, size_t n_frames, size_t r_stride,
                size_t n_coeffs, double *out);
/* LPC::lpc_mut(n_coeffs, ac, kc, tmp) (src/spectrum.rs:62-84): as vbx_lpc_f64, and out_kc: [F, n_coeffs]
 * (optional) receives the reflection coefficients the reference leaves in `kc` (`tmp` is scratch there). */
int vbx_lpc_mut_f64(vbx_ctx *ctx, const double *r, size_t n_frames, size_t r_stride,
                    size_t n_coeffs, double *out_ac, double *out_kc);

/* frame.autocorrelate(n_coeffs+1) [-> .normalize()] -> .lpc(n_coeffs) fused, one pass over the
 * samples (LPCSolver usage, src/spectrum.rs:40-42,470-479).  out_r: [F, n_coeffs+1] (after the
 * optional normalize), out_lpc: [F, n_coeffs+1]; either may be NULL.
 * Ill-conditioned rows (round 6; also the LPC column of vbx_analyze_frames_f64): every row's conditioning is probed -- the
 * recursion repeated on lag sums moved by +-16 eps of r[0] -- and a row such a perturbation moves by more than 1e-6 in the parity
 * metric is recomputed from the frame's samples with the lag sums and the recursion in double-double: the exact row of the f64
 * frame, rounded once, where the reference's own f64 row (src/periodic.rs:284 + src/spectrum.rs:63-84) is 1e-6 .. 3e-4 from it
 * (frame_len <= 4096, n_coeffs <= 31; VBX_LPC_EXACT=0 turns it off).  That is the default policy; a caller that
 * must return the crate's own rows bit for bit sets VBX_LPC_POLICY_REFERENCE (below): then neither probe nor redo runs. */
int vbx_autocorr_lpc_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len,
                         size_t stride, const double *window, size_t n_coeffs, int normalize,
                         double *out_r, double *out_lpc);

/* Which LPC rows a context computes from frames (ABI 5, added): a per-context setting, read by vbx_autocorrelate_f64,
 * vbx_autocorr_lpc_f64, vbx_lpc_f64 / vbx_lpc_mut_f64 and the LPC column of vbx_analyze_frames_f64 / _pcm16.
 *  VBX_LPC_POLICY_EXACT     (default) the probe above + the double-double redo of the rows it lists: within 1e-6 of the EXACT row
 *  VBX_LPC_POLICY_PLAIN     no probe, no redo: the rows of rounds 1-5 (what VBX_LPC_EXACT=0 gives) -- neither exact nor the crate's
 *  VBX_LPC_POLICY_REFERENCE the crate's own f64 arithmetic, BIT FOR BIT: every lag sum the sequential fold of src/periodic.rs:276-289
 *                           (seeded with x[0], each product rounded before the add), [normalize as src/waves.rs:60-76,] the recursion
 *                           of src/spectrum.rs:63-84, no contraction -- at every frame length and order these entry points accept.
 *                           The other columns of an analyze record are unchanged.  Costs the lag sums' FFT / matrix-core forms
 *                           (DESIGN.md section 1 has the measured rates).
 * The initial value comes from the environment: VBX_LPC_EXACT=0 gives PLAIN, anything else EXACT; set overrides it.
 * set: VBX_E_INVALID for an unknown value. */
#define VBX_LPC_POLICY_EXACT 0
#define VBX_LPC_POLICY_PLAIN 1
#define VBX_LPC_POLICY_REFERENCE 2
int vbx_ctx_set_lpc_policy(vbx_ctx *ctx, int policy);
int vbx_ctx_get_lpc_policy(const vbx_ctx *ctx, int *h_policy);

/* LPC::lpc_praat(n_coeffs) per frame (Burg, src/spectrum.rs:94-146).  out: [F, n_coeffs]
 * (no leading 1, sign-flipped as the reference); status[F]: VBX_FRAME_ERR_LPC when denum <= 0.
 * Orders 8, 10, 12, 13, 14, 16 on frames of 256..2048 samples (also inside vbx_find_formants_f64 and vbx_analyze_frames_*): one pass over
 * the frame -- its p + 1 lag sums and first / last p + 1 samples, then an O(p^2) recursion per frame that yields the reference's
 * reflection coefficients (csrc/k_burg_fast.hip).  That recursion is exact in real arithmetic but amplifies the lag sums'
 * rounding by the frame's conditioning, so the kernel bounds its own error per frame: a row is written only if the bound
 * is inside 5e-7 in the parity metric |d| <= 1e-6 max(|a_j|, 1e-6 max|a|); every other frame is computed by the reference's
 * own per-order sums, as all frames of every other order and length are.  HOW MANY frames that is depends on the material:
 * ~1 % of the bench's synthetic 48 kHz signal at order 12; 40 % of a real 44.1 kHz recording at order 13 (68 % without a
 * -70 dB dither: oversampled speech has almost no energy above 8 kHz, its covariance matrix is ill conditioned, and there the
 * one-pass recursion's error is real -- 14 % of such frames are off by more than 1e-7, 5 % by more than 5e-7,
 * tools/experiments/burg_guard_vs_error.py); every pure tone / DC / silent / NaN frame.  The results are the direct
 * recursion's either way; the cost is its speed on those frames (about 4x the one-pass form's instructions per frame;
 * bench.py --signal speech: the pipeline on such a recording runs within 4 % of what the same material would without it).
 * Environment: VBX_BURG_DIRECT=1 (read per call) takes the per-order sums for every frame. */
int vbx_lpc_burg_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len,
                     size_t stride, const double *window, size_t n_coeffs, double *out, int32_t *status);

/* ------------------------------------------------------------------ polynomial.rs */

/* Polynomial::find_roots_mut on F polynomials of `len` coefficients (coefficient of x^j at
 * index j), src/polynomial.rs:92-152: Laguerre from -2-2i with deflation, quadratic/linear
 * tail; roots are written in discovery order, remainder zeroed.  polys: [F, len] in/out. */
int vbx_find_roots_c64(vbx_ctx *ctx, vbx_complex *polys, size_t n_polys, size_t len, int32_t *status);

/* Polynomial::laguerre(start) (src/polynomial.rs:34-72) on F polynomials; out: [F]. */
int vbx_laguerre_c64(vbx_ctx *ctx, const vbx_complex *polys, size_t n_polys, size_t len,
                     vbx_complex start, vbx_complex *out);

/* Polynomial::div_polynomial_mut (src/polynomial.rs:155-195) on F polynomials: polys[f] / (x + others[f]);
 * the quotient is left in polys, rem: [F, len] receives the remainder exactly as the reference leaves it.
 * status: VBX_FRAME_ERR_POLYNOMIAL where others[f] == 0 ("Tried to divide by zero"). */
int vbx_div_polynomial_c64(vbx_ctx *ctx, vbx_complex *polys, const vbx_complex *others, size_t n_polys, size_t len,
                           vbx_complex *rem, int32_t *status);
/* Polynomial::degree / off_low (src/polynomial.rs:26-32) of one HOST polynomial (trivial scans, no device work) */
size_t vbx_degree_c64(const vbx_complex *h_poly, size_t len);
size_t vbx_off_low_c64(const vbx_complex *h_poly, size_t len);

/* The f32 instantiation of Polynomial (Complex<f32>, exercised by the reference's own tests at
 * src/polynomial.rs:336-386): same algorithms in single precision.  polys: [F, len] of {float re, im}. */
typedef struct { float re, im; } vbx_complex32;
int vbx_find_roots_c32(vbx_ctx *ctx, vbx_complex32 *polys, size_t n_polys, size_t len, int32_t *status);
int vbx_laguerre_c32(vbx_ctx *ctx, const vbx_complex32 *polys, size_t n_polys, size_t len,
                     vbx_complex32 start, vbx_complex32 *out);

/* ------------------------------------------------------------------ spectrum.rs: resonances, tracker */

/* ToResonance::to_resonance(sample_rate) per row of roots (src/spectrum.rs:165-210): roots with
 * im >= 0, reflected inside the unit circle, 50 Hz < f < nyquist-50, sorted by frequency.
 * roots: [F, n_roots]; out_res: [F, n_roots] zero padded; out_count[F]. */
int vbx_to_resonance_c64(vbx_ctx *ctx, const vbx_complex *roots, size_t n_rows, size_t n_roots,
                         double sample_rate, vbx_resonance *out_res, int32_t *out_count);

/* EstimateFormants::estimate_formants carried frame to frame = FormantExtractor
 * (src/spectrum.rs:216-369).  The scan is sequential in the reference (the caller passes the
 * previous frame's estimates back in, tests/lib.rs:75-79); here utterances of 384 frames or more are
 * scanned in parallel chunks with exact repair (bit-identical rows, about a millisecond for any batch:
 * utterance length is not a cost).  It is batched per utterance:
 * h_seg_start[n_segments] (HOST array) are the ascending frame indices at which the caller's
 * state is reset to est_init (h_seg_start[0] must be 0; NULL/0 = one segment).  res: [F, n_res]
 * resonance rows exactly as the reference passes them (zero padded); frame_status (optional):
 * frames with status != 0 leave the state untouched.  out: [F, n_est] estimates after each frame.
 * Alignment: res and out need 8 bytes (an array of vbx_resonance), frame_status 4. */
int vbx_estimate_formants_f64(vbx_ctx *ctx, const vbx_resonance *res, size_t n_frames, size_t n_res,
                              const int64_t *h_seg_start, size_t n_segments,
                              const vbx_resonance *h_est_init, size_t n_est,
                              const int32_t *frame_status, vbx_resonance *out);

/* vox_box::find_formants(buf, sample_rate, 1.0, .., n_coeffs, .., formants) over F frames
 * (src/lib.rs:40-116): periodic Hanning -> Burg -> reversed complex polynomial -> find_roots_mut
 * -> Resonance::from_root (im > 0) -> sort -> estimate_formants.  `window` must be NULL for
 * rectangular input frames as in tests/lib.rs:71 (the periodic Hanning is applied inside).
 * out_formants: [F, n_est]; out_res (optional): [F, 32] zero padded; out_res_count (optional): [F];
 * out_coeffs (optional): [F, n_coeffs] Burg coefficients; status[F].
 * At the orders 8, 10, 12, 13, 14, 16 the resonance rows come from converged roots of the real polynomial found pair by
 * pair (csrc/k_roots_fast.hip: one Laguerre solve per conjugate pair, deflation by the real quadratic, a Newton step on the
 * original polynomial as polish and check) instead of a replay of find_roots_mut's iteration: the reference runs that
 * iteration to convergence too (20 steps per root) and sorts the result by frequency, so the rows agree to ~1e-10 relative
 * (gate 1e-4; counts and statuses equal).  A frame that fails the check is redone by the reference's own iteration, as
 * every frame of the other orders is.  Environment: VBX_ROOTS_DIRECT=1 (read per call) replays the reference's
 * iteration for every frame; VBX_BURG_DIRECT=1 see vbx_lpc_burg_f64.
 * Alignment: out_formants and out_res need 8 bytes (arrays of vbx_resonance), out_res_count and status 4. */
int vbx_find_formants_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len,
                          size_t stride, double sample_rate, size_t n_coeffs,
                          const int64_t *h_seg_start, size_t n_segments,
                          const vbx_resonance *h_est_init, size_t n_est,
                          vbx_resonance *out_formants, vbx_resonance *out_res, int32_t *out_res_count,
                          double *out_coeffs, int32_t *status);

/* ------------------------------------------------------------------ spectrum.rs: MFCC */

/* MFCC::mfcc(num_coeffs, (lo, hi), sample_rate) per frame (src/spectrum.rs:401-441).
 * out: [F, num_coeffs]; status[F]: VBX_FRAME_ERR_PANIC when a mel bin exceeds the spectrum.
 * Which kernel runs depends on the frame length (results within 1e-6 of the reference's arithmetic in every case): a length
 * that is (half of) a transform's takes the fused kernels' forward transform; other lengths from 513 samples take that transform
 * of the zero-padded frame with the frame's DFT bins interpolated from it (vbx_analyze_frames_f64 below explains the
 * interpolation; design error < 1e-14 of the largest bin) where that is the fastest form, the matrix-core two-stage DFT where
 * the length factors suitably and is below 1400 samples, the chirp-z kernel where the filters reach above a quarter of the
 * sampling rate, Goertzel below 600 samples.  VBX_MFCC_INTERP=0 in the environment: no interpolated form anywhere. */
int vbx_mfcc_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                 const double *window, size_t num_coeffs, double lo_hz, double hi_hz,
                 double sample_rate, double *out, int32_t *status);
/* The mel filter bank's bins for that call, on the host: h_bins[num_coeffs + 2] = floor((frame_len + 1) * hz / sample_rate)
 * at num_coeffs + 2 mel-spaced points (src/spectrum.rs:411-414; two points lie beyond hi_hz, and the scale is frame_len + 1:
 * Q14).  Returns 1 (not an error code) when the geometry makes the reference panic on every frame -- a bin beyond the
 * spectrum or descending bins -- which vbx_mfcc_f64 reports as VBX_FRAME_ERR_PANIC per frame. */
int vbx_mfcc_bins(size_t frame_len, size_t num_coeffs, double lo_hz, double hi_hz, double sample_rate, int32_t *h_bins);

/* dct (src/spectrum.rs:384-398) on rows: in/out [F, n]. */
int vbx_dct_f64(vbx_ctx *ctx, const double *in, size_t n_rows, size_t n, double *out);

/* ------------------------------------------------------------------ front end (N2, N3) */

/* 16-bit PCM -> f64 as the reference's tests read WAV data: sample / (i32::MAX >> (32 - bits)) = / 32767
 * (tests/lib.rs:17-19).  pcm: n int16 samples on the device; out: n doubles.  Framing is then the
 * (stride = hop) view of `out`: window::Windower::{rectangle,hanning} without copying frames. */
int vbx_pcm16_to_f64(vbx_ctx *ctx, const int16_t *pcm, size_t n_samples, double *out);

/* float samples -> f64, exactly (every float is a double: subnormals, -0.0, infinities and NaNs arrive as the same values): the
 * counterpart of vbx_pcm16_to_f64 for the float32 tensors that torchaudio / soundfile, float WAVs and model outputs hand over.
 * x: n float samples on the device (4-byte aligned); out: n doubles.  The fused frame loop does not need it: see
 * vbx_analyze_frames_ex_f32in. */
int vbx_f32_to_f64(vbx_ctx *ctx, const float *x, size_t n_samples, double *out);

/* RMS::rms per frame (src/waves.rs:10-23).  out: [F]. */
int vbx_rms_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                const double *window, double *out);

/* Filter::preemphasis(factor) per frame (src/waves.rs:82-96): x[i] += 2*pi*factor * x[i+1], backwards.
 * The reference filters in place; frames of a hop-strided view overlap, so the result is written to the
 * dense batch out: [F, frame_len] (out may equal x when stride == frame_len). */
int vbx_preemphasis_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                        double factor, double *out);

/* The resample front end of find_formants (resample_ratio != 1.0, src/lib.rs:42,57-61):
 * sample 0.10's Linear::new(buf[0], buf[1]) + Converter::scale_sample_hz(.., ratio), take(ceil(ratio*len)).
 * That arithmetic lives in the un-vendored `sample` crate and no reference test runs this branch, so this
 * entry point is "parity unpinned" (it is bit-identical to the oracle's restatement of the crate).
 * out: dense [F, vbx_resampled_len(frame_len, ratio)].  find_formants with a ratio is then
 * vbx_find_formants_f64 on that dense batch (frame_len = stride = resampled length). */
size_t vbx_resampled_len(size_t frame_len, double resample_ratio);
int vbx_resample_linear_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                            double resample_ratio, double *out);

/* VecDeque input (`impl Autocorrelate<T> for VecDeque<T>`, src/periodic.rs:291-304 -- the streaming form of the
 * trait): logical sample i of the deque is ring[(head + i) % capacity].  Copies the Windower view over the deque
 * (frame t = logical samples [t*stride, t*stride + frame_len)) into the dense batch out[F, frame_len], which every
 * entry point above accepts with stride = frame_len.  Requires (n_frames-1)*stride + frame_len <= capacity. */
int vbx_ring_frames_f64(vbx_ctx *ctx, const double *ring, size_t capacity, size_t head, size_t n_frames,
                        size_t frame_len, size_t stride, double *out);

/* ------------------------------------------------------------------ Sample = f32 (N4) */

/* The slice traits are generic over the Sample type: `impl<T: Sample> Autocorrelate<T> for [T]`
 * (src/periodic.rs:276-289), `impl<T: Float> LPC<T> for [T]` (src/spectrum.rs:56), `Normalize` (src/waves.rs:60-76),
 * `MFCC<T>` (src/spectrum.rs:401-409).  These are their f32 instantiation: the arguments mean what they mean in the
 * _f64 entry points with float in place of double (frames, windows, outputs).
 * Two forms of each.  The plain names are REFERENCE-FAITHFUL: every fold, product and quotient the generic code performs in
 * T runs in f32, in the reference's order, with no fused multiply-add (the lag sums of src/periodic.rs:284 as sequential
 * f32 folds, one lane per lag; Levinson and Burg as sequential f32 recursions, one lane per frame; Pitched<f32, f32>::pitch
 * with its lag curve built and normalised in f32 and T = f32 roundings of the candidates) -- the results are the bits
 * the crate returns at f32 (tests/test_gpu_f32.py: equal to the f32 restatement, which no reference test pins: parity
 * unpinned).  The *_f32_wide names widen on load, compute in f64 with the f64 kernels and round once: more accurate and as
 * fast as f64, but not those bits.  MFCC exists only in the wide form (rustfft's f32 arithmetic is not in the tree).
 * vbx_window_table_f32: the f64 table rounded to f32 (the sample crate's own f32 window path is not verifiable
 * here: parity unpinned). */
int vbx_window_table_f32(int kind, size_t n, float *h_out);
int vbx_autocorrelate_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                          size_t stride, const float *window, size_t n_lags, float *out);
int vbx_autocorrelate_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                          size_t stride, const float *window, size_t n_lags, float *out);
int vbx_normalize_f32(vbx_ctx *ctx, float *data, size_t n_rows, size_t n);
int vbx_lpc_mut_f32(vbx_ctx *ctx, const float *r, size_t n_frames, size_t r_stride,
                    size_t n_coeffs, float *out_ac, float *out_kc);
int vbx_lpc_mut_f32_wide(vbx_ctx *ctx, const float *r, size_t n_frames, size_t r_stride,
                    size_t n_coeffs, float *out_ac, float *out_kc);
int vbx_autocorr_lpc_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                         size_t stride, const float *window, size_t n_coeffs, int normalize,
                         float *out_r, float *out_lpc);
int vbx_autocorr_lpc_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                         size_t stride, const float *window, size_t n_coeffs, int normalize,
                         float *out_r, float *out_lpc);
int vbx_lpc_burg_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                     size_t stride, const float *window, size_t n_coeffs, float *out, int32_t *status);
int vbx_lpc_burg_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len,
                     size_t stride, const float *window, size_t n_coeffs, float *out, int32_t *status);
int vbx_mfcc_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                 const float *window, size_t num_coeffs, double lo_hz, double hi_hz,
                 double sample_rate, float *out, int32_t *status);
/* Pitched<f32, f32>::pitch (src/periodic.rs:356-358,396-455 at S = T = f32): as vbx_pitch_f64 with float frames, float
 * parameters and Pitch<f32> candidates.  The lag curve and the refinement run in f64 on the widened frame. */
typedef struct { float frequency; float strength; } vbx_pitch32;
int vbx_pitch_f32(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                  const float *window, float sample_rate, float threshold, float fmin, float fmax,
                  size_t kmax, vbx_pitch32 *out_cand, int32_t *out_count, int32_t *status);
int vbx_pitch_f32_wide(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                  const float *window, float sample_rate, float threshold, float fmin, float fmax,
                  size_t kmax, vbx_pitch32 *out_cand, int32_t *out_count, int32_t *status);

/* ------------------------------------------------------------------ the user's frame loop, fused */

/* What a user of the crate writes per frame (examples/pitch_detection.rs:23-30, tests/lib.rs:71-83,
 * examples/formant_extraction/src/main.rs:72-88), as ONE call over F frames of the Windower view:
 *   hanning frame -> pitch::<Hanning>(sr, threshold, _, _, fmin, fmax)[0]        (PitchExtractor output)
 *   hanning frame -> autocorrelate(lpc_order + 1) -> lpc(lpc_order)              (raw, un-normalised autocorrelation)
 *   rectangle frame -> find_formants(.., 1.0, .., formant_order, .., formants)   (state carried per segment)
 *   hanning frame -> mfcc(mfcc_coeffs, (lo, hi), sr)
 * Each part with order / count 0 is skipped.  The library is free to share work between the parts (one pass over
 * the samples, one spectral transform feeding several of them); results obey the same tolerances as the
 * separate entry points.  MFCC shares the pitch path's transform at EVERY frame length from 513 to 4096 samples: where the
 * length divides the transform's (512, 600, 800, 1024, 1200, 2048, 4096) the frame's DFT bins are bins of the transform; at
 * the other lengths (25 ms at 44.1 kHz = 1102 / 1103 samples, ...) each bin is interpolated from 24-40 of the transform's --
 * the frame fills at most half of it, so its spectrum is oversampled twofold and the interpolation's error is a design
 * parameter: < 1e-14 of the largest bin (tests/test_mfcc_interp_table.py), MFCC values within 1e-11 of the chirp-z kernel's exact arithmetic.
 * (Bins above a quarter of the transform -- mfcc_hi_hz beyond ~sample_rate / 4 at a length just below the transform's half --
 * fall back to vbx_mfcc_f64's kernel beside the fused one; VBX_MFCC_INTERP=0 in the environment forces that everywhere.)
 * Output: one record of vbx_record_doubles(params) doubles per frame,
 *   [ pitch.frequency, pitch.strength | formants[n_est] {frequency, bandwidth} | mfcc[mfcc_coeffs] | lpc[lpc_order + 1] ]
 * at out_records + f * record_ld (record_ld even, >= the record size; out_records 16-byte ALIGNED -- the one pointer of this
 * header that needs more than its type's alignment: a base at 8 mod 16 is rejected with VBX_E_INVALID, "records must be 16-byte
 * aligned", before anything is written; x and status3 need 8 / 4 bytes, pcm 2): the fixed-size
 * per-frame record that the multi-GPU gather below moves.  status3 (optional): [3, F] = pitch / formant / mfcc
 * status rows.  Asynchronous on the context's stream (a second, context-owned stream is used inside and joined). */
typedef struct {
    double sample_rate;
    double pitch_threshold, pitch_fmin, pitch_fmax;
    size_t lpc_order;
    size_t formant_order;
    size_t n_est;
    vbx_resonance est_init[VBX_FORMANT_SLOTS];
    size_t mfcc_coeffs;
    double mfcc_lo_hz, mfcc_hi_hz;
} vbx_analysis_params;
size_t vbx_record_doubles(const vbx_analysis_params *h_params);
int vbx_analyze_frames_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                           const vbx_analysis_params *h_params, const int64_t *h_seg_start, size_t n_segments,
                           double *out_records, size_t record_ld, int32_t *status3);

/* The same frame loop on 16-bit PCM: what a WAV reader hands the reference's callers before the `as f64 / 32767` of
 * tests/lib.rs:17-19 and examples/formant_extraction/src/main.rs.  `pcm` holds the recording's samples (device memory);
 * frame t is pcm[t*stride .. +frame_len), widened in registers exactly as vbx_pcm16_to_f64 would (s / 32767, correctly
 * rounded), so the records are BIT-IDENTICAL to vbx_pcm16_to_f64 followed by vbx_analyze_frames_f64 -- at a quarter of
 * the input bytes (960 instead of 3840 new bytes per 48 kHz / 10 ms frame): the form for host-fed operation, where the
 * samples cross PCIe.  Full 1200-sample frames with lpc_order in {0, 12} read the PCM directly; other shapes are widened
 * into a context-owned f64 copy of the view first. */
int vbx_analyze_frames_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                             const vbx_analysis_params *h_params, const int64_t *h_seg_start, size_t n_segments,
                             double *out_records, size_t record_ld, int32_t *status3);

/* The frame loop with the TRACKED pitch contour (added in ABI 5): vbx_analyze_frames_f64 / _pcm16 whose columns 0-1 hold
 * out_path[t] of vbx_pitch_path_f64 -- the chosen list entry for a voiced state, {0.0, u_t} for an unvoiced one -- instead of
 * candidates[0], from ONE call: the fused kernel runs at the caller's kmax and writes the frames' candidate lists (what
 * vbx_pitch_f64 writes at that kmax, to the fused kernels' ~1e-7), max |x| per frame (what vbx_frame_peak_f64 writes; on PCM an
 * integer max over the 16-bit samples, widened once: the same bits) is taken beside it on the context's second stream, and the
 * path runs behind both, once per segment of h_seg_start, writing straight into the records.  Every other column, all three
 * status rows, the record layout, the alignment rule for out_records and the state the call leaves (vbx_track_stitch_f64, the
 * LPC probe's count) are those of the plain call, bit for bit; vbx_internal_last_path_chunks_redone reports the path's count.
 * The samples are read once by the spectral pass and once by the peak kernel; no f64 copy of a PCM recording is needed by the
 * caller (shapes without a PCM kernel are widened into the context-owned copy, as in the plain call).
 * h_track->kmax: the list length the path runs over, 1..63 (vbx_pitch_f64 takes at least 1026 at every frame_len, so 1..63 is the
 * whole rule; frame_len itself must be one vbx_pitch_f64 takes: >= 4 samples);
 * h_track->path: as vbx_pitch_path_f64, except that time_step == 0 means stride / sample_rate.
 * h_outputs (optional device arrays; the struct pointer or any member may be NULL): the lists, counts, peaks and path indices,
 * so that vbx_pitch_path_f64 can be run again with other costs (1-2 ms per 4.5 M frames) without recomputing the lists.  Where a member
 * is NULL the library keeps that array in a context-owned workspace: at most F * (16 kmax + 16) bytes (lists, peaks, counts; the pitch
 * status row when status3 is NULL), plus the path's own workspace (F * G bytes of back-pointers, G = the power of two >= kmax + 1,
 * and a few hundred bytes per 256-frame chunk).  With silence_threshold == 0 and peak NULL no peak kernel runs.
 * VBX_E_INVALID, before anything is written and with the context left usable: a NULL h_track, kmax 0 or > 63, any path parameter
 * vbx_pitch_path_f64 rejects (other than time_step == 0), anything vbx_analyze_frames_f64 rejects.  n_frames == 0 succeeds.
 * Sharded runs (below): by this call alone the path is NOT carried across a shard cut -- a rank's contour is the path of the frames it
 * analysed.  vbx_pitch_path_shard_begin_f64 / _enter / _finish over the lists this call returns in h_outputs carry it: they turn
 * columns 0-1 into the rows of the whole recording's path, bit for bit ("The pitch path across a shard cut", below).
 * Measured (one MI355X, 4.5 M frames of 1200 / 480 at 48 kHz, all parts on): 9.5 M frames/s at kmax 4, 5.0 M at kmax 15 (f64 and PCM
 * alike), against 7.9 M / 4.5 M for vbx_analyze_frames_f64 + vbx_pitch_f64(kmax) + vbx_frame_peak_f64 + vbx_pitch_path_f64: the
 * call saves the kmax = 1 pitch pass, ~90-100 ms of those frames; the list at kmax is what remains. */
typedef struct {
    size_t kmax;                   /* list length the path runs over: 1..63 (below vbx_pitch_f64's own cap at every frame_len) */
    vbx_pitch_path_params path;    /* as vbx_pitch_path_f64; time_step == 0 here means stride / sample_rate */
} vbx_pitch_track_params;
typedef struct {                   /* optional device outputs; the struct pointer or any member may be NULL */
    vbx_pitch *cand;               /* [F, kmax]  the lists the path ran over (what vbx_pitch_f64 writes at this kmax) */
    int32_t   *count;              /* [F] */
    double    *peak;               /* [F]  local_peak (what vbx_frame_peak_f64 writes) */
    int32_t   *index;              /* [F]  out_index of vbx_pitch_path_f64 */
} vbx_pitch_track_outputs;
int vbx_analyze_frames_tracked_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                                   const vbx_analysis_params *h_params, const vbx_pitch_track_params *h_track,
                                   const int64_t *h_seg_start, size_t n_segments,
                                   double *out_records, size_t record_ld, int32_t *status3,
                                   const vbx_pitch_track_outputs *h_outputs);
int vbx_analyze_frames_tracked_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                                     const vbx_analysis_params *h_params, const vbx_pitch_track_params *h_track,
                                     const int64_t *h_seg_start, size_t n_segments,
                                     double *out_records, size_t record_ld, int32_t *status3,
                                     const vbx_pitch_track_outputs *h_outputs);

/* The frame loop of the reference's one complete program (ABI 5, added): examples/formant_extraction/src/main.rs:72-88 calls
 * find_formants with resample_ratio = 10000 / 44100 (src/lib.rs:40-64: the frame is resampled to m = vbx_resampled_len(frame_len,
 * ratio) samples before the periodic Hanning window and Burg) and keeps the frame's RMS next to the formants and the pitch
 * (main.rs:84).  vbx_analyze_frames_ex_f64 / _pcm16 are vbx_analyze_frames_f64 / _pcm16 (h_track NULL: columns 0-1 = candidates[0])
 * or vbx_analyze_frames_tracked_f64 / _pcm16 (h_track non-NULL) with that loop's two extras, from ONE call:
 *   formant_resample_ratio  find_formants' resample_ratio.  The formant columns and the formant status row are those of
 *                           vbx_resample_linear_f64 into a dense [F, m] batch followed by vbx_find_formants_f64 on it, BIT FOR BIT --
 *                           but the batch never exists: Burg's kernels form each resampled, windowed sample in registers from the
 *                           caller's hop-strided frames (f64, or 16-bit PCM widened in registers), for every resampled length
 *                           2 <= m <= 1280 from frames of up to VBX_MAX_FRAME_LEN samples.  Other shapes (m > 1280, longer source
 *                           frames) are resampled into a context-owned dense batch, a chunk of frames at a time: at most 256 MiB,
 *                           or one resampled frame (8 m bytes) if that is more; PCM is then widened into the context-owned copy first.
 *   formant_sample_rate     the sample_rate find_formants is given; 0: sample_rate * formant_resample_ratio, the true rate of the
 *                           resampled frame (formants in Hz).
 *   rms                     != 0: RMS::rms of the rectangular frame (src/waves.rs:10-23) -- exactly what vbx_rms_f64(window = NULL)
 *                           returns on the f64 or widened samples -- as one more column, the LAST of the record:
 *                             [ pitch | formants | mfcc | lpc | rms ],  vbx_record_doubles_ex(params, ext) doubles.
 *                           It is taken on the context's second stream from the caller's own samples (a PCM recording is never widened
 *                           for it); a tracked call that also needs local_peak reads the samples once for both.
 * The example passes the NEW rate to pitch as well (main.rs:78-80): params.sample_rate = 10000 with formant_sample_rate = 10000
 * reproduces it literally; a caller who wants true Hz passes the recording's rate as params.sample_rate and leaves
 * formant_sample_rate 0.
 * Every existing column keeps its offset; the alignment rules, status3, the state left for vbx_track_stitch_f64, the LPC probe's count
 * and vbx_internal_last_burg_direct_count behave as in the plain and tracked calls.  With h_ext NULL or all zero (or a ratio of 1.0)
 * the call IS the plain call (h_track NULL) or the tracked call (h_track non-NULL), bit for bit.
 * VBX_E_INVALID, before anything is written and with the context left usable: a negative or non-finite ratio or rate, a ratio above
 * 64 (the bound of vbx_resample_linear_f64), a resampled frame of fewer than 2 samples or an order Burg refuses on it, a ratio other
 * than 0 / 1.0 with formant_order == 0, anything the plain or tracked call rejects.  n_frames == 0 succeeds.
 * Measured (one MI355X, 4.5 M frames of 1200 / 480 at 48 kHz, all parts on, formants at ratio 10000 / 48000 and order 12, RMS on):
 * 120.6 ms = 37.3 M frames/s (PCM: 121.3 ms) against 128.4 ms (PCM: 132.5 ms) for the calls it replaces -- vbx_analyze_frames_f64
 * without formants, vbx_resample_linear_f64 into a 9 GB batch, vbx_find_formants_f64, vbx_rms_f64. */
typedef struct {
    double formant_resample_ratio;  /* find_formants' resample_ratio; 0 or 1.0: none (src/lib.rs:57,62-64) */
    double formant_sample_rate;     /* the sample_rate find_formants is given; 0: sample_rate * ratio */
    int32_t rms;                    /* != 0: one more column, the LAST of the record */
} vbx_analysis_ext;
size_t vbx_record_doubles_ex(const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext);
int vbx_analyze_frames_ex_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                              const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext,
                              const vbx_pitch_track_params *h_track /* NULL: columns 0-1 = candidates[0] */,
                              const int64_t *h_seg_start, size_t n_segments,
                              double *out_records, size_t record_ld, int32_t *status3,
                              const vbx_pitch_track_outputs *h_outputs);
int vbx_analyze_frames_ex_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride,
                                const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext,
                                const vbx_pitch_track_params *h_track /* NULL: columns 0-1 = candidates[0] */,
                                const int64_t *h_seg_start, size_t n_segments,
                                double *out_records, size_t record_ld, int32_t *status3,
                                const vbx_pitch_track_outputs *h_outputs);
/* vbx_analyze_frames_ex_f64 on FLOAT32 samples: frame t is x[t*stride .. +frame_len).  The suffix is _f32in, not _f32: only the INPUT
 * is float -- the records, the candidate lists, the peaks, the arithmetic and everything else written stay f64 (elsewhere in this
 * header _f32 means float results too).  One call covers three forms: h_ext NULL and h_track NULL is the plain loop, h_track non-NULL
 * the tracked loop.
 * Every byte the call writes -- the records, status3, all four h_outputs arrays -- and everything it leaves behind (the state for
 * vbx_track_stitch_f64, the vbx_internal_last_* counts, vbx_internal_last_path_chunks_redone) is what vbx_f32_to_f64 into a caller-owned
 * buffer followed by vbx_analyze_frames_ex_f64 on that buffer gives, BIT FOR BIT, at every shape, parameter set and LPC policy that
 * call accepts: widening is exact, so a NaN frame reports VBX_FRAME_ERR_NAN exactly as there.
 * Which shapes read the floats directly (the rule of the PCM form): full 1200-sample frames through the fused spectral kernel with
 * lpc_order 0 or 12 and MFCC fused -- under every LPC policy: the pitch fallback list, the double-double LPC list and the REFERENCE
 * rows have float forms --, with the formant chain at any order, resampled (the shapes Burg's resampled loaders take) or not.  There
 * the f64 copy never exists: 4 B per sample resident instead of 4 + 8, and no widening pass.  Every other shape takes ONE widening
 * pass of the view into a context-owned f64 copy (8 B per sample of the view, kept for the next call), queued on the context's stream
 * ahead of the fork, and runs the f64 path from there.  The RMS column and local_peak are always taken from the caller's floats, on
 * the context's second stream (the peak as a float max widened once: the same bits).
 * x needs 4-byte alignment only: wider loads are taken where a frame's own address allows them (8 bytes in the fused kernel: an odd
 * stride alternates frame by frame), with the same bits either way.  It takes no stream or event of its own.
 * VBX_E_INVALID, before anything is written: what vbx_analyze_frames_ex_f64 rejects, and a NULL x with n_frames > 0.  n_frames == 0
 * succeeds.  Measured: DESIGN.md section 5d. */
int vbx_analyze_frames_ex_f32in(vbx_ctx *ctx, const float *x, size_t n_frames, size_t frame_len, size_t stride,
                                const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext,
                                const vbx_pitch_track_params *h_track /* NULL: columns 0-1 = candidates[0] */,
                                const int64_t *h_seg_start, size_t n_segments,
                                double *out_records, size_t record_ld, int32_t *status3,
                                const vbx_pitch_track_outputs *h_outputs);
/* vox_box::find_formants(buf, sample_rate, resample_ratio, ..) over F frames (src/lib.rs:40-116) with the ratio: all five outputs
 * are those of vbx_resample_linear_f64 + vbx_find_formants_f64(sample_rate) on the dense batch, bit for bit, without the batch (the
 * shapes and the fallback's workspace bound are those of vbx_analyze_frames_ex_f64).  sample_rate is what find_formants is given
 * (the example: 10000).  resample_ratio 0 or 1.0: vbx_find_formants_f64 itself.  VBX_E_INVALID as above. */
int vbx_find_formants_resampled_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride,
                                    double sample_rate, double resample_ratio, size_t n_coeffs,
                                    const int64_t *h_seg_start, size_t n_segments,
                                    const vbx_resonance *h_est_init, size_t n_est,
                                    vbx_resonance *out_formants, vbx_resonance *out_res, int32_t *out_res_count,
                                    double *out_coeffs, int32_t *status);

/* ------------------------------------------------------------------ host-resident recordings (ABI 5, added) */

/* What a WAV reader hands over, as the type the frame loop reads natively: channel `channel` of n_sample_frames interleaved sample
 * frames of `channels` samples each (element i * channels + channel), d_src and d_out on the device.
 *   VBX_SAMPLE_PCM16  int16                           -> int16, copied (the frame loop's PCM kernels divide by 32767: vbx_pcm16_to_f64)
 *   VBX_SAMPLE_PCM24  packed 3-byte LE two's complement -> double, s / 8388607    (tests/lib.rs:17-19 at bits_per_sample = 24)
 *   VBX_SAMPLE_PCM32  int32                           -> double, s / 2147483647
 *   VBX_SAMPLE_F32    float                           -> float, as it is (bit patterns are copied: NaN payloads, -0.0, subnormals survive)
 *   VBX_SAMPLE_F64    double                          -> double, as it is
 *   VBX_SAMPLE_U8     unsigned 8-bit PCM (WAV, 8 bits per sample) -> double, (b - 128) / 127   (tests/lib.rs:17-19 at bits_per_sample = 8)
 *   VBX_SAMPLE_ULAW   G.711 mu-law, one byte          -> int16, the 16-bit linear value below
 *   VBX_SAMPLE_ALAW   G.711 A-law, one byte           -> int16, the 16-bit linear value below
 * PCM24 and PCM32 results are the correctly rounded quotient (IEEE division), bit for bit numpy.float64(s) / denom.
 * 8-bit telephone audio (ABI 5, added).  U8 is the same kind of quotient, bit for bit numpy.float64(b - 128) / 127,
 * from -128/127 to 1.  ULAW and ALAW are the ITU-T G.711 expansions that ffmpeg, sox and CPython's audioop implement:
 *   mu-law: u = ~b & 0xff, e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 0x84) << e) - 0x84; the value is -mag if u & 0x80, else mag
 *           (+-32124 at most; 0x7f and 0xff both give 0);
 *   A-law:  a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15, mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1); the value is mag if
 *           a & 0x80, else -mag (+-32256 at most; there is no zero code).
 * The decoded int16 means what every PCM16 sample means to this library, s / 32767, and is handed to the PCM16 kernels as it is.  The
 * decode is integer arithmetic in registers inside the reader kernels (no table); vbx_g711_table runs the same function on the host.
 * Contract: every byte a call writes for a ULAW or ALAW source equals, bit for bit, what the same call writes for PCM16 on the decoded
 * int16 samples, and every byte it writes for U8 equals what it writes for F64 on (b - 128) / 127 (tests/test_gpu_unpack8.py,
 * tests/test_gpu_analyze_sample8.py).  An 8-bit source has no alignment requirement.  Profiled as unpack_u8 / unpack_ulaw / unpack_alaw.
 * The values 6 and 7 -- the WAV format tags of A-law and mu-law -- are NOT formats of this library: 0, 6 to 15 and 19 and above are
 * rejected.  Container parsing stays with the caller (which WAV tag maps to which constant).
 * Alignment: a PCM24 source may sit at any byte address; every other source and every destination needs its type's natural
 * alignment.  A 16-byte aligned destination is written by 16-byte stores, a mono source of matching alignment read by the widest
 * loads; the results are the same bits either way.  channels == 1 with PCM16, F32 or F64 is a plain copy.  One pass, asynchronous
 * on the context's stream; profiled as unpack_pcm16 / unpack_pcm24 / unpack_pcm32 / unpack_f32 / unpack_f64.
 * VBX_E_INVALID: an unknown format, channels < 1, channel outside [0, channels), a NULL pointer with n_sample_frames > 0, a
 * misaligned pointer.  n_sample_frames == 0 succeeds. */
#define VBX_SAMPLE_PCM16 1
#define VBX_SAMPLE_PCM24 2
#define VBX_SAMPLE_PCM32 3
#define VBX_SAMPLE_F32 4
#define VBX_SAMPLE_F64 5
#define VBX_SAMPLE_U8 16     /* unsigned 8-bit PCM (WAV, 8 bits per sample): (b - 128) / 127      -> double */
#define VBX_SAMPLE_ULAW 17   /* G.711 mu-law: the 16-bit linear value above                        -> int16  */
#define VBX_SAMPLE_ALAW 18   /* G.711 A-law:  the 16-bit linear value above                        -> int16  */
int vbx_unpack_samples(vbx_ctx *ctx, const void *d_src, size_t n_sample_frames, int format, int channels, int channel, void *d_out);

/* The 256 values of a G.711 law: h_out[b] = the 16-bit linear value of code b, by the same function the reader kernels run.  Host
 * arithmetic only: no context, no GPU (a caller can decode a header's worth of samples with it).  VBX_E_INVALID: a format other
 * than VBX_SAMPLE_ULAW or VBX_SAMPLE_ALAW, a NULL h_out. */
int vbx_g711_table(int format, int16_t *h_out /* [256] */);

/* The frame loop on a recording that lives in HOST memory, of any length, from one call: vbx_analyze_frames_ex_* fed chunk by chunk.
 * h_audio holds n_sample_frames interleaved sample frames in h_fmt->format; channel h_fmt->channel is analysed;
 * F = vbx_frame_count(n_sample_frames, frame_len, stride) frames.  out_records [F, record_ld], status3 [3, F] (optional) and the
 * h_outputs arrays (F rows each) are DEVICE memory: the recording itself is never resident, only the records are (288 B per frame
 * with all parts on).
 * Contract: every byte written to out_records, status3 and the four h_outputs arrays equals, bit for bit, what the resident call
 * writes on the whole selected channel -- vbx_analyze_frames_ex_pcm16 for PCM16, vbx_analyze_frames_ex_f32in for F32,
 * vbx_analyze_frames_ex_f64 on the converted samples (vbx_unpack_samples) for PCM24, PCM32 and F64 -- for every
 * chunk_frames >= VBX_SHARD_WARM_FRAMES, every segment list, the plain, tracked and ext forms, every LPC policy, pinned and pageable
 * h_audio (tests/test_gpu_analyze_host.py).  Where the mono PCM16 / F32 call reads the samples without a copy (1200-sample frames:
 * the rule of vbx_analyze_frames_pcm16) the chunks do too; elsewhere the widening pass runs per chunk into the context-owned copy,
 * which is then chunk-sized.
 * How.  Chunk c covers frames [lo, hi) = [c * chunk_frames, ...) (vbx_host_chunk_plan).  Its sample frames -- those of frames
 * [lo - warm, hi), i.e. with the frame_len - stride halo -- are uploaded on a context-owned copy stream into one of two raw staging
 * slots; the upload of chunk c + 1 is issued before chunk c's analysis is queued.  On the context's stream, behind the upload:
 * vbx_unpack_samples into a typed chunk buffer (skipped for mono PCM16 / F32 / F64: the slot is read as it is), the frame loop on
 * frames [lo - warm, hi) into chunk-local records and status rows, the formant tracker's stitch from row lo - 1 of out_records
 * when the cut lies inside an utterance (vbx_track_stitch_f64: the warm-up and the exact repair of the sharded runs below), and a
 * copy of the chunk's own rows into place.  The tracked form writes each chunk's candidate lists, counts and peaks at their global
 * offsets -- the caller's h_outputs arrays, or a context workspace of F * (16 kmax + 16) bytes -- and runs the pitch path ONCE over
 * the whole recording behind the last chunk, straight into columns 0-1: the lists are per frame and all there, so the contour is
 * vbx_pitch_path_f64's by construction.
 * Device memory in use: the two raw slots, the typed chunk buffer, the chunk-local records and status rows, the frame loop's own
 * chunk-sized workspaces, the caller's outputs.
 * Host timing: the call returns when the last byte of h_audio has been read (the caller may free or overwrite it); kernels may still
 * be running, and the outputs are ordered on the context's stream like every call's.  Pinned h_audio (vbx_malloc_host) is uploaded
 * beside the previous chunk's analysis; pageable memory works, but nothing overlaps.  vbx_sync drains the copy stream too.
 * Host calls may follow one another on a context with no wait between them (several channels of one file from one upload:
 * vbx_analyze_host_channels, below): every
 * upload waits for its staging slot's last reader, the previous call's included.
 * Afterwards the vbx_internal_last_* probes describe the LAST chunk's call only (not part of the contract), and the context holds
 * no state for vbx_track_stitch_f64, which returns VBX_E_INVALID.  Not capturable into a graph.
 * h_fmt->chunk_frames: analysis frames per chunk; 0 = the library's default, 250,000 frames (120 M samples at a 480-sample hop).
 * 8-bit sources (VBX_SAMPLE_U8 / ULAW / ALAW, one byte per sample, any byte address): every byte written for a ULAW or ALAW source
 * equals, bit for bit, what the same call writes for PCM16 on the decoded int16 samples (vbx_g711_table), and every byte written for
 * U8 equals what it writes for F64 on (b - 128) / 127 -- the bytes are decoded inside this call's own reader kernel, never in a pass before it.
 * VBX_E_INVALID, before anything is written and with the context left usable: a NULL h_fmt, an unknown format, channels < 1,
 * channel outside [0, channels), reserved != 0, a NULL h_audio with F > 0, 0 < chunk_frames < VBX_SHARD_WARM_FRAMES, anything the
 * resident call rejects.  F == 0 succeeds. */
typedef struct {
    int32_t format;        /* VBX_SAMPLE_* */
    int32_t channels;      /* >= 1, interleaved */
    int32_t channel;       /* the one analysed, < channels */
    int32_t reserved;      /* 0 */
    size_t  chunk_frames;  /* analysis frames per chunk; 0: the library's default (250,000) */
} vbx_host_audio;
#define VBX_HOST_DEFAULT_CHUNK_FRAMES 250000

int vbx_analyze_host(vbx_ctx *ctx, const void *h_audio, size_t n_sample_frames, const vbx_host_audio *h_fmt,
                     size_t frame_len, size_t stride,
                     const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                     const int64_t *h_seg_start, size_t n_segments,
                     double *out_records /* device */, size_t record_ld, int32_t *status3 /* device, [3, F] */,
                     const vbx_pitch_track_outputs *h_outputs /* device arrays of F rows */);
/* pinned host memory for h_audio (hipHostMalloc / hipHostFree): uploads from it overlap the analysis */
int vbx_malloc_host(vbx_ctx *ctx, void **out, size_t bytes);
int vbx_free_host(vbx_ctx *ctx, void *p);

/* vbx_unpack_samples for n_sel selected channels in ONE pass over the interleaved sample frames: plane k is n_sample_frames elements
 * of the format's output type (int16 for PCM16, float for F32, double for PCM24, PCM32 and F64) starting at element k * plane_ld of
 * d_out, and equals, bit for bit, what vbx_unpack_samples(..., channel = h_channels[k], ...) writes -- the correctly rounded PCM24 /
 * PCM32 quotients, the copied bit patterns of floats.  Elements [n_sample_frames, plane_ld) of a plane are not written.
 * h_channels is HOST memory: n_sel distinct values in [0, channels), in any order, 1 <= n_sel <= min(channels,
 * VBX_HOST_MAX_CHANNELS); the selection travels as a kernel argument, so the call allocates and uploads nothing.
 * How: a block stages a tile of whole sample frames in LDS by contiguous 16-byte loads (dword loads for a source on a dword boundary
 * only), and each lane gathers the 16 output bytes it owns in one plane and stores them at once: the interleaved frames are read
 * from memory once, whatever n_sel.  The per-element form takes over -- same bits -- for a source off a dword boundary (PCM24 at an
 * odd byte address, PCM16 at an odd element), a destination off a 16-byte boundary or a plane_ld that leaves a later plane off one,
 * a sample frame too wide for 16 of them to fit a tile, and the tail behind the last whole tile; channels == 1 is
 * vbx_unpack_samples itself.  The per-element form is correct but slow (scalar stores, a division per element): keep d_out 16-byte
 * aligned and choose plane_ld as a multiple of 8 elements (n_sample_frames rounded up), which keeps every plane on the tiled form.
 * Measured rates, subsets included: DESIGN.md section 5f.  Asynchronous on the context's stream; profiled as unpack_all_pcm16 / unpack_all_pcm24 /
 * unpack_all_pcm32 / unpack_all_f32 / unpack_all_f64.
 * 8-bit sources (VBX_SAMPLE_U8 / ULAW / ALAW, one byte per sample, any byte address): every byte written for a ULAW or ALAW source
 * equals, bit for bit, what the same call writes for PCM16 on the decoded int16 samples (vbx_g711_table), and every byte written for
 * U8 equals what it writes for F64 on (b - 128) / 127 -- the bytes are decoded inside this call's own reader kernel, never in a pass before it.
 * VBX_E_INVALID, with nothing written: an unknown format, channels < 1, n_sel outside [1, min(channels, VBX_HOST_MAX_CHANNELS)], a
 * NULL h_channels, a repeated or out-of-range channel, plane_ld < n_sample_frames, a NULL pointer with n_sample_frames > 0, a pointer
 * that breaks its type's natural alignment (a PCM24 source has none).  n_sample_frames == 0 succeeds. */
#define VBX_HOST_MAX_CHANNELS 64
int vbx_unpack_channels(vbx_ctx *ctx, const void *d_src, size_t n_sample_frames, int format, int channels,
                        const int32_t *h_channels, size_t n_sel, void *d_out, size_t plane_ld);

/* vbx_analyze_host for n_sel channels of one recording from ONE upload per chunk (a stereo file, a microphone array): every chunk's
 * interleaved bytes cross the bus once, one vbx_unpack_channels launch turns them into n_sel typed planes, and the channels are then
 * analysed one after another on the context's stream.  h_fmt->channel must be 0; the selection is h_channels (as for
 * vbx_unpack_channels).  All channels share one parameter set, one segment list and one record_ld; h_out holds n_sel entries, entry k
 * the device outputs of channel h_channels[k]: records [F, record_ld] (16-byte aligned), status3 [3, F] (optional), outputs (optional:
 * device arrays of F rows, as h_outputs of vbx_analyze_host).
 * Contract: every byte written through h_out[k] equals, bit for bit, what vbx_analyze_host writes with h_fmt->channel = h_channels[k]
 * and the same other arguments -- by that call's contract the resident call's output -- for every chunk_frames >=
 * VBX_SHARD_WARM_FRAMES, every segment list, the plain, tracked and ext forms, every LPC policy, pinned and pageable h_audio
 * (tests/test_gpu_analyze_host_channels.py).
 * How.  Chunks, the two raw slots, their ready / freed events and the overlapped upload are vbx_analyze_host's (a slot holds all
 * `channels` channels, as it does there).  Per chunk: one unpack launch into n_sel planes whose pitch keeps every plane 256-byte
 * aligned (each is read as a resident recording would be: 1200-sample PCM16 / F32 frames without a widening copy), the slot's freed
 * event right behind it; then per selected channel the frame loop on its plane into the chunk-local records and status rows (reused
 * from channel to channel), the tracker's stitch from row lo - 1 of THAT channel's records, and the copy of the chunk's own rows into
 * h_out[k].  channels == 1: the slot is read as it is for PCM16, F32 and F64.  The tracked form keeps each channel's candidate lists,
 * counts, peaks and status rows for the whole recording until the end -- in the caller's arrays where h_out[k] supplies them, else in
 * the context workspace, which then grows to n_sel * F * (16 kmax + 16) bytes -- and runs the pitch path once per channel behind the
 * last chunk, into columns 0-1 of that channel's records.
 * Device memory in use: the two raw slots, n_sel typed planes, one set of chunk-local records and status rows, the frame loop's
 * chunk-sized workspaces, the tracked form's per-channel lists, the caller's outputs.
 * Host timing, vbx_sync, calls that follow one another with no wait between them, "not capturable into a graph" and the state left
 * behind (the probes describe the last chunk's last channel; none for vbx_track_stitch_f64) are as for vbx_analyze_host.
 * 8-bit sources (VBX_SAMPLE_U8 / ULAW / ALAW, one byte per sample, any byte address): every byte written for a ULAW or ALAW source
 * equals, bit for bit, what the same call writes for PCM16 on the decoded int16 samples (vbx_g711_table), and every byte written for
 * U8 equals what it writes for F64 on (b - 128) / 127 -- the bytes are decoded inside this call's own reader kernel, never in a pass before it.
 * VBX_E_INVALID, before anything is written and with the context left usable: everything vbx_analyze_host rejects; a bad selection
 * (as vbx_unpack_channels); h_fmt->channel != 0; a NULL h_out; an entry whose records are NULL or not 16-byte aligned; two entries
 * whose [F, record_ld] record ranges overlap.  F == 0 succeeds. */
typedef struct {
    double  *records;                        /* device, [F, record_ld], 16-byte aligned */
    int32_t *status3;                        /* device, [3, F], optional */
    const vbx_pitch_track_outputs *outputs;  /* optional; device arrays of F rows, as in vbx_analyze_host */
} vbx_channel_outputs;
int vbx_analyze_host_channels(vbx_ctx *ctx, const void *h_audio, size_t n_sample_frames, const vbx_host_audio *h_fmt,
                              const int32_t *h_channels, size_t n_sel, size_t frame_len, size_t stride,
                              const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext,
                              const vbx_pitch_track_params *h_track, const int64_t *h_seg_start, size_t n_segments,
                              const vbx_channel_outputs *h_out /* n_sel entries */, size_t record_ld);

/* ------------------------------------------------------------------ live sessions (ABI 5, added) */

/* Audio that ARRIVES -- a microphone, a socket, a decoder, a model emitting a waveform: a session is opened once on a context for
 * ONE channel of one stream of audio, fed blocks of any size as they come, and every push delivers the records of the frames that
 * block completes.  (The reference's streaming form is `impl Autocorrelate for VecDeque`, src/periodic.rs:291-304, under a user
 * loop that consumes a Windower frame by frame.)
 * Contract: concatenate every block ever pushed, and concatenate every row the pushes wrote: the result equals, bit for bit, what
 * the resident call writes on the whole recording -- vbx_analyze_frames_ex_pcm16 for PCM16, vbx_analyze_frames_ex_f32in for F32,
 * vbx_analyze_frames_ex_f64 on the vbx_unpack_samples output for PCM24, PCM32 and F64 -- for EVERY way of cutting the recording
 * into blocks: blocks of one sample, blocks shorter than a hop that complete no frame, blocks of exactly one hop, blocks of hundreds
 * of thousands of frames (tests/test_gpu_session.py).
 * vbx_session_plan is the arithmetic of one push, pure host code: a session that has consumed `consumed` sample frames, whose
 * current utterance began at frame utt_frame, is pushed n_new more.
 * vbx_session_open: h_fmt as for vbx_analyze_host (chunk_frames and reserved must be 0); the parameters are copied.  Everything the
 * session will ever need for blocks of up to max_block_sample_frames is allocated here -- two typed carry buffers of
 * (VBX_SHARD_WARM_FRAMES + 1) * stride + frame_len + max_block_sample_frames samples each, two raw staging slots, the chunk-local
 * records, status rows and lists of max_block_sample_frames / stride + 1 + VBX_SHARD_WARM_FRAMES frames, the tracker state -- and
 * the shape is warmed by one frame-loop call at that frame count on the zeroed carry, which is also where everything only the frame
 * loop's parts know (orders, the resampled shape, the MFCC geometry) is rejected.  After that no push allocates or drains a stream on
 * its own account.
 * vbx_session_push: h_block is HOST memory, n_sample_frames interleaved sample frames in the session's format.  Rows [0, n) of
 * out_records (device, 16-byte aligned, record_ld as in the resident call) receive frames [lo, hi) of the plan, n = hi - lo; row k
 * of the three status rows is written at status3 + k * status_ld, n entries (status3 optional; a caller filling one global [3, F]
 * array passes status3 + lo and status_ld = F); *h_n_frames = n (optional), which vbx_session_plan tells beforehand.  A push that
 * completes no frame only appends to the carry and writes nothing; n_sample_frames == 0 is a no-op.
 * How.  The block is uploaded on the context's copy stream into one of the session's two raw slots (ready / freed events as in
 * vbx_analyze_host: the host runs at most two blocks ahead).  On the context's stream: ONE session_ingest launch writes the carry's
 * kept tail and the selected channel of the block, as the frame loop's type, into the session's other carry buffer; the frame loop
 * runs on frames [lo - warm, hi) of it into the chunk-local buffers, with no segment list -- warm never reaches before the
 * utterance's start, so the analysed range lies in ONE utterance; where the push continues an utterance the tracker is stitched from
 * the session's state, the formant row of the last frame delivered (vbx_track_stitch_f64's repair; a frame with a bad status passes
 * the state through, so that row is always the true state); ONE session_deliver launch copies the push's own rows into the caller's
 * arrays and the last formant row into the state.  A block's device work is its own frames plus at most VBX_SHARD_WARM_FRAMES.
 * Host timing follows vbx_analyze_host: the push returns when the last byte of h_block has been read; the outputs are ordered on the
 * context's stream; pinned blocks (vbx_malloc_host) upload beside the previous block's analysis.  Blocks of up to 128 KiB (a hop, a
 * hundred hops of 16-bit mono) do not take the copy stream: they are copied on the host into one of two session-owned pinned buffers and uploaded from
 * there on the context's own stream, so that such a push waits for no second stream and for no upload (the host still runs at most
 * two blocks ahead: a staging buffer is reused when its upload of two pushes ago has left it).  vbx_session_push_device reads
 * d_block (device memory) in stream order on the context's stream, with no staging and no host wait.
 * Utterances: vbx_session_mark_utterance makes the next frame delivered -- frame vbx_frame_count(consumed) at the time of the call --
 * the start of a new utterance.  With marks at frames m1 < m2 < ... the session's output equals the resident call's with
 * h_seg_start = [0, m1, m2, ...].
 * The tracked form (h_track non-NULL) runs the fused kernel at kmax and writes the new frames' candidate lists, counts and (where
 * the path needs them) peaks through h_outputs, n rows each: cand and count are required, peak when silence_threshold != 0, index must
 * be NULL.  Columns 0-1 of the pushed records are NOT written: the caller runs vbx_pitch_path_f64 over an utterance's rows when it
 * ends, and because the lists are per frame and equal the resident call's, that contour equals the resident tracked call's columns
 * 0-1, bit for bit.  Or the session is bound to an online path (vbx_session_path_bind, below), and every push also delivers the
 * rows of the contour that are decided: exact where decided, forced rows only at the cap, P fixed at peak_ref.
 * The LPC policy is the context's at the time of each push.  Several sessions may live on one context, each owning its carry; any
 * other entry point may be called on the context between pushes without changing a session's output.  After a push the
 * vbx_internal_last_* probes describe that push's frame-loop call, and the context holds no state for vbx_track_stitch_f64.  Not
 * capturable into a graph.  vbx_session_reset drops the carried samples and all state (as a freshly opened session);
 * vbx_session_info reports the sample frames consumed, the frames delivered and the sample frames carried; vbx_session_close frees
 * the session (behind the work queued on the context's stream; close every session before its context).
 * Kernel launches per push and measured round trips: DESIGN.md section 5g.
 * 8-bit sources (VBX_SAMPLE_U8 / ULAW / ALAW, one byte per sample, any byte address): every byte written for a ULAW or ALAW source
 * equals, bit for bit, what the same call writes for PCM16 on the decoded int16 samples (vbx_g711_table), and every byte written for
 * U8 equals what it writes for F64 on (b - 128) / 127 -- the bytes are decoded inside this call's own reader kernel, never in a pass before it.
 * VBX_E_INVALID, before anything is queued and with session and context left usable: a NULL argument where one is required, an unknown
 * format, channels < 1, channel outside [0, channels), non-zero reserved or chunk_frames, max_block_sample_frames == 0, a push larger
 * than max_block_sample_frames, records misaligned, record_ld odd or too small, status_ld < n, the tracked form's missing or
 * forbidden h_outputs members, everything the resident call rejects from its arguments. */
typedef struct vbx_session vbx_session;

/* pure host arithmetic, no GPU: what a push of n_new sample frames does to a session that has consumed `consumed` sample
 * frames and whose current utterance began at frame utt_frame (utt_frame <= vbx_frame_count(consumed); WARM = VBX_SHARD_WARM_FRAMES) */
typedef struct {
    size_t lo, hi;        /* frames this push delivers: [vbx_frame_count(consumed), vbx_frame_count(consumed + n_new)) */
    size_t warm;          /* frames analysed before lo: min(lo - utt_frame, WARM); 0 when hi == lo */
    int continues_prev;   /* lo > utt_frame and hi > lo: the tracker continues from the last delivered row */
    size_t read_from;     /* first sample frame the push's analysis reads: (lo - warm) * stride */
    size_t keep_from;     /* first sample frame still carried afterwards: min(consumed + n_new, (hi - min(hi - utt_frame, WARM)) * stride) */
} vbx_session_plan_t;
int vbx_session_plan(size_t consumed, size_t utt_frame, size_t n_new, size_t frame_len, size_t stride, vbx_session_plan_t *h_out);

int vbx_session_open(vbx_ctx *ctx, const vbx_host_audio *h_fmt /* chunk_frames and reserved must be 0 */,
                     size_t frame_len, size_t stride, const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext,
                     const vbx_pitch_track_params *h_track, size_t max_block_sample_frames, vbx_session **out);
int vbx_session_push(vbx_session *s, const void *h_block, size_t n_sample_frames,
                     double *out_records /* device */, size_t record_ld, int32_t *status3 /* device, optional */, size_t status_ld,
                     const vbx_pitch_track_outputs *h_outputs /* device arrays of n rows */, size_t *h_n_frames);
int vbx_session_push_device(vbx_session *s, const void *d_block, size_t n_sample_frames,
                            double *out_records, size_t record_ld, int32_t *status3, size_t status_ld,
                            const vbx_pitch_track_outputs *h_outputs, size_t *h_n_frames);
int vbx_session_mark_utterance(vbx_session *s);   /* the next frame delivered starts a new utterance (an h_seg_start entry) */
int vbx_session_reset(vbx_session *s);            /* drop the carried samples and all state: as a freshly opened session */
int vbx_session_info(const vbx_session *s, size_t *h_consumed, size_t *h_frames, size_t *h_carried);
void vbx_session_close(vbx_session *s);

/* ------------------------------------------------------------------ the pitch path while the lists arrive (ABI 5, added) */

/* vbx_pitch_path_f64's contour, committed while the candidate lists arrive: a path stream is opened once on a context, pushed the
 * lists of the frames that have come (any number per push), and every push writes the rows of the frames whose state is DECIDED.
 * Definition.
 *   Recursion.  lambda, c, D, psi and the leader are vbx_pitch_path_f64's, operation for operation, in IEEE binary64 with no fused
 *     multiply-add (the same device code computes them).  chunk_frames is ignored: the true D is carried from push to push, so
 *     nothing is speculated and nothing repaired.
 *   Silence term.  The resident call divides by P, the utterance's largest local_peak, which is not causal.  Here P = peak_ref, fixed
 *     at open: the format's full scale, or a level from calibration.  With silence_threshold == 0 or a NULL local_peak
 *     u_t = voicing_threshold and peak_ref is ignored.
 *   Decided frames.  When T frames of the current utterance have been scanned, decided(T) is the length of the longest prefix on
 *     which the psi traces from ALL active states of frame T - 1 agree (T itself when that frame has one state).  Every continuation
 *     of the utterance passes through one of those states, so the states of that prefix are the whole utterance's path, bit for bit,
 *     whatever follows.  decided(T) never shrinks.
 *   Commit.  A push commits every decided frame that is not yet committed.  Rows are written in frame order from row 0 of the output
 *     arrays: row i at out_path + i * path_ld doubles, with out_index[i] and out_forced[i] (both optional).  The row format is
 *     vbx_pitch_path_f64's: the chosen list entry, or {0.0, u_t}; the index is the list position, or -1.
 *   Cap.  At most max_pending frames are ever held.  If, after committing what is decided, max_pending frames are still pending when
 *     another frame must be scanned, the oldest ceil(max_pending / 2) of them are committed along the trace from the CURRENT leader,
 *     with out_forced = 1.  A forced row may differ from the whole utterance's path.  Decidedness depends on psi alone, so every row
 *     that is not forced equals the whole path, forced rows before it or not.
 *   Utterance end.  end_utterance != 0 commits all pending frames along the trace from the first state with D = 0, as the resident
 *     path ends (out_forced = 0: these rows are exact); the next frame starts a new utterance with D_0 = e_0 - max e_0.
 *     n_frames == 0 with the flag set is allowed.
 *   *d_commit (device memory, written in stream order; read it after a sync or an event).  first: the index of row 0, counted in
 *     frames pushed since open or reset; n: rows written; n_forced: how many of them were forced; pending: frames still held.
 *   Output size.  The arrays must hold max_pending + n_frames rows.  Rows beyond n are not touched.
 *   Schedule independence.  Decisions are evaluated when the ring is full and at the end of a push.  So the states, the forced flags
 *     and the number of frames committed once frame T has been pushed depend only on the frames pushed so far and on max_pending,
 *     never on how the frames were cut into pushes (tests/test_gpu_path_stream.py holds one-frame, seven-frame, random and whole
 *     pushes to the same rows and the same commits).
 * Everything is asynchronous on the context's stream: the lists are read in stream order and may be reused behind the push (the
 * stream keeps what a later commit needs in its own ring of max_pending frames, allocated at open); no push allocates, nothing
 * returns to the host.  A push of any n_frames is accepted; it is ONE launch of one lane group (pitch_path_online in the profile),
 * sequential by nature: about the resident call's sequential rate on large pushes -- large resident batches
 * have vbx_pitch_path_f64's chunked form.  Several streams may live on one context.  vbx_path_stream_reset: as freshly opened
 * (pending frames are dropped).  vbx_path_stream_close frees the stream behind the work queued on the context's stream.
 * VBX_E_INVALID: kmax 0 or above 63, max_pending 0 (or above 2^24), the parameters vbx_pitch_path_f64 rejects, silence_threshold > 0 with a NULL
 * local_peak or with peak_ref negative or not finite, a NULL stream, out_path or d_commit, NULL lists with n_frames > 0, path_ld < 2.
 *
 * vbx_session_path_bind: the contour from a live session.  Allowed on a session opened with h_track, before the first push or after
 * a reset (between pushes again, to change the destinations only: peak_ref and max_pending must repeat, the state is kept).  Every
 * push of a bound session (a push of n_sample_frames == 0 stays a no-op and reports nothing) then runs one more launch behind session_deliver: the online path over the push's own rows of the
 * session-owned lists, counts, pitch status row and peaks (time_step == 0: stride / sample_rate, as in the tracked call); the
 * committed rows go to the bound arrays from row 0 (they hold max_pending + the frames of the largest push), the commit to d_commit.
 * vbx_session_mark_utterance on a bound session ends the path's utterance at once (one launch, n_frames = 0, end_utterance = 1): the
 * rest of the contour is there when the mark is made.  vbx_session_reset resets the path and drops the binding; vbx_session_close
 * frees it.  Records, status rows and h_outputs of a bound session's pushes are what they were; an unbound session is unchanged.
 * Contract: with silence_threshold == 0 and no forced row, the committed rows of all pushes, concatenated, equal columns 0-1 and
 * `index` of the resident tracked call on the concatenated blocks (marks: h_seg_start), for every way of cutting the audio into
 * blocks; with silence_threshold > 0 they equal the world-1 shard protocol (vbx_pitch_path_shard_begin_f64 / _enter / _finish)
 * with every utterance's seg_peak = peak_ref. */
typedef struct vbx_path_stream vbx_path_stream;
typedef struct { int64_t first, n, n_forced, pending; } vbx_path_commit;   /* device memory */

int vbx_path_stream_open(vbx_ctx *ctx, size_t kmax, const vbx_pitch_path_params *h_params, double peak_ref, size_t max_pending,
                         vbx_path_stream **out);
int vbx_path_stream_push(vbx_path_stream *ps, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                         const double *local_peak, size_t n_frames, int end_utterance,
                         vbx_pitch *out_path, size_t path_ld, int32_t *out_index, uint8_t *out_forced, vbx_path_commit *d_commit);
int vbx_path_stream_reset(vbx_path_stream *ps);
void vbx_path_stream_close(vbx_path_stream *ps);
int vbx_session_path_bind(vbx_session *s, double peak_ref, size_t max_pending,
                          vbx_pitch *out_path, size_t path_ld, int32_t *out_index, uint8_t *out_forced, vbx_path_commit *d_commit);

/* ------------------------------------------------------------------ live sessions over several channels (ABI 5, added) */

/* Every selected channel of live audio -- a stereo interface, a microphone array, the channels of one decoder -- from ONE session and
 * ONE frame-loop call per push.  vbx_session_open_channels opens a session for n_sel channels of one stream of interleaved sample
 * frames: h_fmt as for vbx_session_open with h_fmt->channel == 0 (chunk_frames and reserved must be 0); h_channels / n_sel follow
 * vbx_unpack_channels (HOST memory, distinct values in [0, channels), any order, 1 <= n_sel <= min(channels, VBX_HOST_MAX_CHANNELS)).
 * All channels share one parameter set, one cut into blocks and one list of utterance marks.  Open allocates and warms the largest
 * shape, as vbx_session_open does; no push allocates or drains a stream.
 * vbx_session_push_channels (h_block in HOST memory) / vbx_session_push_channels_device (d_block in device memory, read in stream
 * order): h_out holds n_sel entries (a HOST array, read before the call returns); entry k receives rows [0, n) of this push for
 * channel h_channels[k], n = hi - lo of vbx_session_plan: records (device, 16-byte aligned, rows record_ld doubles apart), status3
 * (optional; row j of the three status rows at status3 + j * status_ld) and, in the tracked form, outputs with cand and count, peak
 * when silence_threshold != 0, index NULL.  *h_n_frames = n (optional).  Stricter than vbx_session_push in one point: h_out itself
 * must be non-NULL for every push of n_sample_frames > 0, also for one that completes no frame (its entries are then not read).
 * Contract: for every k, the rows all pushes wrote through h_out[k], concatenated, equal bit for bit what a one-channel session
 * opened with h_fmt->channel = h_channels[k] writes when it is pushed the same blocks -- by that session's contract the resident call
 * on the whole channel (vbx_analyze_frames_ex_pcm16 / _f32in / _f64 on the vbx_unpack_samples output, marks as h_seg_start) -- for
 * every way of cutting the stream into blocks, every format, the plain, tracked and ext forms, every LPC policy, pinned and pageable
 * blocks and the device form (tests/test_gpu_session_channels.py).  A NaN or Inf in one channel touches no other channel's rows.
 * How.  The block is uploaded ONCE (the two routes of vbx_session_push: pinned staging on the context's stream up to 128 KiB, the
 * copy stream with ready / freed events above).  Then, whatever n_sel: ONE session_ingest_all_<fmt> launch writes the other carry
 * buffer -- n_sel planes, plane k = the kept tail of the old plane k and channel h_channels[k] of the block as the frame loop's type
 * (the block is read from memory once: tiles of whole sample frames through LDS, 16-byte stores into every plane; per-element code with
 * the same bits for a source off a dword boundary, sample frames too wide for a tile, the group where tail and block meet and the
 * ragged end); ONE frame-loop call over all planes as one recording with the segment list [0, Q, 2Q, ...] (vbx_session_channels_plan:
 * plane k starts at element k * Q * stride, Q rounded up so that every plane base is a multiple of 256 bytes; channel k's frames are
 * [kQ, kQ + m), m = warm + n; the frames [kQ + m, (k + 1)Q) read stale or zeroed samples -- the carry is zeroed at open -- lie
 * BEHIND channel k's own frames in channel k's segment, so the causal tracker cannot let them reach a delivered row, and are never
 * delivered); ONE batched tracker stitch (a block per channel, each from its own state row: vbx_track_stitch_f64's repair); ONE
 * session_deliver_all launch that copies every channel's own rows to its destinations (kernel arguments) and its last formant row
 * into its state.  Launches per push do not depend on n_sel.
 * vbx_session_mark_utterance (a mark applies to every channel), vbx_session_reset, vbx_session_info and vbx_session_close work on
 * such a session unchanged.  The one-channel and the multi-channel calls do not mix: vbx_session_push, vbx_session_push_device and
 * vbx_session_path_bind on a session opened here, and the _channels calls (vbx_session_path_bind_channels included) on a
 * one-channel session, return VBX_E_INVALID with nothing queued.  n_sel == 1 is allowed and equals the one-channel session.  Device memory: n_sel carry planes (twice) and n_sel
 * times the chunk-local buffers of vbx_session_open.
 * 8-bit sources (VBX_SAMPLE_U8 / ULAW / ALAW, one byte per sample, any byte address): every byte written for a ULAW or ALAW source
 * equals, bit for bit, what the same call writes for PCM16 on the decoded int16 samples (vbx_g711_table), and every byte written for
 * U8 equals what it writes for F64 on (b - 128) / 127 -- the bytes are decoded inside this call's own reader kernel, never in a pass before it.
 * VBX_E_INVALID, before anything is queued and with the session left usable: everything the one-channel calls reject; a bad selection;
 * h_fmt->channel != 0; a NULL h_out; an entry with NULL or misaligned records; two entries whose [n, record_ld] ranges overlap; more
 * than 0x7fffffff frames in the largest frame-loop call.
 * vbx_session_channels_plan: pure host arithmetic, no GPU -- vbx_session_plan for the push (every channel shares it) and the plane
 * layout for samples of elem_bytes bytes (2: PCM16, 4: F32, 8: PCM24 / PCM32 / F64); h_seg_start (optional, n_sel entries) receives
 * the segment list. */
typedef struct {
    vbx_session_plan_t push;  /* what vbx_session_plan gives for (consumed, utt_frame, n_new) */
    size_t frames;            /* m: frames analysed per channel, warm + (hi - lo); 0 when the push completes no frame */
    size_t base;              /* first sample frame a plane holds after the push: read_from, or keep_from when hi == lo */
    size_t keep;              /* elements of a plane that come from the old plane: consumed - base, or 0 */
    size_t len;               /* elements of a plane the ingest writes: consumed + n_new - base */
    size_t plane_frames;      /* Q: the plane pitch in frames */
    size_t plane_ld;          /* Q * stride: plane k starts at element k * plane_ld (a multiple of 256 bytes) */
    size_t call_frames;       /* frames of the one frame-loop call: (n_sel - 1) * Q + m; 0 when m == 0 */
    size_t capacity;          /* elements of a plane the call may read: nothing is read beyond n_sel * capacity */
} vbx_session_channels_plan_t;
int vbx_session_channels_plan(size_t consumed, size_t utt_frame, size_t n_new, size_t frame_len, size_t stride, size_t elem_bytes,
                              size_t n_sel, vbx_session_channels_plan_t *h_out, int64_t *h_seg_start);

int vbx_session_open_channels(vbx_ctx *ctx, const vbx_host_audio *h_fmt /* channel, chunk_frames and reserved must be 0 */,
                              const int32_t *h_channels, size_t n_sel, size_t frame_len, size_t stride,
                              const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track,
                              size_t max_block_sample_frames, vbx_session **out);
int vbx_session_push_channels(vbx_session *s, const void *h_block, size_t n_sample_frames,
                              const vbx_channel_outputs *h_out /* n_sel entries */, size_t record_ld, size_t status_ld,
                              size_t *h_n_frames);
int vbx_session_push_channels_device(vbx_session *s, const void *d_block, size_t n_sample_frames,
                                     const vbx_channel_outputs *h_out /* n_sel entries */, size_t record_ld, size_t status_ld,
                                     size_t *h_n_frames);
/* vbx_session_path_bind for a multi-channel session: every channel gets its own online path (its own state and ring of max_pending
 * frames, one peak_ref and max_pending for all), and every push of the bound session runs ONE more launch behind session_deliver_all
 * -- pitch_path_online_all, a lane group per channel, each over its own channel's rows of the session-owned lists -- that commits
 * channel h_channels[k]'s decided rows through h_out[k] (n_sel entries, a HOST array of device pointers: out_path and d_commit
 * required, out_index and out_forced optional; each array holds max_pending + the frames of the largest push rows, rows path_ld
 * doubles apart).  The rules are vbx_session_path_bind's: a session opened with h_track, before the first push or after a reset;
 * between pushes again to change the destinations only.  vbx_session_mark_utterance on a bound session ends EVERY channel's path
 * utterance in one launch; vbx_session_reset resets the paths and drops the binding.
 * Contract: per channel the committed rows, indices, forced flags and commit records of every push equal those of a bound one-channel
 * session on that channel pushed the same blocks (tests/test_gpu_session_channels_path.py). */
typedef struct {
    vbx_pitch *out_path;       /* device, rows path_ld doubles apart */
    int32_t *out_index;        /* device, optional */
    uint8_t *out_forced;       /* device, optional */
    vbx_path_commit *d_commit; /* device */
} vbx_channel_path_outputs;
int vbx_session_path_bind_channels(vbx_session *s, double peak_ref, size_t max_pending,
                                   const vbx_channel_path_outputs *h_out /* n_sel entries */, size_t path_ld);

/* ------------------------------------------------------------------ a batch of variable-length clips (ABI 5, added) */

/* A corpus -- a speech dataset, a padded [B, Tmax] batch with lengths[B], the utterances a VAD cut out of a day of audio -- is many
 * short clips in separate device buffers, of ragged lengths, each with its first frame at its own sample 0.  vbx_analyze_clips
 * analyses all of them from ONE call: h_clip holds n_clips DEVICE pointers (the array itself in HOST memory), h_len their lengths in
 * samples; the clips are mono, contiguous, of h_fmt->format (h_fmt->reserved must be 0).  Clip b gives n_rows_b =
 * vbx_frame_count(h_len[b], frame_len, stride) rows; the outputs hold total_rows = sum n_rows_b rows, clip after clip: out_records
 * [total_rows, record_ld] (16-byte aligned), status3 [3, total_rows] (optional) and the arrays of h_outputs (tracked form; each
 * optional, as in the resident call) with total_rows rows.
 * Contract: for every clip b, rows [row_start_b, row_start_b + n_rows_b) of every output -- the records, the three status rows, cand /
 * count / peak / index -- are bit for bit what the resident call writes when it analyses clip b alone: vbx_analyze_frames_ex_pcm16 /
 * _f32in / _f64 on the clip's own samples (PCM24 / PCM32: _f64 on vbx_unpack_samples' doubles), one segment, the same other
 * arguments -- for every list of lengths, every group_frames, the plain, tracked and ext forms, every LPC policy and every frame
 * shape the resident call accepts (frames beyond 4096 samples and stride > frame_len included; tests/test_gpu_clips.py).  A clip
 * shorter than one frame has no rows and is not read (its pointer may be NULL); clips may overlap or repeat in memory; samples past
 * h_len[b] are never read; a NaN or Inf in one clip touches no other clip's rows.  The host arrays may be reused as soon as the call
 * returns.
 * How.  vbx_clips_plan cuts the clips, in order, into groups of whole clips of about group_frames analysed
 * frames.  Per group: ONE clips_pack_<fmt> launch gathers the group's clips through a device table into one plane of the type the
 * frame loop reads natively (int16 / float / double; PCM24 / PCM32 through vbx_unpack_samples' arithmetic), clip b's sample 0 at
 * element plane_frame_b * stride, the gap of fewer than `stride` elements behind a clip zero-filled; ONE frame-loop call over the
 * plane with the segment list [plane_frame_b] (every clip a segment of its own: the causal tracker never carries one clip's state
 * into the next, and the few frames that straddle two clips lie BEHIND the first one's own frames in its segment); ONE clips_deliver
 * launch copies each clip's own rows to rows [row_start_b, ...) of the caller's arrays.  The straddling rows are computed and never
 * delivered.  The tracked form then runs the pitch path over the COMPACTED lists with the segment list [row_start_b], straight into
 * columns 0-1 of out_records.
 * The call is asynchronous on the context's stream.  It may WAIT ON THE HOST for a previous upload of its tables (the staged uploads
 * of the segment lists and of the clip table: a buffer is reused once its last copy has left it), and it is NOT capturable into a
 * graph.  Device memory: context-owned workspaces for one group's plane and staging rows, about VBX_CLIPS_PLANE_BYTES at the default
 * group size.  Afterwards there is no state for vbx_track_stitch_f64, and the vbx_internal_last_* probes describe the last group only.
 * 8-bit sources (VBX_SAMPLE_U8 / ULAW / ALAW, one byte per sample, any byte address): every byte written for a ULAW or ALAW source
 * equals, bit for bit, what the same call writes for PCM16 on the decoded int16 samples (vbx_g711_table), and every byte written for
 * U8 equals what it writes for F64 on (b - 128) / 127 -- the bytes are decoded inside this call's own reader kernel, never in a pass before it.
 * VBX_E_INVALID, before anything is written and with the context left usable: a NULL array with n_clips > 0; a NULL clip pointer
 * with a length that gives a frame; a clip pointer not aligned to its element type (PCM24: any address); an unknown format or a
 * non-zero reserved; 0 < group_frames < VBX_CLIPS_MIN_GROUP_FRAMES; more than 0x7fffffff total rows; anything
 * vbx_analyze_frames_ex_f64 rejects.  n_clips == 0, or no clip with a frame, succeeds and writes nothing.
 * vbx_clips_plan: pure host arithmetic, no GPU.  Groups are greedy runs of whole clips in order: a group closes when the next clip
 * with frames would take it past group_frames analysed frames; a clip that is larger on its own is a group by itself.  group_frames
 * == 0: the default -- the largest count whose f64 plane (stride * 8 bytes a frame) stays within VBX_CLIPS_PLANE_BYTES, at least
 * VBX_CLIPS_MIN_GROUP_FRAMES and at most VBX_HOST_DEFAULT_CHUNK_FRAMES.  Inside a group the first clip with frames has plane_frame
 * 0 and the next one starts ceil(len / stride) frames behind it; the group analyses frames [0, plane_frame_last + n_rows_last), and
 * its plane ends where that last frame ends.  One exception: with frame_len > VBX_MAX_FRAME_LEN every clip is a group by itself,
 * whatever group_frames -- the long-frame kernels choose how they split a frame's sums from the frame count of the call, so only a
 * call of the clip's own frame count gives the resident call's bits (launches then grow with the clip count).  h_total_rows and
 * h_n_groups are optional. */
#define VBX_CLIPS_MIN_GROUP_FRAMES 64
#define VBX_CLIPS_PLANE_BYTES 268435456
typedef struct {
    int32_t format;        /* VBX_SAMPLE_* : PCM16, PCM24, PCM32, F32, F64, U8, ULAW, ALAW -- mono, contiguous samples */
    int32_t reserved;      /* must be 0 */
    size_t group_frames;   /* analysis frames per internal group; 0: the library's default */
} vbx_clip_format;
typedef struct {
    int64_t row_start;     /* first output row of the clip (prefix sum of the frame counts) */
    int64_t n_rows;        /* vbx_frame_count(len, frame_len, stride) */
    int64_t group;         /* which internal group analyses it; -1: no frame */
    int64_t plane_frame;   /* its first frame inside that group's packed plane */
} vbx_clip_row;
int vbx_clips_plan(const size_t *h_len, size_t n_clips, size_t frame_len, size_t stride, size_t group_frames,
                   vbx_clip_row *h_rows /* [n_clips] */, size_t *h_total_rows, size_t *h_n_groups);
int vbx_analyze_clips(vbx_ctx *ctx, const void *const *h_clip /* [n_clips] DEVICE pointers, in HOST memory */,
                      const size_t *h_len /* [n_clips] samples */, size_t n_clips, const vbx_clip_format *h_fmt,
                      size_t frame_len, size_t stride,
                      const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext,
                      const vbx_pitch_track_params *h_track,
                      double *out_records, size_t record_ld, int32_t *status3 /* [3, total_rows] */,
                      const vbx_pitch_track_outputs *h_outputs /* arrays of total_rows rows */);

/* ------------------------------------------------------------------ a pool of live streams (ABI 5, added) */

/* A gateway or a call-centre tap carries hundreds to thousands of INDEPENDENT calls at once, each delivering a packet per tick.
 * One vbx_session per call costs a launch chain per call and tick (about 0.29 ms a push); a multi-channel
 * session (section 5i) shares one cut into blocks and one list of marks between its channels, which independent calls do not have.
 * A session pool is max_streams stream SLOTS on one context that share one sample format (mono), one frame shape and one parameter
 * set, each slot with its own timeline: samples consumed, utterance start, carried tail, tracker state.  One TICK, vbx_pool_push,
 * hands over a list of (slot, block) entries -- any sizes, any subset of the slots, in any order -- and delivers the rows of the
 * frames each block completes, entry after entry, into ONE set of output arrays.  The kernel launches and host-to-device copies of a
 * tick do not depend on how many streams it holds.
 * Contract: for every slot, concatenate the rows all ticks delivered for it -- the records, the three status rows and, in the tracked
 * form, cand / count / peak: the result equals, bit for bit, what a one-channel vbx_session opened with the same arguments writes when
 * it is given the same blocks, marks and resets in the same order (by that session's contract: the resident call on the stream's
 * concatenated blocks with the marks as h_seg_start) -- for every way of cutting every stream into blocks, every assignment of blocks
 * to ticks (streams that skip ticks, a tick of one entry, a tick that completes no frame, an empty tick), every entry order within a
 * tick, all eight sample formats, the plain, tracked and ext forms and every LPC policy (the context's at the time of the tick;
 * tests/test_gpu_pool.py).  A NaN or Inf in one stream touches no other stream's rows.
 * vbx_pool_open: h_fmt as for vbx_session_open with channels == 1, channel == 0, chunk_frames == 0 and reserved == 0 (streams are
 * mono); frame_len <= VBX_MAX_FRAME_LEN (the long-frame kernels choose how they split a frame's sums from the frame count of the
 * call, so only a per-stream call gives the resident call's bits: use one vbx_session per stream there); a block holds at most
 * max_block_sample_frames, a tick's blocks together at most max_tick_sample_frames.  Everything is allocated here: two carry
 * regions per slot of VBX_SHARD_WARM_FRAMES * stride + frame_len - 1 elements (rounded up to 16 bytes), the tick's plane, two pinned
 * staging buffers and two raw device slots of the tick's largest byte count plus its table, the chunk-local records, status rows and
 * lists of the largest frame-loop call, max_streams tracker state rows; the largest shape is warmed by one frame-loop call with
 * max_streams segments on zeroed memory, which is also where everything only the frame loop's parts know is rejected.  Afterwards no
 * tick allocates or drains a stream on its own account.
 * vbx_pool_push: h_entries is a HOST array; entry i names a slot and a block of n_sample_frames samples in HOST memory
 * (vbx_pool_push_device: in DEVICE memory, read in stream order).  Entry i delivers n_rows_i = hi - lo of vbx_session_plan for its
 * slot into rows [row_start_i, row_start_i + n_rows_i) of every output array, row_start the prefix sum in entry order; h_rows[i] =
 * {row_start, n_rows} and *h_total_rows are reported on the host (both optional; vbx_pool_plan tells them beforehand).  out_records
 * [total_rows, record_ld] (device, 16-byte aligned), status3 row j at status3 + j * status_ld (optional), and in the tracked form
 * h_outputs as for vbx_session_push: cand and count required, peak when silence_threshold != 0, index must be NULL; columns 0-1 of
 * the records are not written.  An entry with n_sample_frames == 0 is a no-op with zero rows; an empty tick succeeds and queues
 * nothing; a tick that completes no frame only updates the carried tails.  The host form returns when every block has been read:
 * the blocks are gathered by memcpy into the pool's pinned staging, so the caller's memory is free on return, and the host runs at
 * most two ticks ahead.
 * Per tick, whatever the number of entries: ONE upload -- the gathered blocks and the tick's device table in
 * one pinned buffer and one copy on the context's stream (the device form: the table alone); ONE pool_ingest_<fmt> launch that
 * writes, through the table, every entry's plane region (the samples from read_from on: the slot's carried tail, then the block, as
 * the type the frame loop reads natively, the gap of fewer than `stride` elements behind a region zero-filled) and every entry's new
 * carried tail into the slot's OTHER carry region (each slot keeps its own ping-pong: a slot that is not pushed keeps its tail);
 * ONE frame-loop call over the plane with every entry a segment of its own (the rows between two regions lie behind an entry's own
 * frames in its own segment: the causal tracker cannot carry them into a delivered row, and they are never delivered); ONE
 * tracker_stitch_pool launch that repairs, a lane per entry, the rows of every entry that continues an utterance from its slot's
 * state row; ONE pool_deliver launch that copies each entry's own rows to the caller's rows and its last formant row to the state.
 * vbx_pool_mark_utterance / vbx_pool_reset_stream are host bookkeeping and launch nothing: the next frame the slot delivers starts a
 * new utterance; a reset slot behaves like a freshly opened session (its first push has continues_prev == 0 and reads nothing of
 * the stale tail and state) -- this is how a slot is reused for the next call.  vbx_pool_info reports a slot's sample frames
 * consumed, frames delivered and sample frames carried; vbx_pool_close frees the pool behind the work queued on the context's stream
 * (close every pool before its context).
 * The online pitch path (vbx_session_path_bind) of every slot comes from vbx_pool_path_bind, below: one more launch per tick,
 * whatever the number of streams.  An unbound pool's caller runs vbx_pitch_path_f64 over a call's rows when the call ends, as an
 * unbound session's caller does; a host-side delivery of the contour is NOT offered.  A pool, sessions and any other
 * entry point may share one context; a tick may WAIT ON THE HOST for the staged upload of two ticks ago and is not capturable into a
 * graph; afterwards the vbx_internal_last_* probes describe the tick's frame-loop call and there is no state for vbx_track_stitch_f64.
 * vbx_pool_plan: pure host arithmetic, no GPU -- per entry (consumed, utt_frame, n_new) of its slot: the vbx_session_plan_t, its rows,
 * `frames` = m = warm + n_rows analysed (0 when no frame completes) and plane_frame (-1 then); per tick total_rows and call_frames.
 * Layout (as vbx_clips_plan's): the first entry with frames has plane_frame 0; its plane region holds samples [read_from, (hi - 1) *
 * stride + frame_len) of its stream from element plane_frame * stride on; the next entry with frames starts ceil(span / stride)
 * frames behind it; call_frames = plane_frame_last + m_last, and the segment list is the list of plane_frames.
 * VBX_E_INVALID, before anything is queued and with the pool left usable and its state unchanged: a NULL where an argument is
 * required; a slot outside [0, max_streams); a slot listed twice in one tick; a block larger than max_block_sample_frames; a tick
 * whose lengths sum past max_tick_sample_frames; a device block off its type's alignment (PCM24 and the 8-bit formats: any
 * address); vbx_session_push's rules for the output arrays applied to total_rows; frame_len > VBX_MAX_FRAME_LEN; channels != 1;
 * max_streams == 0 or a largest call beyond 0x7fffffff frames. */
typedef struct vbx_pool vbx_pool;
typedef struct {
    int32_t stream;            /* the slot, in [0, max_streams) */
    const void *block;         /* n_sample_frames mono samples of the pool's format (host memory; _device: device memory) */
    size_t n_sample_frames;
} vbx_pool_entry;
typedef struct { int64_t row_start; int64_t n_rows; } vbx_pool_rows;
typedef struct {
    vbx_session_plan_t plan;   /* the slot's push */
    int64_t row_start;         /* first output row of the entry (prefix sum of n_rows in entry order) */
    int64_t n_rows;            /* plan.hi - plan.lo */
    int64_t frames;            /* frames the entry has in the tick's frame-loop call: plan.warm + n_rows; 0: no frame completes */
    int64_t plane_frame;       /* its first frame in the tick's plane; -1: no frame completes */
} vbx_pool_plan_row;
int vbx_pool_plan(const size_t *h_consumed, const size_t *h_utt_frame, const size_t *h_n_new, size_t n_entries,
                  size_t frame_len, size_t stride, vbx_pool_plan_row *h_rows /* [n_entries] */, size_t *h_total_rows,
                  size_t *h_call_frames);
int vbx_pool_open(vbx_ctx *ctx, const vbx_host_audio *h_fmt /* channels 1, channel 0, chunk_frames 0, reserved 0 */,
                  size_t frame_len, size_t stride, const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext,
                  const vbx_pitch_track_params *h_track, size_t max_streams, size_t max_block_sample_frames,
                  size_t max_tick_sample_frames, vbx_pool **out);
int vbx_pool_push(vbx_pool *pool, const vbx_pool_entry *h_entries, size_t n_entries,
                  double *out_records /* device */, size_t record_ld, int32_t *status3 /* device, optional */, size_t status_ld,
                  const vbx_pitch_track_outputs *h_outputs /* device arrays of total_rows rows */,
                  vbx_pool_rows *h_rows /* [n_entries], optional */, size_t *h_total_rows);
int vbx_pool_push_device(vbx_pool *pool, const vbx_pool_entry *h_entries, size_t n_entries,
                         double *out_records, size_t record_ld, int32_t *status3, size_t status_ld,
                         const vbx_pitch_track_outputs *h_outputs, vbx_pool_rows *h_rows, size_t *h_total_rows);
int vbx_pool_mark_utterance(vbx_pool *pool, int32_t stream);   /* the next frame the slot delivers starts a new utterance */
int vbx_pool_reset_stream(vbx_pool *pool, int32_t stream);     /* the slot behaves as that of a freshly opened pool */
int vbx_pool_info(const vbx_pool *pool, int32_t stream, size_t *h_consumed, size_t *h_frames, size_t *h_carried);
void vbx_pool_close(vbx_pool *pool);

/* The live pitch contour of every slot (ABI 5, added): what vbx_session_path_bind is to a one-channel session.
 * vbx_pool_path_bind, on a pool opened with h_track, gives every slot an online path of its own (vbx_path_stream_open's state and
 * ring of max_pending frames, P = peak_ref, time_step == 0 meaning stride / sample_rate as in the tracked call) over the POOL-OWNED
 * lists of a tick's frame-loop call -- the caller's h_outputs arrays are not read -- and from then on every vbx_pool_push /
 * _push_device queues ONE more launch behind pool_deliver, pitch_path_online_pool, whatever the number of entries: a lane group per
 * VISITED slot, which are every entry with n_sample_frames > 0 (one that completes no frame reports n = 0 and what is pending, as a
 * bound session's push does) and every slot with a deferred mark or reset, listed in the tick or not.  The launch's table (slot,
 * first list row, frame count, flags) travels in the tick's single pinned buffer and single copy.
 * Layout: everything slot s commits in a tick goes to rows [s * slot_rows, s * slot_rows + n) of out_path (rows path_ld doubles
 * apart; columns 0-1 are written), out_index and out_forced (both optional), and its vbx_path_commit to d_commit[s]: slot-indexed and
 * fixed, because the committed counts exist only on the device.  slot_rows >= vbx_pool_path_slot_rows(max_pending,
 * max_block_sample_frames, stride) = max_pending + ceil(max_block_sample_frames / stride): a slot never writes more than the frames
 * it held plus the frames its block completes.  Rows past n, and the rows and records of slots a tick does not visit, are not touched:
 * read d_commit[s] behind a tick that visited s.
 * On a bound pool vbx_pool_mark_utterance and vbx_pool_reset_stream stay host bookkeeping that launches nothing; for the path they are
 * DEFERRED to the next tick's launch.  A marked slot first ends its path utterance -- all pending frames go along the leader's trace
 * with out_forced = 0, as end_utterance does -- and then scans its new frames, if any, as a new utterance; the rows of both follow
 * each other in the slot's area and d_commit[s] is the merge of the two: `first` of the first, n and n_forced summed, `pending` of the
 * last.  A reset slot has its path state zeroed first (vbx_path_stream_reset: pending frames are dropped, the counters restart at 0),
 * before anything else for that slot: to keep the rest of a call's contour, mark, tick, then reset.  An EMPTY tick (n_entries == 0) on
 * a bound pool with marked or reset slots queues the single upload and the single path launch for them -- the tail of a contour
 * without audio; with nothing flagged it queues nothing, as before.
 * Contract: for every slot, the rows, indices and forced flags of all ticks, concatenated, are those a bound one-channel session
 * writes on the same blocks, marks and resets, bit for bit, for every cut into blocks, every assignment to ticks and every entry
 * order (tests/test_gpu_pool_path.py); by that session's contract, with silence_threshold == 0 the unforced rows are columns 0-1 and
 * `index` of the resident tracked call, and with silence_threshold > 0 those of the shard protocol with seg_peak = peak_ref.
 * The first bind comes before the first tick that queues work and allocates the slots' states (zeroed) and rings; a later bind with
 * the same peak_ref, max_pending and slot_rows only changes the destinations and keeps the state.  The binding lasts until
 * vbx_pool_close; an unbound pool runs exactly what it ran before.
 * VBX_E_INVALID, with nothing queued and the pool usable: a NULL pool, h_out, out_path or d_commit; a pool without h_track; a first bind
 * after work was queued; a rebind that changes peak_ref, max_pending or slot_rows; path_ld < 2; max_pending of 0 or above 2^24;
 * slot_rows below the minimum; silence_threshold > 0 with peak_ref negative or not finite.  An allocation failure (VBX_E_RUNTIME)
 * leaves the pool unbound and usable. */
typedef struct {
    vbx_pitch *out_path;        /* device: max_streams * slot_rows rows, rows path_ld doubles apart */
    int32_t *out_index;         /* device, optional: max_streams * slot_rows */
    uint8_t *out_forced;        /* device, optional: max_streams * slot_rows */
    vbx_path_commit *d_commit;  /* device: max_streams records */
} vbx_pool_path_outputs;
size_t vbx_pool_path_slot_rows(size_t max_pending, size_t max_block_sample_frames, size_t stride);  /* host arithmetic, no GPU */
int vbx_pool_path_bind(vbx_pool *pool, double peak_ref, size_t max_pending,
                       const vbx_pool_path_outputs *h_out, size_t path_ld, size_t slot_rows);

/* ------------------------------------------------------------------ multi-GPU: frame-range sharding */

/* The reference has no distribution of any kind; frames are independent (the tracker per utterance), so a long
 * recording shards by contiguous frame ranges, one process per GPU, and the only exchange is ONE gather of the
 * fixed-size per-frame records to a destination rank: grouped ncclSend / ncclRecv (RCCL), each peer's payload
 * crossing its own xGMI link.  No reduction, no all-to-all.
 *
 * vbx_shard_range: frames [*lo, *hi) of rank `rank`: the even split (first ranks take the remainder); with h_seg_start
 * (ascending utterance starts, h_seg_start[0] == 0) a cut moves up to an utterance start that lies within 1/32 of a shard
 * after it.  A cut INSIDE an utterance is fine: ONE long utterance -- what the reference's user loop over a file produces
 * (tests/lib.rs:75-79, src/spectrum.rs:357-369) -- splits evenly, and its formant track is carried across the cut (below).
 * vbx_shard_samples: the samples [*s0, *s1) those frames read, i.e. including the frame_len - hop halo. */
int vbx_shard_range(size_t n_frames, int world, int rank, const int64_t *h_seg_start, size_t n_segments,
                    size_t *lo, size_t *hi);
int vbx_shard_samples(size_t lo, size_t hi, size_t frame_len, size_t hop, size_t *s0, size_t *s1);

/* The formant tracker is the one sequential step of the path (EstimateFormants, src/spectrum.rs:232-333: the estimates after
 * frame t feed frame t + 1).  A rank whose range starts inside an utterance therefore
 *   1. analyses `warm` extra frames before its range, frames [lo - warm, hi), starting the tracker from the initial estimates:
 *      the tracker forgets -- after a few dozen frames its state no longer depends on where it started -- so the rows of
 *      [lo, hi) are, almost always, already the sequential scan's;
 *   2. receives the formant row its predecessor ENDS with (the true state before frame lo), compares it bit for bit with its
 *      own row of frame lo - 1, and where they differ redoes the scan from the true state until it meets rows it already
 *      holds (vbx_track_stitch_f64; over a communicator: vbx_comm_stitch_tracks_f64, which also passes the rank's own last
 *      row on).  The result is the single-process scan, bit for bit, for every world size.
 * vbx_shard_plan: lo, hi as vbx_shard_range; warm = min(frames since the utterance's start, VBX_SHARD_WARM_FRAMES);
 * stop = index, counted from frame lo - warm, at which the utterance that holds frame lo ends inside the shard (or the
 * shard's end); continues_prev: the utterance starts more than `warm` frames before lo (the state must come from rank - 1);
 * continues_next: the same for the next rank's first frame.
 * vbx_shard_local_segments: the utterance starts of frames [lo - warm, hi), re-based to the shard (first entry 0): the
 * h_seg_start of the rank's vbx_analyze_frames_f64 / vbx_find_formants_f64 call.  *n_out = entries needed (h_out may be NULL).
 * The formant track is carried across a cut by vbx_track_stitch_f64, the pitch path of vbx_pitch_path_f64 /
 * vbx_analyze_frames_tracked_* by vbx_pitch_path_shard_*_f64 (further down), over the same plan. */
#define VBX_SHARD_WARM_FRAMES 64
typedef struct {
    size_t lo, hi, warm, stop;
    int continues_prev, continues_next;
} vbx_shard_plan_t;
int vbx_shard_plan(size_t n_frames, int world, int rank, const int64_t *h_seg_start, size_t n_segments, vbx_shard_plan_t *h_out);
int vbx_shard_local_segments(const vbx_shard_plan_t *h_plan, const int64_t *h_seg_start, size_t n_segments,
                             int64_t *h_out, size_t cap, size_t *n_out);
/* Pure host arithmetic: chunk c of a host-resident recording of n_frames frames cut every chunk_frames frames (vbx_analyze_host).
 * h_out: lo, hi = the chunk's own frames [c * chunk_frames, min(n_frames, (c + 1) * chunk_frames)); warm = min(frames since the
 * utterance of frame lo began, VBX_SHARD_WARM_FRAMES) frames analysed before them; stop = index, counted from frame lo - warm, at
 * which that utterance ends inside the chunk (or the chunk's end); continues_prev: frame lo is not an utterance start (the tracker's
 * state comes from row lo - 1; with warm < VBX_SHARD_WARM_FRAMES the warm-up began at the utterance's start and the stitch changes
 * nothing); continues_next: the same for frame hi.  [*s0, *s1): the sample frames of frames [lo - warm, hi), what the chunk uploads.
 * VBX_E_INVALID: a NULL output, chunk_frames 0, frame_len or stride 0, c beyond the last chunk, a bad segment list. */
int vbx_host_chunk_plan(size_t n_frames, size_t chunk_frames, size_t c, size_t frame_len, size_t stride,
                        const int64_t *h_seg_start, size_t n_segments, vbx_shard_plan_t *h_out, size_t *s0, size_t *s1);
/* Step 2 on one device: `formants` are the rows the LAST vbx_find_formants_f64 (out_formants, formants_ld = 2 n_est) or
 * vbx_analyze_frames_* call (out_records + 2, formants_ld = record_ld) on this context wrote, n_frames of them (call it right
 * after that call: it reads the resonance rows the context still holds); d_state_in (device, n_est entries) is the true state
 * before frame `first`; rows [first, stop) are corrected where needed.  *d_changed (device, optional) = rows rewritten.
 * Alignment: formants as the call that wrote them took it (8 bytes for out_formants; the records' 16), d_state_in 8, d_changed 4. */
int vbx_track_stitch_f64(vbx_ctx *ctx, vbx_resonance *formants, size_t n_frames, size_t formants_ld, size_t first, size_t stop,
                         const vbx_resonance *d_state_in, int32_t *d_changed);

/* The pitch path across a shard cut (ABI 5, added): the rows every rank writes are those of vbx_pitch_path_f64 on the whole
 * recording, bit for bit in out_path and equal in out_index, for any world size, cut positions, segment list, kmax and
 * chunk_frames.  A rank analyses local frames [0, n) = global frames [lo - warm, hi) of vbx_shard_plan; first = warm: local
 * frames [0, first) precede its range (they are analysed so that frame first - 1, the frame before the cut, has its list here:
 * both ranks compute the list of a shared frame from the same samples with the same kernel, so its rows -- and with them the
 * list positions the states are named by -- are the same bits on both; the formant stitch rests on the same property).
 * Three small device arrays cross a cut:
 *   state     VBX_PITCH_PATH_STATES doubles: the normalised D of ONE frame in that frame's state order (list positions
 *             0..m-1, the appended unvoiced state at m), -inf where there is no state.  The frame is the one before the cut:
 *             the sender's last (hi - 1), the receiver's local frame first - 1.
 *   back map  VBX_PITCH_PATH_STATES int32: back_map[s] = the state of local frame first - 1 on the path that is in state s at
 *             the rank's last frame n - 1 (constant when the utterance of frame first - 1 ends inside the shard; 0 beyond the
 *             states; all 0 when first == 0).
 *   end state one int32: the state of the rank's last frame on the whole recording's path.
 * The silence term couples the ranks once more: u_t divides by P, the largest local_peak of the whole utterance.
 * vbx_pitch_path_segment_peaks_f64 returns the NaN-ignoring max of local_peak per LOCAL segment (out_peak: device,
 * n_segments entries, 1 when h_seg_start is NULL; NaN for an empty segment); the caller takes the max over the ranks that
 * share a cut utterance and hands the result to _begin as seg_peak, which then REPLACES P of every local segment (NULL: P is
 * the local max, as in vbx_pitch_path_f64).
 * The protocol, every call asynchronous on the context's stream:
 *   1. _begin on every rank, in any order: the speculative scan of all local frames, with nothing from another rank.
 *      Arguments as vbx_pitch_path_f64; cand / count / status / local_peak must stay valid until _finish.  With continues_prev
 *      local frame 0 is not the utterance's start.  VBX_E_INVALID: what vbx_pitch_path_f64 rejects, first > n_frames,
 *      continues_prev with first == 0 or with an utterance start within [1, first], either flag with n_frames == 0,
 *      continues_next with an empty last utterance.
 *   2. _enter in rank order, each passing its d_state_out on as the next rank's d_state_in (NULL exactly when the rank was
 *      begun without continues_prev): d_state_in is compared bit for bit with the scan's own D of frame first - 1; where they
 *      differ the chunk that begins at `first` is redone from the true state and the repair is carried on, chunk by chunk,
 *      inside that utterance only, until it meets states the scan already holds.  Then d_state_out (the D of frame n - 1;
 *      d_state_in passed through when first == n_frames) and d_back_map are written; either may be NULL.
 *      *d_changed (device, optional) = chunks this call redid.  d_state_out may be d_state_in.
 *   3. on the host, from the last rank backwards: end[r] = back_map[r + 1][end[r + 1]] wherever rank r continues into r + 1.
 *   4. _finish on every rank, in any order: d_end_state (device; NULL exactly when the rank was begun without
 *      continues_next: its last utterance ends at its own leader) selects the path; rows [first, n) are written, row t at
 *      out_path + t * path_ld doubles (path_ld = 2: dense rows; record_ld: columns 0-1 of frame records) and out_index[t]
 *      (optional); rows [0, first) are not touched.  An end state outside the frame's states is taken modulo the row width.
 * _enter and _finish continue the context's LAST _begin: after any other path or frame-batch call on the context they return
 * VBX_E_INVALID (the rule of vbx_track_stitch_f64), as does _finish before _enter; nothing is written then and the context
 * stays usable.  vbx_internal_last_path_chunks_redone reports the running count of _begin's and _enter's repairs. */
#define VBX_PITCH_PATH_STATES 64
int vbx_pitch_path_segment_peaks_f64(vbx_ctx *ctx, const double *local_peak, size_t n_frames, const int64_t *h_seg_start,
                                     size_t n_segments, double *out_peak);
int vbx_pitch_path_shard_begin_f64(vbx_ctx *ctx, const vbx_pitch *cand, const int32_t *count, const int32_t *status,
                                   size_t n_frames, size_t kmax, const double *local_peak, const double *seg_peak,
                                   const int64_t *h_seg_start, size_t n_segments, const vbx_pitch_path_params *h_params,
                                   size_t first, int continues_prev, int continues_next);
int vbx_pitch_path_shard_enter_f64(vbx_ctx *ctx, const double *d_state_in, double *d_state_out, int32_t *d_back_map,
                                   int32_t *d_changed);
int vbx_pitch_path_shard_finish_f64(vbx_ctx *ctx, const int32_t *d_end_state, vbx_pitch *out_path, size_t path_ld,
                                    int32_t *out_index);

typedef struct vbx_comm vbx_comm;
#define VBX_UNIQUE_ID_BYTES 128
#define VBX_COMM_SLOTS 4
/* ncclGetUniqueId on the root; the caller ships the 128 bytes to the other ranks (MPI, TCP store, file ...). */
int vbx_comm_unique_id(void *h_id);
/* One communicator per (context, process): rank `rank` of `world` on the context's device.  Collective call. */
int vbx_comm_create(vbx_ctx *ctx, const void *h_id, int world, int rank, vbx_comm **out);
void vbx_comm_destroy(vbx_comm *comm);
/* Gathers per-frame records to rank dst: rank r contributes h_rows[r] rows of row_doubles doubles (`local`, device),
 * which land in `out` (device, on dst only) at row offset h_rows[0] + .. + h_rows[r-1].  On dst, `local` may point
 * into `out` at its own offset (kernels write their records in place: no copy).  The transfer is queued on the
 * communicator's own stream behind the work already queued on the context's stream, so the context's next
 * batch overlaps it; `slot` in [0, VBX_COMM_SLOTS) names the buffer being sent for vbx_comm_wait. */
int vbx_gather_records_f64(vbx_ctx *ctx, vbx_comm *comm, const double *local, const int64_t *h_rows,
                           size_t row_doubles, int dst, double *out, int slot);
/* Step 2 across ranks (RCCL, on the communicator's stream, behind the work queued on the context's stream): receives the
 * previous rank's last formant row when h_plan->continues_prev (it sends it after its own stitch: the ranks of one utterance
 * form a chain of 2 n_est doubles each over the direct xGMI links), corrects this rank's rows, and sends this rank's last row
 * on when h_plan->continues_next.  n_frames = hi - lo + warm rows as in vbx_track_stitch_f64.  Queue the record gather after
 * it with the same `slot`: vbx_comm_wait(slot) then covers both.  A rank that receives makes the context's stream wait (on
 * the device) until its stitch is through: the repair reads the resonance rows the context holds, which the context's next
 * call overwrites.  Errors: argument / plan checks run before the first RCCL call; once this rank's receive is posted its send
 * is posted too whatever fails in between (the next rank waits for it), and the first error is returned afterwards -- a
 * VBX_E_* from this call means the chain's rows are not to be trusted: destroy the communicator on EVERY rank. */
int vbx_comm_stitch_tracks_f64(vbx_ctx *ctx, vbx_comm *comm, vbx_resonance *formants, size_t n_frames, size_t formants_ld,
                               const vbx_shard_plan_t *h_plan, int32_t *d_changed, int slot);
/* The transfer list of that gather as one rank sees it, on the host (no GPU, no RCCL: what vbx_gather_records_f64 posts,
 * exposed so that a caller -- and the CPU tests -- can check the layout for any world size and uneven h_rows):
 * for every rank r, h_offset[r] = element offset (doubles) of rank r's rows in `out`, h_count[r] = doubles rank r
 * contributes; h_op[r] = what THIS rank does for peer r: VBX_GATHER_NONE, VBX_GATHER_RECV (this rank is dst and r sends),
 * VBX_GATHER_SEND (r == dst and this rank has rows), VBX_GATHER_COPY (r == rank == dst: device copy unless in place).
 * Arrays of `world` entries; any of the three may be NULL. */
enum { VBX_GATHER_NONE = 0, VBX_GATHER_RECV = 1, VBX_GATHER_SEND = 2, VBX_GATHER_COPY = 3 };
int vbx_gather_plan(const int64_t *h_rows, int world, int rank, int dst, size_t row_doubles,
                    int64_t *h_offset, int64_t *h_count, int32_t *h_op);
/* Live communicators of this process (the bench prints it: exactly one RCCL instance per rank). */
int vbx_comm_live_count(void);
/* Makes the context's stream wait (on the device, not the host) until the gather that used `slot` has finished:
 * call before overwriting that buffer. */
int vbx_comm_wait(vbx_ctx *ctx, vbx_comm *comm, int slot);
/* Host waits for every queued gather. */
int vbx_comm_sync(vbx_comm *comm);
/* Loopback self-test: a grouped ncclSend/ncclRecv of n doubles from this rank to itself on the communicator's
 * stream, verified on the host.  Exercises the RCCL path on a single GPU.  Returns 0 when the data arrived intact. */
int vbx_comm_selftest(vbx_ctx *ctx, vbx_comm *comm, size_t n_doubles);

/* ------------------------------------------------------------------ bench utility */

/* Deterministic speech-like synthetic audio (DESIGN.md "synthetic signal"): samples
 * [sample_offset, sample_offset + n_samples) of an endless 48 kHz-style stream defined in
 * closed form per sample, so any shard can be generated in place on its own GPU. */
int vbx_synth_speech_f64(vbx_ctx *ctx, double *out, size_t n_samples, uint64_t sample_offset,
                         double sample_rate, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* VOXBOX_HIP_H */
