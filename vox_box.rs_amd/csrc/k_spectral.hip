// k_spectral.hip -- one spectral pass per frame feeding pitch, LPC and MFCC: the transform of 2400 real points, for frames of
// 1200 samples (25 ms at 48 kHz) and, zero padded, of 1025..1199 (k_spectral_pow2*.hip hold the 1024 / 2048 / 4096 forms).
// The same kernel also serves MFCC::mfcc alone and Autocorrelate::autocorrelate with many lags (MODE), and this file holds
// the host side shared by all forms: which transform serves a frame length (spectral_plan), the twiddle tables, the launch.
//
// Reference rows served: A1-A3 (autocorrelate, normalize, lag window), A4-A9 (pitch, through
// vbx_pitch_refine.hpp), A10 (lpc on r[0..12]), A14 (mfcc).  What the reference computes with an O(N^2) fold per lag
// (src/periodic.rs:276-289) and a separate rustfft call (src/spectrum.rs:416-419) is here ONE real FFT of the
// zero-padded windowed frame, length M = 2N = 2400:
//     X = FFT_M(x_w padded)                      |X[k]|^2 -> inverse FFT -> S[lag] = sum_i x[i] x[i+lag], every lag
//     X[2k'] = the N-point DFT bin k' of the frame  -> the |X|^2 and |X| the mel filters of MFCC::mfcc read
//     S[0..12]                                      -> the lag sums of LPC::lpc (round 6: the recursion itself, like MFCC's log10 + DCT,
//                                                      runs afterwards in levinson_rows_kernel_t, k_lpc.hip: a lane per record)
// (Q1: the reference's fold is seeded with x[0], r[lag] = S[lag] - x0*x[lag] + x0; applied afterwards.)  This replaces
// 1.44 MFLOP of autocorrelation MACs per frame by about 0.3 MFLOP and removes the MFCC and LPC kernels' passes over the
// same frame.  Accuracy: forward + inverse f64 FFT, error ~1e-16 * S[0] per lag (measured against the oracle in
// tests/test_gpu_parity.py), far inside the 1e-6 relative tolerance of the autocorrelation / LPC / MFCC rows.
//
// One wavefront per frame, the transform lives in registers:
//   real FFT by the packing trick: z[j] = x[2j] + i x[2j+1], complex FFT of length N_c = 1200 = 20 * 20 * 3, then the
//   split into the spectrum of the real sequence; the inverse likewise with the roles exchanged.
//   complex FFT (decimation in frequency, n = 60 a + 3 b + c, k = ka + 20 kb + 400 kc):
//     stage 1  lane n' = 3b + c (60 lanes): 20-point DFT over a in registers (4 x 5 prime-factor form, no twiddles
//              inside), times W_1200^(n' ka)
//     stage 2  lane (ka, c) (60 lanes): 20-point DFT over b, times W_60^(c kb)
//     stage 3  lane q = ka + 20 kb, 7 per lane: 3-point DFT over c -> X[q + 400 kc], natural order
//   between the stages the values change lanes through LDS, real and imaginary parts in two passes (one 1200-double
//   buffer, which the lag curve y later overwrites: the frame state stays at 13.5 KB = 12 wavefronts per CU).
#include "vbx_spectral_1200.hpp"

namespace vbx {

static size_t spectral_lds_bytes(int n) {
    size_t need = (size_t)pitch_refine_lds_bytes(n);
    const size_t t2_end = (size_t)SP_T2_LDS_OFFSET + 60 * sizeof(double2);     // exchange buffer | mel sums | T2 copy
    if (t2_end > need) need = t2_end;
    return (need + 15) & ~(size_t)15;
}

int spectral_plan(int n) {
    static const int min_n = [] { const char *e = getenv("VBX_SPECTRAL_MIN_N"); return e ? atoi(e) : SPECTRAL_MIN_N; }();
    if (n < min_n || n < 64) return SPECTRAL_PLAN_NONE;
    if (n <= 1024) return SPECTRAL_PLAN_1024;
    if (n <= SP_N) return SPECTRAL_PLAN_1200;
    if (n <= 2048) return SPECTRAL_PLAN_2048;
    if (n <= 4096) return SPECTRAL_PLAN_4096;
    return SPECTRAL_PLAN_NONE;
}

int spectral_plan_nc(int plan) {
    return plan == SPECTRAL_PLAN_1200 ? SP_N : plan == SPECTRAL_PLAN_1024 ? 1024 : plan == SPECTRAL_PLAN_2048 ? 2048 :
           plan == SPECTRAL_PLAN_4096 ? 4096 : 0;
}

int spectral_tab_complex(int plan) {
    return plan == SPECTRAL_PLAN_1200 ? SPECTRAL_TAB_COMPLEX : spectral_pow2_tab_complex(plan);
}

// twiddles, evaluated in long double and rounded once
void spectral_fill_tab(int plan, double *h) {
    if (plan != SPECTRAL_PLAN_1200) { spectral_pow2_fill_tab(plan, h); return; }
    const long double two_pi = 6.283185307179586476925286766559005768L;
    size_t o = 0;
    auto put = [&](long num, long den) {             // e^{-2 pi i num / den}
        const long double ang = two_pi * (long double)(num % den) / (long double)den;
        h[o++] = (double)cosl(ang); h[o++] = (double)(-sinl(ang));
    };
    for (long np = 0; np < 60; np++) for (long ka = 0; ka < 20; ka++) put(np * ka, 1200);
    for (long c = 0; c < 3; c++) for (long kb = 0; kb < 20; kb++) put(c * kb, 60);
    for (long m = 0; m <= 600; m++) put(m, 2400);
}

// The fused kernel serves: pitch for every frame length with a plan; LPC of order 12 with it; MFCC with it when the frame
// divides the transform (the mel filters read the n-point DFT bins = every (M / n)-th bin of the M-point transform).
bool spectral_supported(int n, int lpc_order, int mfcc_nb, int mfcc_b_lo, int num_coeffs) {
    const int plan = spectral_plan(n);
    if (plan == SPECTRAL_PLAN_NONE) return false;
    if (lpc_order != 0 && lpc_order != SP_LPC_P) return false;
    if (num_coeffs != 0 && ((2 * spectral_plan_nc(plan)) % n != 0 || (n & 1) || num_coeffs > 64 || mfcc_nb < 1 || mfcc_b_lo < 0 || mfcc_b_lo + mfcc_nb > n / 2)) return false;
    return true;
}

// The plan for the fused frame loop when MFCC is wanted: the frame's DFT bins must be bins of the transform, i.e. the frame
// length must divide the transform's M = 2 Nc.  512 divides the 1024 plan's 2048; 600 and 800 do not, but they divide the
// 1200 plan's 2400 -- a 17 % longer transform instead of a second kernel over the same frames (MFCC::mfcc alone costs about
// what the whole fused kernel does).
int spectral_plan_mfcc(int n) {
    const int plan = spectral_plan(n);
    if (plan == SPECTRAL_PLAN_NONE) return plan;
    if ((2 * spectral_plan_nc(plan)) % n == 0) return plan;
    if (n <= SP_N && (2 * SP_N) % n == 0 && !(n & 1)) return SPECTRAL_PLAN_1200;
    return plan;
}
bool spectral_supported_plan(int plan, int n, int lpc_order, int mfcc_nb, int mfcc_b_lo, int num_coeffs) {
    if (plan == SPECTRAL_PLAN_NONE || n > spectral_plan_nc(plan)) return false;
    if (lpc_order != 0 && lpc_order != SP_LPC_P) return false;
    if (num_coeffs != 0 && ((2 * spectral_plan_nc(plan)) % n != 0 || (n & 1) || num_coeffs > 64 || mfcc_nb < 1 || mfcc_b_lo < 0 || mfcc_b_lo + mfcc_nb > n / 2)) return false;
    return true;
}

// ---- tables of the interpolated MFCC bins (mfcc_interp_t, vbx_kernels.hpp), host side, in long double ----
// threads per frame of the plan's kernel (the bins are dealt to them) and the LDS the interpolation may use: what costs at most one
// of the twelve / eight frames of a CU (a chirp-z kernel over the same frames costs more), none of the 4096-point plan's four
static void mfcc_interp_geom(int plan, long *M, int *nt, int *lds_cap) {
    *M = 2L * spectral_plan_nc(plan);
    *nt = plan == SPECTRAL_PLAN_4096 ? 128 : 64;
    *lds_cap = (plan == SPECTRAL_PLAN_1200 || plan == SPECTRAL_PLAN_1024) ? (160 * 1024) / 11 : plan == SPECTRAL_PLAN_2048 ? (160 * 1024) / 7 : (160 * 1024) / 4;
}
static int mfcc_interp_slots(int plan, int nb) { long M; int nt, cap; mfcc_interp_geom(plan, &M, &nt, &cap); return (nb + nt - 1) / nt; }

// Taps per bin.  The cut's error falls like e^{-pi tau W} / (pi W / 2) (tau = 1/2 - n / 2M, the Kaiser-Bessel bump's half-width; the sinc's
// envelope at the cut): 40 taps up to M / n = 2.47, 32 up to 5, 24 beyond hold it at ~1e-15 of the transform's largest |X| -- the size of
// the transform's own rounding, so that the interpolation is never the limiting term, whatever the frame's dynamic range
// (tests/test_mfcc_interp_table.py measures every class against the exact DFT: < 1e-14; tests/test_gpu_analyze.py: a pure tone, whose
// filters hold only leakage).  The first choice of round 5 -- 32 taps at M / n = 2.18: 4e-13 -- measured no faster (29.3 against 29.6 M frames/s
// at 1103 / 441 on one box, 30.3 against 30.0 on another: ~1 %) and passed the same tests; kept as VBX_EXP_INTERP_FEWER_TAPS.
int mfcc_interp_taps(int plan, int n) {
    long M; int nt, cap; mfcc_interp_geom(plan, &M, &nt, &cap);
    const double tau = 0.5 - (double)n / (2.0 * (double)M);
#ifdef VBX_EXP_INTERP_FEWER_TAPS
    return tau >= 0.36 ? 24 : tau >= 0.268 ? 32 : MFCC_INTERP_MAX_TAPS;
#endif
    return tau >= 0.401 ? 24 : tau >= 0.298 ? 32 : MFCC_INTERP_MAX_TAPS;     // the smallest W of 24 / 32 / 40 with e^{-pi tau W} / (pi W / 2) <= 2e-15
}

size_t mfcc_interp_table_bytes(int plan, int nb) {
    long M; int nt, cap; mfcc_interp_geom(plan, &M, &nt, &cap);
    const size_t slots = (size_t)mfcc_interp_slots(plan, nb);
    return (size_t)(M / 4 + 1) * 16 + slots * (MFCC_INTERP_MAX_TAPS / 2) * nt * 16 + slots * nt * 4;
}
size_t mfcc_interp_coef_offset(int plan) { return (size_t)(2L * spectral_plan_nc(plan) / 4 + 1) * 16; }
size_t mfcc_interp_j0_offset(int plan, int nb) {
    long M; int nt, cap; mfcc_interp_geom(plan, &M, &nt, &cap);
    return mfcc_interp_coef_offset(plan) + (size_t)mfcc_interp_slots(plan, nb) * (MFCC_INTERP_MAX_TAPS / 2) * nt * 16;
}

bool mfcc_interp_fill(int plan, int n, int b_lo, int nb, void *h_table, mfcc_interp_t *d) {
    if (plan == SPECTRAL_PLAN_NONE) return false;
    long M; int NT, cap;
    mfcc_interp_geom(plan, &M, &NT, &cap);
    const long quarter = M / 4;
    if (n < 2 || 2L * n > M || M % n == 0 || nb < 1 || nb > 4096 || b_lo < 0) return false;
    const int SL = mfcc_interp_slots(plan, nb);
    const int W = mfcc_interp_taps(plan, n), HT = W / 2;
    const long double pi = 3.141592653589793238462643383279502884L;
    const long double tau = 0.5L - (long double)n / (2.0L * (long double)M);                   // the bump's half-width
    const long double beta = pi * tau * (long double)W;
    auto sinhc = [](long double s) { return s < 1e-6L ? 1.0L + s * s / 6.0L : sinhl(s) / s; };
    const long double norm = sinhc(beta);
    char *base = static_cast<char *>(h_table);
    double *rot = reinterpret_cast<double *>(base);
    double *coef = reinterpret_cast<double *>(base + mfcc_interp_coef_offset(plan));
    int32_t *j0t = reinterpret_cast<int32_t *>(base + mfcc_interp_j0_offset(plan, nb));
    for (long j = 0; j <= quarter; j++) {                                                      // e^{2 pi i j c / M}, c = (n - 1) / 2
        const long double ang = 2.0L * pi * (long double)((j * (long)(n - 1)) % (2 * M)) / (long double)(2 * M);
        rot[2 * j] = (double)cosl(ang); rot[2 * j + 1] = (double)sinl(ang);
    }
    long jmin = 1L << 40, jmax = -(1L << 40);
    for (int i = 0; i < nb; i++) {
        const long first = ((long)(b_lo + i) * M) / n - W / 2 + 1;
        if (first < jmin) jmin = first;
        if (first + W - 1 > jmax) jmax = first + W - 1;
    }
    if (jmax > quarter || jmin < -quarter) return false;
    for (int i = 0; i < NT * SL; i++) {
        const int u = i / NT, th = i % NT;
        const long k = b_lo + i;
        const long first = (i < nb) ? (k * M) / n - W / 2 + 1 : jmin;
        j0t[i] = (int32_t)(first - jmin);
        for (int t = 0; t < W; t++) {
            long double c = 0.0L;
            if (i < nb) {
                const long num = k * M - (first + t) * (long)n;                                // nu = num / n, |nu| <= W / 2
                if (num == 0) c = 1.0L;
                else {
                    const long double nu = (long double)num / (long double)n;
                    long r = num % (2L * n); if (r < 0) r += 2L * n;                           // sin(pi nu) from the reduced numerator
                    const long double sn = sinl(pi * (long double)r / (long double)n);
                    const long double arg = beta * beta - (2.0L * pi * tau * nu) * (2.0L * pi * tau * nu);
                    const long double bump = sinhc(arg > 0.0L ? sqrtl(arg) : 0.0L) / norm;
                    c = sn / (pi * nu) * bump;
                }
            }
            coef[(((size_t)u * HT + t / 2) * NT + th) * 2 + (t & 1)] = (double)c;
        }
    }
    const int zn = (int)(jmax - jmin + 1), nbp = (nb + 1) & ~1;
    d->jmin = (int)jmin; d->jmax = (int)jmax; d->taps = W;
    d->pu_off = 2 * zn;
    d->lds_bytes = (2 * zn + 2 * nbp + 64) * 8;
    d->rot = nullptr; d->coef = nullptr; d->j0 = nullptr;                                      // the caller's: device addresses
    return d->lds_bytes <= cap;
}

// The launch-specialised instance (SP_SPEC_*, vbx_spectral.hpp) serves the three-wavefront launch of full f64 / PCM frames with
// everything it was compiled for in place; every other launch -- and every launch of an experiment build that reads the work
// pointer or the count early (VBX_EXP_PHASES, VBX_EXP_STOP) -- takes the generic one.  L.allow_spec: the context's
// VBX_SPECTRAL_SPEC switch (0: the generic one; A/B, tests).  w3, extra: choose_analyze's own three-wavefront decision and LDS list.
static bool spectral_want3() {
    static const bool want3 = [] { const char *e = getenv("VBX_SPECTRAL_W3"); return e == nullptr || atoi(e) != 0; }();
    return want3;
}
static int spectral_spec(const spectral_launch_t &L, bool w3, size_t extra) {
#if defined(VBX_EXP_PHASES) || VBX_EXP_STOP != 0
    return SP_SPEC_NONE;
#else
    if (!L.allow_spec || !w3 || extra != 0 || L.plan != SPECTRAL_PLAN_1200 || L.n != SP_N || L.mfcc_only || L.out_r != nullptr) return SP_SPEC_NONE;
    if (L.x.kind != SAMPLE_F64 && L.x.kind != SAMPLE_PCM16) return SP_SPEC_NONE;
    if (!L.lag_rcp || pitch_full_list_bytes(L.n, L.kmax) != 0) return SP_SPEC_NONE;
    if (L.out_mfcc != nullptr && !(L.mfcc_defer && L.num_coeffs <= 16)) return SP_SPEC_NONE;
    return L.x.kind == SAMPLE_PCM16 ? SP_SPEC_PCM16 : SP_SPEC_F64;
#endif
}

// THE choice (vbx_kernels.hpp): which instance of which family serves L, with what geometry -- or none (refused).
analyze_choice_t choose_analyze(const spectral_launch_t &L) {
    analyze_choice_t c{};
    c.plan = L.plan; c.sample = L.x.kind; c.burg = L.burg_scratch != nullptr; c.spec = SP_SPEC_NONE;
    // (PCM / float32: full 1200-sample frames only -- the host side asks for nothing else; Burg's lag sums: launch-specialised instances only)
    c.refused = L.x.kind != SAMPLE_F64 && (L.plan != SPECTRAL_PLAN_1200 || L.n != SP_N);
    if (c.refused) return c;
    if (L.plan != SPECTRAL_PLAN_1200) {
        if (c.burg) c.refused = true; else c = choose_analyze_pow2(L);
        return c;
    }
    c.family = SP_FAMILY_1200;
    const size_t base = spectral_lds_bytes(L.n);
    size_t extra = pitch_full_list_bytes(L.n, L.kmax);
    c.list = extra ? SP_LIST_LDS : SP_LIST_LANES; c.full_off = extra ? (int)base : 0;
    // kmax = VBX_PITCH_MAX_CANDIDATES(frame_len) (the whole Vec of every frame fits its output row): the refined candidates
    // are parked in the row itself instead of an extra LDS region, which keeps the frame state at 13.5 KB = twelve
    // wavefronts per CU (the form compiled for three wavefronts per SIMD, below).  The parked list is read and written as double2: only
    // where the rows are 16-byte aligned -- cand_ld is even, so the base decides; a caller's vbx_pitch array at 8 mod 16 keeps the list
    // in LDS, the same candidates in the same order.
    const bool rows16 = (((uintptr_t)L.out_cand) & 15) == 0 && (L.cand_ld & 1) == 0;
    if (extra != 0 && L.kmax >= pitch_full_list_entries(L.n) && L.out_r == nullptr && !L.mfcc_only && rows16) { c.list = SP_LIST_PARKED; c.full_off = -1; extra = 0; }
    c.lds = base + extra;
    c.lpc = L.out_lpc != nullptr; c.mf = L.out_mfcc != nullptr; c.full = L.n == SP_N; c.waves = VBX_SPECTRAL_WAVES; c.mode = SP_ANALYZE;
    const bool interp = L.interp && L.n != SP_N;             // a padded frame whose MFCC bins are interpolated from the transform's
    const size_t lds_ip = ((size_t)L.ip.lds_bytes + 15) & ~(size_t)15;
    // Three wavefronts per SIMD (twelve frames of 13.5 KB fill the CU's LDS; 168 registers) wherever the frame state allows it,
    // i.e. no full-list region in LDS.  Round 3 had it for pitch alone from kmax = 2 (the refinement is a chain of dependent
    // operations that two wavefronts do not cover); at kmax = 1 and in the fused loop the transforms' ~55 spilled registers
    // cost more than the third wavefront brought.  Round 4: with the twiddle products in pinned batches (twiddle_tight) the
    // 168-register instances spill 12-29 registers instead of 146-171, and three wavefronts win everywhere: pitch at kmax = 1
    // 33.7 -> 37.8 M frames/s, the fused loop (the headline) 30.0 -> 33.5 M.  VBX_SPECTRAL_W3=0: two wavefronts as before (A/B).
    auto waves_for = [&](size_t lds) { return (spectral_want3() && extra == 0 && 12 * lds <= 160 * 1024) ? 3 : VBX_SPECTRAL_WAVES; };
    if (L.mfcc_only) {                                       // n == SP_N, or a padded frame with interpolated bins
        c.lpc = false; c.mf = true; c.full = !interp; c.mode = interp ? SP_MFCC_ONLY_INTERP : SP_MFCC_ONLY;
        c.lds = (interp && (size_t)L.ip.lds_bytes >= spectral_lds_bytes(0)) ? lds_ip : spectral_lds_bytes(0);
    } else if (L.out_r != nullptr) {                         // autocorrelate(n_lags) alone
        c.lpc = c.mf = false; c.mode = SP_AC_ONLY; c.lds = spectral_lds_bytes(0);
    } else if (L.x.kind == SAMPLE_F32) {
        c.family = SP_FAMILY_F32IN; c.waves = waves_for(c.lds);
    } else if (const int spec = spectral_spec(L, waves_for(c.lds) == 3, extra); spec != SP_SPEC_NONE) {
        c.spec = spec; c.waves = 3;
    } else if (interp && c.mf) {
        c.mode = SP_ANALYZE_INTERP;
        if ((size_t)L.ip.lds_bytes >= c.lds) c.lds = lds_ip;
        c.waves = waves_for(c.lds);
    } else c.waves = waves_for(c.lds);                       // a full frame, or a padded one: MFCC from the transform's own bins when its length divides 2400
    c.refused = !sp_1200_instance(c.lpc, c.mf, c.full, c.mode, c.waves, c.spec, c.burg, c.family == SP_FAMILY_F32IN);
    return c;
}

// Would launch_analyze leave Burg's lag sums (BURG) for L?  The choice's own answer to L with that request.
bool spectral_burg_fusable(const spectral_launch_t &L) {
    static double requested;                                 // (any address: the choice reads no memory)
    spectral_launch_t Q = L;
    Q.burg_scratch = &requested;
    return !choose_analyze(Q).refused;
}

int launch_analyze(hipStream_t s, const spectral_launch_t &L, analyze_choice_t *acted) {
    analyze_choice_t c = choose_analyze(L);
    // Burg's lag sums from the frame's own wavefront: frames [burg_f0, burg_f0 + burg_nf) of the batch (refused before anything is launched)
    if (c.burg && ((((uintptr_t)L.burg_window) & 15) != 0 || L.burg_window == nullptr || L.burg_f0 < 0 || L.burg_nf < 1 || L.burg_f0 + L.burg_nf > L.F)) c.refused = true;
    if (acted) *acted = c;
    if (c.refused) return 0;
    spectral_args_t a;
    a.frames = static_cast<const double *>(L.x.p);           // (the kernels take PCM / float32 through the f64 argument: a.pcm says PCM, k_spectral_f32in.hip is compiled for float32)
    a.n_frames = c.burg ? L.burg_nf : L.F; a.stride = L.stride; a.window = L.window; a.lag_window = L.lag_window;
    a.tab = reinterpret_cast<const double2 *>(L.tab);
    a.n = L.n;
    a.pp.sample_rate = L.sample_rate; a.pp.threshold = L.threshold; a.pp.fmin = L.fmin; a.pp.fmax = L.fmax; a.pp.kmax = L.kmax; a.pp.f32 = 0;
    a.pp.full_off = c.full_off; a.pp.ncurve = c.ncurve;
    a.out_cand = reinterpret_cast<double *>(L.out_cand); a.cand_ld = L.cand_ld; a.out_count = L.out_count;
    a.pitch_status = L.pitch_status; a.work = L.work;
    a.out_lpc = L.out_lpc; a.lpc_ld = L.lpc_ld;
    a.out_mfcc = L.out_mfcc; a.mfcc_ld = L.mfcc_ld; a.mfcc_status = L.mfcc_status;
    a.bins = L.bins; a.slopes = L.slopes; a.dct = L.dct; a.num_coeffs = L.num_coeffs; a.nb = L.nb;
    a.unsure_list = L.unsure_list; a.unsure_count = L.unsure_count;
    a.out_r = L.out_r; a.n_lags = L.n_lags;
    a.pcm = (L.x.kind == SAMPLE_PCM16 ? SP_FLAG_PCM : 0) | (L.lag_rcp ? SP_FLAG_LAG_RCP : 0) | ((L.mfcc_defer && L.num_coeffs <= 16) ? SP_FLAG_MFCC_DEFER : 0);
    a.mfcc_q = (L.plan != SPECTRAL_PLAN_NONE && L.n > 0) ? (2 * spectral_plan_nc(L.plan)) / L.n : 2;
    a.ip = (sp_is_interp(c.mode) || sp_is_split(c.mode)) ? L.ip : mfcc_interp_t{};
    a.burg_scratch = c.burg ? L.burg_scratch : nullptr; a.burg_window = c.burg ? L.burg_window : nullptr; a.burg_f0 = c.burg ? L.burg_f0 : 0;
    if (c.family == SP_FAMILY_POW2) return launch_analyze_pow2(s, L, c, a);
    if (c.family == SP_FAMILY_F32IN) return launch_analyze_f32in(s, c, a) ? 1 : 0;
    constexpr int W2 = VBX_SPECTRAL_WAVES;
    const bool w3 = c.waves == 3, pcm = c.spec == SP_SPEC_PCM16;
    const bool launched =
        c.mode == SP_MFCC_ONLY_INTERP ? sp_launch_1200<SP_MFCC_ONLY_INTERP, W2, double>(s, c, a) :
        c.mode == SP_MFCC_ONLY ? sp_launch_1200<SP_MFCC_ONLY, W2, double>(s, c, a) :
        c.mode == SP_AC_ONLY ? sp_launch_1200<SP_AC_ONLY, W2, double>(s, c, a) :
        c.mode == SP_ANALYZE_INTERP ? (w3 ? sp_launch_1200<SP_ANALYZE_INTERP, 3, double>(s, c, a) : sp_launch_1200<SP_ANALYZE_INTERP, W2, double>(s, c, a)) :
        c.burg ? (pcm ? sp_launch_1200<SP_ANALYZE, 3, sp_launch_pcm16_burg_t>(s, c, a) : sp_launch_1200<SP_ANALYZE, 3, sp_launch_f64_burg_t>(s, c, a)) :
        c.spec != SP_SPEC_NONE ? (pcm ? sp_launch_1200<SP_ANALYZE, 3, sp_launch_pcm16_t>(s, c, a) : sp_launch_1200<SP_ANALYZE, 3, sp_launch_f64_t>(s, c, a)) :
        w3 ? sp_launch_1200<SP_ANALYZE, 3, double>(s, c, a) : sp_launch_1200<SP_ANALYZE, W2, double>(s, c, a);
    return launched ? 1 : 0;
}

}  // namespace vbx
