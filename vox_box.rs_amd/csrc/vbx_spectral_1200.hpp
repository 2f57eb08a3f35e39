// vbx_spectral_1200.hpp -- the device side of the 1200-point plan (k_spectral.hip has the description, the host side and the f64 /
// PCM instantiations; k_spectral_f32in.hip the ones that read float samples): the 2400-point real transform in registers and the
// fused per-frame analysis built on it.
#pragma once

#include <type_traits>
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"
#include "vbx_mfcc_tail.hpp"
#include "vbx_mfcc_interp.hpp"
#include "vbx_pitch_refine.hpp"
#include "vbx_spectral.hpp"
#include "vbx_burg_fast.hpp"

namespace vbx {

constexpr int SP_N = SPECTRAL_N;             // frame length = complex FFT length
constexpr int SP_M = 2 * SP_N;               // real FFT length
constexpr int SP_S1 = 61;                    // exchange 1 row stride [ka][n']   (odd: the 20 rows hit distinct banks)
constexpr int SP_S2 = 404;                   // exchange 2 row stride [c][ka + 20 kb]
constexpr int SP_T1 = 0;                     // twiddle table (complex entries): T1[60][20] = W_1200^(n' ka)
constexpr int SP_T2 = SP_T1 + 60 * 20;       //                                  T2[3][20]  = W_60^(c kb)
constexpr int SP_TM = SP_T2 + 3 * 20;        //                                  WM[601]    = W_2400^m
static_assert(SP_TM + 601 == SPECTRAL_TAB_COMPLEX, "table layout");
// LDS: [0, 9760) exchange buffer (later the lag curve), [0, 10144) the mel sums between the transforms, then the copy of T2
constexpr int SP_T2_LDS_OFFSET = (2 * 602 + 64) * 8;
static_assert(SP_T2_LDS_OFFSET >= (20 * SP_S1 > 3 * SP_S2 ? 20 * SP_S1 : 3 * SP_S2) * 8 && SP_T2_LDS_OFFSET % 16 == 0, "T2 behind both");

__device__ __forceinline__ void dft5(double &r0, double &i0, double &r1, double &i1, double &r2, double &i2,
                                     double &r3, double &i3, double &r4, double &i4) {
    constexpr double C5 = 0.55901699437494742410;    // (cos 72 - cos 144) / 2
    constexpr double S1 = 0.95105651629515357212;    // sin 72
    constexpr double S2 = 0.58778525229247312917;    // sin 144
    const double t1r = r1 + r4, t1i = i1 + i4, t3r = r1 - r4, t3i = i1 - i4;
    const double t2r = r2 + r3, t2i = i2 + i3, t4r = r2 - r3, t4i = i2 - i3;
    const double t5r = t1r + t2r, t5i = t1i + t2i;
    const double m1r = fma(-0.25, t5r, r0), m1i = fma(-0.25, t5i, i0);
    const double m2r = C5 * (t1r - t2r), m2i = C5 * (t1i - t2i);
    const double s1r = m1r + m2r, s1i = m1i + m2i, s2r = m1r - m2r, s2i = m1i - m2i;
    // u = S1 t3 + S2 t4, v = S2 t3 - S1 t4;  X1 = s1 - i u, X4 = s1 + i u, X2 = s2 - i v, X3 = s2 + i v
    const double ur = fma(S1, t3r, S2 * t4r), ui = fma(S1, t3i, S2 * t4i);
    const double vr = fma(S2, t3r, -(S1 * t4r)), vi = fma(S2, t3i, -(S1 * t4i));
    r0 = r0 + t5r; i0 = i0 + t5i;
    r1 = s1r + ui; i1 = s1i - ur;
    r4 = s1r - ui; i4 = s1i + ur;
    r2 = s2r + vi; i2 = s2i - vr;
    r3 = s2r - vi; i3 = s2i + vr;
}

// 20-point DFT in place, prime-factor form (gcd(4, 5) = 1: no twiddles between the 4- and the 5-point parts).
// Input index a sits in slot a; output index k is left in slot dft20_slot(k).
__host__ __device__ constexpr int dft20_in(int n1, int n2) { return (5 * n1 + 4 * n2) % 20; }
__host__ __device__ constexpr int dft20_slot(int k) { return (5 * (k % 4) + 4 * (k % 5)) % 20; }

__device__ __forceinline__ void dft20(double (&re)[20], double (&im)[20]) {
#pragma unroll
    for (int n2 = 0; n2 < 5; n2++)
        dft4(re[dft20_in(0, n2)], im[dft20_in(0, n2)], re[dft20_in(1, n2)], im[dft20_in(1, n2)],
             re[dft20_in(2, n2)], im[dft20_in(2, n2)], re[dft20_in(3, n2)], im[dft20_in(3, n2)]);
#pragma unroll
    for (int k1 = 0; k1 < 4; k1++)
        dft5(re[dft20_in(k1, 0)], im[dft20_in(k1, 0)], re[dft20_in(k1, 1)], im[dft20_in(k1, 1)],
             re[dft20_in(k1, 2)], im[dft20_in(k1, 2)], re[dft20_in(k1, 3)], im[dft20_in(k1, 3)],
             re[dft20_in(k1, 4)], im[dft20_in(k1, 4)]);
}

// Complex FFT of length 1200.  In: lane n' < 60 holds z[60 a + n'] in (re[a], im[a]).  Out: lane l holds
// X[l + 64 t + 400 kc] in (xr[t][kc], xi[t][kc]) for l + 64 t < 400 (KC = 3: every output; KC = 2: kc = 0, 1 only).
// ex: LDS exchange buffer (>= 20 * SP_S1 doubles).  tab: twiddle table.
// The twenty twiddle products of a stage in batches of TWB (two), each batch finished before the next one's loads may start: the
// products are pinned (an empty asm with the value as in/out operand) and the loads fenced (a compiler memory barrier).  Left
// alone the compiler requests all twenty twiddles at once -- 80 registers -- right after the 20-point DFT, whose results it
// spills to make room (the 168-register instance: ~100 scratch round trips per transform).  Batches of 2 / 5 / 10: 0 / 12 / 9
// spilled registers in the fused kernel, 34.1 / 34.3 / 34.6 M frames/s -- two it is: no scratch traffic at all.
#ifndef VBX_EXP_TWB
#define VBX_EXP_TWB 2
#endif
constexpr int TWB = VBX_EXP_TWB;
#ifndef VBX_EXP_MB1
#define VBX_EXP_MB1 3
#endif
template <int TWB = vbx::TWB>
__device__ __forceinline__ void twiddle_tight(double (&re)[20], double (&im)[20], const double2 *tw_row) {
#pragma unroll
    for (int h = 0; h < 20 / TWB; h++) {
        double2 tw[TWB];
#pragma unroll
        for (int k = 0; k < TWB; k++) tw[k] = tw_row[TWB * h + k];
#pragma unroll
        for (int k = 0; k < TWB; k++) {
            if (TWB * h + k == 0) continue;
            const int s = dft20_slot(TWB * h + k);
            const double a = re[s], b = im[s];
            re[s] = fma(a, tw[k].x, -(b * tw[k].y));
            im[s] = fma(a, tw[k].y, b * tw[k].x);
            asm volatile("" : "+v"(re[s]), "+v"(im[s]));
        }
        asm volatile("" ::: "memory");
    }
}

// TIGHT (the instance compiled for three wavefronts per SIMD, 168 registers): the scheduler may not move the twiddle loads
// above the 20-point DFT they follow -- hoisted there to hide their latency they hold 40..80 registers while the DFT needs
// them, and the DFT's own values spill (scratch round trips inside both transforms).
// t2: the stage-2 twiddles T2[3][20] (960 B) in LDS (analyze_kernel copies them there once per frame, into a region that only
// the refinement uses later): ten dependent round trips to the L1 / L2 per transform become LDS reads.  (Round 5: s_memtime
// at the phase boundaries showed a wavefront spending 23 % of its life in the two transforms and the split between them
// for 16 % of its instructions -- twenty batches of two twiddle loads per transform, each waited for.)
template <int KC, bool TIGHT = false>
__device__ __forceinline__ void fft1200(double (&re)[20], double (&im)[20], double (&xr)[7][3], double (&xi)[7][3],
                                        double *ex, const double2 *tab, const double2 *t2) {
    const int lane = lane_id();
    const int np = (lane < 60) ? lane : 59;                 // lanes 60..63 shadow lane 59 (they never write)
    const bool act = lane < 60;
    // stage 1 (the twiddles arrive in two batches of ten: the 20-point DFT needs the registers)
    dft20(re, im);
    if constexpr (TIGHT) twiddle_tight(re, im, tab + SP_T1 + np * 20);
    else {
#pragma unroll
    for (int h = 0; h < 2; h++) {
        double2 tw[10];
#pragma unroll
        for (int k = 0; k < 10; k++) tw[k] = tab[SP_T1 + np * 20 + 10 * h + k];
#pragma unroll
        for (int k = 0; k < 10; k++) {
            if (10 * h + k == 0) continue;
            const int s = dft20_slot(10 * h + k);
            const double a = re[s], b = im[s];
            re[s] = fma(a, tw[k].x, -(b * tw[k].y));
            im[s] = fma(a, tw[k].y, b * tw[k].x);
        }
    }
    }
    // exchange 1: [ka][n'] -> lane (ka2, c2) = (lane % 20, lane / 20) reads n' = 3 b + c2
    const int ka2 = np % 20, c2 = np / 20;
    double br[20], bi[20];
    wave_sync();
#pragma unroll
    for (int k = 0; k < 20; k++) if (act) ex[k * SP_S1 + lane] = re[dft20_slot(k)];
    wave_sync();
#pragma unroll
    for (int b = 0; b < 20; b++) br[b] = ex[ka2 * SP_S1 + 3 * b + c2];
    wave_sync();
#pragma unroll
    for (int k = 0; k < 20; k++) if (act) ex[k * SP_S1 + lane] = im[dft20_slot(k)];
    wave_sync();
#pragma unroll
    for (int b = 0; b < 20; b++) bi[b] = ex[ka2 * SP_S1 + 3 * b + c2];
    // stage 2
    dft20(br, bi);
    if constexpr (TIGHT) twiddle_tight<4>(br, bi, t2 + c2 * 20);
    else {
#pragma unroll
    for (int h = 0; h < 2; h++) {
        double2 tw[10];
#pragma unroll
        for (int k = 0; k < 10; k++) tw[k] = t2[c2 * 20 + 10 * h + k];
#pragma unroll
        for (int k = 0; k < 10; k++) {
            if (10 * h + k == 0) continue;
            const int s = dft20_slot(10 * h + k);
            const double a = br[s], b = bi[s];
            br[s] = fma(a, tw[k].x, -(b * tw[k].y));
            bi[s] = fma(a, tw[k].y, b * tw[k].x);
        }
    }
    }
    // exchange 2: [c][ka + 20 kb] -> lane l reads q = l + 64 t for c = 0..2
    double vr[7][3], vi[7][3];
    wave_sync();
#pragma unroll
    for (int k = 0; k < 20; k++) if (act) ex[c2 * SP_S2 + ka2 + 20 * k] = br[dft20_slot(k)];
    wave_sync();
#pragma unroll
    for (int t = 0; t < 7; t++)
#pragma unroll
        for (int c = 0; c < 3; c++) vr[t][c] = (t < 6 || lane < 16) ? ex[c * SP_S2 + lane + 64 * t] : 0.0;
    wave_sync();
#pragma unroll
    for (int k = 0; k < 20; k++) if (act) ex[c2 * SP_S2 + ka2 + 20 * k] = bi[dft20_slot(k)];
    wave_sync();
#pragma unroll
    for (int t = 0; t < 7; t++)
#pragma unroll
        for (int c = 0; c < 3; c++) vi[t][c] = (t < 6 || lane < 16) ? ex[c * SP_S2 + lane + 64 * t] : 0.0;
    wave_sync();
    // stage 3: X[kc] = v0 + v1 W3^kc + v2 W3^(2 kc)
    constexpr double H3 = 0.86602540378443864676;           // sin 60
#pragma unroll
    for (int t = 0; t < 7; t++) {
        const double sr = vr[t][1] + vr[t][2], si = vi[t][1] + vi[t][2];
        const double dr = vr[t][1] - vr[t][2], di = vi[t][1] - vi[t][2];
        xr[t][0] = vr[t][0] + sr; xi[t][0] = vi[t][0] + si;
        const double mr = fma(-0.5, sr, vr[t][0]), mi = fma(-0.5, si, vi[t][0]);
        xr[t][1] = fma(H3, di, mr); xi[t][1] = fma(-H3, dr, mi);           // m - i H3 d
        if (KC == 3) { xr[t][2] = fma(-H3, di, mr); xi[t][2] = fma(H3, dr, mi); }
        else { xr[t][2] = 0.0; xi[t][2] = 0.0; }
    }
}

// WAVES: wavefronts per SIMD the instance is compiled for.  Two: the transforms take ~230 registers.  Three (168 registers, what
// launch_analyze picks since the end of round 4): with the twiddle products in pinned batches (twiddle_tight) nothing spills in
// the fused kernel; before that ~55 registers did and the third wavefront cost more than it brought.
#ifndef VBX_SPECTRAL_WAVES
#define VBX_SPECTRAL_WAVES 2
#endif
// FULL: the frame fills the transform (n == 1200, the bounds tests fold away); otherwise n < 1200, zero padded: 1025..1199,
// and 600 / 800 when MFCC is wanted (they divide M = 2400: spectral_plan_mfcc).
// MODE: SP_ANALYZE the fused analysis; SP_MFCC_ONLY MFCC::mfcc alone (vbx_mfcc_f64 on a full frame): the forward transform and
// the mel / DCT tail, nothing after them; SP_AC_ONLY Autocorrelate::autocorrelate alone (vbx_autocorrelate_f64 with many lags):
// both transforms, the fold seed, the lag sums stored.
// WAVES: wavefronts per SIMD the kernel is compiled for.  2 (the default: no spills) for kmax = 1, where the two transforms
// are a third of the kernel; 3 for 2 <= kmax <= 64, where the kernel is almost all refinement -- chains of dependent FP64
// operations that two wavefronts do not cover (measured at kmax = 2 / 8 / 64: 12.1 -> 13.6, 4.55 -> 5.65, 2.2 -> 2.7 M
// frames/s; kmax = 1: 32.5 -> 31.7, hence the split).  The transforms then spill ~55 registers, which the refinement hides.
// TIN: what a.frames points to.  double (the default; every instantiation of k_spectral.hip): f64 samples, or -- flagged at run time in
// a.pcm -- 16-bit PCM.  float (k_spectral_f32in.hip only): float32 samples, widened in registers before the window product (every float
// is a double: the frame is the one vbx_f32_to_f64 would have written, bit for bit).  A compile-time choice, so that the f64 / PCM
// instantiations are instruction for instruction what they were before the float form existed.  Full frames only.
// Whole blocks of samples per cell the one-candidate refinement keeps in registers (improve_extremum_sinc_wave<NB>): the most
// at which no instance of this kernel, at two or three wavefronts, f64 / PCM or float samples, uses a register or a byte of
// scratch more than at 0 (tools/resource_usage.sh; at 4 the three-wavefront instances spill 17-52 registers).
#ifndef VBX_EXP_CELL_NB
#define VBX_EXP_CELL_NB 3
#endif
#ifndef VBX_EXP_CELL_NB_F32IN
#define VBX_EXP_CELL_NB_F32IN VBX_EXP_CELL_NB
#endif
// The candidate front end with its values computed once (pitch_refine_store<.., ONCE>): every instance of this kernel but the
// three-wavefront forms of full f64 / PCM frames without MFCC, which spill two to four registers more with it (4 -> 8 and 4 -> 6,
// tools/resource_usage.sh) and keep the plain form; no other instance uses a register or a byte of scratch more.
#ifndef VBX_EXP_FRONT_END_ONCE
#define VBX_EXP_FRONT_END_ONCE 1
#endif
__host__ __device__ constexpr bool sp_front_end_once(bool mfcc, bool full, int waves, bool f32) {
    return VBX_EXP_FRONT_END_ONCE != 0 && !(!mfcc && full && waves >= 3 && !f32);
}
__host__ __device__ constexpr int sp_cell_blocks(int waves, bool f32) { return f32 ? VBX_EXP_CELL_NB_F32IN : VBX_EXP_CELL_NB; }
template <int MODE, typename TIN = double> using sp_args_of = typename std::conditional<sp_wide_args(MODE), spectral_args_t,
                                                         typename std::conditional<sp_burg_of<TIN>(), spectral_args_1200_burg_t, spectral_args_1200_t>::type>::type;
// The kernel's own argument block where it lies, in the argument segment (the block is the kernel's only argument: offset 0), for the
// SPEC instances' fields that are read where they are used.  The pointer passes through an empty asm at every use, so that the
// compiler can neither move the scalar load up to the kernel's entry nor merge it with the entry's loads -- which is how sixteen
// dwords of output pointers came to be held, in lanes of the spill register, from the first transform to the frame's last store.
template <typename ARGS>
__device__ __forceinline__ const __attribute__((address_space(4))) ARGS *sp_args_where_used() {
    const __attribute__((address_space(4))) ARGS *p = (const __attribute__((address_space(4))) ARGS *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
// TIN = sp_launch_f64_t / sp_launch_pcm16_t: f64 / 16-bit PCM samples with the launch-uniform choices compiled in (SP_SPEC_*,
// vbx_spectral.hpp); three-wavefront SP_ANALYZE instances of full frames only.
// BURG (TIN = sp_launch_f64_burg_t / sp_launch_pcm16_burg_t: launch-specialised instances only): the frame's wavefront also leaves what burg_recursion_kernel<SP_BURG_P> reads -- the order-12
// lag sums of the frame under the PERIODIC Hanning window (find_formants' own, not the pitch window) and its first and last 13
// windowed samples -- in the launch's scratch tile, bit for bit what burg_lags_kernel<20, 12, TIN> writes there (the arithmetic is
// that kernel's own: burg_lag_parts / burg_lag_totals, vbx_burg_fast.hpp).  The block runs FIRST, while the frame's registers are
// free: twenty contiguous samples per lane (a second read of cache lines the wavefront requests anyway a moment later), the
// transpose buffer in the exchange buffer.  The launch covers frames [a.burg_f0, a.burg_f0 + a.n_frames) of the batch.
template <bool LPC, bool MFCC, bool FULL, int MODE = SP_ANALYZE, int WAVES = VBX_SPECTRAL_WAVES, typename TIN = double>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(sp_is_mfcc_only(MODE) ? 2 : WAVES, sp_is_mfcc_only(MODE) ? 4 : WAVES))) void analyze_kernel(const sp_args_of<MODE, TIN> a) {
    constexpr bool F32 = std::is_same<TIN, float>::value;
    using args_t = sp_args_of<MODE, TIN>;
    constexpr int SPEC = sp_spec_of<TIN>();
    constexpr bool BURG = sp_burg_of<TIN>();
    static_assert(SPEC == SP_SPEC_NONE || (FULL && MODE == SP_ANALYZE && WAVES >= 3), "the launch-specialised form: full f64 / PCM frames, three wavefronts");
    constexpr bool SP = SPEC != SP_SPEC_NONE;
    static_assert(!BURG || SP, "Burg's lag sums ride on the launch-specialised instances only");
    // launch-uniform choices: a SPEC instance's at compile time, the generic instance's from the argument block -- written as macros so
    // that the generic instances hold, use for use, the expressions they always held.
    // (NOT the window's presence: with it a constant, a sample's window product feeds the first butterfly's addition directly and
    // the compiler contracts the two into one FMA -- a transform that differs in its last bits from the generic instance's, where the
    // choice between x w and x stands between them.  Measured: LPC and pitch columns of 67 frames moved by up to 1e-11.)
#define VBX_SP_PCM_IN (SP ? SPEC == SP_SPEC_PCM16 : (a.pcm & SP_FLAG_PCM) != 0)
#define VBX_SP_LAG_RCP (SP || (a.pcm & SP_FLAG_LAG_RCP) != 0)
    static_assert(!F32 || (FULL && MODE == SP_ANALYZE), "float samples: the fused analysis of full frames");
    static_assert(MODE != SP_MFCC_ONLY || (MFCC && FULL && !LPC), "the MFCC-only form needs the full frame and has no lag sums");
    static_assert(MODE != SP_AC_ONLY || (!MFCC && !LPC), "the autocorrelation-only form");
    static_assert(!sp_is_interp(MODE) || (MFCC && !FULL), "interpolated bins: a padded frame's MFCC");
    static_assert(MODE != SP_MFCC_ONLY_INTERP || !LPC, "the MFCC-only forms have no lag sums");
    constexpr bool PITCH = !sp_is_mfcc_only(MODE);           // the second transform runs
    constexpr bool INTERP = sp_is_interp(MODE);              // MFCC's bins lie between the transform's (mfcc_interp_t, vbx_kernels.hpp)
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const long fl = xcd_item(blockIdx.x, a.n_frames);           // neighbouring frames on the same XCD: their overlap hits its L2
    if (fl >= a.n_frames) return;
    long f = fl;
    if constexpr (BURG) f += a.burg_f0;                         // (BURG: fl counts inside the launch, f inside the batch)
    const int lane = lane_id();
    const int np = (lane < 60) ? lane : 59;
    const int n = FULL ? SP_N : a.n;                         // frame length, <= SP_N (shorter: longer zero padding)
    double *ex = smem;                                       // exchange buffer, later the lag curve y
    const double *xf = a.frames + f * a.stride;
    // stage-2 twiddles into LDS, behind the exchange buffer and the mel sums (fft1200; ordered by the first exchange's wave_sync)
    double2 *t2 = reinterpret_cast<double2 *>(reinterpret_cast<char *>(smem) + SP_T2_LDS_OFFSET);
    VBX_PHASE_INIT();

    if constexpr (BURG) {
        // ---- Burg's lag sums and edge samples of this frame: lane l holds samples [20 l, 20 l + 20) times the periodic Hanning window ----
        constexpr int EPL = 20, NL = SP_BURG_P + 1, TS = NL | 1;
        static_assert(64 * EPL >= SP_N && 60 * EPL == SP_N, "sixty lanes of twenty samples, lanes 60..63 zero as in burg_lags_kernel<20, ..>");
        static_assert((64 * TS + 3 * NL) * 8 <= SP_T2_LDS_OFFSET, "transpose buffer and record inside the exchange buffer");
        double *TR = smem, *REC = smem + 64 * TS;
        double ext[EPL + NL - 1];
        // (the block's own copy of the lane index, opaque to the compiler: nothing derived from it here is kept for the frame's loads below,
        // whose registers are counted to the last one)
        int lane = lane_id();
        asm volatile("" : "+v"(lane));
        const int np = (lane < 60) ? lane : 59;
        {
            const double2 *wv = reinterpret_cast<const double2 *>(a.burg_window + np * EPL);     // (the table is 16-byte aligned: launch_analyze)
            if (VBX_SP_PCM_IN) {
                const int16_t *xb = reinterpret_cast<const int16_t *>(a.frames) + f * a.stride + np * EPL;
                if ((((uintptr_t)xb) & 3) == 0) {
#pragma unroll
                    for (int e = 0; e < EPL; e += 2) {
                        const int w = *reinterpret_cast<const int *>(xb + e);
                        const double2 h = wv[e / 2];
                        ext[e] = pcm16_value((int)(short)(w & 0xffff)) * h.x;
                        ext[e + 1] = pcm16_value(w >> 16) * h.y;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < EPL; e += 2) {
                        const int lo = xb[e], hi = xb[e + 1];
                        const double2 h = wv[e / 2];
                        ext[e] = pcm16_value(lo) * h.x;
                        ext[e + 1] = pcm16_value(hi) * h.y;
                    }
                }
            } else {
                const double *xb = xf + np * EPL;
                if ((((uintptr_t)xf) & 15) == 0) {                 // uniform: ten 16-byte loads per lane
#pragma unroll
                    for (int e = 0; e < EPL; e += 2) {
                        const double2 v = *reinterpret_cast<const double2 *>(xb + e);
                        const double2 h = wv[e / 2];
                        ext[e] = v.x * h.x; ext[e + 1] = v.y * h.y;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < EPL; e += 2) {
                        const double lo = xb[e], hi = xb[e + 1];
                        const double2 h = wv[e / 2];
                        ext[e] = lo * h.x; ext[e + 1] = hi * h.y;
                    }
                }
            }
            if (lane >= 60) {                                      // past the frame's end: the zeros they are in burg_lags_kernel
#pragma unroll
                for (int e = 0; e < EPL; e++) ext[e] = 0.0;
            }
        }
        burg_lag_parts<EPL, NL>(ext, TR, lane);
        if (lane == 0) {                                           // x_w[0..12]
#pragma unroll
            for (int k = 0; k < NL; k++) REC[NL + k] = ext[k];
        }
        if (lane == 59) {                                          // x_w[1199 - k], k = 0..12
#pragma unroll
            for (int k = 0; k < NL; k++) REC[2 * NL + k] = ext[EPL - 1 - k];
        }
        wave_sync();
        burg_lag_totals<NL>(TR, lane, [&](int rl, double tot) { REC[rl] = tot; });
        wave_sync();
        // the scratch is tiled [64 frames: one wavefront of the recursion][value][frame]
        if (lane < 3 * NL) a.burg_scratch[(fl >> 6) * (3 * NL * 64) + lane * 64 + (fl & 63)] = REC[lane];
        wave_sync();                                               // before the transform's first exchange takes the buffer
        asm volatile("" ::: "memory");                             // the frame's own loads start behind this block: its registers are free again
    }

    // ---- load: z[60 a + n'] = (xw[120 a + 2 n'], xw[120 a + 2 n' + 1]), a < 10 (the rest is the zero padding) ----
    double re[20], im[20];
    const int16_t *x16 = reinterpret_cast<const int16_t *>(a.frames) + f * a.stride;       // the frame when a.pcm (FULL only)
    const float *x32 = reinterpret_cast<const float *>(a.frames) + f * a.stride;            // the frame when TIN = float
    {
        const bool al = ((((uintptr_t)xf) | ((uintptr_t)a.window)) & 15) == 0;      // uniform
        double2 xv[10], wv[10];
        float2 xs32[F32 ? 10 : 1];                           // (the float pairs wait for the window as they were loaded: half the registers)
#pragma unroll
        for (int q = 0; q < 10; q++) {
            const int i = 120 * q + 2 * np;
            if constexpr (F32) {
                // float32 in: 1920 B of new samples per frame instead of 3840.  One 8-byte load where THIS frame's address allows it
                // (uniform; an odd stride alternates frame by frame), two 4-byte loads otherwise: the same bits either way
                float lo, hi;
                if ((((uintptr_t)x32) & 7) == 0) { const float2 w = *reinterpret_cast<const float2 *>(x32 + i); lo = w.x; hi = w.y; }
                else { lo = x32[i]; hi = x32[i + 1]; }
                xs32[q] = float2{lo, hi};
                wv[q] = (a.window != nullptr) ? (((uintptr_t)a.window & 15) == 0 ? *reinterpret_cast<const double2 *>(a.window + i)
                                                                                  : double2{a.window[i], a.window[i + 1]}) : double2{1.0, 1.0};
            } else if (FULL && VBX_SP_PCM_IN) {
                // 16-bit PCM in: 960 B of new samples per frame instead of 3840 (the host-fed case: PCIe carries the PCM);
                // widened here exactly as vbx_pcm16_to_f64 would have (bit-identical frames, tests/test_gpu_frontend.py)
                int lo, hi;
                if ((((uintptr_t)x16) & 3) == 0) { const int w = *reinterpret_cast<const int *>(x16 + i); lo = (short)(w & 0xffff); hi = w >> 16; }
                else { lo = x16[i]; hi = x16[i + 1]; }
                xv[q] = double2{pcm16_value(lo), pcm16_value(hi)};
                wv[q] = (a.window != nullptr) ? (((uintptr_t)a.window & 15) == 0 ? *reinterpret_cast<const double2 *>(a.window + i)
                                                                                  : double2{a.window[i], a.window[i + 1]}) : double2{1.0, 1.0};
            } else if (al && i + 1 < n) {
                xv[q] = *reinterpret_cast<const double2 *>(xf + i);
                wv[q] = (a.window != nullptr) ? *reinterpret_cast<const double2 *>(a.window + i) : double2{1.0, 1.0};
            } else {
                xv[q] = double2{0.0, 0.0}; wv[q] = double2{1.0, 1.0};
                if (i < n) { xv[q].x = xf[i]; if (a.window != nullptr) wv[q].x = a.window[i]; }
                if (i + 1 < n) { xv[q].y = xf[i + 1]; if (a.window != nullptr) wv[q].y = a.window[i + 1]; }
            }
        }
#pragma unroll
        for (int q = 0; q < 10; q++) {
            if constexpr (F32) xv[q] = double2{(double)xs32[q].x, (double)xs32[q].y};
            re[q] = (a.window != nullptr) ? xv[q].x * wv[q].x : xv[q].x;
            im[q] = (a.window != nullptr) ? xv[q].y * wv[q].y : xv[q].y;
        }
#pragma unroll
        for (int q = 10; q < 20; q++) { re[q] = 0.0; im[q] = 0.0; }
    }
    const double x0 = readlane_f64(re[0], 0);               // x_w[0], for the fold seed (Q1)
    if (lane < 60) t2[lane] = a.tab[SP_T2 + lane];          // (here, not before the frame's loads: the registers are fewest)
    VBX_PHASE(a.work, f, 0);

    // ---- forward transform of the packed frame ----
    double xr[7][3], xi[7][3];
    fft1200<3, (WAVES >= 3)>(re, im, xr, xi, ex, a.tab, t2);
    VBX_PHASE(a.work, f, 1);

    // ---- exchange 3: natural order, then each lane takes the pairs (m, N - m), m = lane + 64 t <= 600 ----
    double ar[10], ai[10], br[10], bi[10];
#pragma unroll
    for (int t = 0; t < 7; t++)
#pragma unroll
        for (int kc = 0; kc < 3; kc++) if (t < 6 || lane < 16) ex[lane + 64 * t + 400 * kc] = xr[t][kc];
    wave_sync();
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const int m = lane + 64 * t;
        const bool ok = m <= 600;
        ar[t] = ok ? ex[m] : 0.0;
        br[t] = ok ? ex[(m == 0) ? 0 : SP_N - m] : 0.0;
    }
    wave_sync();
#pragma unroll
    for (int t = 0; t < 7; t++)
#pragma unroll
        for (int kc = 0; kc < 3; kc++) if (t < 6 || lane < 16) ex[lane + 64 * t + 400 * kc] = xi[t][kc];
    wave_sync();
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const int m = lane + 64 * t;
        const bool ok = m <= 600;
        ai[t] = ok ? ex[m] : 0.0;
        bi[t] = ok ? ex[(m == 0) ? 0 : SP_N - m] : 0.0;
    }
    wave_sync();

    // ---- spectrum of the real sequence: X[m] = E + T, X[N - m] = conj(E - T); powers; the inverse transform's input ----
    //   E = (A + conj B) / 2, O = -i (A - conj B) / 2, T = W_M^m O;   P[m] = |E + T|^2, P[N - m] = |E - T|^2
    //   the inverse's input G[m] = S - i D w, G[N - m] = S - i D conj(w)   (S = P[m] + P[N-m], D = P[m] - P[N-m], w = W_M^m)
    const int b_lo = MFCC ? a.bins[0] : 0;
    double pk[10], pn[10];                                   // P[m], P[N - m]
    double2 *zc = reinterpret_cast<double2 *>(ex);           // INTERP: Z[j - jmin] = X_M[j] e^{2 pi i j c / M}, Z[-j] = conj Z[j]
    double2 rot_m = double2{1.0, 0.0}, rot_step = double2{1.0, 0.0};
    if constexpr (INTERP) { rot_m = reinterpret_cast<const double2 *>(a.ip.rot)[lane]; rot_step = reinterpret_cast<const double2 *>(a.ip.rot)[64]; }
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const int m = lane + 64 * t;
        const double2 w = a.tab[SP_TM + ((m <= 600) ? m : 0)];
        const double er = 0.5 * (ar[t] + br[t]), ei = 0.5 * (ai[t] - bi[t]);
        const double o_r = 0.5 * (ai[t] + bi[t]), o_i = -0.5 * (ar[t] - br[t]);
        const double tr = fma(w.x, o_r, -(w.y * o_i)), ti = fma(w.x, o_i, w.y * o_r);
        const double pr = er + tr, pi = ei + ti, qr = er - tr, qi = ei - ti;
        pk[t] = fma(pr, pr, pi * pi);
        pn[t] = fma(qr, qr, qi * qi);
        if constexpr (INTERP) {                              // (every lane is past exchange 3's last read: the buffer is free)
            asm volatile("" : "+v"(pk[t]), "+v"(pn[t]));     // the powers NOW: two values wait for exchange 4, not the four they are made of
            mfcc_interp_stage(zc, a.ip, m, pr, pi, rot_m, rot_step, t == 0);
        }
    }

    // ---- MFCC::mfcc at a length that does not divide the transform: each of the frame's DFT bins from 24 .. 40 of the
    //      transform's (lane l: bins b_lo + l + 64 u), BEFORE exchange 4 takes the buffer; then the same products and tail ----
    if constexpr (INTERP) {
        wave_sync();
        VBX_PHASE(a.work, f, 13);
        const int nbp = (a.nb + 1) & ~1;
        double *pu = ex + a.ip.pu_off, *pd = pu + nbp, *en = pd + nbp;
        const double2 *cf = reinterpret_cast<const double2 *>(a.ip.coef) + lane;
        const int HT = a.ip.taps >> 1;                       // 12, 16 or 20 pairs of taps (the host's choice for M / n)
        for (int u = 0; u * 64 < a.nb; u++) {
            const int b = lane + 64 * u;
            const double2 *zp = zc + a.ip.j0[u * 64 + lane];
            const double2 sl = *reinterpret_cast<const double2 *>(a.slopes + 2 * ((b < a.nb) ? b : 0));
            double vr, vi;
            mfcc_interp_bin(HT, cf + (u * HT) * 64, 64, zp, vr, vi);
            const double pw = fma(vr, vr, vi * vi);
            if (b < a.nb) {
                pu[b] = fabs(pw) * sl.x;                     // norm_sqr * multiplier (src/spectrum.rs:426-428)
                pd[b] = fabs(sqrt(pw)) * sl.y;               // norm * multiplier (:432-434)
            }
        }
        wave_sync();
        VBX_PHASE(a.work, f, 14);
        double2 t2v = double2{0.0, 0.0};                     // the products may lie over the stage-2 twiddles: requested now, put back after the tail
        if constexpr (PITCH) t2v = a.tab[SP_T2 + np];
        if (a.num_coeffs <= 16) mfcc_tail_q(pu, pd, en, a.bins, a.dct, a.num_coeffs, b_lo, lane, a.out_mfcc + f * a.mfcc_ld, a.work, f, (a.pcm & SP_FLAG_MFCC_DEFER) != 0);
        else mfcc_tail_m(pu, pd, en, a.bins, a.dct, a.num_coeffs, b_lo, lane, a.out_mfcc + f * a.mfcc_ld);
        if (a.mfcc_status != nullptr && lane == 0) a.mfcc_status[f] = 0;
        wave_sync();
        if (PITCH && lane < 60) t2[lane] = t2v;
        VBX_PHASE(a.work, f, 15);
    }

    if constexpr (PITCH) {
        // ---- exchange 4: G in natural order -> stage-1 layout of the second transform ----
        // (the ten twiddles W_M^m requested together and without a condition -- index 0 stands in past m = 600 --, not one
        // by one behind `if (m <= 600)`: a load inside a branch cannot be moved out of it, and each waited for its own)
        double2 wm[10];
    #pragma unroll
        for (int t = 0; t < 10; t++) { const int m = lane + 64 * t; wm[t] = a.tab[SP_TM + ((m <= 600) ? m : 0)]; }
    #pragma unroll
        for (int t = 0; t < 10; t++) {
            const int m = lane + 64 * t;
            if (m <= 600) {
                const double2 w = wm[t];
                const double sm = pk[t] + pn[t], d = pk[t] - pn[t];
                ex[m] = fma(d, w.y, sm);
                if (m >= 1 && m < 600) ex[SP_N - m] = fma(-d, w.y, sm);
            }
        }
        wave_sync();
    #pragma unroll
        for (int q = 0; q < 20; q++) re[q] = ex[60 * q + np];
        wave_sync();
    #pragma unroll
        for (int t = 0; t < 10; t++) {
            const int m = lane + 64 * t;
            if (m <= 600) {
                const double2 w = wm[t];
                const double gi = -((pk[t] - pn[t]) * w.x);
                ex[m] = gi;
                if (m >= 1 && m < 600) ex[SP_N - m] = gi;
            }
        }
        wave_sync();
    #pragma unroll
        for (int q = 0; q < 20; q++) im[q] = ex[60 * q + np];
        wave_sync();
    }

    VBX_PHASE(a.work, f, 2);
    // ---- MFCC::mfcc from the powers: the frame's n-point DFT bin k' is X_M[q k'], q = M / n (2 for the full frame; a
    //      shorter frame whose length divides M = 2400 -- 800, 600 -- is zero padded and its bins are every q-th one): bin m / q
    //      from P[m] and bin n/2 - m / q from P[N - m] ----
    if constexpr (MFCC && !INTERP) {
        const int nbp = (a.nb + 1) & ~1;
        const int q = FULL ? 2 : a.mfcc_q, half = FULL ? SP_N / 2 : a.n / 2;
        double *pu = ex, *pd = ex + nbp, *en = ex + 2 * nbp; // the exchange buffer is free between the two transforms
        constexpr int MB = 2;     // slots per batch (five: 24 registers spilled in the three-wavefront instance)
        // Can a mirrored bin n/2 - m/q (from P[N - m]) be one of the filters' at all?  Only when they reach above a quarter of
        // the sampling rate (m <= 600: n/2 - m/q >= 600/q).  Below that -- speech settings: 8 kHz of 24 -- only P[m] has bins,
        // half as many slope pairs are wanted, and five slots' pairs are requested together instead of two: two round trips
        // to the L2 per frame instead of five (the phase clocks: 8 k cycles of the frame's 170 k for ~100 instructions).
        const bool two_sided = (half - 600 / q) - b_lo < a.nb;
        if (!two_sided) {
            constexpr int MB1 = VBX_EXP_MB1;               // (batches of three: nothing spills, 18.37 ms per 720,000 frames; of five: six registers, 18.45; round 4's form: 18.56)
#pragma unroll
            for (int h = 0; h < (10 + MB1 - 1) / MB1; h++) {
                double2 s1[MB1];
                int c1[MB1];
#pragma unroll
                for (int u = 0; u < MB1; u++) {
                    const int t = MB1 * h + u, m = lane + 64 * t;
                    if (t >= 10) { c1[u] = -1; continue; }
                    const bool on = m <= 600 && (FULL ? (m & 1) == 0 : m % q == 0);
                    const int b1 = (FULL ? (m >> 1) : m / q) - b_lo;
                    c1[u] = (on && b1 >= 0 && b1 < a.nb) ? b1 : -1;
                    s1[u] = *reinterpret_cast<const double2 *>(a.slopes + 2 * (c1[u] < 0 ? 0 : c1[u]));
                }
#pragma unroll
                for (int u = 0; u < MB1; u++) {
                    const int t = MB1 * h + u;
                    if (t < 10 && c1[u] >= 0) {
                        pu[c1[u]] = fabs(pk[t]) * s1[u].x;   // norm_sqr * multiplier (src/spectrum.rs:426-428)
                        pd[c1[u]] = fabs(sqrt(pk[t])) * s1[u].y;   // norm * multiplier (:432-434)
                    }
                }
            }
        } else
        // (the slope pairs of a few slots requested together, without a condition -- pair 0 stands in for a slot
        // without a bin --, then the products: behind `if (bin in range)` each load waited for its own round trip)
#pragma unroll
        for (int h = 0; h < 10 / MB; h++) {
            double2 s1[MB], s2[MB];
            int c1[MB], c2[MB];
#pragma unroll
            for (int u = 0; u < MB; u++) {
                const int t = MB * h + u, m = lane + 64 * t;
                const bool on = m <= 600 && (FULL ? (m & 1) == 0 : m % q == 0);
                const int mq = FULL ? (m >> 1) : m / q;
                const int b1 = mq - b_lo, b2 = (half - mq) - b_lo;
                c1[u] = (on && b1 >= 0 && b1 < a.nb) ? b1 : -1;
                c2[u] = (on && b2 >= 0 && b2 < a.nb && b2 != b1) ? b2 : -1;
                s1[u] = *reinterpret_cast<const double2 *>(a.slopes + 2 * (c1[u] < 0 ? 0 : c1[u]));
                s2[u] = *reinterpret_cast<const double2 *>(a.slopes + 2 * (c2[u] < 0 ? 0 : c2[u]));
            }
#pragma unroll
            for (int u = 0; u < MB; u++) {
                const int t = MB * h + u;
                if (c1[u] >= 0) {
                    pu[c1[u]] = fabs(pk[t]) * s1[u].x;       // norm_sqr * multiplier (src/spectrum.rs:426-428)
                    pd[c1[u]] = fabs(sqrt(pk[t])) * s1[u].y; // norm * multiplier (:432-434)
                }
                if (c2[u] >= 0) {
                    pu[c2[u]] = fabs(pn[t]) * s2[u].x;
                    pd[c2[u]] = fabs(sqrt(pn[t])) * s2[u].y;
                }
            }
        }
        wave_sync();
        VBX_PHASE(a.work, f, 13);
        if constexpr (SP) {
            // at most sixteen coefficients, log10 + DCT deferred: the one tail, without the DCT table
            mfcc_tail_q(pu, pd, en, a.bins, nullptr, a.num_coeffs, b_lo, lane, a.out_mfcc + f * a.mfcc_ld, nullptr, f, true);
            if (a.mfcc_status != nullptr && lane == 0) a.mfcc_status[f] = 0;
        } else {
        if (a.num_coeffs <= 16) mfcc_tail_q(pu, pd, en, a.bins, a.dct, a.num_coeffs, b_lo, lane, a.out_mfcc + f * a.mfcc_ld, a.work, f, (a.pcm & SP_FLAG_MFCC_DEFER) != 0);
        else mfcc_tail_m(pu, pd, en, a.bins, a.dct, a.num_coeffs, b_lo, lane, a.out_mfcc + f * a.mfcc_ld);
        if (a.mfcc_status != nullptr && lane == 0) a.mfcc_status[f] = 0;
        }
        wave_sync();
    }

    VBX_PHASE(a.work, f, 3);
    if constexpr (!PITCH) return;

    // ---- second transform: Y = FFT(G);  S[2j] = Re Y[j] / M, S[2j+1] = -Im Y[j] / M, j < 600 only ----
    fft1200<2, (WAVES >= 3)>(re, im, xr, xi, ex, a.tab, t2);
    VBX_PHASE(a.work, f, 4);

    // r[lag] = (S[lag] - x0 x[lag]) + x0 (Q1), lane l: j = l + 64 t (kc = 0) and j = 400 + l + 64 t < 600 (kc = 1)
    constexpr double INV_M = 1.0 / (double)SP_M;
    double r_e[11], r_o[11];                                 // slots 0..6: kc = 0, t = 0..6;  7..10: kc = 1, t = 0..3
    int jj[11];
#pragma unroll
    for (int s = 0; s < 11; s++) {
        const int t = (s < 7) ? s : s - 7, kc = (s < 7) ? 0 : 1;
        const int q = lane + 64 * t;
        const bool ok = (kc == 0) ? (q < 400) : (q < 200);
        jj[s] = ok ? q + 400 * kc : -1;
        r_e[s] = xr[t][kc] * INV_M;
        r_o[s] = -(xi[t][kc] * INV_M);
    }
    const double s0 = readlane_f64(r_e[0], 0);               // S[0], the scale of the transform's rounding error
    if (x0 != 0.0) {                                         // rectangular frames: the fold seed differs from S (uniform branch)
#pragma unroll
        for (int s = 0; s < 11; s++) {
            const int i = 2 * jj[s];
            if (jj[s] >= 0 && i < n) {
                const double xs = F32 ? (double)x32[i] : (FULL && VBX_SP_PCM_IN) ? pcm16_value(x16[i]) : xf[i];
                const double xe = (a.window != nullptr) ? xs * a.window[i] : xs;
                r_e[s] = (r_e[s] - x0 * xe) + x0;
            }
            if (jj[s] >= 0 && i + 1 < n) {
                const double xs = F32 ? (double)x32[i + 1] : (FULL && VBX_SP_PCM_IN) ? pcm16_value(x16[i + 1]) : xf[i + 1];
                const double xo = (a.window != nullptr) ? xs * a.window[i + 1] : xs;
                r_o[s] = (r_o[s] - x0 * xo) + x0;
            }
        }
    }
    if constexpr (MODE == SP_AC_ONLY) {                      // autocorrelate(n_lags): the lag sums and nothing else
        double *row = a.out_r + f * (long)a.n_lags;
        const bool al = ((((uintptr_t)a.out_r) & 15) == 0) && (a.n_lags & 1) == 0;      // uniform: every row 16-byte aligned
#pragma unroll
        for (int s = 0; s < 11; s++) {
            const int i = 2 * jj[s];
            if (jj[s] >= 0 && i + 1 < a.n_lags && al) *reinterpret_cast<double2 *>(row + i) = double2{r_e[s], r_o[s]};
            else {
                if (jj[s] >= 0 && i < a.n_lags) row[i] = r_e[s];
                if (jj[s] >= 0 && i + 1 < a.n_lags) row[i + 1] = r_o[s];
            }
        }
        return;
    }
    if (LPC) {                                               // the raw autocorrelation r[0..12] into the frame's LPC row: lane l holds r[2l], r[2l + 1];
        // levinson_rows_kernel_t makes it LPC::lpc(12) afterwards, one row per lane (vbx_spectral.hpp)
        static_assert(SP_LPC_P == 12, "seven lanes hold r[0..12]");
        double *row = a.out_lpc + f * a.lpc_ld;
        if (lane < 7) { row[2 * lane] = r_e[0]; if (lane < 6) row[2 * lane + 1] = r_o[0]; }
    }
    double amax = -1.0;                                      // max_amplitude over ALL n lags (Q2; NaN never wins)
#pragma unroll
    for (int s = 0; s < 11; s++) {
        const int i = 2 * jj[s];
        const double ae = fabs(r_e[s]), ao = fabs(r_o[s]);
        if (jj[s] >= 0 && i < n) amax = (ae > amax) ? ae : amax;
        if (jj[s] >= 0 && i + 1 < n) amax = (ao > amax) ? ao : amax;
    }
    amax = wave_max(amax);
    const double scale = 1.0 / amax;                         // normalize (:404), then / lag window (:406-408)
    double *ys = smem;
    wave_sync();                                             // every lane is done with the exchange buffer
    // uniform: the table's reciprocals serve (quotient_by_table, vbx_spectral.hpp) unless the scale is not a normal finite number
    const bool by_table = VBX_SP_LAG_RCP && fabs(scale) < 1e290 && fabs(scale) > 1e-290;
    const double *lag_rcp = a.lag_window + lag_rcp_offset(n);
    if (by_table) {
        // (window entries and reciprocals of a few slots requested together, without a condition -- entry 0 stands in for a slot
        // without lags --, then their quotients: all eleven slots' pairs at once are 88 registers the instance does not have)
#ifndef VBX_EXP_LB
#define VBX_EXP_LB 4
#endif
        constexpr int LB = VBX_EXP_LB;
#pragma unroll
        for (int h = 0; h < (11 + LB - 1) / LB; h++) {
            double2 lwv[LB], rwv[LB];
#pragma unroll
            for (int u = 0; u < LB; u++) {
                const int s = LB * h + u;
                if (s >= 11) continue;
                const int i = 2 * jj[s];
                const int at = (jj[s] >= 0 && i + 1 < n) ? i : 0;
                lwv[u] = *reinterpret_cast<const double2 *>(a.lag_window + at);
                rwv[u] = *reinterpret_cast<const double2 *>(lag_rcp + at);
            }
#pragma unroll
            for (int u = 0; u < LB; u++) {
                const int s = LB * h + u;
                if (s >= 11) continue;
                const int i = 2 * jj[s];
                if (jj[s] >= 0 && i + 1 < n) {
                    double2 y;
                    y.x = quotient_by_table(r_e[s] * scale, lwv[u].x, rwv[u].x);
                    y.y = quotient_by_table(r_o[s] * scale, lwv[u].y, rwv[u].y);
                    *reinterpret_cast<double2 *>(ys + i) = y;
                } else if (jj[s] >= 0 && i < n) {            // the last lag of an odd n
                    ys[i] = (r_e[s] * scale) / a.lag_window[i];
                }
            }
            asm volatile("" ::: "memory");                   // the next batch's loads stay behind this one's quotients (registers)
        }
    } else {
        // (the lag window's entries requested together, without a condition: entry 0 stands in for a slot without lags)
        double2 lwv[11];
#pragma unroll
        for (int s = 0; s < 11; s++) {
            const int i = 2 * jj[s];
            lwv[s] = *reinterpret_cast<const double2 *>(a.lag_window + ((jj[s] >= 0 && i + 1 < n) ? i : 0));
        }
#pragma unroll
        for (int s = 0; s < 11; s++) {
            const int i = 2 * jj[s];
            if (jj[s] >= 0 && i + 1 < n) {
                const double2 lw = lwv[s];
                double2 y;
                y.x = (r_e[s] * scale) / lw.x;
                y.y = (r_o[s] * scale) / lw.y;
                *reinterpret_cast<double2 *>(ys + i) = y;
            } else if (jj[s] >= 0 && i < n) {                // the last lag of an odd n
                ys[i] = (r_e[s] * scale) / a.lag_window[i];
            }
        }
    }
    if (lane < Y_PAD) ys[n + lane] = 0.0;
#ifndef VBX_EXP_NO_EXACT_TAIL
    if (!FULL) spectral_exact_tail(ys, n, xf, a.window, a.lag_window, x0, scale, lane);
#endif
    wave_sync();
    VBX_PHASE(a.work, f, 5);
    // Rounding error of the two transforms: a few ulp of S[0] per lag (measured: < 8 eps S[0]); y = r * scale / w_lag
    // with w_lag >= 1/6 on the searched half.  SP_UNC_EPS bounds the error of a DIFFERENCE of two entries with a wide
    // margin; frames with a peak decision inside it go to the direct-sum kernel (launch_pitch_list).
    const double unc_tol = SP_UNC_EPS * fabs(s0) * scale;
    if constexpr (SP) {
        // the list in the lanes, f64 roundings, the whole curve: the launch's own values of full_off / f32 / ncurve, as constants; the
        // output arguments arrive inside pitch_refine_store, at the frame's last stores (`late`)
        pitch_params_t pp;
        pp.sample_rate = a.pp.sample_rate; pp.threshold = a.pp.threshold; pp.fmin = a.pp.fmin; pp.fmax = a.pp.fmax; pp.kmax = a.pp.kmax;
        pp.full_off = 0; pp.f32 = 0; pp.ncurve = 0;
        auto late = [&](auto &out_cand, auto &cand_ld, auto &out_count, auto &status, auto &work) __attribute__((always_inline)) {
            const auto *l = sp_args_where_used<args_t>();
            out_cand = l->out_cand; cand_ld = l->cand_ld; out_count = l->out_count; status = l->pitch_status; work = l->work;
        };
        if (!pitch_refine_store<0, sp_cell_blocks(WAVES, F32), sp_front_end_once(MFCC, FULL, WAVES, F32)>(ys, n, pp, f, nullptr, 0, nullptr, nullptr, nullptr, unc_tol, nullptr,
                                                                                                        nullptr, 0, nullptr, late)) {
            const auto *l = sp_args_where_used<args_t>();
            int32_t *const unsure_count = l->unsure_count;
            if (lane == 0) l->unsure_list[atomicAdd(unsure_count, 1)] = (int32_t)f;
        }
        return;
    }
    double2 *full = a.pp.full_off > 0 ? reinterpret_cast<double2 *>(reinterpret_cast<char *>(smem) + a.pp.full_off)
                  : a.pp.full_off < 0 ? reinterpret_cast<double2 *>(a.out_cand + f * a.cand_ld) : nullptr;
    if (!pitch_refine_store<0, sp_cell_blocks(WAVES, F32), sp_front_end_once(MFCC, FULL, WAVES, F32)>(ys, n, a.pp, f, a.out_cand, a.cand_ld, a.out_count, a.pitch_status, a.work, unc_tol, full)) {
        if (lane == 0) a.unsure_list[atomicAdd(a.unsure_count, 1)] = (int32_t)f;
    }
}
#undef VBX_SP_PCM_IN
#undef VBX_SP_LAG_RCP

// Which instances of analyze_kernel exist, beside the (MODE, WAVES, TIN) its launchers name: the flags each form admits.  choose_analyze
// (k_spectral.hip) asks it at run time -- a choice it rejects is a refusal --, sp_launch_1200 at compile time -- nothing else is compiled.
__host__ __device__ constexpr bool sp_1200_instance(bool lpc, bool mf, bool full, int mode, int waves, int spec, bool burg, bool f32) {
    if (f32 || spec != SP_SPEC_NONE || burg) {
        if (mode != SP_ANALYZE || !full || (!f32 && waves != 3) || (burg && spec == SP_SPEC_NONE)) return false;
        // (PCM frames with MFCC and without LPC: that BURG form spills two registers where the instance it rides on spills none -- such calls keep burg_lags_kernel)
        return !(burg && spec == SP_SPEC_PCM16 && mf && !lpc);
    }
    return mode == SP_ANALYZE ? true : mode == SP_ANALYZE_INTERP ? (mf && !full) : waves != VBX_SPECTRAL_WAVES ? false :
           mode == SP_MFCC_ONLY ? (!lpc && mf && full) : mode == SP_MFCC_ONLY_INTERP ? (!lpc && mf && !full) : mode == SP_AC_ONLY ? (!lpc && !mf) : false;
}
// the one launch site of analyze_kernel: the flags from the choice, the instance's own argument block from the whole one
template <int MODE, int WAVES, typename TIN>
inline bool sp_launch_1200(hipStream_t s, const analyze_choice_t &c, const spectral_args_t &a) {
    return sp_with_flags(c.lpc, c.mf, c.full, [&](auto lpc, auto mf, auto full) {
        constexpr bool LPC = decltype(lpc)::value, MF = decltype(mf)::value, FULL = decltype(full)::value;
        if constexpr (sp_1200_instance(LPC, MF, FULL, MODE, WAVES, sp_spec_of<TIN>(), sp_burg_of<TIN>(), std::is_same<TIN, float>::value)) {
            const sp_args_of<MODE, TIN> block(a);
            hipLaunchKernelGGL((analyze_kernel<LPC, MF, FULL, MODE, WAVES, TIN>), dim3((unsigned)a.n_frames), dim3(64), c.lds, s, block);
            return true;
        } else return false;
    });
}

}  // namespace vbx
