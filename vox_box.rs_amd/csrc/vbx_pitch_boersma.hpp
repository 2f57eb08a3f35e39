// vbx_pitch_boersma.hpp -- Boersma (1993) pitch candidates of ONE frame by one wavefront: the lag curve of Pitched::pitch
// (src/periodic.rs:400-411, unchanged), then the refinement the crate's comment describes and its code misses (SURVEY Appendix A:
// Q5 the parabola's sign, Q6 the swapped sample indices of interpolate_sinc, Q8 a minimiser called as a maximiser, all three undone).
// include/voxbox_hip.h (vbx_pitch_boersma_f64) has the definition; tests/pitch_boersma_model.py is its executable form.
//
//  1) curve      the frame image into LDS, the all-lag autocorrelation on the FP64 matrix cores, scale and lag-window division into
//                ys: the front of pitch_frame_mfma (vbx_pitch_frame.hpp), repeated here so that pitch_kernel's code stays as it is;
//  2) peaks      strict local maxima of y[1 .. H-1), the parabolic lag x0 and the frequency filter, lane-parallel, compacted in
//                lag order into an LDS list; the first-pass strength s1 = S_30(x0) by groups of 16 lanes, four peaks at a time;
//  3) selection  Praat's rule: the m = min(kmax, count) entries with the largest s1 (the unvoiced entry competes with s1 =
//                threshold), by a rank count across lanes -- a tie goes to the earlier entry -- kept in list order;
//  4) refinement brent_maximize's iteration (src/periodic.rs:103-188) on -S_1200 over [x0 - 1, x0 + 1] for every kept voiced
//                entry, G lanes per entry (64: one entry at a time, every decision taken once per wavefront; 16: four at a time);
//  5) order      stable rank sort by descending strength, the row and the count.
#pragma once

#include "vbx_autocorr.hpp"
#include "vbx_kernels.hpp"
#include "vbx_pitch_refine.hpp"

namespace vbx {

constexpr int BOERSMA_DEPTH_FIRST = 30, BOERSMA_DEPTH_REFINE = 1200;
constexpr int BOERSMA_MAX_KMAX = 63;             // the pitch path's cap (vbx_pitch_path_f64)
constexpr int BOERSMA_MIN_FRAME = 16, BOERSMA_MAX_FRAME = 4096;

// the peak list: at most n / 4 strict maxima below n / 2, and the unvoiced entry
__host__ __device__ constexpr int boersma_list_entries(int n) { return n / 4 + 8; }
size_t pitch_boersma_lds_bytes(int n);
// group: lanes per refined entry, 64 or 16
void launch_pitch_boersma(hipStream_t s, const double *x, long F, int n, long stride, const double *window,
                          const double *lag_window, double sample_rate, double threshold, double fmin, double fmax,
                          int kmax, int group, pitch_t *out_cand, int32_t *out_count, int32_t *status);

#ifdef __HIPCC__

// One lane's share of S_depth(x) when the clamped depth D is small (D < G): the terms n = lig / 2, + G / 2, ... < D of one side.
// The term n = D of either side has the taper 0.5 + 0.5 cos(pi) = 0 and is not evaluated (a non-finite last lag cannot reach the sum).
template <int G>
__device__ __forceinline__ double boersma_terms_general(const double *y, int nl, int nr, double phil, double phir, int D) {
    const int lig = lane_id() & (G - 1);
    const int side = lig & 1;
    const double ph = side ? phir : phil;
    const double s0 = sin_poly(M_PI * fmin(phil, phir));      // sin(pi (ph + n)) = (-1)^n sin(pi ph), the same on both sides
    const double h2 = M_PI * rcp_nr2(ph + (double)D);
    double acc = 0.0;
    for (int n = lig >> 1; n < D; n += G / 2) {
        const double a = ph + (double)n;
        const double r_lag = y[side ? (nr + n) : (nl - n)];
        const double first = ((n & 1) ? -s0 : s0) * rcp_nr2(M_PI * a);
        const double second = fma(0.5, cos_0_pi(h2 * a), 0.5);
        acc = fma(r_lag * first, second, acc);
    }
    return acc;
}

// The same share by the stream machinery of sinc_terms_fast (vbx_pitch_refine.hpp) with each side reading its OWN samples: the
// left stream descends from y[nl], the right one ascends from y[nr].  D >= G: every lane has at least two terms and the
// recurrence's angle step pi (G / 2) / (ph + D) stays below pi / 2.
template <int G>
__device__ __forceinline__ double boersma_terms_fast(const double *y, int nl, int nr, double phil, double phir, int D) {
    constexpr int NSTEP = G / 2;
    const int lig = lane_id() & (G - 1);
    const int side = lig & 1;
    const int n0 = lig >> 1;
    const double s0 = sin_poly(M_PI * fmin(phil, phir));
    const int nterms = (D - 1 - n0) / NSTEP + 1;              // n = n0, n0 + NSTEP, ... <= D - 1
    sinc_stream_t s;
    sinc_stream_init<NSTEP>(s, y, side, n0, nl, nr, phil, phir, D);
    const int step = side ? NSTEP : -NSTEP;
    int j = 0;
    for (; j + 4 <= nterms; j += 4) sinc_stream_block4<NSTEP>(s, step);
    if (j < nterms) sinc_stream_tail<NSTEP>(s, step, nterms - j);
    return sinc_stream_result(s, n0, s0 * (0.5 * 0.31830988618379067154));
}

// S_depth(x) of the definition, cooperative over groups of G lanes: x is uniform inside a group and the result is bit-identical
// in all its lanes; lanes with active == false contribute nothing.  y[0 .. n) is the curve and Y_PAD zeros follow it; x lies in [-1, n / 2 + 1), so
// every index read is in [0, n].  Must be called from converged code.
template <int G>
__device__ __forceinline__ double boersma_interp(const double *y, double x, int depth, bool active) {
    bool summed = false, fast = false;
    double special = 0.0, phil = 0.5, phir = 0.5;
    int nl = 0, D = 0;
    if (active) {
        if (!(x >= 0.0)) special = y[0];                                       // :40
        else {
            const double fl = floor(x);
            nl = (int)fl;
            phil = x - fl;
            phir = 1.0 - phil;
            if (fabs(x - (double)nl) < 1.0e-10) special = y[nl];               // :41
            else if (fabs(x - (double)(nl + 1)) < 1.0e-10) special = y[nl + 1];  // :42
            else {
                D = (depth < nl) ? depth : nl;
                summed = true;
                fast = D >= G;
            }
        }
    }
    double acc = 0.0;
    if (summed) {
        if (fast) acc = boersma_terms_fast<G>(y, nl, nl + 1, phil, phir, D);
        else acc = boersma_terms_general<G>(y, nl, nl + 1, phil, phir, D);
    }
    const double total = group_sum<G>(acc);
    const double v = summed ? total : special;
    if constexpr (G == 64) return readfirstlane_f64(v);       // one entry per wavefront: the value, and every decision on it, is scalar
    return v;
}

// brent_maximize (src/periodic.rs:103-188) on f = -S_depth over [x0 - 1, x0 + 1]: the reference's iteration -- golden constant,
// tol = 1e-10, the sqrt(EPSILON) term, at most 60 iterations -- as improve_extremum_sinc runs it, on the negated interpolant.
// One entry per group of G lanes; returns (xmid, S_depth(xmid)).  Must be called from converged code.
template <int G>
__device__ __forceinline__ void boersma_brent(const double *y, double x0, int depth, bool active, double &xmid, double &smax) {
#pragma clang fp contract(off)
    const double golden = 1. - 0.6180339887498948482045868343656381177203091798057628621;
    const double sqrt_epsilon = 1.4901161193847656e-08;   // sqrt(f64::EPSILON)
    const double eps = 2.220446049250313e-16;
    const double tol = 1e-10;
    double a = x0 - 1., b = x0 + 1.;
    double v = a + golden * (b - a);
    double fv = -boersma_interp<G>(y, v, depth, active);
    double x = v, w = v, fx = fv, fw = fv;
    bool done = !active;
    for (int it = 1; it <= 60; it++) {
        const double range = b - a;
        const double middle_range = (a + b) * 0.5;
        const double tol_act = sqrt_epsilon * fabs(x) + tol / 3.;
        if (!done && fabs(x - middle_range) + range * 0.5 <= 2. * tol_act) done = true;
        if (!__any(!done)) break;
        double new_step = (x < middle_range) ? golden * (b - x) : golden * (a - x);
        if (fabs(x - w) >= tol_act) {
            const double t = (x - w) * (fx - fv);
            double q = (x - v) * (fx - fw);
            double p = (x - v) * q - (x - w) * t;
            q = 2. * q - t;
            if (q > 0.) p = -p; else q = -q;
            if (fabs(p) < fabs(new_step * q) && p > q * (a - x + 2. * tol_act) && p < q * (b - x - 2. * tol_act))
                new_step = p / q;
        }
        if (fabs(new_step) < tol_act) new_step = (new_step > 0.) ? tol_act : -tol_act;
        const double t = x + new_step;
        const double ft = -boersma_interp<G>(y, t, depth, !done);
        if (!done) {
            if (ft <= fx) {
                if (t < x) b = x; else a = x;
                v = w; w = x; x = t;
                fv = fw; fw = fx; fx = ft;
            } else {
                if (t < x) a = t; else b = t;
                if (ft <= fw || fabs(w - x) < eps) {
                    v = w; w = t;
                    fv = fw; fw = ft;
                } else if (ft <= fv || fabs(v - x) < eps || fabs(v - w) < eps) {
                    v = t;
                    fv = ft;
                }
            }
        }
    }
    xmid = x; smax = -fx;
}

// selection and sort key: a NaN strength ranks first, so that it is selected and reported (VBX_FRAME_ERR_NAN), never dropped
__device__ __forceinline__ double boersma_key(double s) { return (s != s) ? __builtin_inf() : s; }
__device__ __forceinline__ double boersma_reflect(double s) { return (s > 1.0) ? 1.0 / s : s; }

// ALIAS: a single autocorrelation pass (n <= AC_MF_NT * 256): y takes the image's place in LDS.  G: lanes per refined entry.
template <bool ALIAS, int G>
__device__ __forceinline__ void pitch_boersma_frame(
    double *smem, const long f, const double *__restrict__ frames, int n, long stride, const double *__restrict__ window,
    const double *__restrict__ lag_window, double sample_rate, double threshold, double fmin, double fmax,
    int kmax, double *__restrict__ out_cand, int32_t *__restrict__ out_count, int32_t *__restrict__ status) {
    const int lane = lane_id();
    double *zs = smem;                              // padded image of the windowed frame (vbx_autocorr.hpp)
    // y[n + Y_PAD] | list x0 | list s1 | selected x0[64] | selected s1[64] | refined frequency[64] | refined strength[64]
    double *ys = ALIAS ? smem : smem + ((ac_mf_lds_doubles(n) + 1) & ~1);
    double *lx = ys + n + Y_PAD, *ls = lx + boersma_list_entries(n);
    double *selx = ls + boersma_list_entries(n), *sels = selx + 64, *resf = sels + 64, *ress = resf + 64;

    // ---- 1) the curve: pitch_frame_mfma's steps 1-2 (f64 frames only) ----
    {
        const double *xf = frames + f * stride;
        constexpr int NB = 8;
        for (int p = lane; p < ac_mf_phys(0); p += 64) zs[p] = 0.0;
        for (int p = ac_mf_phys(n) + lane; p < ac_mf_lds_doubles(n); p += 64) zs[p] = 0.0;
        for (int i0 = 0; i0 < n; i0 += 64 * NB) {
            double xv[NB], wv[NB];
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const int i = i0 + 64 * j + lane;
                xv[j] = (i < n) ? xf[i] : 0.0;
                wv[j] = (window != nullptr && i < n) ? window[i] : 1.0;
            }
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const int i = i0 + 64 * j + lane;
                if (i < n) zs[ac_mf_phys(i)] = (window != nullptr) ? xv[j] * wv[j] : xv[j];
            }
        }
        wave_sync();
    }
    const double xw0 = zs[ac_mf_phys(0)];
    double amax = -1.0;                             // max_amplitude over ALL lags (Q2; NaN never wins)
    if (ALIAS) {
        double rv[AC_MF_NT * 4];
        autocorr_mfma(zs, n, n, [&](int slot, int lag, double s) {
            const double r = (lag < n) ? (s - xw0 * zs[ac_mf_phys(lag)]) + xw0 : 0.0;
            rv[slot] = r;
            const double a = fabs(r);
            amax = (lag < n && a > amax) ? a : amax;
        });
        wave_sync();                                // every lane is done with the image
        amax = wave_max(amax);
        const double scale = 1.0 / amax;
#pragma unroll
        for (int slot = 0; slot < AC_MF_NT * 4; slot++) {
            const int lag = (slot >> 2) * AC_MF_TILE + 64 * (slot & 3) + lane;
            if (lag < n) ys[lag] = (rv[slot] * scale) / lag_window[lag];
        }
        if (lane < Y_PAD) ys[n + lane] = 0.0;
    } else {
        autocorr_mfma(zs, n, n, [&](int, int lag, double s) {
            if (lag < n) {
                const double r = (s - xw0 * zs[ac_mf_phys(lag)]) + xw0;
                ys[lag] = r;
                const double a = fabs(r);
                amax = (a > amax) ? a : amax;
            }
        });
        wave_sync();
        amax = wave_max(amax);
        const double scale = 1.0 / amax;
        for (int i = lane; i < n; i += 64) ys[i] = (ys[i] * scale) / lag_window[i];
        if (lane < Y_PAD) ys[n + lane] = 0.0;
    }
    wave_sync();

    // ---- 2) peaks, parabolic lag, filter; first-pass strength ----
    const int H = n / 2;
    int ncand = 0;
    for (int base = 0; base < H - 1; base += 64) {
#pragma clang fp contract(off)
        const int k = base + lane;
        bool keep = false;
        double x0 = 0.0;
        if (k >= 1 && k < H - 1) {
            const double ym = ys[k - 1], yk = ys[k], yp = ys[k + 1];
            if (ym < yk && yk > yp) {
                const double dr = 0.5 * (yp - ym);
                const double d2r = 2.0 * yk - ym - yp;
                const double dx = dr / d2r;                      // |dx| < 0.5 but for cancellation in d2r
                x0 = (double)k + dx;
                const double f0 = sample_rate / x0;
                keep = fmin < f0 && f0 < fmax && fabs(dx) <= 1.0;
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) lx[ncand + __popcll(mask & ((1ull << lane) - 1ull))] = x0;
        ncand += __popcll(mask);
    }
    wave_sync();
    for (int c0 = 0; c0 < ncand; c0 += PNG) {
        const int q = c0 + lane / PG;
        const bool have = q < ncand;
        const double s = boersma_interp<PG>(ys, have ? lx[q] : 0.0, BOERSMA_DEPTH_FIRST, have);
        if (have && (lane & (PG - 1)) == 0) ls[q] = boersma_reflect(s);
    }
    if (lane == 0) { lx[ncand] = 0.0; ls[ncand] = threshold; }      // the unvoiced entry (0, threshold): x0 == 0 marks it
    wave_sync();

    // ---- 3) selection: the m entries with the largest s1, in list order ----
    const int total = ncand + 1;
    const int m = (kmax < total) ? kmax : total;
    if (total <= kmax) {
        for (int i = lane; i < total; i += 64) { selx[i] = lx[i]; sels[i] = ls[i]; }
    } else {
        int nsel = 0;
        for (int base = 0; base < total; base += 64) {
            const int i = base + lane;
            const bool have = i < total;
            const double ki = boersma_key(have ? ls[i] : 0.0);
            int rank = 0;
            for (int j = 0; j < total; j++) {
                const double kj = boersma_key(ls[j]);
                rank += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
            }
            const bool sel = have && rank < m;
            const unsigned long long mask = __ballot(sel);
            if (sel) {
                const int pos = nsel + __popcll(mask & ((1ull << lane) - 1ull));
                selx[pos] = lx[i]; sels[pos] = ls[i];
            }
            nsel += __popcll(mask);
        }
    }
    wave_sync();

    // ---- 4) refinement of the kept voiced entries ----
    for (int j0 = 0; j0 < m; j0 += 64 / G) {
        const int q = j0 + lane / G;
        const bool have = q < m;
        double xq = have ? selx[q] : 0.0;
        if constexpr (G == 64) xq = readfirstlane_f64(xq);
        const bool voiced = have && xq != 0.0;
        double xmid, smax;
        boersma_brent<G>(ys, voiced ? xq : 2.0, BOERSMA_DEPTH_REFINE, voiced, xmid, smax);
        if (have && (lane & (G - 1)) == 0) {
            resf[q] = voiced ? sample_rate / xmid : 0.0;
            ress[q] = voiced ? boersma_reflect(smax) : sels[q];
        }
    }
    wave_sync();

    // ---- 5) status, stable sort by descending strength, the row ----
    const bool mine = lane < m;
    const double fq = mine ? resf[lane] : 0.0, sq = mine ? ress[lane] : 0.0;
    const double s1q = mine ? sels[lane] : 0.0;
    const bool bad = __any(mine && (sq != sq || s1q != s1q));
    int rank = 0;
    for (int j = 0; j < m; j++) {
        const double sj = ress[j];
        rank += (sj > sq || (sj == sq && j < lane)) ? 1 : 0;
    }
    double *row = out_cand + f * (2 * (long)kmax);
    if (lane < kmax && (lane >= m || bad)) store_pair8(row + 2 * lane, double2{0.0, 0.0});
    if (mine && !bad) store_pair8(row + 2 * rank, double2{fq, sq});
    if (lane == 0) {
        out_count[f] = bad ? 0 : total;
        if (status != nullptr) status[f] = bad ? 3 : 0;              // VBX_FRAME_ERR_NAN : VBX_FRAME_OK
    }
}

#endif  // __HIPCC__

}  // namespace vbx
