// vbx_lpc_ref.hpp -- the crate's own f64 LPC rows from frames: the kernel (k_lpc_ref.hip has the description and the f64 / PCM
// launcher; k_lists_f32in.hip the one for float samples).
#pragma once

#include "vbx_device.hpp"
#include "vbx_kernels.hpp"

namespace vbx {

namespace {

constexpr int LREF_T = 128;          // samples per tile
constexpr int LREF_HALO = 64;        // lags per pass (lane offsets into the lag side)
constexpr int LREF_NB = LREF_T + LREF_HALO;   // the lag side of a tile: 192 = 3 x 64 samples, three per lane and frame
#ifndef VBX_LREF_FIXED_P
#define VBX_LREF_FIXED_P 12
#endif
constexpr int LREF_FIXED_P = VBX_LREF_FIXED_P;   // the order whose recursion runs in registers (-1: none; A/B builds)
constexpr int LREF_GMAX = 4;         // frames per wavefront at most (the staging registers: 3 samples per lane and frame)

// frames per wavefront and lanes per frame for n_lags lags
__host__ __device__ inline int lref_lanes(int n_lags) { return n_lags < 64 ? n_lags : 64; }
__host__ __device__ inline int lref_frames(int n_lags) { const int g = 64 / lref_lanes(n_lags); return g < LREF_GMAX ? g : LREF_GMAX; }
// doubles of one frame's LDS slot: the lag side (tile + halo); past 64 lags also the sample side of the tile.  Padded so that
// slot stride = lanes per frame (mod 32): lane g * L + l of the wave then reads x[i + lag] of its frame at double g * S + k + l
// = lane + k (mod 32) -- 16 consecutive lanes always hit 32 distinct banks, across frame boundaries too
__host__ __device__ inline int lref_slot(int n_lags) {
    const int base = LREF_NB + (n_lags > 64 ? LREF_T : 0);   // a multiple of 32
    return base + (lref_lanes(n_lags) & 31);
}
// The launch geometry of lpc_ref_kernel for F frames of n_lags lags, whatever the sample type (both launchers use it: the kernel
// carves its LDS by the same terms).
struct lpc_ref_geom { size_t lds; unsigned grid; };
inline lpc_ref_geom lpc_ref_geometry(long F, int n_lags) {
    const int G = lref_frames(n_lags);
    const long groups = (F + G - 1) / G;
    return {(size_t)G * lref_slot(n_lags) * sizeof(double), (unsigned)(groups < (1L << 24) ? groups : (1L << 24))};
}

// max_amplitude + normalize of r[0..n) in place (src/waves.rs:44-58,68-75): the fold starts from |r[0]| and keeps its value
// unless an amplitude is strictly greater (a NaN never wins; one in r[0] stays); amplitude(s) = s < 0 ? s * -1 : s
__device__ __forceinline__ void normalize_ref(double *r, int n) {
#pragma clang fp contract(off)
    auto amp = [](double s) { return (s < 0.0) ? s * -1.0 : s; };
    double m = amp(r[0]);
    for (int i = 1; i < n; i++) { const double a = amp(r[i]); if (a > m) m = a; }
    const double scale = 1.0 / m;
    for (int i = 0; i < n; i++) r[i] = r[i] * scale;
}

// LPC::lpc_mut (src/spectrum.rs:63-84) with lpc's zeroed work vectors (:86-92), at a runtime order: ac[0..p], tmp[0..p)
// scratch, kc[0..p) (optional) the reflection coefficients
__device__ __forceinline__ void levinson_ref(const double *r, int p, double *ac, double *tmp, double *kc, long kc_step) {
#pragma clang fp contract(off)
    double err = r[0];
    ac[0] = 1.0;
    for (int i = 1; i <= p; i++) ac[i] = 0.0;
    for (int i = 1; i <= p; i++) {
        double acc = r[i];
        for (int j = 1; j < i; j++) acc = acc + (ac[j] * r[i - j]);
        const double k = -acc / err;
        ac[i] = k;
        if (kc != nullptr) kc[(long)(i - 1) * kc_step] = k;
        for (int j = 1; j < i; j++) tmp[j] = ac[j];          // (the reference copies all of ac; only tmp[1 .. i) is read)
        for (int j = 1; j < i; j++) ac[j] = ac[j] + (k * tmp[i - j]);
        err = err * (1.0 - (k * k));
    }
}

// the same at a compile-time order, every array in registers
template <int P>
__device__ __forceinline__ void levinson_ref_fixed(const double (&r)[P + 1], double (&ac)[P + 1]) {
#pragma clang fp contract(off)
    double tmp[P + 1];
    double err = r[0];
    ac[0] = 1.0;
#pragma unroll
    for (int i = 1; i <= P; i++) ac[i] = 0.0;
#pragma unroll
    for (int i = 1; i <= P; i++) {
        double acc = r[i];
#pragma unroll
        for (int j = 1; j < i; j++) acc = acc + (ac[j] * r[i - j]);
        const double k = -acc / err;
        ac[i] = k;
#pragma unroll
        for (int j = 1; j < i; j++) tmp[j] = ac[j];
#pragma unroll
        for (int j = 1; j < i; j++) ac[j] = ac[j] + (k * tmp[i - j]);
        err = err * (1.0 - (k * k));
    }
}

// sample j of frame f as the crate's callers hand it to the traits: f64 (or 16-bit PCM widened as vbx_pcm16_to_f64 widens it),
// times the window's entry with one rounding.  Split in two: the raw load (issued a tile ahead) and the widening + window
// product (when the tile is written to LDS).
// (F32: float32 samples, every one a double: widened as they are)
template <bool PCM, bool F32 = false> struct ref_raw { using type = double; };
template <> struct ref_raw<true, false> { using type = int; };
template <> struct ref_raw<false, true> { using type = float; };
template <bool PCM, bool F32 = false>
__device__ __forceinline__ typename ref_raw<PCM, F32>::type ref_load(const void *x, long f, long stride, int j, int n) {
    static_assert(!(PCM && F32), "one sample format");
    if (j >= n) return 0;
    if constexpr (PCM) return (int)static_cast<const int16_t *>(x)[f * stride + j];
    else if constexpr (F32) return static_cast<const float *>(x)[f * stride + j];
    else return static_cast<const double *>(x)[f * stride + j];
}
template <bool PCM, bool F32 = false>
__device__ __forceinline__ double ref_value(typename ref_raw<PCM, F32>::type v, double w) {
#pragma clang fp contract(off)
    double d;
    if constexpr (PCM) d = pcm16_value(v);
    else d = (double)v;
    return d * w;                                            // w = 1 without a window: the same bits
}

// One wavefront per G frames.  lane = g * L + l: frame f0 + g, lag lag0 + l.  P: the order when it is 12 (the recursion in
// registers), 0 otherwise (p at run time; p == 0: lag sums only).
// Tiles are software-pipelined: the samples of tile c + T are loaded into registers (3 per lane and frame, + 2 of the sample side
// past 64 lags) while tile c folds out of LDS, and written to LDS after it.
template <bool PCM, int P, bool F32 = false>
__global__ __launch_bounds__(64) void lpc_ref_kernel(const void *__restrict__ x, long F, int n, long stride, const double *__restrict__ window,
                                                     int n_lags, int p, int normalize, double *__restrict__ out_r, long r_ld,
                                                     double *__restrict__ out_lpc, long lpc_ld) {
#pragma clang fp contract(off)
    using raw_t = typename ref_raw<PCM, F32>::type;
    extern __shared__ __attribute__((aligned(16))) double lref_sm[];
    const int L = lref_lanes(n_lags), G = lref_frames(n_lags), S = lref_slot(n_lags);
    const int lane = lane_id();
    const int g = lane / L, l = lane - g * L;
    const long n_groups = (F + G - 1) / G;
    for (long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const long f0 = grp * G;
        const int gn = (F - f0 < G) ? (int)(F - f0) : G;     // frames of this group
        const bool mine = g < gn;
        const long f = f0 + g;
        double *slot = lref_sm + (mine ? g : 0) * S;
        for (int lag0 = 0; lag0 < n_lags; lag0 += 64) {
            const int lag = lag0 + l;
            const bool act = mine && lag < n_lags;
            // lag side B[j] = x[c + lag0 + j], j < T + 64; sample side A[j] = x[c + j], j < T (B itself while lag0 == 0)
            raw_t pb_raw[LREF_GMAX][3], pa_raw[2];
            double wb[3], wa[2];
            auto issue = [&](int c) {
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const int j = c + lag0 + lane + 64 * q;
                    wb[q] = (window != nullptr && j < n) ? window[j] : 1.0;
#pragma unroll
                    for (int h = 0; h < LREF_GMAX; h++)
                        if (h < gn) pb_raw[h][q] = ref_load<PCM, F32>(x, f0 + h, stride, j, n);
                }
                if (lag0 > 0) {                               // (one frame per wave)
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        const int j = c + lane + 64 * q;
                        wa[q] = (window != nullptr && j < n) ? window[j] : 1.0;
                        pa_raw[q] = ref_load<PCM, F32>(x, f0, stride, j, n);
                    }
                }
            };
            const int c_end = n - lag0;                       // lags >= lag0: i + lag < n needs i < n - lag0
            double acc = 0.0;
            issue(0);
            for (int c = 0; c < c_end; c += LREF_T) {
                wave_sync();                                  // the previous tile's reads are done
#pragma unroll
                for (int h = 0; h < LREF_GMAX; h++)
                    if (h < gn)
#pragma unroll
                        for (int q = 0; q < 3; q++) lref_sm[h * S + lane + 64 * q] = ref_value<PCM, F32>(pb_raw[h][q], wb[q]);
                if (lag0 > 0)
#pragma unroll
                    for (int q = 0; q < 2; q++) lref_sm[LREF_NB + lane + 64 * q] = ref_value<PCM, F32>(pa_raw[q], wa[q]);
                wave_sync();
                if (c + LREF_T < c_end) issue(c + LREF_T);    // in flight during the fold below
                const double *A = (lag0 > 0) ? slot + LREF_NB : slot, *B = slot;
                if (c == 0) acc = A[0];                       // the fold's seed (Q1)
                const int lo = c > 1 ? c : 1;
                int hi = n - lag;
                if (hi > c + LREF_T) hi = c + LREF_T;
                const int m = act ? hi - lo : 0;              // i in [lo, hi): A[i - c], B[i - c + l]
                const double *pa = A + (lo - c), *pb = B + (lo - c) + l;
                int k = 0;
                for (; k + 4 <= m; k += 4) {
                    acc = acc + pa[k] * pb[k];
                    acc = acc + pa[k + 1] * pb[k + 1];
                    acc = acc + pa[k + 2] * pb[k + 2];
                    acc = acc + pa[k + 3] * pb[k + 3];
                }
                for (; k < m; k++) acc = acc + pa[k] * pb[k];
            }
            if (p == 0) {
                if (act) out_r[f * r_ld + lag] = acc;
                continue;
            }
            // LPC rows (n_lags = p + 1 <= 63: one pass): the frame's lag sums into its slot, the recursion on lane g * L
            wave_sync();
            if (act) slot[l] = acc;
            wave_sync();
            if (mine && l == 0) {
                double *r = slot;
                if (normalize) normalize_ref(r, n_lags);
                if (out_r != nullptr)
                    for (int i = 0; i < n_lags; i++) out_r[f * r_ld + i] = r[i];
                if (out_lpc != nullptr) {
                    double *o = out_lpc + f * lpc_ld;
                    if constexpr (P > 0) {
                        double rr[P + 1], ac[P + 1];
#pragma unroll
                        for (int i = 0; i <= P; i++) rr[i] = r[i];
                        levinson_ref_fixed<P>(rr, ac);
#pragma unroll
                        for (int i = 0; i <= P; i++) o[i] = ac[i];
                    } else {
                        double *ac = slot + 64, *tmp = slot + 128;
                        levinson_ref(r, p, ac, tmp, nullptr, 0);
                        for (int i = 0; i <= p; i++) o[i] = ac[i];
                    }
                }
            }
        }
        wave_sync();                                          // the slots are refilled by the next group
    }
}

}  // namespace

}  // namespace vbx
