// vbx_burg_resampled_direct.hpp -- Burg's direct recursion on the resampled view: the kernel and the launchers' choice of its template
// parameters (k_burg_resampled.hip has the description and the f64 / PCM launchers; k_burg_f32in.hip the ones for float samples).
#pragma once

#include "vbx_burg_direct.hpp"          // burg_small_groups_ok / burg_half_wave_ok: one rule for both views
#include "vbx_burg_resampled.hpp"

namespace vbx {

// n: the RESAMPLED length m (what burg_kernel calls n); window: the periodic Hanning window of length m, never null;
// rs: where sample k of the resampled frame comes from.  Everything below the load is burg_kernel<G, EPL, double>.
template <int G, int EPL, typename TIN>
__global__ __launch_bounds__(64) void burg_resampled_kernel(
    const TIN *__restrict__ x, long n_frames, int n, long stride, const double *__restrict__ window, const resample_src_t rs,
    int p, double *__restrict__ out, int32_t *__restrict__ status, const frame_map_t map,
    const int32_t *__restrict__ list = nullptr, const int32_t *__restrict__ list_count = nullptr) {
    constexpr int NG = 64 / G;
    static_assert(G == 16 || G == 32 || G == 64, "one coefficient per lane of the group: orders up to G (the launchers choose)");
    const int lane = lane_id();
    const int gid = lane / G, lig = lane % G;
    const long blk = (NG == 1 && list == nullptr) ? xcd_item(blockIdx.x, gridDim.x) : (long)blockIdx.x;
    for (long it = blk * NG;; it += (long)gridDim.x * NG) {
    long f;
    if (list != nullptr) {
        const long cnt = *list_count;
        if (it >= cnt) break;
        f = (it + gid < cnt) ? (long)list[it + gid] : -1;
    } else f = frame_map(map, it + gid, n_frames);
    const bool have = f >= 0;
    const TIN *xf = x + (have ? f : 0) * stride;

    double b1[EPL], b2[EPL];
    if constexpr (BURG_RS_LDS) {
        // the wavefront forms the windowed samples of its NG frames in order (lane l: k = l, l + 64, ..: neighbouring lanes read
        // neighbouring pairs), LDS hands them to the lanes that own them; one padding slot per EPL samples (vbx_burg_resampled.hpp)
        constexpr int ROW = G * (EPL + 1);
        __shared__ double S[NG * ROW];
        wave_sync();                                  // the list form comes round again: the last round's reads are done
#pragma unroll
        for (int g = 0; g < NG; g++) {
            long fg;                                  // the frame of group g: wave-uniform
            if (list != nullptr) fg = (it + g < *list_count) ? (long)list[it + g] : -1;
            else fg = frame_map(map, it + g, n_frames);
            if (fg < 0) continue;                     // (its lanes read nothing back)
            const TIN *xg = x + fg * stride;
            for (int k = lane; k < n; k += 64) S[g * ROW + k + k / EPL] = resampled_sample<TIN>(xg, rs, k) * window[k];
        }
        wave_sync();
#pragma unroll
        for (int e = 0; e < EPL; e++) b1[e] = (have && lig * EPL + e < n) ? S[gid * ROW + lig * (EPL + 1) + e] : 0.0;
    } else {
        // the lane's EPL windowed samples of the resampled frame: 2 EPL gathered source samples, zero past the resampled frame
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            const int j = lig * EPL + e;
            double v = 0.0;
            if (have && j < n) v = resampled_sample<TIN>(xf, rs, j) * window[j];
            b1[e] = v;
        }
    }
    const bool last_lane = (lig == G - 1);          // its "next lane" belongs to another frame
    // b2[j] = x[j+1]  (zero past the frame);  b1[j] = x[j] for j <= n-2  (src/spectrum.rs:108-114)
    {
        const double fetched = from_next_lane(b1[0]);   // DPP outside any lane-dependent branch
        const double nxt = last_lane ? 0.0 : fetched;
#pragma unroll
        for (int e = 0; e < EPL - 1; e++) b2[e] = b1[e + 1];
        b2[EPL - 1] = nxt;
        const int last = n - 1;
        const int kb = __builtin_amdgcn_readfirstlane(last % EPL), lb = last / EPL;
#pragma unroll
        for (int e = 0; e < EPL; e++) if (e == kb) { asm volatile("" : "+v"(b1[e])); if (lig == lb) b1[e] = 0.0; }   // the empty asm pins the branch
    }

    int st = 0;
    double aa = 0.0, co = 0.0;                       // lane t of the group: aa[t], coeffs[t]  (src/spectrum.rs:116-139)
    const int gbase = lane - lig;
    constexpr bool DEN_RECURSION = (G == 64);
    bool den_known = false;                          // den of this order follows from the previous order (wave-uniform)
    double den_next = 0.0, den_first = 0.0;
    for (int i = 1; i <= p; i++) {
        double num0 = 0.0, num1 = 0.0;
#pragma unroll
        for (int e = 0; e + 1 < EPL; e += 2) {
            num0 = fma(b1[e], b2[e], num0);
            num1 = fma(b1[e + 1], b2[e + 1], num1);
        }
        if (EPL & 1) num0 = fma(b1[EPL - 1], b2[EPL - 1], num0);
        double num = group_sum<G>(num0 + num1), den;
        if (den_known) den = den_next;
        else {
            double da0 = 0.0, da1 = 0.0, db0 = 0.0, db1 = 0.0;
#pragma unroll
            for (int e = 0; e + 1 < EPL; e += 2) {
                da0 = fma(b1[e], b1[e], da0);
                da1 = fma(b1[e + 1], b1[e + 1], da1);
                db0 = fma(b2[e], b2[e], db0);
                db1 = fma(b2[e + 1], b2[e + 1], db1);
            }
            if (EPL & 1) { da0 = fma(b1[EPL - 1], b1[EPL - 1], da0); db0 = fma(b2[EPL - 1], b2[EPL - 1], db0); }
            den = group_sum<G>((da0 + da1) + (db0 + db1));
            if (i == 1) den_first = den;
        }
        if (st == 0 && den <= 0.0) st = 1;           // Err(LPC), src/spectrum.rs:123-125 (NaN falls through)
        const double c = 2.0 * num / den;
        {   // coeffs[i-1] = c;  coeffs[j-1] = aa[j-1] - c * aa[i-j-1], j = 1..i-1   (t = j-1 <-> lane t)
            int srcl = i - 2 - lig;
            srcl = (srcl < 0) ? 0 : srcl;
            const double rev = __shfl(aa, gbase + srcl, 64);
            if (lig < i - 1) co = aa - c * rev;
            else if (lig == i - 1) co = c;
        }
        if (i < p) {
            if (lig < i) aa = co;                    // aa[j-1] = coeffs[j-1], j = 1..i
            const double a = c;                      // aa[i-1] == coeffs[i-1]
            const double f1 = from_next_lane(b1[0]), f2 = from_next_lane(b2[0]);
            const double nb1 = last_lane ? 0.0 : f1;
            const double nb2 = last_lane ? 0.0 : f2;
            const double e_front = fma(-a, b1[0], b2[0]);    // lane 0 of the group: the element the shift drops, b2[0] - mu b1[0]
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                const double b1n = (e + 1 < EPL) ? b1[e + 1] : nb1;   // old b1[j+1]
                const double b2n = (e + 1 < EPL) ? b2[e + 1] : nb2;   // old b2[j+1]
                const double t1 = fma(-a, b2[e], b1[e]);
                const double t2 = fma(-a, b1n, b2n);
                b1[e] = t1;
                b2[e] = t2;
            }
            // element n-i-1 leaves the valid range (the update loop runs j-1 < n-i-1)
            const int drop = n - i - 1;
            den_known = false;
            if (drop >= 0) {
                const int kb = __builtin_amdgcn_readfirstlane(drop % EPL), lb = drop / EPL;
                double e_back = 0.0;                 // lane lb of the group: b1[last] - mu b2[last], just computed
#pragma unroll
                for (int e = 0; e < EPL; e++)
                    if (e == kb) { asm volatile("" : "+v"(b1[e]), "+v"(b2[e])); e_back = b1[e]; if (lig == lb) { b1[e] = 0.0; b2[e] = 0.0; } }
                if constexpr (DEN_RECURSION) {
                    const double eb = readlane_f64(e_back, __builtin_amdgcn_readfirstlane(lb)), ef = readlane_f64(e_front, 0);
                    const double omm = fma(-a, a, 1.0);
                    den_next = fma(-ef, ef, fma(-eb, eb, omm * den));
                    const bool fine = omm > 0x1p-20 && den_next > den_first * 0x1p-24;     // NaN: not fine
                    den_known = __builtin_amdgcn_readfirstlane((int)fine) != 0;            // identical in every lane
                }
            }
        }
    }
    if (have) {
        if (lig < p) out[f * (long)p + lig] = (st == 0) ? co * -1.0 : 0.0;   // :142-144
        if (status != nullptr && lig == 0) status[f] = st;
    }
    if (list == nullptr) break;
    }
}

// launch_burg's choice of <G, EPL> at length m (launch_burg_t<double>, k_burg.hip): the dense batch is f64 whatever the source
template <typename TIN>
static void launch_burg_resampled_t(hipStream_t s, const TIN *x, long F, int m, long stride, const double *window, resample_src_t rs,
                          int p, double *out, int32_t *status, frame_map_t map) {
    dim3 b(64);
    const long items = frame_map_items(map, F);
#define VBX_BURG_RS(GG, E)                                                                                                  \
    hipLaunchKernelGGL((burg_resampled_kernel<GG, E, TIN>), dim3((unsigned)((items + (64 / GG) - 1) / (64 / GG))), b, 0, s, \
                       x, F, m, stride, window, rs, p, out, status, map, nullptr, nullptr)
    const bool g16 = burg_small_groups_ok(p);
    if (g16 && m <= 16 * 8) VBX_BURG_RS(16, 8);
    else if (g16 && m <= 16 * 16) VBX_BURG_RS(16, 16);
    else if (g16 && m <= 16 * 32) VBX_BURG_RS(16, 32);
    else if (m <= 32 * 32 && burg_half_wave_ok(p)) VBX_BURG_RS(32, 32);
    else VBX_BURG_RS(64, 20);                                 // m <= 1280 (burg_resampled_supported)
#undef VBX_BURG_RS
}

// launch_burg_list's choice (launch_burg_list_t, k_burg.hip): the frames the one-pass guard turned away
template <typename TIN>
static void launch_burg_resampled_list_t(hipStream_t s, const TIN *x, long F, int m, long stride, const double *window, resample_src_t rs,
                        int p, double *out, int32_t *status, const int32_t *list, const int32_t *count) {
    dim3 b(64);
    const frame_map_t map{0, 0, 0};
    const long cap = 8192;                                   // wavefronts (8 per SIMD); each strides over the list
#define VBX_BURG_RSL(GG, E)                                                                                                   \
    hipLaunchKernelGGL((burg_resampled_kernel<GG, E, TIN>), dim3((unsigned)((F + (64 / GG) - 1) / (64 / GG) < cap ? (F + (64 / GG) - 1) / (64 / GG) : cap)), b, 0, s, \
                       x, F, m, stride, window, rs, p, out, status, map, list, count)
    const bool g16 = burg_small_groups_ok(p);
    if (g16 && m <= 16 * 32) VBX_BURG_RSL(16, 32);
    else if (m <= 32 * 32 && burg_half_wave_ok(p)) VBX_BURG_RSL(32, 32);
    else VBX_BURG_RSL(64, 20);
#undef VBX_BURG_RSL
}

}  // namespace vbx
