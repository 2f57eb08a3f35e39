// vbx_burg_resampled.hpp (k_burg_resampled.hip: the direct recursion and the dispatch; k_burg_resampled_p*.hip: the lag kernels,
// one translation unit per order) -- Burg straight from the UN-RESAMPLED view: find_formants with resample_ratio != 1.0
// (src/lib.rs:40-64) runs Burg on the m = ceil(ratio * frame_len) samples
//     r[k] = (x[li[k] + 1] - x[li[k]]) * frac[k] + x[li[k]]          (two roundings, zero past the frame: resample_kernel, k_front.hip)
// times the periodic Hanning window of length m.  The kernels here are burg_kernel (k_burg.hip) and burg_lags_kernel
// (vbx_burg_fast.hpp) with that expression as the frame source: a lane produces its EPL windowed samples from the caller's
// hop-strided frames, and everything after the samples are in registers is those kernels' code at the template parameters
// the dense path picks for length m -- the results are the dense path's (vbx_resample_linear_f64 into a [F, m] batch, then
// vbx_find_formants_f64 on it) BIT FOR BIT, without the batch's 8 m bytes per frame written to HBM and read back.
// Access pattern (DESIGN.md section 5c has the measurements).  The kernels want sample k = lane * EPL + e in lane `lane`; loaded
// that way, one wave instruction reads 64 addresses ~4.8 EPL samples apart -- 64 cache lines per instruction, and the address
// path bounds the kernel (VBX_BURG_RS_GATHER=1 builds that form, for the A/B).  Instead the wavefront forms the frame's samples
// in order -- lane l takes k = l, l + 64, ..: neighbouring lanes read neighbouring pairs, ~19 lines per instruction at ratio
// 0.21 -- multiplies them by the window and hands them to their owners through LDS, one padding slot per EPL samples so that
// the owners' contiguous reads are free of bank conflicts: 8 (EPL + 1) bytes per lane, 4.6 .. 17 KB per wavefront.
#pragma once

#include "vbx_burg_fast.hpp"

#ifndef VBX_BURG_RS_GATHER
#define VBX_BURG_RS_GATHER 0
#endif

namespace vbx {

constexpr bool BURG_RS_LDS = VBX_BURG_RS_GATHER == 0;        // the resampled frame through LDS (default), or per-lane gathers

// sample k of the resampled frame (resample_src_t, vbx_kernels.hpp: li / frac = the context's resample table, n_src = the
// caller's frame length); TIN = int16_t: 16-bit PCM widened by pcm16_value first; TIN = float: float32 samples, widened as they are
template <typename TIN>
__device__ __forceinline__ double resampled_sample(const TIN *__restrict__ xf, const resample_src_t &rs, int k) {
#pragma clang fp contract(off)   // (diff * value) + left, two roundings as resample_kernel
    const int li = rs.li[k];
    double left = 0.0, right = 0.0;
    if constexpr (sizeof(TIN) == 2) {
        if (li < rs.n_src) left = pcm16_value((int)xf[li]);
        if (li + 1 < rs.n_src) right = pcm16_value((int)xf[li + 1]);
    } else {
        if (li < rs.n_src) left = xf[li];
        if (li + 1 < rs.n_src) right = xf[li + 1];
    }
    const double diff = right - left;
    return (diff * rs.frac[k]) + left;
}

// burg_lags_kernel<EPL, P, TIN> of vbx_burg_fast.hpp on the resampled view: n = m, the resampled length (<= 64 EPL); `window`:
// the periodic Hanning window of length m.  Same scratch, same recursion kernel behind it.
template <int EPL, int P, typename TIN>
__global__ __launch_bounds__(64) void burg_lags_resampled_kernel(
    const TIN *__restrict__ x, long n_frames, int n, long stride, const double *__restrict__ window, const resample_src_t rs,
    const frame_map_t map, long item0, long items, double *__restrict__ scratch) {
    constexpr int FPW = bf_fpw<EPL>::value;
    constexpr int NL = P + 1;
    constexpr int TS = NL | 1;
    static_assert(EPL % 2 == 0 && EPL >= 2, "pairs of samples per lane");
    // per-frame transpose buffer [lane][lag]; before the lag sums exist it carries the windowed frame to the lanes that own it
    // (S below: read before TR is written, written again only behind the reduction's wave_sync)
    constexpr int S_LEN = BURG_RS_LDS ? 64 * (EPL + 1) : 0;
    __shared__ double TR[64 * TS > S_LEN ? 64 * TS : S_LEN];
    __shared__ double REC[3 * NL * FPW];             // [value][frame of the batch]: C, then HD, then TL
    const int lane = lane_id();
    const long i0 = item0 + (long)blockIdx.x * FPW;
    if (i0 >= item0 + items) return;
    const int nf = (int)((item0 + items - i0 < FPW) ? (item0 + items - i0) : FPW);

    double *const S = TR;
    // slot e of a lane holds sample k = lane * EPL + e of the resampled frame (the layout of burg_lags_kernel), or -- on the
    // way through LDS -- sample k = lane + 64 e
    auto sample_of = [&](int e) { return BURG_RS_LDS ? lane + 64 * e : lane * EPL + e; };
    double wreg[EPL];
#pragma unroll
    for (int e = 0; e < EPL; e++) {
        const int i = sample_of(e);
        wreg[e] = (i < n) ? ((window != nullptr) ? window[i] : 1.0) : 0.0;
    }
    // the lane's EPL resampled samples of frame g of the batch (zero past the resampled frame, or without a frame)
    auto load_frame = [&](int g, double (&dst)[EPL]) {
        const long f = frame_map(map, i0 + g, n_frames);
        const TIN *xf = x + (f < 0 ? 0 : f) * stride;
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            const int k = sample_of(e);
            dst[e] = (f >= 0 && k < n) ? resampled_sample<TIN>(xf, rs, k) : 0.0;
        }
    };
    // frames in flight: burg_lags_kernel's two (the gather form); through LDS one -- its loads are issued once the frame before
    // it has gone into LDS and fly under that frame's products, and the registers of the other two buffers are what the form
    // needs to keep burg_lags_kernel's occupancy
    double cur[EPL], nxt[EPL], nx2[BURG_RS_LDS ? 1 : EPL];
    load_frame(0, cur);
    if constexpr (!BURG_RS_LDS) { if (nf > 1) load_frame(1, nxt); }
    const int red_lag = lane >> 2, red_part = lane & 3;

    for (int g = 0; g < nf; g++) {
        double ext[EPL + NL - 1];
        if constexpr (BURG_RS_LDS) {
            // (the previous frame's reads of S lie before the two wave_sync() of its reduction)
#pragma unroll
            for (int e = 0; e < EPL; e++) { const int k = lane + 64 * e; S[k + k / EPL] = cur[e] * wreg[e]; }
            wave_sync();
            if (g + 1 < nf) load_frame(g + 1, nxt);
#pragma unroll
            for (int e = 0; e < EPL; e++) ext[e] = S[lane * (EPL + 1) + e];
        } else {
            if (g + 2 < nf) load_frame(g + 2, nx2);
#pragma unroll
            for (int e = 0; e < EPL; e++) ext[e] = cur[e] * wreg[e];
        }
#pragma unroll
        for (int e = EPL; e < EPL + NL - 1; e++) ext[e] = from_next_lane(ext[e - EPL]);
        double part[NL];
#pragma unroll
        for (int lag = 0; lag < NL; lag++) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int e = 0; e < EPL; e += 2) { s0 = fma(ext[e], ext[e + lag], s0); s1 = fma(ext[e + 1], ext[e + 1 + lag], s1); }
            part[lag] = s0 + s1;
        }
#pragma unroll
        for (int lag = 0; lag < NL; lag++) TR[lane * TS + lag] = part[lag];
        // the frame's first and last P + 1 samples
        if (lane * EPL <= P || (lane + 1) * EPL >= n - 1 - P) {
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                const int i = lane * EPL + e;
                if (i <= P) REC[(NL + i) * FPW + g] = ext[e];
                if (i < n && i >= n - 1 - P) REC[(2 * NL + (n - 1 - i)) * FPW + g] = ext[e];
            }
        }
        wave_sync();
#pragma unroll
        for (int lbase = 0; lbase < NL; lbase += 16) {   // 16 lags per sweep (4 lanes per lag)
            const int rl = lbase + red_lag;
            double tot = 0.0;
            if (rl < NL) {
#pragma unroll
                for (int t = 0; t < 16; t++) tot += TR[(red_part * 16 + t) * TS + rl];
            }
            tot += dpp_f64<DPP_QUAD_XOR1>(tot);
            tot += dpp_f64<0x4E>(tot);               // quad_perm [2,3,0,1]
            if (red_part == 0 && rl < NL) REC[rl * FPW + g] = tot;
        }
        wave_sync();
        if constexpr (BURG_RS_LDS) {
#pragma unroll
            for (int e = 0; e < EPL; e++) cur[e] = nxt[e];
        } else {
#pragma unroll
            for (int e = 0; e < EPL; e++) { cur[e] = nxt[e]; nxt[e] = nx2[e]; }
        }
    }
    static_assert(64 % FPW == 0, "a batch stays inside one tile");
    const long c0 = i0 - item0;
    double *o = scratch + (c0 >> 6) * (3 * NL * 64) + (c0 & 63);
    for (int idx = lane; idx < 3 * NL * FPW; idx += 64) {
        const int v = idx / FPW, g = idx % FPW;
        if (g < nf) o[v * 64 + g] = REC[idx];
    }
}

constexpr int BURG_RESAMPLED_MAX_M = 64 * 20;        // the lag kernels with all of a lane's samples in registers (EPL 8 / 16 / 20)

// per-order launcher: explicit instantiations live in k_burg_resampled_p<P>.hip
template <int P, typename TIN>
void launch_burg_lags_resampled_p(hipStream_t s, const TIN *x, long F, int m_len, long stride, const double *window,
                                  resample_src_t rs, frame_map_t map, long i0, long m, double *scratch);

// (the definition apart, for the translation units that instantiate it for another sample type)
#define VBX_BURG_RESAMPLED_DEFINE                                                                                             \
    template <int PP, typename TIN>                                                                                           \
    void launch_burg_lags_resampled_p(hipStream_t s, const TIN *x, long F, int n, long stride, const double *window,         \
                                      resample_src_t rs, frame_map_t map, long i0, long m, double *scratch) {                 \
        const dim3 grid((unsigned)((m + BF_FPW - 1) / BF_FPW)), b(64);                                                        \
        const dim3 grid8((unsigned)((m + bf_fpw<8>::value - 1) / bf_fpw<8>::value));                                          \
        if (n <= 64 * 8) hipLaunchKernelGGL((burg_lags_resampled_kernel<8, PP, TIN>), grid8, b, 0, s, x, F, n, stride, window, rs, map, i0, m, scratch);       \
        else if (n <= 64 * 16) hipLaunchKernelGGL((burg_lags_resampled_kernel<16, PP, TIN>), grid, b, 0, s, x, F, n, stride, window, rs, map, i0, m, scratch); \
        else hipLaunchKernelGGL((burg_lags_resampled_kernel<20, PP, TIN>), grid, b, 0, s, x, F, n, stride, window, rs, map, i0, m, scratch);                   \
    }

#define VBX_BURG_RESAMPLED_INSTANTIATE(P)                                                                                     \
    VBX_BURG_RESAMPLED_DEFINE                                                                                                 \
    template void launch_burg_lags_resampled_p<P, double>(hipStream_t, const double *, long, int, long, const double *, resample_src_t, frame_map_t, long, long, double *);   \
    template void launch_burg_lags_resampled_p<P, int16_t>(hipStream_t, const int16_t *, long, int, long, const double *, resample_src_t, frame_map_t, long, long, double *);

}  // namespace vbx
