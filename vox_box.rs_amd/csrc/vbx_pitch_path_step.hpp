// vbx_pitch_path_step.hpp -- one frame of the pitch path's recursion, as a lane group computes it: what k_pitch_path.hip's kernels
// (the chunked resident path, the shard hand-off, the online path) and k_pitch_path_channels.hip (the online path of every channel of
// a multi-channel session in one launch) share.  Device code only.  The definition's arithmetic, operation for operation: every unit
// that includes this file compiles it without fused multiply-adds.
#pragma once
#include "vbx_kernels.hpp"

#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)

namespace vbx {

constexpr int PP_TILE = 256;                                   // frames of psi per LDS tile: 256 G bytes per group, 16 KB per wavefront

// ---- one frame of the recursion ---------------------------------------------------------------------------------------------
struct pp_raw_t { int cnt, st; pitch_t e; double lp; };
struct pp_frame_t { double lam, lf; int n; bool voiced, active; unsigned long long vmask; };

template <int G> __device__ __forceinline__ unsigned long long pp_gmask() { return (G == 64) ? ~0ull : ((1ull << G) - 1ull); }

// the frame's raw inputs as lane s sees them: independent loads, requested one frame ahead of their use
__device__ __forceinline__ void pp_fetch(const pp_par_t &P, long t, int s, pp_raw_t &r) {
    r.st = (P.status != nullptr) ? P.status[t] : 0;
    r.cnt = P.count[t];
    r.e = (s < P.kmax) ? P.cand[t * (long)P.kmax + s] : pitch_t{0.0, 0.0};
    r.lp = (P.use_u) ? P.lpk[t] : 0.0;
}

// u_t = voicing_threshold + max(0, 2 - rho / q), rho = local_peak / P (0 when P == 0)
__device__ __forceinline__ double pp_unvoiced(const pp_par_t &P, double lp, int seg) {
    if (!P.use_u) return P.vt;
    const double pk = P.spk[seg];
    const double rho = (pk == 0.0) ? 0.0 : lp / pk;
    const double v = 2.0 - rho / P.q;
    return P.vt + ((v > 0.0) ? v : 0.0);
}

// states, voicedness, log2 f and lambda of lane s (group-uniform control flow: the ballots see the whole group)
template <int G>
__device__ __forceinline__ void pp_decode(const pp_par_t &P, const pp_raw_t &r, int seg, int s, int gbase, pp_frame_t &fr) {
    int m = (r.st == 0) ? r.cnt : 0;                           // a frame whose status is not OK has only the unvoiced state
    m = (m < 0) ? 0 : ((m > P.kmax) ? P.kmax : m);
    const bool listed = s < m;
    const unsigned long long zb = __ballot(listed && r.e.frequency == 0.0);
    const unsigned long long vb = __ballot(listed && r.e.frequency > 0.0);
    const bool has_zero = ((zb >> gbase) & pp_gmask<G>()) != 0ull;
    fr.n = m + (has_zero ? 0 : 1);                             // the appended unvoiced state sits at index m
    fr.vmask = (vb >> gbase) & pp_gmask<G>();
    fr.active = s < fr.n;
    fr.voiced = listed && r.e.frequency > 0.0;
    if (fr.voiced) {
        fr.lf = log2(r.e.frequency);
        fr.lam = r.e.strength - P.oc * (P.Lc - fr.lf);
    } else {
        fr.lf = 0.0;
        fr.lam = pp_unvoiced(P, r.lp, seg);
    }
}

// D_t of lane s from D_{t-1} (prev[p] = {D(p), log2 f_p}, pn states, voiced mask pv); arg = psi_t(s)
template <int G>
__device__ __forceinline__ double pp_step(const pp_par_t &P, const pp_frame_t &fr, bool first, const double2 *prev, int pn,
                                          unsigned long long pv, int &arg) {
    double e;
    arg = 0;
    if (first) {
        e = fr.lam;
    } else {
        double best = 0.0;
        for (int p = 0; p < pn; p++) {
            const double2 q = prev[p];                         // broadcast within the group
            const bool vp = ((pv >> p) & 1ull) != 0ull;
            double c;
            if (fr.voiced && vp) c = P.cj * fabs(q.y - fr.lf);
            else c = (fr.voiced != vp) ? P.cvu : 0.0;
            const double v = q.x - c;
            if (p == 0 || v > best) { best = v; arg = p; }     // strict >: ties go to the lower index
        }
        e = best + fr.lam;
    }
    if (!fr.active) { e = -INFINITY; arg = 0; }
    double m = e;
#pragma unroll
    for (int d = 1; d < G; d <<= 1) { const double o = __shfl_xor(m, d, G); m = (o > m) ? o : m; }
    m = __shfl(m, 0, G);                                       // one value for the whole group
    return fr.active ? e - m : -INFINITY;
}

// the first state with D == 0 (the leader)
template <int G>
__device__ __forceinline__ int pp_leader(double D, bool active, int gbase) {
    const unsigned long long z = (__ballot(active && D == 0.0) >> gbase) & pp_gmask<G>();
    return (z == 0ull) ? 0 : __builtin_ctzll(z);
}

// A pending frame is named by its distance d from the newest frame (0 = newest); `head` is the slot the next frame takes, so the
// frame at distance d lives in slot head - 1 - d (mod cap).  cap <= 2^24: cap * G fits an int.
__device__ __forceinline__ int pp_ring_slot(int head, int d, int cap) { const int v = head - 1 - d; return (v < 0) ? v + cap : v; }

}  // namespace vbx
