// k_pitch_path_channels.hip -- the online pitch path of EVERY channel of a bound multi-channel session in one launch
// (vbx_session_path_bind_channels): block k is one lane group that runs pp_online_kernel's scan (k_pitch_path.hip: the same
// pp_fetch / pp_decode / pp_step / pp_leader of vbx_pitch_path_step.hpp, the same decisions, commits and forced rows, statement for
// statement) on channel k's rows of the session-owned lists -- frames [k * plane_frames, k * plane_frames + F) of the one frame-loop
// call's arrays -- from channel k's own stream state and ring into channel k's own destinations.  The blocks share nothing.  A
// unit of its own: k_pitch_path.hip's kernels are held to their recorded registers line for line, and this one must not move them.
// The scan's body is a COPY of pp_online_kernel's, a recorded decision: tests/test_path_stream_bindings.py holds that kernel's body
// -- with its pp_fetch / pp_decode / pp_step / pp_leader calls -- to the text of k_pitch_path.hip and that unit's compile to exactly its
// recorded kernels, so the body can neither move into the shared header nor this kernel into that unit.  Only the prologue differs
// (the block's channel: its rows of the lists, its stream allocation, its destinations).  A change to the merge test, the forced rows
// or the ring is made in BOTH; tests/test_gpu_session_channels_path.py holds the two to equal rows, flags and commits push by push.
#include "vbx_kernels.hpp"

#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)   // the definition's arithmetic, operation for operation: no multiply-add may be fused

#include "vbx_pitch_path_step.hpp"

namespace vbx {

// P_: cand / count / status / lpk of CHANNEL 0's first frame, F frames per channel; O_: cap, end, peak and ld (the pointers come
// from A); A: the plane pitch, the ring's offsets inside a stream's allocation, and every channel's allocation and destinations
template <int G>
__global__ __launch_bounds__(64) void pp_online_all_kernel(const pp_par_t P_, const pp_online_t O_, const pp_online_all_t A) {
    __shared__ double2 lds[2][64];
    __shared__ uint8_t path[PP_TILE];
    const int s = threadIdx.x;                                 // blockDim.x == G: gbase 0
    // this block's channel: its rows of the shared lists, its own stream state and ring, its own destinations
    const pp_online_ch_t ch = A.ch[blockIdx.x];
    pp_online_t O = O_;
    {
        char *mem = static_cast<char *>(ch.mem);
        O.st = reinterpret_cast<pp_online_state_t *>(mem);
        O.row = reinterpret_cast<pitch_t *>(mem + A.off_row); O.psi = reinterpret_cast<uint8_t *>(mem + A.off_psi);
        O.idx = reinterpret_cast<int8_t *>(mem + A.off_idx);
        O.out_path = ch.out_path; O.out_index = ch.out_index; O.out_forced = ch.out_forced; O.commit = ch.commit;
    }
    pp_online_state_t *S = O.st;
    __shared__ double peak;                                    // P = peak_ref: what pp_unvoiced reads as the peak of "segment" 0
    if (s == 0) peak = O.peak;
    __syncthreads();
    pp_par_t P = P_;
    P.spk = &peak;
    if (P.F > 0) {                                             // (a mark: no frames, the lists are not read)
        const long r0 = (long)blockIdx.x * A.plane_frames;
        P.cand += r0 * (long)P.kmax; P.count += r0;
        if (P.status != nullptr) P.status += r0;
        if (P.lpk != nullptr) P.lpk += r0;
    }
    const int cap = (int)O.cap;
    double D = S->D[s], lf = S->lf[s];
    int pn = S->n, buf = 0;
    unsigned long long pv = S->vmask;
    int pend = (int)(S->scanned - S->committed), head = (int)(S->scanned % cap);
    bool fresh = S->utt == 0;                                  // (lane s has a state in the newest frame iff s < pn)
    int pend0 = pend;                                          // the frame at distance d is output row pend0 + t - 1 - d
    // what only the row stores use lives in vector registers: the scalar file is full (no spill), and these feed vector addresses
    double *out_path = reinterpret_cast<double *>(O.out_path);
    int32_t *out_index = O.out_index;
    uint8_t *out_forced = O.out_forced;
    long ld = O.ld;
    asm volatile("" : "+v"(pend0), "+v"(out_path), "+v"(out_index), "+v"(out_forced), "+v"(ld));
    long n_forced = 0;
    lds[buf][s] = make_double2(D, lf);
    pp_raw_t r, nx;
    pp_frame_t fr;
    if (P.F > 0) pp_fetch(P, 0, s, r);
    for (long t = 0;; t++) {
        const bool last = t == P.F;
        if ((last || pend == cap) && pend > 0) {
            // decisions: when the ring is full, and at the end of the push.  Pass 0 is the merge test: each lane walks its own state's
            // trace back from the newest frame until a ballot shows one state for all (lanes without a state walk with lane 0, whose
            // state always exists).  Pass 1 follows the leader's trace: to relieve a ring that is still full of its oldest
            // ceil(cap / 2) frames (flag 1), or to end the utterance (flag 0).  Either pass commits distances [d_hi, pend).
            __syncthreads();                                   // the ring stores of the frames scanned, before other lanes read them
            for (int pass = 0; pass < 2 && pend > 0; pass++) {
                int d_hi = -1, cur = (s < pn) ? s : 0, flag = 0;
                if (pass == 0) {
                    int sl = head;
                    for (int d = 0; d < pend; d++) {
                        sl = (sl == 0) ? cap - 1 : sl - 1;
                        const int ref = __shfl(cur, 0, G);
                        if ((__ballot(cur != ref) & pp_gmask<G>()) == 0ull) { d_hi = d; break; }
                        cur = O.psi[sl * G + cur] & (G - 1);
                    }
                    if (d_hi < 0) continue;
                } else {
                    const bool end = last && O.end != 0;
                    if (!end && (last || pend < cap)) break;
                    flag = end ? 0 : 1;
                    d_hi = end ? 0 : pend - (cap + 1) / 2;
                    cur = pp_leader<G>(D, s < pn, 0);
                    int sl = head;
                    for (int d = 0; d < d_hi; d++) {
                        sl = (sl == 0) ? cap - 1 : sl - 1;
                        cur = O.psi[sl * G + cur] & (G - 1);
                    }
                }
                // every lane holds the trace's state at distance d_hi: walk it back tile by tile (lane 0 stages the states in LDS),
                // then all lanes write the tile's rows
                for (int d0 = d_hi; d0 < pend; d0 += PP_TILE) {
                    const int d1 = (d0 + PP_TILE < pend) ? d0 + PP_TILE : pend;
                    int sl = pp_ring_slot(head, d0, cap);
                    for (int d = d0; d < d1; d++) {
                        if (s == 0) path[d - d0] = (uint8_t)cur;
                        cur = O.psi[sl * G + cur] & (G - 1);
                        sl = (sl == 0) ? cap - 1 : sl - 1;
                    }
                    __syncthreads();
                    for (int d = d0 + s; d < d1; d += G) {
                        const int at = pp_ring_slot(head, d, cap) * G + path[d - d0];
                        const long row = t + (pend0 - 1 - d);
                        const pitch_t o = O.row[at];
                        double *dst = out_path + row * ld;                     // (rows of any ld: two 8-byte stores)
                        dst[0] = o.frequency; dst[1] = o.strength;
                        if (out_index != nullptr) out_index[row] = (int32_t)O.idx[at];
                        if (out_forced != nullptr) out_forced[row] = (uint8_t)flag;
                    }
                    __syncthreads();                           // the tile, and the slots these rows came from, are free again
                }
                if (flag) n_forced += pend - d_hi;
                pend = d_hi;
            }
        }
        if (last) break;
        if (t + 1 < P.F) pp_fetch(P, t + 1, s, nx);
        pp_decode<G>(P, r, 0, s, 0, fr);
        int arg;
        D = pp_step<G>(P, fr, fresh, &lds[buf][0], pn, pv, arg);
        int m = (r.st == 0) ? r.cnt : 0;                       // the listed entries, as pp_decode counts them
        m = (m < 0) ? 0 : ((m > P.kmax) ? P.kmax : m);
        const int at = head * G + s;
        O.psi[at] = (uint8_t)arg;
        O.row[at] = fr.voiced ? r.e : pitch_t{0.0, fr.lam};    // the chosen list entry, or {0, u_t}
        O.idx[at] = (int8_t)((s < m) ? s : -1);
        buf ^= 1;
        lf = fr.lf;
        lds[buf][s] = make_double2(D, lf);
        pn = fr.n; pv = fr.vmask;
        head = (head + 1 == cap) ? 0 : head + 1;
        pend++; fresh = false;
        r = nx;
    }
    S->D[s] = D; S->lf[s] = lf;
    if (s == 0) {
        const long scanned = S->scanned + P.F, first = S->committed;
        S->n = pn; S->vmask = pv; S->scanned = scanned; S->committed = scanned - pend;
        S->utt = (fresh || O.end != 0) ? 0 : 1;
        *O.commit = pp_commit_t{first, P.F + (pend0 - pend), n_forced, (long)pend};
    }
}

#define VBX_PP_DISPATCH(G_, CALL)                    \
    switch (G_) {                                    \
        case 4: { constexpr int G = 4; CALL; } break;   \
        case 8: { constexpr int G = 8; CALL; } break;   \
        case 16: { constexpr int G = 16; CALL; } break; \
        case 32: { constexpr int G = 32; CALL; } break; \
        default: { constexpr int G = 64; CALL; } break; \
    }

void launch_pitch_path_online_all(hipStream_t s, const pp_par_t &P, int G_, const pp_online_t &O, const pp_online_all_t &A, int n_sel) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_online_all_kernel<G>, dim3((unsigned)n_sel), dim3(G), 0, s, P, O, A));
}
#undef VBX_PP_DISPATCH

}  // namespace vbx
