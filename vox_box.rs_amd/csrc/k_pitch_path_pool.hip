// k_pitch_path_pool.hip -- the online pitch path of every visited slot of a bound session pool in one launch (vbx_pool_path_bind;
// DESIGN.md section 5m): block k is one lane group that reads row k of the tick's path table -- a slot, the first row and the count
// of the slot's frames in the pool-owned lists, the slot's deferred reset and mark -- and runs pp_online_kernel's scan
// (k_pitch_path.hip: the same pp_fetch / pp_decode / pp_step / pp_leader of vbx_pitch_path_step.hpp, the same decisions, commits and
// forced rows, statement for statement) from the slot's own stream state and ring into the slot's own area of the bound arrays.
// The blocks share nothing.  A unit of its own, for the reason k_pitch_path_channels.hip gives: k_pitch_path.hip's kernels are held
// to their text and their recorded registers, and neither the body can move into the shared header nor this kernel into that unit.
// The scan's body is therefore a COPY, a recorded decision: a change to the merge test, the forced rows or the ring is now made in
// ALL THREE -- pp_online_kernel (k_pitch_path.hip), pp_online_all_kernel (k_pitch_path_channels.hip) and the kernel below;
// tests/test_gpu_pool_path.py holds this one to a bound one-channel session's rows, flags and commits tick by tick.
// Only the prologue is new: the table row; the slot's state, ring and destinations from the slot index and the launch-wide bases;
// the reset (the state zeroed, as vbx_path_stream_reset's memset does); the end phase of a deferred mark (the decision pass with no
// frame and end = 1, what a push of 0 frames with end_utterance does); then the scan of the slot's new frames.  The phases run the
// one copy of the body in turn, each from the state the one before left in memory, as two launches would.
#include "vbx_kernels.hpp"

#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)   // the definition's arithmetic, operation for operation: no multiply-add may be fused

#include "vbx_pitch_path_step.hpp"

namespace vbx {

// P_: cand / count / status / lpk of row 0 of the tick's lists; O_: cap, peak and ld (the pointers come from A and the slot);
// A: the table, the slots' allocations and the bound arrays
template <int G>
__global__ __launch_bounds__(64) void pp_online_pool_kernel(const pp_par_t P_, const pp_online_t O_, const pp_online_pool_t A) {
    __shared__ double2 lds[2][64];
    __shared__ uint8_t path[PP_TILE];
    const int s = threadIdx.x;                                 // blockDim.x == G: gbase 0
    // this block's slot: its rows of the shared lists, its own stream state and ring, its own area of the destinations
    const pp_pool_row_t tr = A.tab[blockIdx.x];
    pp_online_t O = O_;
    {
        char *mem = A.mem + (size_t)tr.slot * A.slot_bytes;
        O.st = reinterpret_cast<pp_online_state_t *>(mem);
        O.row = reinterpret_cast<pitch_t *>(mem + A.off_row); O.psi = reinterpret_cast<uint8_t *>(mem + A.off_psi);
        O.idx = reinterpret_cast<int8_t *>(mem + A.off_idx);
    }
    pp_online_state_t *S = O.st;
    __shared__ double peak;                                    // P = peak_ref: what pp_unvoiced reads as the peak of "segment" 0
    if (s == 0) peak = O.peak;
    if (tr.flags & PP_POOL_RESET) {                            // before anything else: the state a freshly opened stream has
        for (int i = s; i < 64; i += G) { S->D[i] = 0.0; S->lf[i] = 0.0; }
        if (s == 0) { S->vmask = 0ull; S->n = 0; S->pad = 0; S->scanned = 0; S->committed = 0; S->utt = 0; }
    }
    __syncthreads();
    const int cap = (int)O.cap;
    // what only the row stores use lives in vector registers: the scalar file is full (no spill), and these feed vector addresses
    const long area = (long)tr.slot * A.slot_rows;
    double *out_path = reinterpret_cast<double *>(A.out_path) + area * O.ld;
    int32_t *out_index = (A.out_index != nullptr) ? A.out_index + area : nullptr;
    uint8_t *out_forced = (A.out_forced != nullptr) ? A.out_forced + area : nullptr;
    long ld = O.ld;
    // ... and so does what only the phases' seams use: the slot's state, and the merged commit of the launch's phases -- `first` of
    // the first, n and n_forced summed, `pending` of the last -- with where it goes
    pp_commit_t *commit = A.commit + tr.slot;
    long c_first = 0, c_n = 0, c_forced = 0, c_pending = 0;
    asm volatile("" : "+v"(out_path), "+v"(out_index), "+v"(out_forced), "+v"(ld), "+v"(S), "+v"(commit), "+v"(c_first), "+v"(c_n), "+v"(c_forced),
                 "+v"(c_pending));
    pp_par_t P = P_;
    P.spk = &peak;
    if (tr.frames > 0) {
        P.cand += tr.row0 * (long)P.kmax; P.count += tr.row0;
        if (P.status != nullptr) P.status += tr.row0;
        if (P.lpk != nullptr) P.lpk += tr.row0;
    }
    // (the per-frame constants of the unvoiced and octave terms feed vector arithmetic only)
    asm volatile("" : "+v"(P.vt), "+v"(P.q), "+v"(P.oc), "+v"(P.Lc));
    c_first = S->committed;
    for (int end = (tr.flags & PP_POOL_MARK) ? 1 : 0; end >= 0; end--) {
        P.F = end ? 0 : tr.frames;                             // the end phase of a mark: no frames, the lists are not read
        double D = S->D[s], lf = S->lf[s];
        int pn = S->n, buf = 0;
        unsigned long long pv = S->vmask;
        int pend = (int)(S->scanned - S->committed), head = (int)(S->scanned % cap);
        bool fresh = S->utt == 0;                              // (lane s has a state in the newest frame iff s < pn)
        int pend0 = pend;                                      // the frame at distance d is output row pend0 + t - 1 - d
        asm volatile("" : "+v"(pend0));
        long n_forced = 0;
        asm volatile("" : "+v"(n_forced));
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
                __syncthreads();                               // the ring stores of the frames scanned, before other lanes read them
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
                        const bool fin = last && end != 0;
                        if (!fin && (last || pend < cap)) break;
                        flag = fin ? 0 : 1;
                        d_hi = fin ? 0 : pend - (cap + 1) / 2;
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
                            double *dst = out_path + row * ld;                 // (rows of any ld: two 8-byte stores)
                            dst[0] = o.frequency; dst[1] = o.strength;
                            if (out_index != nullptr) out_index[row] = (int32_t)O.idx[at];
                            if (out_forced != nullptr) out_forced[row] = (uint8_t)flag;
                        }
                        __syncthreads();                       // the tile, and the slots these rows came from, are free again
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
            int m = (r.st == 0) ? r.cnt : 0;                   // the listed entries, as pp_decode counts them
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
        __syncthreads();                                       // every lane has read the state this phase started from
        S->D[s] = D; S->lf[s] = lf;
        const long n = P.F + (pend0 - pend);
        if (s == 0) {
            const long scanned = S->scanned + P.F;
            S->n = pn; S->vmask = pv; S->scanned = scanned; S->committed = scanned - pend;
            S->utt = (fresh || end != 0) ? 0 : 1;
            c_n += n; c_forced += n_forced; c_pending = (long)pend;
        }
        // the next phase's rows follow this one's in the slot's area; it starts from the state just stored
        out_path += n * ld;
        if (out_index != nullptr) out_index += n;
        if (out_forced != nullptr) out_forced += n;
        __syncthreads();
    }
    if (s == 0) *commit = pp_commit_t{c_first, c_n, c_forced, c_pending};
}

#define VBX_PP_DISPATCH(G_, CALL)                    \
    switch (G_) {                                    \
        case 4: { constexpr int G = 4; CALL; } break;   \
        case 8: { constexpr int G = 8; CALL; } break;   \
        case 16: { constexpr int G = 16; CALL; } break; \
        case 32: { constexpr int G = 32; CALL; } break; \
        default: { constexpr int G = 64; CALL; } break; \
    }

void launch_pitch_path_online_pool(hipStream_t s, const pp_par_t &P, int G_, const pp_online_t &O, const pp_online_pool_t &A, long n_rows) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_online_pool_kernel<G>, dim3((unsigned)n_rows), dim3(G), 0, s, P, O, A));
}
#undef VBX_PP_DISPATCH

}  // namespace vbx
