// k_pitch_path.hip -- the pitch path over the candidate lists of vbx_pitch_f64 (Boersma 1993 path cost; the "third pass"
// src/periodic.rs:394-395 describes and PitchExtractor, src/periodic.rs:320-354, takes the parameters of but never runs).
//
// The definition (include/voxbox_hip.h, DESIGN.md "Pitch path") is a Viterbi recursion over at most kmax + 1 <= 64 states per
// frame, normalised so that the leader of every frame is exactly 0.  All arithmetic is IEEE binary64 in the order written
// there, with no fused multiply-add.
//
// Parallel form (the same scheme as the formant tracker's chunked scan, k_tracker.hip):
//   peak    pp_chunk_peak_kernel / pp_seg_peak_kernel   P = max local_peak per segment (only when u_t uses it)
//   A       pp_spec_kernel    one lane GROUP of G = pow2 >= states lanes per chunk of C frames (64 / G groups per wavefront):
//                             warm up over the W frames before the chunk from a fresh start, scan the chunk, store psi [F][G]
//                             (uint8), the entry state D and the exit state D.  Lane s owns state s; the predecessor loop reads
//                             {D(p), log2 f_p} of the previous frame from LDS (one broadcast ds_read_b128 per p).
//   B       pp_check_kernel / pp_repair_kernel (rounds)  a chunk whose entry D is not bit for bit its predecessor's exit D is
//                             redone from that exit, in parallel.
//   S       pp_mask_kernel + pp_sweep_kernel   one group per segment walks the chunks in order and redoes what is still
//                             inconsistent: this pass alone makes psi the sequential scan's; the rounds leave it little to do.
//   back    pp_map_kernel     per chunk, every lane walks psi back through the NEXT chunk of the segment (staged in LDS):
//                             the map  state at this chunk's last frame <- state at the next chunk's last frame.
//           pp_compose_kernel a log-depth suffix composition of those maps (the last chunk of a segment holds the constant
//                             map to the segment's leader) gives every chunk's true end state.
//           pp_write_kernel   per chunk, the group walks back from that state and writes out_path / out_index.
//   shard   pp_enter_kernel / pp_open_map_kernel / pp_export_kernel / pp_select_kernel   the hand-off across a shard cut
//                             (vbx_pitch_path_shard_*): the kernels above run unchanged on a rank's frames, these connect them to
//                             the neighbouring ranks (at the end of the file).
//   online  pp_online_kernel  vbx_path_stream_push: one group scans the frames a push brings from the true carried state, keeps
//                             psi and the rows of the pending frames in a device ring, and commits every frame whose state is
//                             decided (behind the shard kernels).
#include "vbx_kernels.hpp"

#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)   // the definition's arithmetic, operation for operation: no multiply-add may be fused

#include "vbx_pitch_path_step.hpp"   // one frame of the recursion: pp_fetch / pp_decode / pp_step / pp_leader (shared with k_pitch_path_channels.hip)

namespace vbx {

// ---- frame peak: max |x| per frame, NaN samples ignored (one wavefront per frame, coalesced) --------------------------------
__global__ __launch_bounds__(256) void frame_peak_kernel(const double *__restrict__ x, long F, long n, long stride,
                                                         double *__restrict__ out) {
    const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= F) return;                                        // wavefront-uniform
    const double *row = x + f * stride;
    double m = __builtin_nan("");                              // fmax(NaN, v) = v: an all-NaN frame stays NaN (np.nanmax)
    for (long i = lane; i < n; i += 64) m = fmax(m, fabs(row[i]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
    if (lane == 0) out[f] = m;
}

void launch_frame_peak(hipStream_t s, const double *x, long F, long n, long stride, double *out) {
    hipLaunchKernelGGL(frame_peak_kernel, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, s, x, F, n, stride, out);
}

// ---- per-segment peak of local_peak: per chunk, then per segment over its chunks (exact: a max is order-free) -------------
__global__ __launch_bounds__(64) void pp_chunk_peak_kernel(const double *__restrict__ lp, const pp_chunk_t *__restrict__ ch, long nch,
                                                           double *__restrict__ cpk) {
    const long c = blockIdx.x;
    if (c >= nch) return;
    const pp_chunk_t k = ch[c];
    double m = __builtin_nan("");
    for (long t = k.f0 + threadIdx.x; t < k.f1; t += 64) m = fmax(m, lp[t]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
    if (threadIdx.x == 0) cpk[c] = m;
}

__global__ __launch_bounds__(64) void pp_seg_peak_kernel(const double *__restrict__ cpk, const int64_t *__restrict__ seg_chunk0, long nseg,
                                                         double *__restrict__ spk) {
    const long sg = blockIdx.x;
    if (sg >= nseg) return;
    double m = __builtin_nan("");
    for (long c = seg_chunk0[sg] + threadIdx.x; c < seg_chunk0[sg + 1]; c += 64) m = fmax(m, cpk[c]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
    if (threadIdx.x == 0) spk[sg] = m;
}

// chunk c redone from the entry state D_in (its previous frame exists: c is not the first chunk of its segment)
template <int G>
__device__ void pp_run(const pp_par_t &P, long c, double D, int s, int gbase, double2 (*lds)[64]) {
    const pp_chunk_t k = P.ch[c];
    pp_raw_t r, nx;
    pp_frame_t fr;
    pp_fetch(P, k.f0 - 1, s, r);
    pp_decode<G>(P, r, k.seg, s, gbase, fr);
    int buf = 0;
    lds[buf][gbase + s] = make_double2(D, fr.lf);
    int pn = fr.n;
    unsigned long long pv = fr.vmask;
    pp_fetch(P, k.f0, s, r);
    for (long t = k.f0; t < k.f1; t++) {
        if (t + 1 < k.f1) pp_fetch(P, t + 1, s, nx);
        pp_decode<G>(P, r, k.seg, s, gbase, fr);
        int arg;
        D = pp_step<G>(P, fr, false, &lds[buf][gbase], pn, pv, arg);
        P.psi[t * G + s] = (uint8_t)arg;
        buf ^= 1;
        lds[buf][gbase + s] = make_double2(D, fr.lf);
        pn = fr.n; pv = fr.vmask;
        r = nx;
    }
    P.exitd[c * G + s] = D;
    const int lead = pp_leader<G>(D, fr.active, gbase);
    if (k.last && s == 0) P.lead[k.seg] = lead;
    if (s == 0) atomicAdd(P.redone, 1ull);
}

// ---- A: speculative chunks ---------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(64) void pp_spec_kernel(const pp_par_t P, long W) {
    __shared__ double2 lds[2][64];
    const int s = threadIdx.x & (G - 1), gbase = threadIdx.x & ~(G - 1);
    const long c = (long)blockIdx.x * (64 / G) + (threadIdx.x / G);
    if (c >= P.nch) return;                                    // group-uniform
    const pp_chunk_t k = P.ch[c];
    const long w = (k.f0 - W > k.s0) ? k.f0 - W : k.s0;        // warm up from a fresh start W frames early
    const bool exact = (w == k.s0);                            // ... which is the true start when the segment begins there
    double D = -INFINITY;
    int pn = 0, buf = 0;
    unsigned long long pv = 0ull;
    pp_raw_t r, nx;
    pp_frame_t fr;
    fr.active = false;
    pp_fetch(P, w, s, r);
    for (long t = w; t < k.f1; t++) {
        if (t + 1 < k.f1) pp_fetch(P, t + 1, s, nx);
        if (t == k.f0) { P.entry[c * G + s] = D; if (s == 0) P.exact[c] = exact ? 1 : 0; }
        pp_decode<G>(P, r, k.seg, s, gbase, fr);
        int arg;
        D = pp_step<G>(P, fr, t == w, &lds[buf][gbase], pn, pv, arg);
        if (t >= k.f0) P.psi[t * G + s] = (uint8_t)arg;
        buf ^= 1;
        lds[buf][gbase + s] = make_double2(D, fr.lf);
        pn = fr.n; pv = fr.vmask;
        r = nx;
    }
    P.exitd[c * G + s] = D;
    const int lead = pp_leader<G>(D, fr.active, gbase);
    if (k.last && s == 0) P.lead[k.seg] = lead;
}

// ---- B: check / repair rounds ------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(64) void pp_check_kernel(const pp_par_t P) {
    const int s = threadIdx.x & (G - 1), gbase = threadIdx.x & ~(G - 1);
    const long c = (long)blockIdx.x * (64 / G) + (threadIdx.x / G);
    if (c >= P.nch) return;
    int redo = 0;
    if (!P.exact[c]) {                                         // not exact: not the first chunk of its segment
        const double want = P.exitd[(c - 1) * G + s];
        const bool diff = __double_as_longlong(want) != __double_as_longlong(P.entry[c * G + s]);
        if (((__ballot(diff) >> gbase) & pp_gmask<G>()) != 0ull) { redo = 1; P.want[c * G + s] = want; }
    }
    if (s == 0) P.redo[c] = redo;
}

template <int G>
__global__ __launch_bounds__(64) void pp_repair_kernel(const pp_par_t P) {
    __shared__ double2 lds[2][64];
    const int s = threadIdx.x & (G - 1), gbase = threadIdx.x & ~(G - 1);
    const long c = (long)blockIdx.x * (64 / G) + (threadIdx.x / G);
    if (c >= P.nch || !P.redo[c]) return;                      // group-uniform
    const double D = P.want[c * G + s];
    P.entry[c * G + s] = D;                                    // what the chunk's psi now follows from
    pp_run<G>(P, c, D, s, gbase, lds);
}

// the check's flags, 64 chunks to a word (the sweep skips 64 clean chunks per read)
__global__ __launch_bounds__(64) void pp_mask_kernel(const pp_par_t P) {
    const long c = (long)blockIdx.x * 64 + threadIdx.x;
    const unsigned long long m = __ballot(c < P.nch && P.redo[c] != 0);
    if (threadIdx.x == 0) P.mask[blockIdx.x] = m;
}

// ---- S: the guarantee.  One group (block of G lanes) per segment, chunk boundaries in order ---------------------------------
template <int G>
__global__ __launch_bounds__(64) void pp_sweep_kernel(const pp_par_t P, const int64_t *__restrict__ seg_chunk0) {
    __shared__ double2 lds[2][64];
    const int s = threadIdx.x;                                 // blockDim.x == G: gbase 0
    const long sg = blockIdx.x;
    const long k0 = seg_chunk0[sg], k1 = seg_chunk0[sg + 1];
    long c = k0 + 1;
    bool forced = false;                                       // the previous chunk was redone: its successor's flag is stale
    while (c < k1) {
        if (!forced) {                                         // next flagged chunk at or after c
            long wi = c >> 6;
            unsigned long long word = P.mask[wi] & (~0ull << (c & 63));
            while (word == 0ull) {
                wi++;
                if (wi * 64 >= k1) break;
                word = P.mask[wi];
            }
            if (word == 0ull) break;
            c = wi * 64 + __builtin_ctzll(word);
            if (c >= k1) break;
        }
        bool redo = false;
        if (!P.exact[c]) {
            const bool diff = __double_as_longlong(P.exitd[(c - 1) * G + s]) != __double_as_longlong(P.entry[c * G + s]);
            redo = ((__ballot(diff) >> 0) & pp_gmask<G>()) != 0ull;
        }
        if (redo) {
            const double D = P.exitd[(c - 1) * G + s];
            P.entry[c * G + s] = D;
            pp_run<G>(P, c, D, s, 0, lds);
        }
        forced = redo;
        c++;
    }
}

// ---- backtrack -----------------------------------------------------------------------------------------------------------------

// the group's lanes copy psi rows [t0, t1) into its tile (rows are G bytes: whole 32-bit words, G >= 4)
template <int G>
__device__ __forceinline__ void pp_stage(const pp_par_t &P, long t0, long t1, int s, uint32_t *tile) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(P.psi + t0 * G);
    const int nw = (int)(t1 - t0) * (G / 4);
    for (int i = s; i < nw; i += G) tile[i] = src[i];
    __builtin_amdgcn_wave_barrier();
}

// map[c][s] = the state at chunk c's last frame when the state at chunk c + 1's last frame is s; a segment's last chunk holds
// the constant map to the segment's leader
template <int G>
__global__ __launch_bounds__(64) void pp_map_kernel(const pp_par_t P, uint8_t *__restrict__ map) {
    __shared__ uint32_t tiles[64 * PP_TILE / 4];
    const int s = threadIdx.x & (G - 1), gbase = threadIdx.x & ~(G - 1);
    const long c = (long)blockIdx.x * (64 / G) + (threadIdx.x / G);
    if (c >= P.nch) return;
    const pp_chunk_t k = P.ch[c];
    if (k.last) { map[c * G + s] = (uint8_t)P.lead[k.seg]; return; }
    const pp_chunk_t n = P.ch[c + 1];
    uint32_t *tile = tiles + gbase * (PP_TILE / 4);
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    int cur = s;
    for (long t1 = n.f1; t1 > n.f0;) {
        const long t0 = (t1 - PP_TILE > n.f0) ? t1 - PP_TILE : n.f0;
        pp_stage<G>(P, t0, t1, s, tile);
        for (long t = t1 - 1; t >= t0; t--) cur = tb[(t - t0) * G + cur];
        __builtin_amdgcn_wave_barrier();
        t1 = t0;
    }
    map[c * G + s] = (uint8_t)cur;
}

// out[c] = in[c] o in[c + d]: after passes d = 1, 2, 4, .. >= the longest segment's chunk count every map is constant
template <int G>
__global__ __launch_bounds__(256) void pp_compose_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long nch, long d) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nch * G) return;
    const long c = i / G;
    out[i] = (c + d < nch) ? in[c * G + in[(c + d) * G + (i % G)]] : in[i];
}

// the true state at every frame of chunk c, walked back from its last frame's, and the outputs
// (out_path row t starts ld doubles after row t - 1: 2 for dense rows, record_ld for columns 0-1 of a frame record)
template <int G>
__global__ __launch_bounds__(64) void pp_write_kernel(const pp_par_t P, const uint8_t *__restrict__ map, pitch_t *__restrict__ out_path,
                                                      long ld, int32_t *__restrict__ out_index) {
    __shared__ uint32_t tiles[64 * PP_TILE / 4];
    __shared__ uint8_t paths[64 / G][PP_TILE];
    const int s = threadIdx.x & (G - 1), gbase = threadIdx.x & ~(G - 1);
    const long c = (long)blockIdx.x * (64 / G) + (threadIdx.x / G);
    if (c >= P.nch) return;
    const pp_chunk_t k = P.ch[c];
    uint32_t *tile = tiles + gbase * (PP_TILE / 4);
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    uint8_t *path = paths[threadIdx.x / G];
    int cur = map[c * G];                                      // constant map: the true state at frame k.f1 - 1
    for (long t1 = k.f1; t1 > k.f0;) {
        const long t0 = (t1 - PP_TILE > k.f0) ? t1 - PP_TILE : k.f0;
        pp_stage<G>(P, t0, t1, s, tile);
        for (long t = t1 - 1; t >= t0; t--) {                  // every lane of the group walks the same states
            if (s == 0) path[t - t0] = (uint8_t)cur;
            cur = tb[(t - t0) * G + cur];
        }
        __builtin_amdgcn_wave_barrier();
        for (long t = t0 + s; t < t1; t += G) {
            const int st = path[t - t0];
            const int status = (P.status != nullptr) ? P.status[t] : 0;
            int m = (status == 0) ? P.count[t] : 0;
            m = (m < 0) ? 0 : ((m > P.kmax) ? P.kmax : m);
            pitch_t o{0.0, 0.0};
            bool voiced = false;
            if (st < m) { o = P.cand[t * (long)P.kmax + st]; voiced = o.frequency > 0.0; }
            if (!voiced) { o.frequency = 0.0; o.strength = pp_unvoiced(P, P.use_u ? P.lpk[t] : 0.0, k.seg); }
            *reinterpret_cast<pitch_t *>(reinterpret_cast<double *>(out_path) + t * ld) = o;
            if (out_index != nullptr) out_index[t] = (st < m) ? st : -1;
        }
        __builtin_amdgcn_wave_barrier();
        t1 = t0;
    }
}

// ---- the shard hand-off (vbx_pitch_path_shard_*): a shard cut is a chunk boundary whose predecessor lives on another rank ------
// The kernels above run unchanged on a rank's local frames; these four connect them to the neighbours.

// enter: the chunk c0 that begins at local frame `first` against the TRUE state of frame first - 1 (64 doubles from the previous
// rank, -inf where inactive).  Where the scan's own entry state is not that state bit for bit the chunk is redone from it, and
// the repair is carried forward chunk by chunk (each redone chunk's exit against its successor's entry, whatever the exact flag
// says: the scan's "exact" start of this utterance was local frame 0, itself a guess) until an exit state meets the entry the
// next chunk already has, or the utterance ends at c1.  One group: the repair is sequential by nature.
template <int G>
__global__ __launch_bounds__(64) void pp_enter_kernel(const pp_par_t P, long c0, long c1, const double *__restrict__ state_in,
                                                      int32_t *__restrict__ changed) {
    __shared__ double2 lds[2][64];
    const int s = threadIdx.x;                                 // blockDim.x == G: gbase 0
    double D = state_in[s];
    int n = 0;
    for (long c = c0; c < c1; c++) {
        const bool diff = __double_as_longlong(D) != __double_as_longlong(P.entry[c * G + s]);
        if ((__ballot(diff) & pp_gmask<G>()) == 0ull) break;
        P.entry[c * G + s] = D;
        pp_run<G>(P, c, D, s, 0, lds);
        D = P.exitd[c * G + s];                                // this lane's own store
        n++;
    }
    if (s == 0 && changed != nullptr) *changed = n;
}

// the last chunk of an OPEN utterance (it continues on the next rank) ends in a state only that rank can name: the identity map
// in place of the constant leader map, so that the suffix composition yields every chunk's map FROM the utterance's end state
__global__ __launch_bounds__(64) void pp_open_map_kernel(uint8_t *__restrict__ map, long c, int G) {
    if ((int)threadIdx.x < G) map[c * G + threadIdx.x] = (uint8_t)threadIdx.x;
}

// the two arrays that leave the rank, in their fixed 64-entry form: the exit state D of the last local frame (padded with -inf)
// and the back map of the chunk that ends at frame first - 1 (padded with 0).  src: ns entries, map: G entries; NULL: all padding.
// (src may be the caller's state_in, which state_out may alias: no __restrict__ on the two, each lane reads before it writes)
__global__ __launch_bounds__(64) void pp_export_kernel(const double *src, int ns, const uint8_t *__restrict__ map, int G,
                                                       double *state_out, int32_t *__restrict__ back_map) {
    const int s = threadIdx.x;
    const double d = (src != nullptr && s < ns) ? src[s] : -INFINITY;
    if (state_out != nullptr) state_out[s] = d;
    if (back_map != nullptr) back_map[s] = (map != nullptr && s < G) ? (int32_t)map[s] : 0;
}

// finish: sel[c][0] = map[c][end state] for the chunks from c0 on -- the form pp_write_kernel reads (a constant map's entry 0).
// end_state: the state of the rank's last frame on the whole recording's path (device; NULL = 0: every map is constant then).
__global__ __launch_bounds__(256) void pp_select_kernel(const uint8_t *__restrict__ map, long c0, long nch, int G,
                                                        const int32_t *__restrict__ end_state, uint8_t *__restrict__ sel) {
    const long c = c0 + (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= nch) return;
    const int e = (end_state != nullptr) ? (*end_state & (G - 1)) : 0;     // never outside the row, whatever arrives
    sel[c * G] = map[c * G + e];
}

// ---- the online path (vbx_path_stream_*): the same recursion while the lists arrive ------------------------------------------
// One group (block of G lanes, gbase 0) scans the push's frames in order from the TRUE state the last push left in O.st: nothing is
// speculated, nothing repaired.  Per frame, lane s stores psi and what a commit of state s would write (the output row and index)
// into slot `frame % cap` of the ring, so the caller's lists are not needed behind the push.  Frame t is DECIDED once the psi traces
// from all states of the newest frame have met at or after t: every continuation passes through one of those states, so the merged
// prefix is the whole utterance's path.  Decisions are evaluated when the ring is full and at the end of the push, which commits
// the same rows as evaluating them after every frame (decided(T) only grows with T); a ring that is still full is relieved of its
// oldest ceil(cap / 2) frames along the leader's trace, flagged as forced.

template <int G>
__global__ __launch_bounds__(64) void pp_online_kernel(const pp_par_t P_, const pp_online_t O) {
    __shared__ double2 lds[2][64];
    __shared__ uint8_t path[PP_TILE];
    const int s = threadIdx.x;                                 // blockDim.x == G: gbase 0
    pp_online_state_t *S = O.st;
    __shared__ double peak;                                    // P = peak_ref: what pp_unvoiced reads as the peak of "segment" 0
    if (s == 0) peak = O.peak;
    __syncthreads();
    pp_par_t P = P_;
    P.spk = &peak;
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

// ---- launches ---------------------------------------------------------------------------------------------------------------
void launch_pitch_path_open_map(hipStream_t s, uint8_t *map, long c, int G) {
    hipLaunchKernelGGL(pp_open_map_kernel, dim3(1), dim3(64), 0, s, map, c, G);
}
void launch_pitch_path_export(hipStream_t s, const double *src, int ns, const uint8_t *map, int G, double *state_out, int32_t *back_map) {
    hipLaunchKernelGGL(pp_export_kernel, dim3(1), dim3(64), 0, s, src, ns, map, G, state_out, back_map);
}
void launch_pitch_path_select(hipStream_t s, const uint8_t *map, long c0, long nch, int G, const int32_t *end_state, uint8_t *sel) {
    hipLaunchKernelGGL(pp_select_kernel, dim3((unsigned)((nch - c0 + 255) / 256)), dim3(256), 0, s, map, c0, nch, G, end_state, sel);
}

void launch_pitch_path_peak(hipStream_t s, const pp_par_t &P, const int64_t *seg_chunk0, long nseg, double *cpk) {
    hipLaunchKernelGGL(pp_chunk_peak_kernel, dim3((unsigned)P.nch), dim3(64), 0, s, P.lpk, P.ch, P.nch, cpk);
    hipLaunchKernelGGL(pp_seg_peak_kernel, dim3((unsigned)nseg), dim3(64), 0, s, cpk, seg_chunk0, nseg, const_cast<double *>(P.spk));
}

#define VBX_PP_DISPATCH(G_, CALL)                    \
    switch (G_) {                                    \
        case 4: { constexpr int G = 4; CALL; } break;   \
        case 8: { constexpr int G = 8; CALL; } break;   \
        case 16: { constexpr int G = 16; CALL; } break; \
        case 32: { constexpr int G = 32; CALL; } break; \
        default: { constexpr int G = 64; CALL; } break; \
    }

static dim3 pp_group_grid(long nch, int G) { return dim3((unsigned)((nch + (64 / G) - 1) / (64 / G))); }

void launch_pitch_path_spec(hipStream_t s, const pp_par_t &P, int G_, long W) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_spec_kernel<G>, pp_group_grid(P.nch, G), dim3(64), 0, s, P, W));
}
void launch_pitch_path_check(hipStream_t s, const pp_par_t &P, int G_) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_check_kernel<G>, pp_group_grid(P.nch, G), dim3(64), 0, s, P));
}
void launch_pitch_path_repair(hipStream_t s, const pp_par_t &P, int G_) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_repair_kernel<G>, pp_group_grid(P.nch, G), dim3(64), 0, s, P));
}
void launch_pitch_path_mask(hipStream_t s, const pp_par_t &P) {
    hipLaunchKernelGGL(pp_mask_kernel, dim3((unsigned)((P.nch + 63) / 64)), dim3(64), 0, s, P);
}
void launch_pitch_path_sweep(hipStream_t s, const pp_par_t &P, int G_, const int64_t *seg_chunk0, long nseg) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_sweep_kernel<G>, dim3((unsigned)nseg), dim3(G), 0, s, P, seg_chunk0));
}
void launch_pitch_path_map(hipStream_t s, const pp_par_t &P, int G_, uint8_t *map) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_map_kernel<G>, pp_group_grid(P.nch, G), dim3(64), 0, s, P, map));
}
void launch_pitch_path_compose(hipStream_t s, long nch, int G_, const uint8_t *in, uint8_t *out, long d) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_compose_kernel<G>, dim3((unsigned)((nch * G + 255) / 256)), dim3(256), 0, s, in, out, nch, d));
}
void launch_pitch_path_write(hipStream_t s, const pp_par_t &P, int G_, const uint8_t *map, pitch_t *out_path, long ld, int32_t *out_index) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_write_kernel<G>, pp_group_grid(P.nch, G), dim3(64), 0, s, P, map, out_path, ld, out_index));
}
void launch_pitch_path_enter(hipStream_t s, const pp_par_t &P, int G_, long c0, long c1, const double *state_in, int32_t *changed) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_enter_kernel<G>, dim3(1), dim3(G), 0, s, P, c0, c1, state_in, changed));
}
void launch_pitch_path_online(hipStream_t s, const pp_par_t &P, int G_, const pp_online_t &O) {
    VBX_PP_DISPATCH(G_, hipLaunchKernelGGL(pp_online_kernel<G>, dim3(1), dim3(G), 0, s, P, O));
}
#undef VBX_PP_DISPATCH

}  // namespace vbx
