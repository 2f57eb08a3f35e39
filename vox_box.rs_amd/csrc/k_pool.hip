// k_pool.hip -- the two kernels a session pool's tick (vbx_pool_push) puts around its one frame-loop call.
// pool_ingest_<fmt>: ONE launch builds, through the tick's device table (pool_entry_t: one entry per pushed block), everything the
//   tick's streams need, whatever their number:
//   - the plane the frame loop runs over: every entry with frames has a region, the samples of ITS stream from read_from on -- the
//     slot's carried tail where they precede the block, the block behind it -- as the type the frame loop reads natively, by the
//     readers' own arithmetic (vbx_reader.hpp: correctly rounded PCM24 / PCM32 / U8 quotients, floats as bit patterns, G.711 decoded
//     to int16; the tail is carried DECODED and copied as bit patterns), and the gap of fewer than one hop behind a region is zeros;
//   - every entry's new carried tail, into the slot's OTHER carry region: no launch reads and writes one region.
//   Latency-bound streaming, clips_pack's structure: the two outputs -- the plane's elements, then the tails' 16-byte groups entry
//   after entry -- are cut into tiles of 256 * POOL_U lane groups of 16 output bytes; a block finds its tile's first and last entry
//   by a binary search of the table (block-uniform), every lane its own group's entry by a search between those two -- no lane walks
//   the table.  A group that lies wholly in one source takes one wide load where that source's address allows it (16 bytes, 8 for
//   PCM32 and G.711, 2 for U8; four dwords for a plain copy on a dword boundary; 16 bytes of the tail); every other group -- the seam
//   between tail and block, a ragged end, the gap, a source off its load's boundary, packed 24-bit samples -- goes element by
//   element through read_one, with the same bits.  Stores are 16 bytes wherever the destination allows it.  Nothing before a tail's
//   first element, past its kept range or past a block's length is read.
// pool_deliver: ONE launch copies each entry's own rows out of the call's staging -- records, the three status rows, lists, counts,
//   peaks -- to the caller's rows (clips_deliver's scheme: the work is indexed by DESTINATION row, and a lane finds its row's entry by
//   a binary search of the same table), and the formant columns of every delivering entry's last row into its slot's state row.  The
//   rows between regions and the warm-up rows have no destination row: they are never delivered.
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"
#include "vbx_reader.hpp"

namespace vbx {

namespace {

#define POOL_U 4

// the last entry of tab[lo, hi] whose off is <= e (tab[lo].off <= e; an entry without frames carries the next region's off, so it
// never is the last of its ties unless no region follows -- and then its off is past the plane)
__device__ __forceinline__ unsigned pool_entry_of_element(const pool_entry_t *__restrict__ tab, unsigned lo, unsigned hi, uint64_t e) {
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo + 1) / 2;
        if (tab[mid].off <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// the same by group of the carry space (an entry with an empty tail has no group: it is never the last of its ties)
__device__ __forceinline__ unsigned pool_entry_of_group(const pool_entry_t *__restrict__ tab, unsigned lo, unsigned hi, uint64_t g) {
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo + 1) / 2;
        if (tab[mid].carry_g0 <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// by destination row (an entry without rows carries the next entry's row_start)
__device__ __forceinline__ unsigned pool_entry_of_row(const pool_entry_t *__restrict__ tab, unsigned n, int64_t row) {
    unsigned lo = 0, hi = n - 1;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo + 1) / 2;
        if (tab[mid].row_start <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// a stream's sources as a lane holds them: position p < 0 is element old_len + p of the tail, p >= 0 sample p of the block
struct pool_src_t { const unsigned char *src; const void *old; uint64_t n_new, old_len; };
__device__ __forceinline__ pool_src_t pool_src_of(const pool_entry_t &e) {
    return pool_src_t{static_cast<const unsigned char *>(e.src), e.old, e.n_new, e.old_len};
}

template <int FMT>
__device__ __forceinline__ typename reader_t<FMT>::out_t pool_one(const pool_src_t &s, int64_t p) {
    using out_t = typename reader_t<FMT>::out_t;
    if (p < 0) return (uint64_t)(-p) <= s.old_len ? static_cast<const out_t *>(s.old)[(int64_t)s.old_len + p] : out_t(0);
    return (uint64_t)p < s.n_new ? read_one<FMT>(s.src, (size_t)p) : out_t(0);
}

// G elements from position p on that lie wholly in the block or wholly in the tail, by one load where the address allows it
template <int FMT>
__device__ __forceinline__ bool pool_group_wide(const pool_src_t &s, int64_t p, typename reader_t<FMT>::out_t *v) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    if (p >= 0) {
        if ((uint64_t)p + R::G > s.n_new) return false;
        if constexpr (FMT != UNPACK_PCM24) {
            const unsigned char *w = s.src + (size_t)p * R::B;
            const uintptr_t a = reinterpret_cast<uintptr_t>(w);
            if ((a & (R::W - 1)) == 0) { read_group_wide<FMT>(w, 0, v); return true; }
            if (R::W == 16 && (a & 3) == 0) {                               // (the plain copies)
                const uint32_t *w4 = reinterpret_cast<const uint32_t *>(w);
                const uint4 q = make_uint4(w4[0], w4[1], w4[2], w4[3]);
                __builtin_memcpy(v, &q, 16);
                return true;
            }
        }
        return false;
    }
    if (p + R::G > 0 || (uint64_t)(-p) > s.old_len) return false;
    const out_t *o = static_cast<const out_t *>(s.old) + ((int64_t)s.old_len + p);
    if ((reinterpret_cast<uintptr_t>(o) & 15) != 0) return false;
    const uint4 q = *reinterpret_cast<const uint4 *>(o);
    __builtin_memcpy(v, &q, 16);
    return true;
}

template <int FMT>
__device__ __forceinline__ void pool_store_group(typename reader_t<FMT>::out_t *dst, const typename reader_t<FMT>::out_t *v, size_t valid) {
    using R = reader_t<FMT>;
    if (valid >= (size_t)R::G && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        uint4 q;
        __builtin_memcpy(&q, v, 16);
        *reinterpret_cast<uint4 *>(dst) = q;
    } else {
#pragma unroll
        for (int j = 0; j < R::G; j++) if ((size_t)j < valid) dst[j] = v[j];
    }
}

template <int FMT>
__global__ __launch_bounds__(256) void pool_ingest_kernel(const pool_entry_t *__restrict__ tab, unsigned n, size_t total,
                                                          typename reader_t<FMT>::out_t *__restrict__ plane, size_t carry_groups) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    static_assert(R::G * sizeof(out_t) == 16, "a lane owns 16 output bytes");
    constexpr size_t TILE = 256 * POOL_U;
    const size_t plane_groups = (total + R::G - 1) / R::G;
    const size_t plane_tiles = (plane_groups + TILE - 1) / TILE, carry_tiles = (carry_groups + TILE - 1) / TILE;
    for (size_t k = blockIdx.x; k < plane_tiles + carry_tiles; k += gridDim.x) {
        if (k < plane_tiles) {                                                  // ---- the plane
            const size_t g0 = k * TILE, g1 = g0 + TILE < plane_groups ? g0 + TILE : plane_groups;
            const size_t e_last = g1 * R::G < total ? g1 * R::G - 1 : total - 1;
            const unsigned c_lo = pool_entry_of_element(tab, 0, n - 1, g0 * R::G), c_hi = pool_entry_of_element(tab, c_lo, n - 1, e_last);
            for (size_t g = g0 + threadIdx.x; g < g1; g += 256) {
                const size_t e0 = g * R::G;
                unsigned c = pool_entry_of_element(tab, c_lo, c_hi, e0);
                pool_src_t s = pool_src_of(tab[c]);
                uint64_t off = tab[c].off, span = tab[c].span;
                int64_t first = tab[c].first;
                const size_t valid = e0 + R::G <= total ? (size_t)R::G : total - e0;
                alignas(16) out_t v[R::G];
                bool done = false;
                if (valid == (size_t)R::G && e0 - off + R::G <= span)           // wholly inside the entry's region
                    done = pool_group_wide<FMT>(s, first + (int64_t)(e0 - off), v);
                if (!done) {
#pragma unroll
                    for (int j = 0; j < R::G; j++) {
                        const size_t e = e0 + j;
                        v[j] = out_t(0);
                        if (e < total) {
                            while (c + 1 < n && tab[c + 1].off <= e) {          // (a region is at least one element long)
                                c++;
                                s = pool_src_of(tab[c]); off = tab[c].off; span = tab[c].span; first = tab[c].first;
                            }
                            if (e - off < span) v[j] = pool_one<FMT>(s, first + (int64_t)(e - off));
                        }
                    }
                }
                pool_store_group<FMT>(plane + e0, v, valid);
            }
        } else {                                                                // ---- the new tails
            const size_t g0 = (k - plane_tiles) * TILE, g1 = g0 + TILE < carry_groups ? g0 + TILE : carry_groups;
            const unsigned c_lo = pool_entry_of_group(tab, 0, n - 1, g0), c_hi = pool_entry_of_group(tab, c_lo, n - 1, g1 - 1);
            for (size_t g = g0 + threadIdx.x; g < g1; g += 256) {
                const unsigned c = pool_entry_of_group(tab, c_lo, c_hi, g);
                const pool_src_t s = pool_src_of(tab[c]);
                const uint64_t j0 = (g - tab[c].carry_g0) * R::G, len = tab[c].carry_len;
                if (j0 >= len) continue;
                const int64_t p0 = tab[c].carry_first + (int64_t)j0;
                const size_t valid = j0 + R::G <= len ? (size_t)R::G : (size_t)(len - j0);
                alignas(16) out_t v[R::G];
                bool done = false;
                if (valid == (size_t)R::G) done = pool_group_wide<FMT>(s, p0, v);
                if (!done) {
#pragma unroll
                    for (int j = 0; j < R::G; j++) v[j] = (size_t)j < valid ? pool_one<FMT>(s, p0 + j) : out_t(0);
                }
                pool_store_group<FMT>(static_cast<out_t *>(tab[c].carry) + j0, v, valid);
            }
        }
    }
}

__global__ __launch_bounds__(256) void pool_deliver_kernel(const pool_deliver_t d) {
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const unsigned n = (unsigned)d.n;
    // destination row r comes from staging row ...
    auto src_row = [&](size_t r) {
        const unsigned c = pool_entry_of_row(d.tab, n, (int64_t)r);
        return (size_t)(d.tab[c].plane_frame + d.tab[c].warm + ((int64_t)r - d.tab[c].row_start));
    };
    // the records: 16-byte pairs of columns, and the last column alone where their count is odd
    const size_t w = d.c1 - d.c0, pairs = w / 2, per_row = pairs + (w & 1);
    for (size_t i = t0; i < d.rows * per_row; i += step) {
        const size_t r = i / per_row, q = i - r * per_row;
        const double *s = d.src + src_row(r) * d.src_ld + d.c0 + 2 * q;
        double *o = d.dst + r * d.dst_ld + d.c0 + 2 * q;
        if (q < pairs) *reinterpret_cast<double2 *>(o) = *reinterpret_cast<const double2 *>(s);
        else *o = *s;
    }
    for (int q = 0; q < 3; q++)
        if (int32_t *st = d.dst_st[q])
            for (size_t r = t0; r < d.rows; r += step) st[r] = d.src_st[q * d.src_n + src_row(r)];
    if (d.dst_cand != nullptr) {
        const size_t w2 = 2 * d.kmax;
        for (size_t i = t0; i < d.rows * w2; i += step) {
            const size_t r = i / w2, q = i - r * w2;
            d.dst_cand[r * w2 + q] = d.src_cand[src_row(r) * w2 + q];
        }
    }
    if (d.dst_count != nullptr)
        for (size_t r = t0; r < d.rows; r += step) d.dst_count[r] = d.src_count[src_row(r)];
    if (d.dst_peak != nullptr)
        for (size_t r = t0; r < d.rows; r += step) d.dst_peak[r] = d.src_peak[src_row(r)];
    if (d.state != nullptr)                                                    // the formant columns of every delivering entry's last row
        for (size_t i = t0; i < d.n * d.n_state; i += step) {
            const size_t c = i / d.n_state, q = i - c * d.n_state;
            const pool_entry_t &e = d.tab[c];
            if (e.n_rows > 0) d.state[(size_t)e.slot * 2 * VBX_FORMANT_SLOTS_K + q] = d.src[(size_t)(e.plane_frame + e.frames - 1) * d.src_ld + 2 + q];
        }
}

template <int FMT>
void launch_pool_ingest_as(hipStream_t s, const pool_entry_t *tab, size_t n, size_t total, void *plane, size_t carry_groups) {
    using R = reader_t<FMT>;
    constexpr size_t TILE = 256 * POOL_U;
    const size_t plane_groups = (total + R::G - 1) / R::G;
    size_t blocks = (plane_groups + TILE - 1) / TILE + (carry_groups + TILE - 1) / TILE;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(pool_ingest_kernel<FMT>, dim3((unsigned)blocks), dim3(256), 0, s, tab, (unsigned)n, total,
                       static_cast<typename R::out_t *>(plane), carry_groups);
}

}  // namespace

void launch_pool_ingest(hipStream_t s, int format, const pool_entry_t *tab, size_t n, size_t total, void *plane, size_t carry_groups) {
    if (n == 0 || (total == 0 && carry_groups == 0)) return;
    switch (format) {
        case UNPACK_PCM16: launch_pool_ingest_as<UNPACK_PCM16>(s, tab, n, total, plane, carry_groups); break;
        case UNPACK_PCM24: launch_pool_ingest_as<UNPACK_PCM24>(s, tab, n, total, plane, carry_groups); break;
        case UNPACK_PCM32: launch_pool_ingest_as<UNPACK_PCM32>(s, tab, n, total, plane, carry_groups); break;
        case UNPACK_F32: launch_pool_ingest_as<UNPACK_F32>(s, tab, n, total, plane, carry_groups); break;
        case UNPACK_F64: launch_pool_ingest_as<UNPACK_F64>(s, tab, n, total, plane, carry_groups); break;
        case UNPACK_U8: launch_pool_ingest_as<UNPACK_U8>(s, tab, n, total, plane, carry_groups); break;
        case UNPACK_ULAW: launch_pool_ingest_as<UNPACK_ULAW>(s, tab, n, total, plane, carry_groups); break;
        case UNPACK_ALAW: launch_pool_ingest_as<UNPACK_ALAW>(s, tab, n, total, plane, carry_groups); break;
    }
}

void launch_pool_deliver(hipStream_t s, const pool_deliver_t &d) {
    if (d.n == 0 || d.rows == 0) return;
    const size_t w = d.c1 - d.c0;
    size_t most = d.rows * (w / 2 + (w & 1));
    if (d.dst_cand != nullptr && d.rows * 2 * d.kmax > most) most = d.rows * 2 * d.kmax;
    if (d.rows > most) most = d.rows;
    if (d.state != nullptr && d.n * d.n_state > most) most = d.n * d.n_state;
    size_t blocks = (most + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(pool_deliver_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d);
}

}  // namespace vbx
