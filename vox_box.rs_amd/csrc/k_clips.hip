// k_clips.hip -- the two kernels vbx_analyze_clips puts around a group's frame-loop call.
// clips_pack_<fmt>: ONE launch gathers the group's clips -- ragged rows in separate buffers, found through a device table of
//   (pointer, length, plane offset) -- into one plane of the type the frame loop reads natively, by the readers' own arithmetic
//   (vbx_reader.hpp: correctly rounded PCM24 / PCM32 quotients, floats as bit patterns), and zero-fills the gap of fewer than one hop
//   behind each clip.  HBM-bound streaming: the plane is cut into tiles of 256 * PACK_U lane groups of 16 output bytes; a block finds
//   its tile's first and last clip by a binary search of the table (block-uniform), every lane its own group's clip by a search
//   between those two -- no lane walks the table.  A group that lies wholly inside one clip's samples takes one wide load where the
//   source address allows it (16 bytes, 8 for PCM32; four dwords for a plain copy on a dword boundary); every other group -- a
//   clip's ragged head or tail, the gap, a source off its load's boundary, packed 24-bit samples -- goes element by element through
//   read_one, with the same bits.  Stores are 16 bytes wherever the plane's base allows it.  No sample past a clip's length is read.
// clips_deliver: ONE launch copies each clip's own rows out of the group's staging -- records, the three status rows, lists, counts,
//   peaks -- to the caller's rows; the work is indexed by DESTINATION row (the group's rows are contiguous there), and a lane finds its
//   row's clip by a binary search of the same table.  The rows between clips have no destination row: they are never delivered.
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"
#include "vbx_reader.hpp"

namespace vbx {

namespace {

#define PACK_U 4

// the last entry of tab[lo, hi] whose off is <= e (tab[lo].off <= e)
__device__ __forceinline__ unsigned clip_of_element(const clip_entry_t *__restrict__ tab, unsigned lo, unsigned hi, uint64_t e) {
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo + 1) / 2;
        if (tab[mid].off <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the same by destination row (row_start ascends strictly: every entry has rows)
__device__ __forceinline__ unsigned clip_of_row(const clip_entry_t *__restrict__ tab, unsigned n, int64_t row) {
    unsigned lo = 0, hi = n - 1;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo + 1) / 2;
        if (tab[mid].row_start <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <int FMT>
__global__ __launch_bounds__(256) void clips_pack_kernel(const clip_entry_t *__restrict__ tab, unsigned n, size_t total,
                                                         typename reader_t<FMT>::out_t *__restrict__ out, bool vec_out) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    static_assert(R::G * sizeof(out_t) == 16, "a lane owns 16 output bytes");
    constexpr size_t TILE = 256 * PACK_U;
    const size_t n_groups = (total + R::G - 1) / R::G, n_tiles = (n_groups + TILE - 1) / TILE;
    for (size_t k = blockIdx.x; k < n_tiles; k += gridDim.x) {
        const size_t g0 = k * TILE, g1 = g0 + TILE < n_groups ? g0 + TILE : n_groups;
        const size_t e_last = g1 * R::G < total ? g1 * R::G - 1 : total - 1;
        const unsigned c_lo = clip_of_element(tab, 0, n - 1, g0 * R::G), c_hi = clip_of_element(tab, c_lo, n - 1, e_last);
        for (size_t g = g0 + threadIdx.x; g < g1; g += 256) {
            const size_t e0 = g * R::G;
            unsigned c = clip_of_element(tab, c_lo, c_hi, e0);
            const unsigned char *src = static_cast<const unsigned char *>(tab[c].src);
            uint64_t len = tab[c].len, off = tab[c].off;
            const bool whole = e0 + R::G <= total;
            alignas(16) out_t v[R::G];
            bool done = false;
            if (whole && e0 - off + R::G <= len) {                              // wholly inside the clip's samples
                if constexpr (FMT != UNPACK_PCM24) {
                    const unsigned char *w = src + (e0 - off) * R::B;
                    const uintptr_t a = reinterpret_cast<uintptr_t>(w);
                    if ((a & (FMT == UNPACK_PCM32 ? 7 : 15)) == 0) { read_group_wide<FMT>(w, 0, v); done = true; }
                    else if (FMT != UNPACK_PCM32 && (a & 3) == 0) {
                        const uint32_t *w4 = reinterpret_cast<const uint32_t *>(w);
                        const uint4 q = make_uint4(w4[0], w4[1], w4[2], w4[3]);
                        __builtin_memcpy(v, &q, 16);
                        done = true;
                    }
                }
            }
            if (!done) {
#pragma unroll
                for (int j = 0; j < R::G; j++) {
                    const size_t e = e0 + j;
                    v[j] = out_t(0);
                    if (e < total) {
                        while (c + 1 < n && tab[c + 1].off <= e) {              // (a clip is at least one hop long: one step an element at most)
                            c++;
                            src = static_cast<const unsigned char *>(tab[c].src); len = tab[c].len; off = tab[c].off;
                        }
                        if (e - off < len) v[j] = read_one<FMT>(src, e - off);
                    }
                }
            }
            if (whole && vec_out) {
                uint4 q;
                __builtin_memcpy(&q, v, 16);
                *reinterpret_cast<uint4 *>(out + e0) = q;
            } else {
#pragma unroll
                for (int j = 0; j < R::G; j++) if (e0 + j < total) out[e0 + j] = v[j];
            }
        }
    }
}

__global__ __launch_bounds__(256) void clips_deliver_kernel(const clips_deliver_t d) {
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const unsigned n = (unsigned)d.n;
    // destination row row0 + r comes from staging row ...
    auto src_row = [&](size_t r) {
        const int64_t row = (int64_t)(d.row0 + r);
        const unsigned c = clip_of_row(d.tab, n, row);
        return (size_t)(d.tab[c].plane_frame + (row - d.tab[c].row_start));
    };
    // the records: 16-byte pairs of columns, and the last column alone where their count is odd
    const size_t w = d.c1 - d.c0, pairs = w / 2, per_row = pairs + (w & 1);
    for (size_t i = t0; i < d.rows * per_row; i += step) {
        const size_t r = i / per_row, q = i - r * per_row;
        const double *s = d.src + src_row(r) * d.src_ld + d.c0 + 2 * q;
        double *o = d.dst + (d.row0 + r) * d.dst_ld + d.c0 + 2 * q;
        if (q < pairs) *reinterpret_cast<double2 *>(o) = *reinterpret_cast<const double2 *>(s);
        else *o = *s;
    }
    for (int q = 0; q < 3; q++)
        if (int32_t *st = d.dst_st[q])
            for (size_t r = t0; r < d.rows; r += step) st[d.row0 + r] = d.src_st[q * d.src_n + src_row(r)];
    if (d.dst_cand != nullptr) {
        const size_t w2 = 2 * d.kmax;
        for (size_t i = t0; i < d.rows * w2; i += step) {
            const size_t r = i / w2, q = i - r * w2;
            d.dst_cand[(d.row0 + r) * w2 + q] = d.src_cand[src_row(r) * w2 + q];
        }
    }
    if (d.dst_count != nullptr)
        for (size_t r = t0; r < d.rows; r += step) d.dst_count[d.row0 + r] = d.src_count[src_row(r)];
    if (d.dst_peak != nullptr)
        for (size_t r = t0; r < d.rows; r += step) d.dst_peak[d.row0 + r] = d.src_peak[src_row(r)];
}

template <int FMT>
void launch_pack_as(hipStream_t s, const clip_entry_t *tab, size_t n, size_t total, void *plane) {
    using R = reader_t<FMT>;
    const size_t n_groups = (total + R::G - 1) / R::G;
    size_t blocks = (n_groups + 256 * PACK_U - 1) / (256 * PACK_U);
    if (blocks > 256 * 32) blocks = 256 * 32;
    const bool vec_out = ((uintptr_t)plane & 15) == 0;
    hipLaunchKernelGGL(clips_pack_kernel<FMT>, dim3((unsigned)blocks), dim3(256), 0, s, tab, (unsigned)n, total,
                       static_cast<typename R::out_t *>(plane), vec_out);
}

}  // namespace

void launch_clips_pack(hipStream_t s, int format, const clip_entry_t *tab, size_t n, size_t total, void *plane) {
    if (n == 0 || total == 0) return;
    switch (format) {
        case UNPACK_PCM16: launch_pack_as<UNPACK_PCM16>(s, tab, n, total, plane); break;
        case UNPACK_PCM24: launch_pack_as<UNPACK_PCM24>(s, tab, n, total, plane); break;
        case UNPACK_PCM32: launch_pack_as<UNPACK_PCM32>(s, tab, n, total, plane); break;
        case UNPACK_F32: launch_pack_as<UNPACK_F32>(s, tab, n, total, plane); break;
        case UNPACK_F64: launch_pack_as<UNPACK_F64>(s, tab, n, total, plane); break;
    }
}

void launch_clips_deliver(hipStream_t s, const clips_deliver_t &d) {
    if (d.n == 0 || d.rows == 0) return;
    const size_t w = d.c1 - d.c0;
    size_t most = d.rows * (w / 2 + (w & 1));
    if (d.dst_cand != nullptr && d.rows * 2 * d.kmax > most) most = d.rows * 2 * d.kmax;
    if (d.rows > most) most = d.rows;
    size_t blocks = (most + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(clips_deliver_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d);
}

}  // namespace vbx
