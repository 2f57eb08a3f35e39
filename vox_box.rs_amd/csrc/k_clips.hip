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
// The pack kernel's text is in vbx_clips_pack.hpp (clips_pack_kernel: read_one<FMT> / read_group_wide<FMT>, the readers' own
// arithmetic); this unit instantiates the formats of two bytes and more, k_sample8.hip the 8-bit ones.
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"
#include "vbx_reader.hpp"
#include "vbx_clips_pack.hpp"

namespace vbx {

namespace {

// the same by destination row (row_start ascends strictly: every entry has rows)
__device__ __forceinline__ unsigned clip_of_row(const clip_entry_t *__restrict__ tab, unsigned n, int64_t row) {
    unsigned lo = 0, hi = n - 1;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo + 1) / 2;
        if (tab[mid].row_start <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
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

}  // namespace

void launch_clips_pack(hipStream_t s, int format, const clip_entry_t *tab, size_t n, size_t total, void *plane) {
    if (n == 0 || total == 0) return;
    switch (format) {
        case UNPACK_PCM16: launch_pack_as<UNPACK_PCM16>(s, tab, n, total, plane); break;
        case UNPACK_PCM24: launch_pack_as<UNPACK_PCM24>(s, tab, n, total, plane); break;
        case UNPACK_PCM32: launch_pack_as<UNPACK_PCM32>(s, tab, n, total, plane); break;
        case UNPACK_F32: launch_pack_as<UNPACK_F32>(s, tab, n, total, plane); break;
        case UNPACK_F64: launch_pack_as<UNPACK_F64>(s, tab, n, total, plane); break;
        default: launch_clips_pack8(s, format, tab, n, total, plane); break;              // the 8-bit formats: k_sample8.hip
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
