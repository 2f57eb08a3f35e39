// k_session_channels.hip -- the two kernels a multi-channel live session (vbx_session_push_channels) puts around the frame loop: what
// k_session.hip does for one channel, for every selected channel in ONE launch each.
// session_ingest_all_<fmt>: builds the push's input in the session's other carry buffer, n_sel planes out_ld elements apart.  Plane p
//   = the kept tail of the old plane p (keep elements from `old`, planes old_ld apart) and behind it channel sel.ch[p] of the new
//   block, turned into the type the frame loop reads by the readers' own arithmetic (vbx_reader.hpp: correctly rounded PCM24 / PCM32
//   quotients, floats as bit patterns).  The interleaved block is read from memory ONCE whatever n_sel: from the first output group
//   that lies wholly in the new samples (element keep + lead, a multiple of G) on, blocks stage tiles of T whole sample frames in LDS
//   by 16-byte loads (dword loads for a source on a dword boundary only) and every lane gathers the 16 output bytes it owns in one
//   plane and stores them at once -- unpack_all_tiled_kernel's scheme (k_reader.hip), through the same lds_stage_tile / lds_one.
//   Everything else is the EDGE, done group by group with the same bits: the kept tail (one 16-byte load per lane where the old
//   plane's address allows it), the group where the tail meets the block, the ragged end behind the last whole tile -- and the whole
//   block where no tile can be used: a source off a dword boundary, sample frames too wide for 16 of them to fit a tile, a destination
//   off a 16-byte boundary.  A mono block of PCM16 / PCM32 / F32 / F64 on its load's boundary is read by read_group_wide there.
// session_deliver_all: ONE launch behind the frame loop and the batched stitch copies every channel's own rows out of the chunk-local
//   buffers (channel k's rows start at frame k * plane_frames + row0): records, the three status rows, lists, counts, peaks, and the
//   formant columns of the last own row into that channel's state.  blockIdx.y is the channel; the destinations are kernel arguments.
// The ingest kernel's text is in vbx_session_ingest_all.hpp (session_ingest_all_kernel: tiles by lds_stage_tile( ... ) and
// lds_one<FMT>, the edge by read_one<FMT> / read_group_wide<FMT>); this unit instantiates the formats of two bytes and more,
// k_sample8.hip the 8-bit ones.
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"
#include "vbx_reader.hpp"
#include "vbx_session_ingest_all.hpp"

namespace vbx {

namespace {

__global__ __launch_bounds__(256) void session_deliver_all_kernel(const session_deliver_all_t d) {
    const size_t k = blockIdx.y;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const size_t w = d.c1 - d.c0, r0 = k * d.plane_frames + d.row0;
    double *rec = d.ch[k].rec;
    for (size_t i = t0; i < d.rows * w; i += step) {
        const size_t r = i / w, c = d.c0 + i % w;
        rec[r * d.dst_ld + c] = d.src[(r0 + r) * d.src_ld + c];
    }
    if (int32_t *st = d.ch[k].st)
        for (size_t i = t0; i < 3 * d.rows; i += step) {
            const size_t q = i / d.rows, r = i % d.rows;
            st[q * d.dst_st_ld + r] = d.src_st[q * d.src_n + r0 + r];
        }
    if (double *cand = d.ch[k].cand)
        for (size_t i = t0; i < d.rows * 2 * d.kmax; i += step) cand[i] = d.src_cand[r0 * 2 * d.kmax + i];
    if (int32_t *count = d.ch[k].count)
        for (size_t i = t0; i < d.rows; i += step) count[i] = d.src_count[r0 + i];
    if (double *peak = d.ch[k].peak)
        for (size_t i = t0; i < d.rows; i += step) peak[i] = d.src_peak[r0 + i];
    if (d.state != nullptr)                                                    // the formant columns of the last own row
        for (size_t i = t0; i < d.n_state; i += step) d.state[k * 2 * VBX_FORMANT_SLOTS_K + i] = d.src[(r0 + d.rows - 1) * d.src_ld + 2 + i];
}

}  // namespace

void launch_session_ingest_all(hipStream_t s, int format, const void *old, size_t old_ld, size_t drop, size_t keep, const void *raw,
                               size_t n_new, size_t channels, const unpack_sel_t &sel, size_t n_sel, void *out, size_t out_ld) {
    if (keep + n_new == 0 || n_sel == 0) return;
    switch (format) {
        case UNPACK_PCM16: launch_ingest_all_as<UNPACK_PCM16>(s, old, old_ld, drop, keep, raw, n_new, channels, sel, n_sel, out, out_ld); break;
        case UNPACK_PCM24: launch_ingest_all_as<UNPACK_PCM24>(s, old, old_ld, drop, keep, raw, n_new, channels, sel, n_sel, out, out_ld); break;
        case UNPACK_PCM32: launch_ingest_all_as<UNPACK_PCM32>(s, old, old_ld, drop, keep, raw, n_new, channels, sel, n_sel, out, out_ld); break;
        case UNPACK_F32: launch_ingest_all_as<UNPACK_F32>(s, old, old_ld, drop, keep, raw, n_new, channels, sel, n_sel, out, out_ld); break;
        case UNPACK_F64: launch_ingest_all_as<UNPACK_F64>(s, old, old_ld, drop, keep, raw, n_new, channels, sel, n_sel, out, out_ld); break;
        default: launch_session_ingest_all8(s, format, old, old_ld, drop, keep, raw, n_new, channels, sel, n_sel, out, out_ld); break;      // k_sample8.hip
    }
}

void launch_session_deliver_all(hipStream_t s, const session_deliver_all_t &d, size_t n_sel) {
    size_t most = d.rows * (d.c1 - d.c0);
    if (d.src_cand != nullptr && d.rows * 2 * d.kmax > most) most = d.rows * 2 * d.kmax;
    size_t blocks = (most + 255) / 256;
    if (blocks > 256 * 4) blocks = 256 * 4;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(session_deliver_all_kernel, dim3((unsigned)blocks, (unsigned)n_sel), dim3(256), 0, s, d);
}

}  // namespace vbx
