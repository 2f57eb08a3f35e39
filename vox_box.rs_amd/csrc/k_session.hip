// k_session.hip -- the two kernels a live session (vbx_session_push) puts around the frame loop.
// session_ingest_<fmt>: ONE launch builds a push's input in the session's other carry buffer: elements [0, keep) are the kept tail of
//   the old buffer (from element `drop`), behind them the selected channel of the new block, turned into the type the frame loop
//   reads by the readers' own arithmetic (vbx_reader.hpp: correctly rounded PCM24 / PCM32 / U8 quotients, floats as bit patterns,
//   G.711 decoded to int16 -- the kept tail is carried DECODED, in the plane's type, for every format).  The
//   two buffers ping-pong, so the move never overlaps itself.  As in k_reader.hip a lane owns 16 consecutive output bytes and stores
//   them at once (the carry's base is 256-byte aligned); a group that lies wholly in the kept tail or wholly in a mono block is loaded
//   by one load per lane where that source's address allows it, element by element otherwise -- the same bits either way.  The
//   kept tail is at most (VBX_SHARD_WARM_FRAMES + 1) hops and a frame, a few tens of thousands of samples: moving it is noise next
//   to a launch, and it keeps the carry contiguous with the new samples for every format, mono PCM16 / F32 / F64 included.
// session_deliver: ONE launch behind the frame loop and the stitch copies the push's own rows out of the session's chunk-local
//   buffers: the records (all columns, or from column 2 in the tracked form), the three status rows with the caller's leading
//   dimension, the tracked form's lists, counts and peaks, and the formant columns of the last own row into the session's state (the
//   next push stitches from there: the caller may reuse its record buffer at once).
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"
#include "vbx_reader.hpp"

namespace vbx {

namespace {

// old: the old carry at its first kept element; raw: the block's first interleaved sample frame
template <int FMT>
__global__ __launch_bounds__(256) void session_ingest_kernel(const typename reader_t<FMT>::out_t *__restrict__ old, size_t keep,
                                                             const unsigned char *__restrict__ raw, size_t n_new, size_t channels,
                                                             size_t channel, typename reader_t<FMT>::out_t *__restrict__ out) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    static_assert(R::G * sizeof(out_t) == 16, "a lane owns 16 output bytes");
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const size_t total = keep + n_new;
    // kernel-uniform: the destination's alignment, the kept tail's, and that of the block's element behind a whole group of kept
    // ones (group g of the new part starts at source element g * G - keep: every such address is aligned when one is)
    const bool vec_out = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const bool wide_old = (reinterpret_cast<uintptr_t>(old) & 15) == 0;
    const size_t lead = (R::G - keep % R::G) % R::G;                            // new elements that complete the group the tail ends in
    const bool wide_new = FMT != UNPACK_PCM24 && channels == 1 &&
                          ((reinterpret_cast<uintptr_t>(raw) + lead * R::B) & (R::W - 1)) == 0;
    auto one = [&](size_t i) -> out_t { return i < keep ? old[i] : read_one<FMT>(raw, (i - keep) * channels + channel); };
    const size_t ng = vec_out ? total / R::G : 0;
    for (size_t g = t0; g < ng; g += step) {
        const size_t i0 = g * R::G;
        alignas(16) out_t v[R::G];
        bool done = false;
        if (i0 + R::G <= keep) {
            if (wide_old) { const uint4 q = *reinterpret_cast<const uint4 *>(old + i0); __builtin_memcpy(v, &q, 16); done = true; }
        } else if (i0 >= keep) {
            if constexpr (FMT != UNPACK_PCM24) { if (wide_new) { read_group_wide<FMT>(raw + (i0 - keep) * R::B, 0, v); done = true; } }
        }
        if (!done) {
#pragma unroll
            for (int j = 0; j < R::G; j++) v[j] = one(i0 + j);
        }
        uint4 q;
        __builtin_memcpy(&q, v, 16);
        *reinterpret_cast<uint4 *>(out + i0) = q;
    }
    for (size_t i = ng * R::G + t0; i < total; i += step) out[i] = one(i);
}

__global__ __launch_bounds__(256) void session_deliver_kernel(const session_deliver_t d) {
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const size_t w = d.c1 - d.c0;
    for (size_t i = t0; i < d.rows * w; i += step) {
        const size_t r = i / w, c = d.c0 + i % w;
        d.dst[r * d.dst_ld + c] = d.src[(d.row0 + r) * d.src_ld + c];
    }
    if (d.dst_st != nullptr)
        for (size_t i = t0; i < 3 * d.rows; i += step) {
            const size_t k = i / d.rows, r = i % d.rows;
            d.dst_st[k * d.dst_st_ld + r] = d.src_st[k * d.src_n + d.row0 + r];
        }
    if (d.dst_cand != nullptr)
        for (size_t i = t0; i < d.rows * 2 * d.kmax; i += step) d.dst_cand[i] = d.src_cand[d.row0 * 2 * d.kmax + i];
    if (d.dst_count != nullptr)
        for (size_t i = t0; i < d.rows; i += step) d.dst_count[i] = d.src_count[d.row0 + i];
    if (d.dst_peak != nullptr)
        for (size_t i = t0; i < d.rows; i += step) d.dst_peak[i] = d.src_peak[d.row0 + i];
    if (d.state != nullptr)                                                    // the formant columns of the last own row
        for (size_t i = t0; i < d.n_state; i += step) d.state[i] = d.src[(d.row0 + d.rows - 1) * d.src_ld + 2 + i];
}

template <int FMT>
void launch_ingest_as(hipStream_t s, const void *old, size_t drop, size_t keep, const void *raw, size_t n_new, size_t channels,
                      size_t channel, void *out) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    size_t blocks = ((keep + n_new) / R::G + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(session_ingest_kernel<FMT>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const out_t *>(old) + drop, keep,
                       static_cast<const unsigned char *>(raw), n_new, channels, channel, static_cast<out_t *>(out));
}

}  // namespace

void launch_session_ingest(hipStream_t s, int format, const void *old, size_t drop, size_t keep, const void *raw, size_t n_new,
                           size_t channels, size_t channel, void *out) {
    if (keep + n_new == 0) return;
    switch (format) {
        case UNPACK_PCM16: launch_ingest_as<UNPACK_PCM16>(s, old, drop, keep, raw, n_new, channels, channel, out); break;
        case UNPACK_PCM24: launch_ingest_as<UNPACK_PCM24>(s, old, drop, keep, raw, n_new, channels, channel, out); break;
        case UNPACK_PCM32: launch_ingest_as<UNPACK_PCM32>(s, old, drop, keep, raw, n_new, channels, channel, out); break;
        case UNPACK_F32: launch_ingest_as<UNPACK_F32>(s, old, drop, keep, raw, n_new, channels, channel, out); break;
        case UNPACK_F64: launch_ingest_as<UNPACK_F64>(s, old, drop, keep, raw, n_new, channels, channel, out); break;
        case UNPACK_U8: launch_ingest_as<UNPACK_U8>(s, old, drop, keep, raw, n_new, channels, channel, out); break;
        case UNPACK_ULAW: launch_ingest_as<UNPACK_ULAW>(s, old, drop, keep, raw, n_new, channels, channel, out); break;
        case UNPACK_ALAW: launch_ingest_as<UNPACK_ALAW>(s, old, drop, keep, raw, n_new, channels, channel, out); break;
    }
}

void launch_session_deliver(hipStream_t s, const session_deliver_t &d) {
    size_t most = d.rows * (d.c1 - d.c0);
    if (d.dst_cand != nullptr && d.rows * 2 * d.kmax > most) most = d.rows * 2 * d.kmax;
    size_t blocks = (most + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(session_deliver_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d);
}

}  // namespace vbx
