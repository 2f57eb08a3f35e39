// vbx_session_ingest_all.hpp -- session_ingest_all_<fmt>, the ingest kernel of a multi-channel live session, as a template over the
// sample format: k_session_channels.hip instantiates it for the five formats of two bytes and more, k_sample8.hip for the 8-bit ones
// (the description is in k_session_channels.hip).  Device code and its launcher, in the unit's own anonymous namespace: every unit
// that includes this gets its own instantiations.
#pragma once
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"
#include "vbx_reader.hpp"

namespace vbx {

namespace {


// old: plane 0 of the old carry at its first kept element; raw: the block's first interleaved sample frame; lead: new elements that
// complete the group the tail ends in; n_tiles tiles of T sample frames start at sample frame `lead` of the block (0: no tiles).
// vec_out: out is 16-byte aligned and out_ld a multiple of G (every lane's 16 output bytes are aligned in every plane).
template <int FMT>
__global__ __launch_bounds__(256) void session_ingest_all_kernel(const typename reader_t<FMT>::out_t *__restrict__ old, size_t old_ld, size_t keep,
                                                                 const unsigned char *__restrict__ raw, size_t n_new, unsigned channels,
                                                                 unpack_sel_t sel, unsigned n_sel, typename reader_t<FMT>::out_t *__restrict__ out,
                                                                 size_t out_ld, size_t lead, size_t n_tiles, unsigned T, bool vec_out) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    static_assert(R::G * sizeof(out_t) == 16, "a lane owns 16 output bytes");
    __shared__ __attribute__((aligned(16))) uint32_t tile[UNPACK_ALL_TILE_BYTES / 4 + 4];      // (+ the dword a last 24-bit sample's read touches)
    __shared__ int s_sel[UNPACK_MAX_SEL];
    const unsigned t = threadIdx.x;
    if (t < n_sel) s_sel[t] = sel.ch[t];
    __syncthreads();
    const unsigned fb = channels * R::B;
    const size_t total = keep + n_new;
    if (n_tiles != 0) {                                                         // (kernel-uniform; vec_out holds)
        const unsigned tile_bytes = T * fb, items = (T / R::G) * n_sel;
        const unsigned char *src = raw + lead * fb;
        const bool wide = (reinterpret_cast<uintptr_t>(src) & 15) == 0;         // tile_bytes is a multiple of 16: every tile starts alike
        const size_t e0 = keep + lead;                                          // a multiple of G
        for (size_t k = blockIdx.x; k < n_tiles; k += gridDim.x) {              // (block-uniform trip count: the barriers are safe)
            lds_stage_tile(tile, src + k * tile_bytes, tile_bytes, wide, t);
            __syncthreads();
            for (unsigned it = t; it < items; it += 256) {
                const unsigned gl = it / n_sel, p = it - gl * n_sel;            // lane group gl of plane p (the plane fastest: k_reader.hip)
                const unsigned b = (gl * R::G * channels + (unsigned)s_sel[p]) * R::B;
                alignas(16) out_t v[R::G];
#pragma unroll
                for (int j = 0; j < R::G; j++) v[j] = lds_one<FMT>(tile, b + j * fb);
                uint4 q;
                __builtin_memcpy(&q, v, 16);
                *reinterpret_cast<uint4 *>(out + p * out_ld + e0 + k * T + (size_t)gl * R::G) = q;
            }
            __syncthreads();
        }
    }
    // the edge: elements [0, a1) and [d0, total) of every plane, group by group (a1 and d0 are multiples of G where tiles ran)
    const size_t a1 = n_tiles != 0 ? keep + lead : total, d0 = n_tiles != 0 ? keep + lead + n_tiles * T : total;
    const size_t nA = (a1 + R::G - 1) / R::G, nE = nA + (total - d0 + R::G - 1) / R::G;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + t, step = (size_t)gridDim.x * blockDim.x;
    for (size_t it = t0; it < nE * n_sel; it += step) {
        const size_t p = it / nE, g = it - p * nE;
        const size_t i0 = g < nA ? g * R::G : d0 + (g - nA) * R::G;
        const out_t *po = old + p * old_ld;
        out_t *dst = out + p * out_ld + i0;
        const bool whole = i0 + R::G <= total;
        alignas(16) out_t v[R::G];
        bool done = false;
        if (i0 + R::G <= keep) {
            if ((reinterpret_cast<uintptr_t>(po + i0) & 15) == 0) { const uint4 q = *reinterpret_cast<const uint4 *>(po + i0); __builtin_memcpy(v, &q, 16); done = true; }
        } else if (i0 >= keep && whole && channels == 1) {
            if constexpr (FMT != UNPACK_PCM24) {
                const unsigned char *w = raw + (i0 - keep) * R::B;
                if ((reinterpret_cast<uintptr_t>(w) & (R::W - 1)) == 0) { read_group_wide<FMT>(w, 0, v); done = true; }
            }
        }
        if (!done) {
#pragma unroll
            for (int j = 0; j < R::G; j++) {
                const size_t i = i0 + j;
                if (i < total) v[j] = i < keep ? po[i] : read_one<FMT>(raw, (i - keep) * channels + (size_t)s_sel[p]);
                else v[j] = out_t(0);
            }
        }
        if (whole && vec_out) {
            uint4 q;
            __builtin_memcpy(&q, v, 16);
            *reinterpret_cast<uint4 *>(dst) = q;
        } else {
#pragma unroll
            for (int j = 0; j < R::G; j++) if (i0 + j < total) dst[j] = v[j];
        }
    }
}

template <int FMT>
void launch_ingest_all_as(hipStream_t s, const void *old, size_t old_ld, size_t drop, size_t keep, const void *raw, size_t n_new,
                          size_t channels, const unpack_sel_t &sel, size_t n_sel, void *out, size_t out_ld) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    const unsigned char *in = static_cast<const unsigned char *>(raw);
    // whole tiles through LDS where a tile holds at least 16 sample frames, the block's first whole group can be read by dwords and
    // every lane's 16 output bytes are aligned in every plane; the rest -- or everything -- group by group
    const size_t fb = channels * R::B, total = keep + n_new;
    const size_t T = fb <= UNPACK_ALL_TILE_BYTES / 16 ? (UNPACK_ALL_TILE_BYTES / fb) & ~(size_t)15 : 0;
    const bool vec_out = ((uintptr_t)out & 15) == 0 && out_ld % R::G == 0;
    const size_t lead = (R::G - keep % R::G) % R::G;
    const bool tiled = T != 0 && vec_out && n_new >= lead + T && ((uintptr_t)(in + lead * fb) & 3) == 0;
    const size_t n_tiles = tiled ? (n_new - lead) / T : 0;
    const size_t edge = tiled ? keep + lead + (n_new - lead - n_tiles * T) : total;
    size_t blocks = ((edge + R::G - 1) / R::G * n_sel + 255) / 256;
    const size_t tile_blocks = n_tiles < 256 * 8 ? n_tiles : 256 * 8;
    if (blocks < tile_blocks) blocks = tile_blocks;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(session_ingest_all_kernel<FMT>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const out_t *>(old) + drop, old_ld, keep,
                       in, n_new, (unsigned)channels, sel, (unsigned)n_sel, static_cast<out_t *>(out), out_ld, lead, n_tiles, (unsigned)T, vec_out);
}

}  // namespace

}  // namespace vbx
