// k_reader.hip -- what a WAV reader hands over, turned into the type the frame loop reads natively (vbx_unpack_samples, and the
// per-chunk step of vbx_analyze_host): ONE channel of interleaved sample frames,
//   16-bit PCM -> int16 (the PCM kernels' input), 24-bit packed / 32-bit PCM -> f64 = s / (i32::MAX >> (32 - bits)), correctly
//   rounded (tests/lib.rs:17-19), float / double -> as they are (copied as bit patterns: NaN payloads survive);
//   one byte per sample: G.711 mu-law / A-law -> int16 (the ITU expansion, integer arithmetic in registers: vbx_sample8.hpp),
//   unsigned 8-bit PCM -> f64 = (b - 128) / 127.  A lane's 16 output bytes are 8 source bytes of G.711 (one 8-byte load from a mono
//   source on an 8-byte boundary) or 2 of unsigned PCM (one 2-byte load); such a source may sit at any byte address.
// HBM-bound byte work: one pass, grid-stride over groups of consecutive OUTPUT elements, capped grid, size_t indices.  A lane
// owns 16 consecutive output bytes per step, so every wave instruction touches ONE contiguous span: with a 16-byte aligned
// destination a wave's store is 1 KiB, and a mono source of matching alignment arrives by one load per lane of the same shape
// (16 bytes; 8 for the two 32-bit samples of a lane).  Packed 24-bit samples are 6 bytes per lane, which no load instruction
// fetches: a mono source on a dword boundary is staged through LDS -- the block reads a tile's dwords as contiguous spans, each lane
// then picks its two samples out of LDS -- and every other 24-bit source is read byte by byte.  The quotients are IEEE divisions:
// div_exact_small (vbx_device.hpp) is proven for 16-bit numerators only, and the divide hides behind the memory traffic.
// unpack_all_*: every selected channel of the interleaved frames in one pass (vbx_unpack_channels, and the per-chunk step of
// vbx_analyze_host_channels): tiles of whole sample frames through LDS, see there.
// host_rows_kernel: a chunk's own record rows and its three status rows, copied from the chunk-local buffers into the caller's.
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"
#include "vbx_reader.hpp"

namespace vbx {

namespace {

template <int FMT>
__global__ __launch_bounds__(256) void unpack_kernel(const unsigned char *__restrict__ src, size_t n, size_t channels, size_t channel,
                                                     typename reader_t<FMT>::out_t *__restrict__ out) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const bool vec_out = (reinterpret_cast<uintptr_t>(out) & 15) == 0;                        // kernel-uniform
    const bool wide_in = FMT != UNPACK_PCM24 && channels == 1 && (reinterpret_cast<uintptr_t>(src) & (R::W - 1)) == 0;
    const size_t ng = vec_out ? n / R::G : 0;
    for (size_t g = t0; g < ng; g += step) {
        alignas(16) out_t v[R::G];
        bool done = false;
        if constexpr (FMT != UNPACK_PCM24) { if (wide_in) { read_group_wide<FMT>(src, g, v); done = true; } }
        if (!done) {
#pragma unroll
            for (int j = 0; j < R::G; j++) v[j] = read_one<FMT>(src, (g * R::G + j) * channels + channel);
        }
        static_assert(R::G * sizeof(out_t) == 16, "a lane owns 16 output bytes");
        uint4 q;
        __builtin_memcpy(&q, v, 16);
        *reinterpret_cast<uint4 *>(out + g * R::G) = q;
    }
    for (size_t i = ng * R::G + t0; i < n; i += step) out[i] = read_one<FMT>(src, i * channels + channel);
}

// Packed 24-bit PCM, mono, source on a dword boundary, destination 16-byte aligned: tiles of 512 samples = 384 dwords.  The block
// reads a tile's dwords into LDS by two loads whose wave instructions are contiguous spans, and lane t then owns samples 2t and
// 2t + 1 of the tile (bytes 6t .. 6t + 5 of LDS) and stores their 16 output bytes.  n_tiles whole tiles only: the
// caller runs the element kernel on the tail.
#define PCM24_TILE 512
__global__ __launch_bounds__(256) void unpack_pcm24_tiled_kernel(const uint32_t *__restrict__ src, size_t n_tiles, double *__restrict__ out) {
    __shared__ uint32_t tile[PCM24_TILE * 3 / 4];
    const unsigned t = threadIdx.x;
    for (size_t k = blockIdx.x; k < n_tiles; k += gridDim.x) {                // (block-uniform trip count: the barriers are safe)
        const uint32_t *w = src + k * (PCM24_TILE * 3 / 4);
        tile[t] = w[t];
        if (t < PCM24_TILE * 3 / 4 - 256) tile[256 + t] = w[256 + t];
        __syncthreads();
        auto half = [&](unsigned q) { return (tile[q >> 1] >> ((q & 1) * 16)) & 0xffffu; };     // 16-bit word q of the tile
        const uint32_t h0 = half(3 * t), h1 = half(3 * t + 1), h2 = half(3 * t + 2);
        const double2 v = make_double2(pcm24_value(sext24(h0 | ((h1 & 0xffu) << 16))), pcm24_value(sext24((h1 >> 8) | (h2 << 8))));
        reinterpret_cast<double2 *>(out)[k * (PCM24_TILE / 2) + t] = v;
        __syncthreads();
    }
}

// ---- every selected channel in one pass (vbx_unpack_channels) ----
// The tiled form of unpack_pcm24_tiled_kernel for any format and channel count: a block stages a tile of T WHOLE sample frames
// (T * channels * B bytes <= UNPACK_ALL_TILE_BYTES, T a multiple of 16, so a tile is whole 16-byte words and whole lane groups of
// every output type) in LDS by contiguous 16-byte loads -- dword loads where the source sits on a dword boundary only -- and a lane
// then owns 16 consecutive output bytes of ONE plane: it gathers its G elements from LDS (channels * B bytes apart) and stores them
// with one 16-byte store.  The interleaved frames are read from memory once, whatever the number of planes.
// LDS reads: the work items of a tile are numbered with the plane FASTEST, so neighbouring lanes read neighbouring samples of one
// sample frame (the same or adjacent dwords; identical addresses broadcast) and the next G sample frames follow n_sel lanes later.
// Lanes that all walked one plane would be G * channels * B bytes apart: 8 dwords for 16-bit stereo, an 8-way conflict in a
// 32-lane group.  Spread over the planes the 32 lanes touch at most 32 / n_sel such spans; with EVERY channel selected that is, for
// 16-bit words, 4-way at worst (channels 2, 4, 8) and 2-way for 3, 5, 6 -- at 128 B per two clocks conflict-free, a quarter of the
// LDS rate is still several times what HBM delivers per CU, so the tile is not padded (padding would break the 16-byte LDS stores
// of the staging loop).  A SUBSET leaves fewer planes to spread over: one channel of 16-bit stereo is the 8-way case above, one of
// eight puts all 32 lanes on one bank (32 dwords apart).  The bits are the same, and the measured rates do not show the difference: one
// channel of two or of eight runs at 0.62-0.66 of the HBM roof in every format.
// 8 KiB tiles: eight blocks per CU keep 64 KiB of loads in flight and use 8 x (8208 + 256) B = 66 of the 160 KiB of LDS.
// n_tiles whole tiles of T sample frames; src on a dword boundary at least, out 16-byte aligned, plane_ld a multiple of G
template <int FMT>
__global__ __launch_bounds__(256) void unpack_all_tiled_kernel(const unsigned char *__restrict__ src, size_t n_tiles, unsigned T, unsigned channels,
                                                               unpack_sel_t sel, unsigned n_sel,
                                                               typename reader_t<FMT>::out_t *__restrict__ out, size_t plane_ld) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    __shared__ __attribute__((aligned(16))) uint32_t tile[UNPACK_ALL_TILE_BYTES / 4 + 4];      // (+ the dword a last 24-bit sample's read touches)
    __shared__ int s_sel[UNPACK_MAX_SEL];
    const unsigned t = threadIdx.x;
    if (t < n_sel) s_sel[t] = sel.ch[t];                                        // (read behind the first barrier)
    const unsigned fb = channels * R::B, tile_bytes = T * fb, items = (T / R::G) * n_sel;
    const bool wide = (reinterpret_cast<uintptr_t>(src) & 15) == 0;             // kernel-uniform; tile_bytes is a multiple of 16
    for (size_t k = blockIdx.x; k < n_tiles; k += gridDim.x) {                  // (block-uniform trip count: the barriers are safe)
        const unsigned char *w = src + k * tile_bytes;
        lds_stage_tile(tile, w, tile_bytes, wide, t);
        __syncthreads();
        for (unsigned it = t; it < items; it += 256) {
            const unsigned gl = it / n_sel, p = it - gl * n_sel;                // lane group gl of plane p
            const unsigned b = (gl * R::G * channels + (unsigned)s_sel[p]) * R::B;
            alignas(16) out_t v[R::G];
#pragma unroll
            for (int j = 0; j < R::G; j++) v[j] = lds_one<FMT>(tile, b + j * fb);
            uint4 q;
            __builtin_memcpy(&q, v, 16);
            *reinterpret_cast<uint4 *>(out + p * plane_ld + k * T + (size_t)gl * R::G) = q;
        }
        __syncthreads();
    }
}

// the per-element form over all planes: element e of plane p is source element e * channels + sel.ch[p]
template <int FMT>
__global__ __launch_bounds__(256) void unpack_all_elem_kernel(const unsigned char *__restrict__ src, size_t n, size_t channels, unpack_sel_t sel,
                                                              size_t n_sel, typename reader_t<FMT>::out_t *__restrict__ out, size_t plane_ld) {
    __shared__ int s_sel[UNPACK_MAX_SEL];
    if (threadIdx.x < n_sel) s_sel[threadIdx.x] = sel.ch[threadIdx.x];
    __syncthreads();
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = t0; i < n * n_sel; i += step) {
        const size_t p = i / n, e = i - p * n;
        out[p * plane_ld + e] = read_one<FMT>(src, e * channels + (size_t)s_sel[p]);
    }
}

// rows [row0, row0 + rows) of src (src_ld doubles apart), columns [c0, c1), to dst rows [0, rows) (dst_ld apart); and the same rows
// of the three status rows: src_st [3, src_n] from column row0 to dst_st [3, dst_n] (dst_st already points at the first column)
__global__ __launch_bounds__(256) void host_rows_kernel(const double *__restrict__ src, size_t src_ld, size_t row0, size_t rows, size_t c0,
                                                        size_t c1, double *__restrict__ dst, size_t dst_ld, const int32_t *__restrict__ src_st,
                                                        size_t src_n, int32_t *__restrict__ dst_st, size_t dst_n) {
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const size_t w = c1 - c0, total = rows * w;
    for (size_t i = t0; i < total; i += step) {
        const size_t r = i / w, c = c0 + i % w;
        dst[r * dst_ld + c] = src[(row0 + r) * src_ld + c];
    }
    if (dst_st != nullptr)
        for (size_t i = t0; i < 3 * rows; i += step) {
            const size_t k = i / rows, r = i % rows;
            dst_st[k * dst_n + r] = src_st[k * src_n + row0 + r];
        }
}

template <int FMT>
void launch_unpack_as(hipStream_t s, const void *src, size_t n, size_t channels, size_t channel, void *out) {
    using R = reader_t<FMT>;
    size_t blocks = (n / R::G + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(unpack_kernel<FMT>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const unsigned char *>(src), n, channels,
                       channel, static_cast<typename R::out_t *>(out));
}

template <int FMT>
void launch_unpack_all_as(hipStream_t s, const void *src, size_t n, size_t channels, const unpack_sel_t &sel, size_t n_sel, void *out, size_t plane_ld) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    const unsigned char *in = static_cast<const unsigned char *>(src);
    out_t *o = static_cast<out_t *>(out);
    // whole tiles through LDS where a tile holds at least 16 sample frames, the source can be read by dwords and every lane's 16
    // output bytes are aligned in every plane; the tail -- or everything -- by the element kernel
    const size_t fb = channels * R::B;
    const size_t T = fb <= UNPACK_ALL_TILE_BYTES / 16 ? (UNPACK_ALL_TILE_BYTES / fb) & ~(size_t)15 : 0;
    const bool tiled = T != 0 && n >= T && ((uintptr_t)src & 3) == 0 && ((uintptr_t)out & 15) == 0 && plane_ld % R::G == 0;
    size_t done = 0;
    if (tiled) {
        const size_t n_tiles = n / T, blocks = n_tiles < 256 * 8 ? n_tiles : 256 * 8;
        hipLaunchKernelGGL(unpack_all_tiled_kernel<FMT>, dim3((unsigned)blocks), dim3(256), 0, s, in, n_tiles, (unsigned)T, (unsigned)channels, sel,
                           (unsigned)n_sel, o, plane_ld);
        done = n_tiles * T;
    }
    if (done < n) {
        size_t blocks = ((n - done) * n_sel + 255) / 256;
        if (blocks > 256 * 32) blocks = 256 * 32;
        hipLaunchKernelGGL(unpack_all_elem_kernel<FMT>, dim3((unsigned)blocks), dim3(256), 0, s, in + done * fb, n - done, channels, sel, n_sel,
                           o + done, plane_ld);
    }
}

}  // namespace

void launch_unpack(hipStream_t s, int format, const void *src, size_t n, size_t channels, size_t channel, void *out) {
    if (format == UNPACK_PCM24 && channels == 1 && ((uintptr_t)src & 3) == 0 && ((uintptr_t)out & 15) == 0 && n >= PCM24_TILE) {
        // whole tiles through LDS; the tail (it starts on a dword and a 16-byte boundary again) by the element kernel
        const size_t n_tiles = n / PCM24_TILE, done = n_tiles * PCM24_TILE;
        const size_t blocks = n_tiles < 256 * 32 ? n_tiles : 256 * 32;
        hipLaunchKernelGGL(unpack_pcm24_tiled_kernel, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint32_t *>(src), n_tiles,
                           static_cast<double *>(out));
        if (done < n) launch_unpack_as<UNPACK_PCM24>(s, static_cast<const unsigned char *>(src) + 3 * done, n - done, 1, 0, static_cast<double *>(out) + done);
        return;
    }
    switch (format) {
        case UNPACK_PCM16: launch_unpack_as<UNPACK_PCM16>(s, src, n, channels, channel, out); break;
        case UNPACK_PCM24: launch_unpack_as<UNPACK_PCM24>(s, src, n, channels, channel, out); break;
        case UNPACK_PCM32: launch_unpack_as<UNPACK_PCM32>(s, src, n, channels, channel, out); break;
        case UNPACK_F32: launch_unpack_as<UNPACK_F32>(s, src, n, channels, channel, out); break;
        case UNPACK_F64: launch_unpack_as<UNPACK_F64>(s, src, n, channels, channel, out); break;
        case UNPACK_U8: launch_unpack_as<UNPACK_U8>(s, src, n, channels, channel, out); break;
        case UNPACK_ULAW: launch_unpack_as<UNPACK_ULAW>(s, src, n, channels, channel, out); break;
        case UNPACK_ALAW: launch_unpack_as<UNPACK_ALAW>(s, src, n, channels, channel, out); break;
    }
}

void launch_unpack_all(hipStream_t s, int format, const void *src, size_t n, size_t channels, const unpack_sel_t &sel, size_t n_sel, void *out,
                       size_t plane_ld) {
    if (n == 0) return;
    if (channels == 1) { launch_unpack(s, format, src, n, 1, 0, out); return; }        // one plane, the mono forms (wide loads, the 24-bit tiles)
    switch (format) {
        case UNPACK_PCM16: launch_unpack_all_as<UNPACK_PCM16>(s, src, n, channels, sel, n_sel, out, plane_ld); break;
        case UNPACK_PCM24: launch_unpack_all_as<UNPACK_PCM24>(s, src, n, channels, sel, n_sel, out, plane_ld); break;
        case UNPACK_PCM32: launch_unpack_all_as<UNPACK_PCM32>(s, src, n, channels, sel, n_sel, out, plane_ld); break;
        case UNPACK_F32: launch_unpack_all_as<UNPACK_F32>(s, src, n, channels, sel, n_sel, out, plane_ld); break;
        case UNPACK_F64: launch_unpack_all_as<UNPACK_F64>(s, src, n, channels, sel, n_sel, out, plane_ld); break;
        case UNPACK_U8: launch_unpack_all_as<UNPACK_U8>(s, src, n, channels, sel, n_sel, out, plane_ld); break;
        case UNPACK_ULAW: launch_unpack_all_as<UNPACK_ULAW>(s, src, n, channels, sel, n_sel, out, plane_ld); break;
        case UNPACK_ALAW: launch_unpack_all_as<UNPACK_ALAW>(s, src, n, channels, sel, n_sel, out, plane_ld); break;
    }
}

void launch_host_rows(hipStream_t s, const double *src, size_t src_ld, size_t row0, size_t rows, size_t c0, size_t c1, double *dst,
                      size_t dst_ld, const int32_t *src_st, size_t src_n, int32_t *dst_st, size_t dst_n) {
    size_t blocks = (rows * (c1 - c0) + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(host_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, src_ld, row0, rows, c0, c1, dst, dst_ld, src_st,
                       src_n, dst_st, dst_n);
}

}  // namespace vbx
