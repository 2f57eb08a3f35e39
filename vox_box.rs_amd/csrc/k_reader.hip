// k_reader.hip -- what a WAV reader hands over, turned into the type the frame loop reads natively (vbx_unpack_samples, and the
// per-chunk step of vbx_analyze_host): ONE channel of interleaved sample frames,
//   16-bit PCM -> int16 (the PCM kernels' input), 24-bit packed / 32-bit PCM -> f64 = s / (i32::MAX >> (32 - bits)), correctly
//   rounded (tests/lib.rs:17-19), float / double -> as they are (copied as bit patterns: NaN payloads survive).
// HBM-bound byte work: one pass, grid-stride over groups of consecutive OUTPUT elements, capped grid, size_t indices.  A lane
// owns 16 consecutive output bytes per step, so every wave instruction touches ONE contiguous span: with a 16-byte aligned
// destination a wave's store is 1 KiB, and a mono source of matching alignment arrives by one load per lane of the same shape
// (16 bytes; 8 for the two 32-bit samples of a lane).  Packed 24-bit samples are 6 bytes per lane, which no load instruction
// fetches: a mono source on a dword boundary is staged through LDS -- the block reads a tile's dwords as contiguous spans, each lane
// then picks its two samples out of LDS -- and every other 24-bit source is read byte by byte.  The quotients are IEEE divisions:
// div_exact_small (vbx_device.hpp) is proven for 16-bit numerators only, and the divide hides behind the memory traffic.
// host_rows_kernel: a chunk's own record rows and its three status rows, copied from the chunk-local buffers into the caller's.
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"

namespace vbx {

namespace {

template <int FMT> struct reader_t;
template <> struct reader_t<UNPACK_PCM16> { using out_t = uint16_t; static constexpr int G = 8; };
template <> struct reader_t<UNPACK_PCM24> { using out_t = double;   static constexpr int G = 2; };
template <> struct reader_t<UNPACK_PCM32> { using out_t = double;   static constexpr int G = 2; };
template <> struct reader_t<UNPACK_F32>   { using out_t = uint32_t; static constexpr int G = 4; };
template <> struct reader_t<UNPACK_F64>   { using out_t = uint64_t; static constexpr int G = 2; };

__device__ __forceinline__ int sext24(uint32_t v) { return (int)(v << 8) >> 8; }
__device__ __forceinline__ double pcm24_value(int s) { return (double)s / 8388607.0; }
__device__ __forceinline__ double pcm32_value(int s) { return (double)s / 2147483647.0; }

// element e of the source (e counts samples, not sample frames)
template <int FMT>
__device__ __forceinline__ typename reader_t<FMT>::out_t read_one(const unsigned char *__restrict__ src, size_t e) {
    if constexpr (FMT == UNPACK_PCM16) return reinterpret_cast<const uint16_t *>(src)[e];
    else if constexpr (FMT == UNPACK_PCM24) {
        const unsigned char *b = src + 3 * e;
        return pcm24_value(sext24((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16)));
    } else if constexpr (FMT == UNPACK_PCM32) return pcm32_value(reinterpret_cast<const int *>(src)[e]);
    else if constexpr (FMT == UNPACK_F32) return reinterpret_cast<const uint32_t *>(src)[e];
    else return reinterpret_cast<const uint64_t *>(src)[e];
}

// G consecutive mono samples from group g of a source aligned for it (wide_in below): one load per lane
template <int FMT>
__device__ __forceinline__ void read_group_wide(const unsigned char *__restrict__ src, size_t g, typename reader_t<FMT>::out_t *v) {
    static_assert(FMT != UNPACK_PCM24, "packed 24-bit samples have no per-lane load: unpack_pcm24_tiled_kernel");
    if constexpr (FMT == UNPACK_PCM32) {
        const int2 q = reinterpret_cast<const int2 *>(src)[g];
        v[0] = pcm32_value(q.x); v[1] = pcm32_value(q.y);
    } else {                                                   // the plain copies: 16 bytes in, 16 bytes out
        const uint4 q = reinterpret_cast<const uint4 *>(src)[g];
        __builtin_memcpy(v, &q, 16);
    }
}

template <int FMT>
__global__ __launch_bounds__(256) void unpack_kernel(const unsigned char *__restrict__ src, size_t n, size_t channels, size_t channel,
                                                     typename reader_t<FMT>::out_t *__restrict__ out) {
    using R = reader_t<FMT>;
    using out_t = typename R::out_t;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const bool vec_out = (reinterpret_cast<uintptr_t>(out) & 15) == 0;                        // kernel-uniform
    const bool wide_in = FMT != UNPACK_PCM24 && channels == 1 && (reinterpret_cast<uintptr_t>(src) & (FMT == UNPACK_PCM32 ? 7 : 15)) == 0;
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
