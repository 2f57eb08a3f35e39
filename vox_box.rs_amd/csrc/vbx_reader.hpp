// vbx_reader.hpp -- the per-sample arithmetic of the readers (k_reader.hip: vbx_unpack_samples; k_session.hip: a live session's
// ingest): what one source sample becomes, and the widest load a lane's 16 output bytes can come from.  Device code only.
#pragma once
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"

namespace vbx {

template <int FMT> struct reader_t;
// out_t: what is written; G: elements in a lane's 16 output bytes; B: bytes of a source sample
template <> struct reader_t<UNPACK_PCM16> { using out_t = uint16_t; static constexpr int G = 8; static constexpr int B = 2; };
template <> struct reader_t<UNPACK_PCM24> { using out_t = double;   static constexpr int G = 2; static constexpr int B = 3; };
template <> struct reader_t<UNPACK_PCM32> { using out_t = double;   static constexpr int G = 2; static constexpr int B = 4; };
template <> struct reader_t<UNPACK_F32>   { using out_t = uint32_t; static constexpr int G = 4; static constexpr int B = 4; };
template <> struct reader_t<UNPACK_F64>   { using out_t = uint64_t; static constexpr int G = 2; static constexpr int B = 8; };

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

}  // namespace vbx
