// vbx_reader.hpp -- the per-sample arithmetic of the readers (k_reader.hip: vbx_unpack_samples; k_session.hip: a live session's
// ingest; vbx_session_ingest_all.hpp, vbx_clips_pack.hpp: the multi-channel ingest and the clip pack): what one source sample becomes,
// and the widest load a lane's 16 output bytes can come from.  Device code only.
#pragma once
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"
#include "vbx_sample8.hpp"

namespace vbx {

template <int FMT> struct reader_t;
// out_t: what is written; G: elements in a lane's 16 output bytes; B: bytes of a source sample; W = G * B: the bytes of the one
// load a lane's group comes from (read_group_wide), which is also the alignment that load needs (0: there is no such load)
template <> struct reader_t<UNPACK_PCM16> { using out_t = uint16_t; static constexpr int G = 8; static constexpr int B = 2; static constexpr int W = 16; };
template <> struct reader_t<UNPACK_PCM24> { using out_t = double;   static constexpr int G = 2; static constexpr int B = 3; static constexpr int W = 0; };
template <> struct reader_t<UNPACK_PCM32> { using out_t = double;   static constexpr int G = 2; static constexpr int B = 4; static constexpr int W = 8; };
template <> struct reader_t<UNPACK_F32>   { using out_t = uint32_t; static constexpr int G = 4; static constexpr int B = 4; static constexpr int W = 16; };
template <> struct reader_t<UNPACK_F64>   { using out_t = uint64_t; static constexpr int G = 2; static constexpr int B = 8; static constexpr int W = 16; };
// one byte per sample: G.711 decodes to the int16 the PCM16 kernels read, unsigned 8-bit PCM to a quotient in double
template <> struct reader_t<UNPACK_U8>    { using out_t = double;   static constexpr int G = 2; static constexpr int B = 1; static constexpr int W = 2; };
template <> struct reader_t<UNPACK_ULAW>  { using out_t = uint16_t; static constexpr int G = 8; static constexpr int B = 1; static constexpr int W = 8; };
template <> struct reader_t<UNPACK_ALAW>  { using out_t = uint16_t; static constexpr int G = 8; static constexpr int B = 1; static constexpr int W = 8; };

// one byte of an 8-bit format, decoded (vbx_sample8.hpp)
template <int FMT>
__device__ __forceinline__ typename reader_t<FMT>::out_t byte_value(uint32_t b) {
    static_assert(reader_t<FMT>::B == 1, "the 8-bit formats");
    if constexpr (FMT == UNPACK_U8) return u8_value(b);
    else if constexpr (FMT == UNPACK_ULAW) return (uint16_t)ulaw_value(b);
    else return (uint16_t)alaw_value(b);
}

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
    else if constexpr (FMT == UNPACK_F64) return reinterpret_cast<const uint64_t *>(src)[e];
    else return byte_value<FMT>(src[e]);
}

// G consecutive mono samples from group g of a source aligned for it (wide_in below): one load per lane
template <int FMT>
__device__ __forceinline__ void read_group_wide(const unsigned char *__restrict__ src, size_t g, typename reader_t<FMT>::out_t *v) {
    static_assert(FMT != UNPACK_PCM24, "packed 24-bit samples have no per-lane load: unpack_pcm24_tiled_kernel");
    if constexpr (FMT == UNPACK_PCM32) {
        const int2 q = reinterpret_cast<const int2 *>(src)[g];
        v[0] = pcm32_value(q.x); v[1] = pcm32_value(q.y);
    } else if constexpr (FMT == UNPACK_U8) {                   // two bytes in
        const uint32_t h = reinterpret_cast<const uint16_t *>(src)[g];
        v[0] = byte_value<FMT>(h & 0xffu); v[1] = byte_value<FMT>(h >> 8);
    } else if constexpr (FMT == UNPACK_ULAW || FMT == UNPACK_ALAW) {      // eight bytes in, decoded in registers
        const uint2 q = reinterpret_cast<const uint2 *>(src)[g];
#pragma unroll
        for (int j = 0; j < 4; j++) { v[j] = byte_value<FMT>((q.x >> (8 * j)) & 0xffu); v[4 + j] = byte_value<FMT>((q.y >> (8 * j)) & 0xffu); }
    } else {                                                   // the plain copies: 16 bytes in, 16 bytes out
        const uint4 q = reinterpret_cast<const uint4 *>(src)[g];
        __builtin_memcpy(v, &q, 16);
    }
}

// ---- tiles of whole sample frames through LDS (k_reader.hip: unpack_all_tiled_kernel; k_session_channels.hip: the ingest) ----
#define UNPACK_ALL_TILE_BYTES 8192
static_assert(UNPACK_ALL_TILE_BYTES / 16 <= 2 * 256, "the staging loop is two 16-byte loads per lane");

// the sample at byte b of the tile (b is a multiple of B: the tile starts on a sample frame)
template <int FMT>
__device__ __forceinline__ typename reader_t<FMT>::out_t lds_one(const uint32_t *tile, unsigned b) {
    if constexpr (FMT == UNPACK_PCM16) return (uint16_t)(tile[b >> 2] >> ((b & 2) * 8));      // (a dword read: lanes on the two halves of one dword broadcast)
    else if constexpr (FMT == UNPACK_PCM24) {                // three bytes at any byte offset: out of the two dwords that hold them
        const uint64_t w = (uint64_t)tile[b >> 2] | ((uint64_t)tile[(b >> 2) + 1] << 32);
        return pcm24_value(sext24((uint32_t)(w >> ((b & 3) * 8))));
    } else if constexpr (FMT == UNPACK_PCM32) return pcm32_value((int)tile[b >> 2]);
    else if constexpr (FMT == UNPACK_F32) return tile[b >> 2];
    else if constexpr (FMT == UNPACK_F64) return reinterpret_cast<const uint64_t *>(tile)[b >> 3];
    else return byte_value<FMT>((tile[b >> 2] >> ((b & 3) * 8)) & 0xffu);      // a byte at any byte offset of the tile's dwords
}

// a block of 256 lanes (lane t) stages tile_bytes (a multiple of 16, <= UNPACK_ALL_TILE_BYTES) from w into the 16-byte aligned tile:
// 16-byte loads where w sits on a 16-byte boundary (wide), dword loads otherwise (w on a dword boundary)
__device__ __forceinline__ void lds_stage_tile(uint32_t *tile, const unsigned char *__restrict__ w, unsigned tile_bytes, bool wide, unsigned t) {
    if (wide) {                                                             // at most 512 words of 16 bytes: both loads of a lane in flight
        const uint4 *w4 = reinterpret_cast<const uint4 *>(w);
        uint4 *tile4 = reinterpret_cast<uint4 *>(tile);
        const unsigned n16 = tile_bytes / 16;
        const bool two = t + 256 < n16;
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
        if (t < n16) q0 = w4[t];
        if (two) q1 = w4[t + 256];
        if (t < n16) tile4[t] = q0;
        if (two) tile4[t + 256] = q1;
    } else for (unsigned i = t; i < tile_bytes / 4; i += 256) tile[i] = reinterpret_cast<const uint32_t *>(w)[i];
}

}  // namespace vbx
