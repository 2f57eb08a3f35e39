// vbx_sample8.hpp -- what one byte of 8-bit telephone audio means (VBX_SAMPLE_ULAW / VBX_SAMPLE_ALAW / VBX_SAMPLE_U8): the ITU-T G.711
// expansions to 16-bit linear PCM, and unsigned 8-bit PCM as the reader of an 8-bit WAV hands it over.  Integer arithmetic in
// registers, no table: the SAME functions run in the readers' kernels (vbx_reader.hpp) and on the host (vbx_g711_table, vbx_host.cpp),
// so a CPU test of the table pins the kernels' arithmetic.  Plain C++: this header is read by host-only units too.
#pragma once
#include <cstdint>

#if defined(__HIP__)                                        // (the compiler's own mark of a HIP translation unit)
#define VBX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define VBX_HD inline
#endif

namespace vbx {

// G.711 mu-law: the complemented byte is sign | 3-bit exponent | 4-bit mantissa; +-32124 at most, 0x7f and 0xff both 0
VBX_HD int16_t ulaw_value(uint32_t b) {
    const uint32_t u = ~b & 0xffu, e = (u >> 4) & 7u, m = u & 15u;
    const int mag = (int)((((m << 3) + 0x84u) << e) - 0x84u);
    return (int16_t)((u & 0x80u) ? -mag : mag);
}

// G.711 A-law: the byte with its even bits inverted is sign | exponent | mantissa; +-32256 at most, no zero code
VBX_HD int16_t alaw_value(uint32_t b) {
    const uint32_t a = (b ^ 0x55u) & 0xffu, e = (a >> 4) & 7u, m = a & 15u;
    const int mag = (int)(e == 0 ? (m << 4) + 8u : ((m << 4) + 0x108u) << (e - 1));
    return (int16_t)((a & 0x80u) ? mag : -mag);
}

// unsigned 8-bit PCM: an 8-bit WAV sample is b - 128, scaled by i32::MAX >> 24 = 127 (tests/lib.rs:17-19 at bits_per_sample = 8); a
// correctly rounded IEEE quotient, as the PCM24 / PCM32 values are
VBX_HD double u8_value(uint32_t b) { return (double)((int)(b & 0xffu) - 128) / 127.0; }

}  // namespace vbx
