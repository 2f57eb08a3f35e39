// vbx_clips_pack.hpp -- clips_pack_<fmt>, the pack kernel of vbx_analyze_clips, as a template over the sample format: k_clips.hip
// instantiates it for the five formats of two bytes and more, k_sample8.hip for the 8-bit ones (the description is in k_clips.hip).
// Device code and its launcher, in the unit's own anonymous namespace: every unit that includes this gets its own instantiations.
#pragma once
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
                    if ((a & (R::W - 1)) == 0) { read_group_wide<FMT>(w, 0, v); done = true; }
                    else if (R::W == 16 && (a & 3) == 0) {                      // (the plain copies)
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

}  // namespace vbx
