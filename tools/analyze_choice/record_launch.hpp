// record_launch.hpp -- a recording build of the library: every hipLaunchKernelGGL prints what it names instead of launching it.
//
//     make -C vox_box.rs_amd BUILD=build_record LIB=lib/libvoxbox_hip_record.so EXTRA="-include ../tools/analyze_choice/record_launch.hpp -Icsrc"
//
// One line per launch on stdout: the kernel's demangled symbol (the address of the kernel's host stub through dladdr: link with
// -rdynamic), grid, block, dynamic LDS bytes and a checksum of the argument block, field by field (the blocks are built member by member
// on the stack: their padding, and the fields a family's kernels never read, hold whatever the stack held).  tools/analyze_choice/driver.cpp
// calls vbx::launch_analyze over a grid of launches in such a build; the transcript of a host-side refactor must equal its parent's.
#pragma once
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#include <cxxabi.h>
#include <dlfcn.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "vbx_spectral.hpp"

namespace vbx_record {

struct fnv_t {
    uint64_t h = 1469598103934665603ull;
    template <typename T> void put(const T &v) {
        unsigned char b[sizeof(T)];
        std::memcpy(b, &v, sizeof(T));
        for (size_t i = 0; i < sizeof(T); i++) { h ^= b[i]; h *= 1099511628211ull; }
    }
    template <typename T, typename... R> void put(const T &v, const R &...r) { put(v); put(r...); }
};

inline void fields(fnv_t &h, const vbx::pitch_params_t &p) { h.put(p.sample_rate, p.threshold, p.fmin, p.fmax, p.kmax, p.full_off, p.f32, p.ncurve); }
inline void fields(fnv_t &h, const vbx::mfcc_interp_t &i) { h.put(i.rot, i.coef, i.j0, i.jmin, i.jmax, i.taps, i.pu_off, i.lds_bytes); }
inline void fields(fnv_t &h, const vbx::spectral_args_1200_t &a, bool) {
    h.put(a.frames, a.n_frames, a.stride, a.window, a.lag_window, a.tab, a.n, a.mfcc_q, a.pcm, a.num_coeffs);
    h.put(a.out_cand, a.cand_ld, a.out_count, a.pitch_status, a.work, a.unsure_list, a.unsure_count, a.nb);
    fields(h, a.pp);
    h.put(a.out_lpc, a.lpc_ld, a.out_mfcc, a.mfcc_ld, a.mfcc_status, a.bins, a.slopes, a.dct);
}
inline void fields(fnv_t &h, const vbx::spectral_args_1200_burg_t &a, bool w) {
    fields(h, static_cast<const vbx::spectral_args_1200_t &>(a), w);
    h.put(a.burg_scratch, a.burg_window, a.burg_f0);
}
// pow2: the kernel reads the batch and split fields (the 1200-point kernels that take the whole block never do, and their launcher leaves them unset)
inline void fields(fnv_t &h, const vbx::spectral_args_t &a, bool pow2) {
    h.put(a.frames, a.n_frames, a.stride, a.window, a.lag_window, a.tab, a.n);
    fields(h, a.pp);
    h.put(a.out_cand, a.cand_ld, a.out_count, a.pitch_status, a.work, a.out_lpc, a.lpc_ld, a.out_mfcc, a.mfcc_ld, a.mfcc_status);
    h.put(a.bins, a.slopes, a.dct, a.num_coeffs, a.nb, a.unsure_list, a.unsure_count, a.out_r, a.n_lags, a.mfcc_q, a.pcm);
    fields(h, a.ip);
    if (pow2) h.put(a.f0, a.n_batch, a.curve, a.curve_ld, a.curve_tol, a.curve_list, a.list_ld, a.reach, a.cand_cap, a.far_list);
}
template <typename T> inline void fields(fnv_t &, const T &, bool) {}            // (kernels of other families: no checksum)

template <typename... A>
inline void launch(const void *stub, dim3 g, dim3 b, size_t lds, const A &...a) {
    Dl_info info{};
    const char *sym = (dladdr(stub, &info) && info.dli_sname) ? info.dli_sname : "?";
    int st = 0;
    char *dm = abi::__cxa_demangle(sym, nullptr, nullptr, &st);
    const char *name = (st == 0 && dm) ? dm : sym;
    const bool pow2 = std::strstr(name, "analyze_kernel<") == nullptr;
    fnv_t h;
    (fields(h, a, pow2), ...);
    std::printf("  launch %s grid=%u,%u,%u block=%u,%u,%u lds=%zu args=%016llx\n", name, g.x, g.y, g.z, b.x, b.y, b.z, lds, (unsigned long long)h.h);
    std::free(dm);
}

}  // namespace vbx_record

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    vbx_record::launch(reinterpret_cast<const void *>(kernel), dim3(grid), dim3(block), (size_t)(lds), __VA_ARGS__)
#endif
