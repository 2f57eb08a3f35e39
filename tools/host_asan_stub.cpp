// The one symbol csrc/vbx_host.cpp takes from the device side of the library, for its host-only sanitizer build
// (vox_box.rs_amd/Makefile: lib/libvbx_host_asan.so).
#include <string>

struct vbx_ctx;
static thread_local std::string g_err;
extern "C" int vbx_internal_fail(vbx_ctx *, int code, const char *msg) { g_err = msg ? msg : ""; return code; }
extern "C" const char *vbx_last_error(const vbx_ctx *) { return g_err.c_str(); }

// -DVBX_HOST_ASAN_MAIN: a stand-alone program over the host arithmetic of a session pool's tick (vbx_pool_plan) and of the fused frame
// loop's launches (launch_ranges_host), for
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DVBX_HOST_ASAN_MAIN -Iinclude
//       vox_box.rs_amd/csrc/vbx_host.cpp tools/host_asan_stub.cpp -o host_asan_pool && ./host_asan_pool
// a few thousand random ticks at five frame shapes, the rows written into exactly sized heap arrays; it checks the prefix sums and
// the layout rule on the way and returns 0 when all hold.
#ifdef VBX_HOST_ASAN_MAIN
#include <cstdint>
#include <cstdio>
#include <vector>

#include "voxbox_hip.h"
#include "../vox_box.rs_amd/csrc/vbx_host.hpp"

int main() {
    const size_t shapes[5][2] = {{400, 160}, {1200, 480}, {200, 80}, {100, 250}, {1, 1}};
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint64_t n) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (size_t)(x % n); };
    size_t ticks = 0;
    for (const auto &sh : shapes) {
        const size_t N = sh[0], H = sh[1];
        for (int t = 0; t < 800; t++, ticks++) {
            const size_t n = rnd(40);
            std::vector<size_t> c(n), u(n), m(n);
            for (size_t i = 0; i < n; i++) {
                c[i] = rnd(N + 300 * H);
                u[i] = rnd(vbx_frame_count(c[i], N, H) + 1);
                m[i] = rnd(4) == 0 ? 0 : rnd(N + 90 * H);
            }
            std::vector<vbx_pool_plan_row> rows(n);
            size_t total = 0, call = 0;
            if (vbx_pool_plan(c.data(), u.data(), m.data(), n, N, H, rows.data(), &total, &call) != VBX_SUCCESS) return 1;
            size_t row = 0, next = 0, last = 0;
            for (size_t i = 0; i < n; i++) {
                const vbx_pool_plan_row &r = rows[i];
                if ((size_t)r.row_start != row || (size_t)r.n_rows != r.plan.hi - r.plan.lo) return 2;
                if (r.n_rows == 0) { if (r.frames != 0 || r.plane_frame != -1) return 3; continue; }
                if ((size_t)r.plane_frame != next || (size_t)r.frames != r.plan.warm + (size_t)r.n_rows) return 4;
                const size_t span = ((size_t)r.frames - 1) * H + N;
                last = next + (size_t)r.frames;
                next += (span + H - 1) / H;
                row += (size_t)r.n_rows;
            }
            if (total != row || call != last) return 5;
        }
    }
    std::printf("vbx_pool_plan: %zu random ticks, all rules hold\n", ticks);
    // the fused frame loop's launches (launch_ranges_host): random utterance starts (with repeats: empty utterances) against a frame-by-frame
    // statement of the same rule; the arrays are exactly sized vectors
    size_t plans = 0;
    for (int t = 0; t < 3000; t++, plans++) {
        const size_t F = 1 + rnd(5000), L = 1 + rnd(t % 3 == 0 ? 40 : 1500), ns = rnd(12);
        std::vector<int64_t> starts;
        if (ns) { starts.push_back(0); for (size_t i = 1; i < ns; i++) starts.push_back(rnd(4) == 0 ? starts.back() : starts.back() + (int64_t)rnd(F - (size_t)starts.back() + 1)); }
        std::vector<int64_t> seg, stitch; std::vector<size_t> off;
        vbx::launch_ranges_host(ns ? starts.data() : nullptr, ns, F, L, seg, off, stitch);
        const size_t launches = (F + L - 1) / L;
        if (off.size() != launches + 1 || stitch.size() != launches || off.back() != seg.size()) return 6;
        for (size_t j = 0; j < launches; j++) {
            const size_t f0 = j * L, f1 = f0 + L < F ? f0 + L : F;
            std::vector<int64_t> want{0};
            bool here = f0 == 0;
            for (int64_t s : starts) { if ((size_t)s == f0) here = true; if ((size_t)s > f0 && (size_t)s < f1) want.push_back(s - (int64_t)f0); }
            if (off[j + 1] - off[j] != want.size()) return 7;
            for (size_t i = 0; i < want.size(); i++) if (seg[off[j] + i] != want[i]) return 8;
            const int64_t cont = here ? 0 : (want.size() > 1 ? want[1] : (int64_t)(f1 - f0));
            if (stitch[j] != cont || cont < 0 || (size_t)cont > f1 - f0) return 9;
        }
    }
    std::printf("launch_ranges_host: %zu random plans, all rules hold\n", plans);
    return 0;
}
#endif
