// The one symbol csrc/vbx_host.cpp takes from the device side of the library, for its host-only sanitizer build
// (vox_box.rs_amd/Makefile: lib/libvbx_host_asan.so).
#include <string>

struct vbx_ctx;
static thread_local std::string g_err;
extern "C" int vbx_internal_fail(vbx_ctx *, int code, const char *msg) { g_err = msg ? msg : ""; return code; }
extern "C" const char *vbx_last_error(const vbx_ctx *) { return g_err.c_str(); }

// -DVBX_HOST_ASAN_MAIN: a stand-alone program over the host arithmetic of a session pool's tick (vbx_pool_plan), for
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DVBX_HOST_ASAN_MAIN -Iinclude
//       vox_box.rs_amd/csrc/vbx_host.cpp tools/host_asan_stub.cpp -o host_asan_pool && ./host_asan_pool
// a few thousand random ticks at five frame shapes, the rows written into exactly sized heap arrays; it checks the prefix sums and
// the layout rule on the way and returns 0 when all hold.
#ifdef VBX_HOST_ASAN_MAIN
#include <cstdint>
#include <cstdio>
#include <vector>

#include "voxbox_hip.h"

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
    return 0;
}
#endif
