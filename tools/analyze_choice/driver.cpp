// driver.cpp -- calls vbx::launch_analyze over a grid of launches in a recording build (record_launch.hpp) and prints, per call, the
// launch's description, what was launched, and what came back.  Not a test; nothing imports it.  No GPU is needed: nothing is launched.
//
//     make -C vox_box.rs_amd BUILD=build_record LIB=lib/libvoxbox_hip_record.so EXTRA="-include ../tools/analyze_choice/record_launch.hpp -Icsrc"
//     hipcc -O1 -std=c++17 -rdynamic -Ivox_box.rs_amd/csrc -Iinclude tools/analyze_choice/driver.cpp vox_box.rs_amd/build_record/*.o \
//           -L/opt/rocm/lib -lrccl -ldl -Wl,-rpath,/opt/rocm/lib -o /tmp/analyze_choice_driver
//     /tmp/analyze_choice_driver > transcript.txt          (the named launches first -- tests/golden/analyze_choice_named.txt --, then the grid)
//
// -DANALYZE_CHOICE_BEFORE: the launcher's interface before choose_analyze existed (the return value 1 / 0 / -1, the launched_spec
// out-parameter, spectral_launch_t::batching), for the transcript of that tree; the lines printed are the same.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "vbx_kernels.hpp"

using namespace vbx;

namespace {

// fixed fake addresses: the launcher compares them with NULL and looks at their low bits, nothing reads them
template <typename T> T *fake(uintptr_t slot, uintptr_t off = 0) { return reinterpret_cast<T *>((uintptr_t)0x100000000ull * (slot + 1) + off); }

struct launch_desc_t {
    int n = 1200, kind = 0, kmax = 4, lpc = 0, coeffs = 0, interp = 0, defer = 0, allow_spec = 1, lag_rcp = 1, whole_curve = 0;
    int base8 = 0, ld_odd = 0, mode = 0 /* 0 analysis, 1 MFCC alone, 2 autocorrelation alone */, n_lags = 0;
    long scratch = 0;                                        // curve_ws_bytes
    int burg = 0;                                            // 0 none, 1 requested, 2 misaligned window, 3 range past the batch
    long F = 67;
    double sample_rate = 48000.0, fmin = 75.0;
    int nb() const { return n / 6; }
    int b_lo() const { return 2; }
};

// the plan the callers take (vbx_api_frames.hip, run_mfcc)
int plan_of(const launch_desc_t &d) {
    if (d.mode == 1 && !d.interp && (d.n == 2048 || d.n == 4096)) return d.n == 2048 ? SPECTRAL_PLAN_1024 : SPECTRAL_PLAN_2048;
    if (d.mode == 1 && !d.interp && d.n == 2400) return SPECTRAL_PLAN_1200;
    if (d.coeffs != 0 && (d.interp || spectral_supported_plan(spectral_plan_mfcc(d.n), d.n, 0, d.nb(), d.b_lo(), d.coeffs))) return spectral_plan_mfcc(d.n);
    return spectral_plan(d.n);
}

// false: the shape has no such launch (no plan; interpolated bins asked where the table has no form)
bool make_launch(const launch_desc_t &d, spectral_launch_t &L) {
    L = spectral_launch_t{};
    L.plan = plan_of(d); L.n = d.n;
    if (L.plan == SPECTRAL_PLAN_NONE) return false;
    L.x = frames_t(fake<void>(0), (sample_kind_t)d.kind);
    L.F = d.F; L.stride = d.n / 2; L.window = fake<double>(1); L.lag_window = fake<double>(2); L.tab = fake<double>(3);
    L.allow_spec = d.allow_spec; L.mfcc_defer = d.defer; L.lag_rcp = d.lag_rcp; L.whole_curve = d.whole_curve;
    L.sample_rate = d.sample_rate; L.threshold = 0.2; L.fmin = d.fmin; L.fmax = 600.0; L.kmax = d.kmax;
    L.out_cand = fake<pitch_t>(4, d.base8 ? 8 : 0); L.cand_ld = 2L * d.kmax + (d.ld_odd ? 1 : 0); L.out_count = fake<int32_t>(5); L.pitch_status = fake<int32_t>(6);
    L.unsure_list = fake<int32_t>(7, 16); L.unsure_count = fake<int32_t>(7);
    L.mfcc_only = d.mode == 1;
    if (d.mode == 0 && d.lpc) { L.out_lpc = fake<double>(8); L.lpc_ld = 13; }
    if (d.mode != 2 && d.coeffs) {
        L.out_mfcc = fake<double>(9); L.mfcc_ld = d.coeffs; L.mfcc_status = fake<int32_t>(10);
        L.bins = fake<int32_t>(11); L.slopes = fake<double>(12); L.dct = fake<double>(13); L.num_coeffs = d.coeffs; L.nb = d.nb();
    }
    if (d.mode == 2) { L.out_r = fake<double>(14); L.n_lags = d.n_lags; }
    if (d.interp) {
        if ((2 * spectral_plan_nc(L.plan)) % d.n == 0) return false;
        std::vector<char> h(mfcc_interp_table_bytes(L.plan, d.nb()), 0);
        if (!mfcc_interp_fill(L.plan, d.n, d.b_lo(), d.nb(), h.data(), &L.ip)) return false;
        L.interp = true; L.ip.rot = fake<double>(15); L.ip.coef = fake<double>(16); L.ip.j0 = fake<int32_t>(17);
    }
    if (d.scratch > 0) { L.curve_ws = fake<double>(18); L.curve_ws_bytes = (size_t)d.scratch; }
    if (d.burg) {
        L.burg_scratch = fake<double>(19); L.burg_window = fake<double>(20, d.burg == 2 ? 8 : 0);
        L.burg_f0 = 3; L.burg_nf = d.burg == 3 ? d.F : d.F - 7;
    }
    return true;
}

void run(const std::string &label, const launch_desc_t &d) {
    spectral_launch_t L;
    if (!make_launch(d, L)) return;
    // (the inputs of vbx_internal_analyze_choice, in its order)
    std::printf("call %s in=%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%ld,%d;%.17g,%.17g F=%ld plan=%d burg=%d\n", label.c_str(), d.n, d.kind, d.kmax, d.lpc, d.coeffs,
                d.nb(), d.b_lo(), d.interp, d.defer, d.allow_spec, d.lag_rcp, d.whole_curve, d.base8 ? 0 : 1, d.ld_odd, d.mode, d.n_lags, d.scratch, d.burg ? 1 : 0,
                d.sample_rate, d.fmin, d.F, L.plan, d.burg);
    std::fflush(stdout);
    int spec = 0; long batches = 0, per = 0;
    const char *what;
#ifdef ANALYZE_CHOICE_BEFORE
    long batching[2] = {0, 0};
    L.batching = batching;
    const int rc = launch_analyze(nullptr, L, &spec);
    what = rc < 0 ? "refused" : rc == 1 ? "split" : "fused";
    if (rc < 0) spec = 0;
    batches = batching[0]; per = batching[1];
#else
    analyze_choice_t c{};
    const int launches = launch_analyze(nullptr, L, &c);
    const bool split = !c.refused && c.per_launch > 0;
    what = c.refused ? "refused" : split ? "split" : "fused";
    spec = c.refused ? 0 : c.spec;
    if (split) { batches = launches; per = c.per_launch; }
#endif
    std::printf("  result %s spec=%d batches=%ld per=%ld\n", what, spec, batches, per);
}

std::string label_of(const launch_desc_t &d) {
    char b[256];
    std::snprintf(b, sizeof b, "n%d.k%d.kmax%d.lpc%d.mf%d.ip%d.df%d.sp%d.rcp%d.wc%d.b%d.m%d.ws%ld.burg%d", d.n, d.kind, d.kmax, d.lpc, d.coeffs, d.interp, d.defer,
                  d.allow_spec, d.lag_rcp, d.whole_curve, d.base8 ? 8 : 0, d.mode, d.scratch, d.burg);
    return b;
}

// scratch for the split form: too small (under 1024 frames, also where the curve is cut to half the frame) / several launches of the batch with a short last one
long scratch_small(int n) { return 64 + 500L * ((long)(n + 80) * 8 + 600); }
long scratch_some(int n) { return 64 + 1100L * ((long)(n + 80) * 8 + 600); }

void named() {
    auto d0 = [] { launch_desc_t d; d.lpc = 1; d.coeffs = 13; d.defer = 1; return d; };
    launch_desc_t d;
    run("headline_f64", d0());
    d = d0(); d.kind = 1; run("headline_pcm16", d);
    d = d0(); d.kind = 2; run("headline_f32", d);
    d = d0(); d.coeffs = 20; d.defer = 0; run("coeffs20_generic", d);
    d = d0(); d.allow_spec = 0; run("spec_switched_off", d);
    d = launch_desc_t{}; d.kmax = 1200 / 4 + 2; run("whole_vec_parked", d);
    d.base8 = 1; run("whole_vec_base8_lds", d);
    d = launch_desc_t{}; d.kmax = 65; run("kmax65_lds_list", d);
    d = d0(); d.n = 1103; d.interp = 1; d.defer = 0; d.sample_rate = 44100.0; run("n1103_interp", d);
    d = d0(); d.n = 1103; d.coeffs = 0; d.defer = 0; d.sample_rate = 44100.0; run("n1103_lpc", d);
    d = d0(); d.n = 1024; d.defer = 0; run("n1024", d);
    d = d0(); d.n = 512; d.defer = 0; run("n512", d);
    d = d0(); d.n = 600; d.defer = 1; run("n600_in_1200", d);
    d = d0(); d.n = 2048; d.defer = 0; run("n2048", d);
    d = d0(); d.n = 4096; d.defer = 0; d.F = 5000; d.scratch = scratch_some(4096); run("n4096_split", d);
    d.scratch = 0; run("n4096_fused_no_scratch", d);
    d.scratch = scratch_small(4096); run("n4096_fused_small_scratch", d);
    d = d0(); d.n = 3001; d.coeffs = 0; d.defer = 0; d.F = 5000; d.scratch = scratch_some(3001); run("n3001_odd_split", d);
    d = d0(); d.n = 3000; d.interp = 1; d.defer = 0; d.F = 5000; d.scratch = scratch_some(3000); run("n3000_interp_split", d);
    d = launch_desc_t{}; d.n = 2400; d.mode = 1; d.coeffs = 13; run("mfcc_only_2400_half", d);
    d = launch_desc_t{}; d.n = 4096; d.mode = 1; d.coeffs = 13; run("mfcc_only_4096_half", d);
    d = launch_desc_t{}; d.n = 1200; d.mode = 1; d.coeffs = 13; run("mfcc_only_1200", d);
    d = launch_desc_t{}; d.n = 1103; d.mode = 1; d.coeffs = 13; d.interp = 1; run("mfcc_only_1103_interp", d);
    d = launch_desc_t{}; d.n = 1200; d.mode = 2; d.n_lags = 1200; run("ac_only_1200", d);
    d = launch_desc_t{}; d.n = 3000; d.mode = 2; d.n_lags = 64; run("ac_only_3000", d);
    d = d0(); d.burg = 1; run("burg_f64", d);
    d = d0(); d.kind = 1; d.burg = 1; run("burg_pcm16", d);
    d = d0(); d.kind = 1; d.lpc = 0; d.burg = 1; run("burg_refused_pcm16_mfcc_no_lpc", d);
    d = d0(); d.coeffs = 20; d.defer = 0; d.burg = 1; run("burg_refused_generic", d);
    d = d0(); d.kind = 2; d.burg = 1; run("burg_refused_f32", d);
    d = d0(); d.n = 1024; d.kind = 1; d.defer = 0; run("pcm16_refused_not_1200", d);
}

void grid() {
    const int lengths[] = {64, 512, 600, 800, 1000, 1024, 1103, 1199, 1200, 1201, 2047, 2048, 2050, 3000, 4095, 4096};
    const int feats[][2] = {{0, 0}, {1, 0}, {0, 13}, {1, 13}, {1, 20}, {0, 20}};
    for (int n : lengths) {
        const int kmaxes[] = {1, 4, 15, 64, 65, n / 4 + 2};
        for (int kind = 0; kind < 3; kind++) {
            if (kind != 0 && n != 1200 && n != 1024) continue;      // (every other length: the same refusal)
            for (auto &ft : feats) for (int interp = 0; interp < 2; interp++) for (int defer = 0; defer < 2; defer++) {
                if ((interp || defer) && !ft[1]) continue;
                for (int kmax : kmaxes) for (int base8 = 0; base8 < 2; base8++) for (int flags = 0; flags < 8; flags++) {
                    const bool big = spectral_plan(n) == SPECTRAL_PLAN_4096;
                    for (int ws = 0; ws < (big ? 3 : 1); ws++) for (int burg = 0; burg < (n == 1200 ? 4 : 2); burg++) {
                        if (burg && (n != 1200 && n != 1024 && n != 1103)) continue;
                        launch_desc_t d;
                        d.n = n; d.kind = kind; d.lpc = ft[0]; d.coeffs = ft[1]; d.interp = interp; d.defer = defer; d.kmax = kmax; d.base8 = base8;
                        d.allow_spec = flags & 1; d.lag_rcp = (flags >> 1) & 1; d.whole_curve = (flags >> 2) & 1;
                        d.F = big ? 5000 : 67; d.scratch = ws == 0 ? 0 : ws == 1 ? scratch_small(n) : scratch_some(n);
                        d.burg = burg; d.sample_rate = (n == 1103) ? 44100.0 : 48000.0;
                        run(label_of(d), d);
                    }
                }
            }
        }
        for (int interp = 0; interp < 2; interp++) for (int coeffs : {13, 20}) {              // MFCC alone (+ the unpadded forms of 2 Nc samples)
            launch_desc_t d; d.n = n; d.mode = 1; d.coeffs = coeffs; d.interp = interp; run(label_of(d), d);
        }
        for (int n_lags : {64, n}) { launch_desc_t d; d.n = n; d.mode = 2; d.n_lags = n_lags; run(label_of(d), d); }      // autocorrelation alone
    }
    { launch_desc_t d; d.n = 2400; d.mode = 1; d.coeffs = 13; run(label_of(d), d); }
}

}  // namespace

int main(int argc, char **argv) {
    named();
    if (argc > 1 && std::string(argv[1]) == "--named") return 0;
    std::printf("grid\n");
    grid();
    return 0;
}
