// vbx_host.cpp -- every entry point of the ABI that is plain host arithmetic: the window / lag-window tables by the sample
// crate's recurrences, the mel bins, the builders of the device tables the context caches (vbx_table_cache.hpp), the work-size and
// frame-count formulas, and the geometry of a recording sharded over ranks (frame ranges, warm-up, gather transfer list).  No HIP here: the same file is built into libvoxbox_hip.so and, under
// -fsanitize=address,undefined, into a host-only library that tests/test_sanitizers.py drives with random arguments
// (tools/host_asan/Makefile).
#include "../../include/voxbox_hip.h"
#include "vbx_host.hpp"
#include "vbx_sample8.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

extern "C" int vbx_internal_fail(vbx_ctx *ctx, int code, const char *msg);   // vbx_api.hip (or the sanitizer build's stub)

namespace {
int fail(vbx_ctx *ctx, int code, const std::string &msg) { return vbx_internal_fail(ctx, code, msg.c_str()); }
}  // namespace

namespace vbx {

// sample 0.10 signal::Phase: yields phase, then phase = (phase + step) % 1.0
static void phase_ramp(std::vector<double> &ph, size_t n, double step) {
    ph.resize(n);
    double next = 0.0;
    for (size_t i = 0; i < n; i++) { ph[i] = next; next = std::fmod(next + step, 1.0); }
}

int window_table_host(int kind, size_t n, double *out) {
    const double pi2 = M_PI * 2.0;
    std::vector<double> ph;
    switch (kind) {
        case VBX_WINDOW_HANNING:            // Window::<Hanning>::new(n)
            phase_ramp(ph, n, 1.0 / ((double)n - 1.0));
            for (size_t i = 0; i < n; i++) out[i] = 0.5 * (1.0 - std::cos(ph[i] * pi2));
            return VBX_SUCCESS;
        case VBX_WINDOW_HANNING_LAG:        // HanningLag::at_phase, src/periodic.rs:239-247 (Q3)
            phase_ramp(ph, n, 1.0 / ((double)n - 1.0));
            for (size_t i = 0; i < n; i++) {
                const double v = ph[i] * pi2;
                out[i] = (1.0 - ph[i]) * (2.0 / 3.0 + (1.0 / 3.0) * std::cos(v)) + (1.0 / pi2) * std::sin(v);
            }
            return VBX_SUCCESS;
        case VBX_WINDOW_HANNING_PERIODIC: { // src/lib.rs:65-70
            const double len_inv = 1.0 / (double)n;
            for (size_t i = 0; i < n; i++) out[i] = 0.5 * (1.0 - std::cos(((double)i * len_inv) * pi2));
            return VBX_SUCCESS;
        }
        case VBX_WINDOW_RECTANGLE:
            for (size_t i = 0; i < n; i++) out[i] = 1.0;
            return VBX_SUCCESS;
    }
    return VBX_E_INVALID;
}

// src/spectrum.rs:411-414 (Q14)
void mel_bins_host(size_t n, size_t k, double lo, double hi, double sr, std::vector<int32_t> &bins, bool &overflow) {
    const double mlo = vbx_hz_to_mel(lo), mel_range = vbx_hz_to_mel(hi) - mlo;
    bins.resize(k + 2);
    overflow = false;
    for (size_t i = 0; i < k + 2; i++) {
        const double point = ((double)i / (double)k) * mel_range + mlo;
        const double b = std::floor((double)(n + 1) * vbx_mel_to_hz(point) / sr);
        if (!(b >= 0.0)) { bins[i] = 0; }
        else if (b > 1.0e9) { bins[i] = 1000000000; overflow = true; }
        else bins[i] = (int32_t)b;
    }
}

// ---- device tables, host side (vbx_host.hpp) ----

size_t window_dev_doubles(int kind, size_t n) { return (kind == VBX_WINDOW_HANNING_LAG) ? ((n + 1) & ~(size_t)1) + n : n; }

int window_dev_fill(int kind, size_t n, double *h, bool *rcp_usable) {
    *rcp_usable = false;
    if (window_table_host(kind, n, h) != VBX_SUCCESS) return VBX_E_INVALID;
    if (kind == VBX_WINDOW_HANNING_LAG) {
        const size_t off = (n + 1) & ~(size_t)1;
        bool usable = true;
        for (size_t i = 0; i < n; i++) {
            h[off + i] = 1.0 / h[i];
            usable = usable && std::isfinite(h[off + i]) && std::fabs(h[off + i]) < 1e290 && std::fabs(h[off + i]) > 1e-290;
        }
        *rcp_usable = usable;
    }
    return VBX_SUCCESS;
}

size_t goertzel_doubles(int nb) { return 2 * (size_t)(nb > 0 ? nb : 1); }

void goertzel_fill(size_t n, int b_lo, int nb, double *h) {
    for (int i = 0; i < nb; i++) {
        const double w = 2.0 * M_PI * (double)((size_t)(b_lo + i) % n) / (double)n;
        if (std::cos(w) > 0.0) { const double sh = std::sin(0.5 * w); h[2 * i] = 4.0 * sh * sh; h[2 * i + 1] = 1.0; }
        else { const double ch = std::cos(0.5 * w); h[2 * i] = 4.0 * ch * ch; h[2 * i + 1] = -1.0; }
    }
}

size_t dft2_ctab_doubles(int n1, int nc) { return (size_t)n1 * nc; }
size_t dft2_twid_doubles(size_t n) { return 2 * n; }

// evaluated in long double and rounded once
void dft2_fill(size_t n, int n1, int nc, double *hc, double *ht) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    const int ncos = n1 / 2 + 1;
    for (int i1 = 0; i1 < n1; i1++)
        for (int c = 0; c < n1; c++) {
            const int k1 = (c < ncos) ? c : c - ncos + 1;
            const long double ang = two_pi * (long double)((long)i1 * k1 % n1) / (long double)n1;
            hc[(size_t)i1 * nc + c] = (double)((c < ncos) ? cosl(ang) : sinl(ang));
        }
    for (size_t j = 0; j < n; j++) {
        const long double ang = two_pi * (long double)j / (long double)n;
        ht[2 * j] = (double)cosl(ang); ht[2 * j + 1] = (double)sinl(ang);
    }
}

void mfma_doubles(int n1, int mt, int ntd, int ntm, size_t doubles[4]) {
    const int n1p = (n1 + 3) & ~3, nc = 32 * ntd;
    doubles[0] = (size_t)n1p * nc;
    doubles[1] = (size_t)mt * ntd * 4 * 128 + 2;
    doubles[2] = (size_t)mt * ntm * 4 * 128 + 2;
    doubles[3] = (size_t)8 * mt * 64;
}

// evaluated in long double and rounded once
void mfma_fill(size_t n, int n1, int n2, int k2_plan, int mt, int ntd, int ntm, int src0, int src1,
               double *hc, double *hd, double *hm, double *hw) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    const int nc = 32 * ntd;
    for (int i1 = 0; i1 < n1; i1++)
        for (int c = 0; c < nc; c++) {
            const bool is_sin = c >= 16 * ntd;
            const int k1 = is_sin ? c - 16 * ntd : c;
            if (k1 >= n1) continue;
            const long double ang = two_pi * (long double)((long)i1 * k1 % n1) / (long double)n1;
            hc[(size_t)i1 * nc + c] = (double)(is_sin ? sinl(ang) : cosl(ang));
        }
    auto twiddle = [&](int i2, int k1, double *dst) {
        if (i2 >= n2 || k1 < 0 || k1 >= n1) { dst[0] = 0.0; dst[1] = 0.0; return; }
        const long double ang = two_pi * (long double)((long)i2 * k1 % (long)n) / (long double)n;
        dst[0] = (double)cosl(ang); dst[1] = (double)sinl(ang);
    };
    for (int m = 0; m < mt; m++)
        for (int r = 0; r < 4; r++)
            for (int l = 0; l < 64; l++) {
                const int i2 = 16 * m + 4 * r + (l >> 4), col = l & 15;
                for (int t = 0; t < ntd; t++)
                    twiddle(i2, 16 * t + col, &hd[((size_t)((m * ntd + t) * 4 + r) * 64 + l) * 2]);
                for (int t = 0; t < ntm; t++) {
                    const int kp = 16 * (t == 0 ? src0 : src1) + col;
                    twiddle(i2, (kp >= 1) ? n1 - kp : -1, &hm[((size_t)((m * ntm + t) * 4 + r) * 64 + l) * 2]);
                }
            }
    // stage-2 A operand: Wm[2 k2 + p][kk], kk = Re rows i2 (0 .. 16 mt) then Im rows; lane l of K-step s holds
    // Wm[l & 15][4 s + (l >> 4)]
    for (int s = 0; s < 8 * mt; s++)
        for (int l = 0; l < 64; l++) {
            const int rowm = l & 15, kk = 4 * s + (l >> 4);
            const bool im_half = kk >= 16 * mt;
            const int i2 = im_half ? kk - 16 * mt : kk, k2 = rowm >> 1, p = rowm & 1;
            if (i2 >= n2 || k2 >= k2_plan) continue;
            const long double ang = two_pi * (long double)((long)i2 * k2 % n2) / (long double)n2;
            const long double c = cosl(ang), sn = sinl(ang);
            // (Bre + i Bim)(c - i sn): Re = Bre c + Bim sn, Im = Bim c - Bre sn
            hw[(size_t)s * 64 + l] = (double)(p == 0 ? (im_half ? sn : c) : (im_half ? c : -sn));
        }
}

size_t dct_doubles(size_t k) { return k * k; }

void dct_fill(size_t k, double *h) {
    for (size_t kk = 0; kk < k; kk++)          // src/spectrum.rs:395
        for (size_t n = 0; n < k; n++)
            h[kk * k + n] = std::cos(M_PI * (double)kk * (2. * (double)n + 1.) / (2. * (double)k));
}

size_t slopes_doubles(const int32_t *hb, size_t k) { const int nb = hb[k + 1] - hb[0]; return 2 * (size_t)(nb > 0 ? nb : 1); }

// one IEEE division each, as in the reference (Q14: the "falling" side rises too)
void slopes_fill(const int32_t *hb, size_t k, double *h) {
    const int b_lo = hb[0];
    for (size_t w = 0; w < k; w++) {
        const int up = hb[w + 1] - hb[w], down = hb[w + 2] - hb[w + 1];
        for (int i = 0; i < up; i++) h[2 * (size_t)(hb[w] + i - b_lo)] = (double)i / (double)up;
        for (int i = 0; i < down; i++) h[2 * (size_t)(hb[w + 1] + i - b_lo) + 1] = (double)i / (double)down;
    }
}

// sample 0.10 Converter: interpolation_value starts at 0, grows by 1/ratio per output, and every whole
// unit advances the (left, right) pair by one source sample; left starts at source index 0
void resample_fill(size_t m, double resample_ratio, int32_t *hi, double *hf) {
    double value = 0.0;
    const double step = 1.0 / resample_ratio;
    long left = 0;
    for (size_t k = 0; k < m; k++) {
        while (value >= 1.0) { left++; value -= 1.0; }
        hi[k] = (left > 0x3fffffff) ? 0x3fffffff : (int32_t)left;
        hf[k] = value;
        value += step;
    }
}

}  // namespace vbx

using namespace vbx;

extern "C" {

int vbx_window_table_f64(int kind, size_t n, double *h_out) {
    if (!h_out || n < 1) return fail(nullptr, VBX_E_INVALID, "vbx_window_table_f64: bad argument");
    int rc = window_table_host(kind, n, h_out);
    if (rc != VBX_SUCCESS) return fail(nullptr, rc, "vbx_window_table_f64: unknown window kind");
    return rc;
}

size_t vbx_frame_count(size_t n_samples, size_t frame_len, size_t hop) {
    if (frame_len == 0 || hop == 0 || n_samples < frame_len) return 0;
    return (n_samples - frame_len) / hop + 1;
}

double vbx_hz_to_mel(double hz) { return 1125. * std::log1p(hz / 700.); }       // src/spectrum.rs:375-377
double vbx_mel_to_hz(double mel) { return 700. * (std::exp(mel / 1125.) - 1.); } // src/spectrum.rs:379-381
size_t vbx_find_formants_real_work_size(size_t buf_len, size_t n_coeffs) { return buf_len * 2 + n_coeffs * 23 + 2; }
size_t vbx_find_formants_complex_work_size(size_t n_coeffs) { return n_coeffs * 7 + 4; }

// The mel filter bank's bins (src/spectrum.rs:411-414: K + 2 mel points, floor((N + 1) hz / sr), Q14).  Returns 1 when the
// reference would panic on every frame of this geometry (a bin beyond the spectrum, or descending bins: usize underflow).
int vbx_mfcc_bins(size_t frame_len, size_t num_coeffs, double lo_hz, double hi_hz, double sample_rate, int32_t *h_bins) {
    if (!h_bins || frame_len < 1 || num_coeffs < 1) return fail(nullptr, VBX_E_INVALID, "vbx_mfcc_bins: bad argument");
    std::vector<int32_t> b; bool bad = false;
    mel_bins_host(frame_len, num_coeffs, lo_hz, hi_hz, sample_rate, b, bad);
    for (size_t i = 0; i + 1 < b.size(); i++) if (b[i + 1] < b[i]) bad = true;
    if (b.back() > (int32_t)(frame_len < 0x7fffffff ? frame_len : 0x7fffffff)) bad = true;
    std::memcpy(h_bins, b.data(), b.size() * sizeof(int32_t));
    return bad ? 1 : VBX_SUCCESS;
}

int vbx_window_table_f32(int kind, size_t n, float *h_out) {
    if (!h_out || n == 0) return fail(nullptr, VBX_E_INVALID, "vbx_window_table_f32: bad argument");
    std::vector<double> t(n);
    int rc = vbx_window_table_f64(kind, n, t.data());
    if (rc != VBX_SUCCESS) return rc;
    for (size_t i = 0; i < n; i++) h_out[i] = (float)t[i];
    return VBX_SUCCESS;
}

// Host only: the builders of the device tables (vbx_host.hpp) for tests and the sanitizer build.  kind: HOST_TABLE_*; ip / dp: its
// integer / double parameters --
//   WINDOW {window kind, n}   LAG_F32 {n}   GOERTZEL {n, b_lo, nb}   DFT2 {n, n1, nc}   DCT {k}   SLOPES {k, bins[0 .. k + 2)}
//   MFMA {n, n1, n2, k2, mt, ntd, ntm, src0, src1}   RESAMPLE {m}, dp {ratio}
// sub_bytes[4]: bytes of each sub-table (0: none); in buf each starts on the next multiple of 16 bytes after the one before, and what
// the packing rules call padding stays zero.
// *flags: bit 0 = the lag window's reciprocals are usable.  buf == nullptr: the sizes only.  VBX_E_INVALID: a parameter outside
// what the library itself would pass, or cap too small.
int vbx_internal_host_table(int kind, const int64_t *ip, const double *dp, size_t *sub_bytes, void *buf, size_t cap, int32_t *flags) {
    if (!ip || !sub_bytes || !flags) return VBX_E_INVALID;
    const int64_t big = 1 << 20;
    auto in = [&](int i, int64_t lo, int64_t hi) { return ip[i] >= lo && ip[i] <= hi; };
    size_t sz[4] = {0, 0, 0, 0};
    double *b[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = VBX_SUCCESS;
    *flags = 0;
    auto place = [&]() {                       // the sizes are known: report them; true: the caller wants the tables, b[] says where
        size_t total = 0, off[4];
        for (int i = 0; i < 4; i++) { sub_bytes[i] = sz[i]; off[i] = total; total += (sz[i] + 15) & ~(size_t)15; }
        if (buf && cap < total) rc = VBX_E_INVALID;
        if (!buf || cap < total) return false;
        std::memset(buf, 0, total);
        for (int i = 0; i < 4; i++) b[i] = reinterpret_cast<double *>(static_cast<char *>(buf) + off[i]);
        return true;
    };
    const size_t n = (size_t)ip[0];
    switch (kind) {
        case HOST_TABLE_WINDOW: {
            if (!(in(0, 0, 3) && in(1, 1, big))) return VBX_E_INVALID;
            bool usable = false;
            sz[0] = window_dev_doubles((int)ip[0], (size_t)ip[1]) * sizeof(double);
            if (place()) { rc = window_dev_fill((int)ip[0], (size_t)ip[1], b[0], &usable); *flags = usable ? 1 : 0; }
            return rc;
        }
        case HOST_TABLE_LAG_F32:
            if (!in(0, 1, big)) return VBX_E_INVALID;
            sz[0] = n * sizeof(float);
            if (place()) rc = vbx_window_table_f32(VBX_WINDOW_HANNING_LAG, n, reinterpret_cast<float *>(b[0]));
            return rc;
        case HOST_TABLE_GOERTZEL:
            if (!(in(0, 1, big) && in(1, 0, big) && in(2, 0, big))) return VBX_E_INVALID;
            sz[0] = goertzel_doubles((int)ip[2]) * sizeof(double);
            if (place()) goertzel_fill(n, (int)ip[1], (int)ip[2], b[0]);
            return rc;
        case HOST_TABLE_DFT2:
            if (!(in(0, 1, big) && in(1, 1, 128) && ip[0] % ip[1] == 0 && in(2, ip[1], 128))) return VBX_E_INVALID;
            sz[0] = dft2_ctab_doubles((int)ip[1], (int)ip[2]) * sizeof(double); sz[1] = dft2_twid_doubles(n) * sizeof(double);
            if (place()) dft2_fill(n, (int)ip[1], (int)ip[2], b[0], b[1]);
            return rc;
        case HOST_TABLE_MFMA:
            if (!(in(1, 4, 63) && in(2, 2, 64) && ip[0] == ip[1] * ip[2] && in(3, 1, 8) && ip[4] == (ip[2] + 15) / 16 && in(5, 1, 2) && in(6, 0, 2) &&
                  in(7, 0, 3) && in(8, 0, 3))) return VBX_E_INVALID;
            mfma_doubles((int)ip[1], (int)ip[4], (int)ip[5], (int)ip[6], sz);
            for (size_t &x : sz) x *= sizeof(double);
            if (place()) mfma_fill(n, (int)ip[1], (int)ip[2], (int)ip[3], (int)ip[4], (int)ip[5], (int)ip[6], (int)ip[7], (int)ip[8], b[0], b[1], b[2], b[3]);
            return rc;
        case HOST_TABLE_DCT:
            if (!in(0, 1, 64)) return VBX_E_INVALID;
            sz[0] = dct_doubles(n) * sizeof(double);
            if (place()) dct_fill(n, b[0]);
            return rc;
        case HOST_TABLE_SLOPES: {
            if (!(in(0, 1, 64) && in(1, 0, big))) return VBX_E_INVALID;
            for (size_t i = 1; i <= n + 1; i++) if (ip[i + 1] < ip[i] || ip[i + 1] > big) return VBX_E_INVALID;
            const std::vector<int32_t> bins(ip + 1, ip + n + 3);
            sz[0] = slopes_doubles(bins.data(), n) * sizeof(double);
            if (place()) slopes_fill(bins.data(), n, b[0]);
            return rc;
        }
        case HOST_TABLE_RESAMPLE:
            if (!(dp && in(0, 1, 0x3fffffff) && dp[0] > 0.0 && dp[0] <= 64.0)) return VBX_E_INVALID;
            sz[0] = n * sizeof(int32_t); sz[1] = n * sizeof(double);
            if (place()) resample_fill(n, dp[0], reinterpret_cast<int32_t *>(b[0]), b[1]);
            return rc;
    }
    return VBX_E_INVALID;
}

size_t vbx_degree_c64(const vbx_complex *h_poly, size_t len) {          // src/polynomial.rs:26-28
    if (!h_poly) return 0;
    for (size_t i = len; i-- > 0;) if (!(h_poly[i].re == 0.0 && h_poly[i].im == 0.0)) return i;
    return 0;
}
size_t vbx_off_low_c64(const vbx_complex *h_poly, size_t len) {         // src/polynomial.rs:30-32
    if (!h_poly) return 0;
    for (size_t i = 0; i < len; i++) if (!(h_poly[i].re == 0.0 && h_poly[i].im == 0.0)) return i;
    return 0;
}

size_t vbx_resampled_len(size_t frame_len, double resample_ratio) {
    return (size_t)std::ceil(resample_ratio * (double)frame_len);          // src/lib.rs:42
}

size_t vbx_record_doubles(const vbx_analysis_params *h_p) {
    if (!h_p) return 0;
    size_t n = 2;                                                   // Pitch { frequency, strength }
    if (h_p->formant_order) n += 2 * h_p->n_est;                    // Resonance { frequency, bandwidth } x n_est
    if (h_p->mfcc_coeffs) n += h_p->mfcc_coeffs;
    if (h_p->lpc_order) n += h_p->lpc_order + 1;
    return n;
}

size_t vbx_record_doubles_ex(const vbx_analysis_params *h_p, const vbx_analysis_ext *h_ext) {
    if (!h_p) return 0;
    return vbx_record_doubles(h_p) + ((h_ext && h_ext->rms) ? 1 : 0);     // RMS: the LAST column
}

int vbx_gather_plan(const int64_t *h_rows, int world, int rank, int dst, size_t row_doubles,
                    int64_t *h_offset, int64_t *h_count, int32_t *h_op) {
    if (!h_rows || world < 1 || rank < 0 || rank >= world || dst < 0 || dst >= world || row_doubles < 1)
        return fail(nullptr, VBX_E_INVALID, "vbx_gather_plan: bad argument");
    int64_t off = 0;
    for (int r = 0; r < world; r++) {
        if (h_rows[r] < 0) return fail(nullptr, VBX_E_INVALID, "vbx_gather_plan: negative row count");
        const int64_t cnt = h_rows[r] * (int64_t)row_doubles;
        if (h_offset) h_offset[r] = off;
        if (h_count) h_count[r] = cnt;
        if (h_op) {
            int32_t op = VBX_GATHER_NONE;
            if (rank == dst) { if (cnt > 0) op = (r == dst) ? VBX_GATHER_COPY : VBX_GATHER_RECV; }
            else if (r == dst && h_rows[rank] > 0) op = VBX_GATHER_SEND;       // whatever dst itself contributes
            h_op[r] = op;
        }
        off += cnt;
    }
    return VBX_SUCCESS;
}

// last utterance start <= f (0 without a segment list)
static size_t seg_start_of(const int64_t *h_seg_start, size_t n_segments, size_t f) {
    size_t best = 0;
    if (h_seg_start) for (size_t i = 0; i < n_segments; i++) { if ((size_t)h_seg_start[i] <= f) best = (size_t)h_seg_start[i]; else break; }
    return best;
}
// first utterance start > f, or n_frames
static size_t seg_start_after(const int64_t *h_seg_start, size_t n_segments, size_t f, size_t n_frames) {
    if (h_seg_start) for (size_t i = 0; i < n_segments; i++) if ((size_t)h_seg_start[i] > f) return (size_t)h_seg_start[i] < n_frames ? (size_t)h_seg_start[i] : n_frames;
    return n_frames;
}

int vbx_shard_range(size_t n_frames, int world, int rank, const int64_t *h_seg_start, size_t n_segments,
                    size_t *lo, size_t *hi) {
    if (!lo || !hi || world < 1 || rank < 0 || rank >= world) return fail(nullptr, VBX_E_INVALID, "vbx_shard_range: bad argument");
    auto even_hi = [&](int r) {                      // end of rank r under the plain even split
        const size_t base = n_frames / (size_t)world, rem = n_frames % (size_t)world;
        return (size_t)(r + 1) * base + ((size_t)(r + 1) < rem ? (size_t)(r + 1) : rem);
    };
    // The even cut, unless an utterance starts within 1/32 of a shard after it: a rank that begins where an utterance
    // begins needs nothing from its predecessor.  A cut INSIDE an utterance is fine too -- the track is carried across
    // it (vbx_shard_plan, vbx_comm_stitch_tracks_f64) -- so one long utterance splits evenly.
    const size_t slack = n_frames / (size_t)world / 32;
    auto cut = [&](int r) -> size_t {
        if (r < 0) return 0;
        if (r >= world - 1) return n_frames;
        const size_t target = even_hi(r);
        if (!h_seg_start || n_segments == 0) return target;
        for (size_t i = 0; i < n_segments; i++) {    // first boundary >= target
            const size_t b = (size_t)h_seg_start[i];
            if (b >= target) return (b <= target + slack && b <= n_frames) ? b : target;
        }
        return target;
    };
    size_t a = cut(rank - 1), b = cut(rank);
    if (b < a) b = a;
    *lo = a; *hi = b;
    return VBX_SUCCESS;
}

int vbx_shard_plan(size_t n_frames, int world, int rank, const int64_t *h_seg_start, size_t n_segments, vbx_shard_plan_t *out) {
    if (!out) return fail(nullptr, VBX_E_INVALID, "vbx_shard_plan: null output");
    if (h_seg_start && n_segments > 0) {
        if (h_seg_start[0] != 0) return fail(nullptr, VBX_E_INVALID, "vbx_shard_plan: seg_start[0] must be 0");
        for (size_t i = 1; i < n_segments; i++)
            if (h_seg_start[i] < h_seg_start[i - 1]) return fail(nullptr, VBX_E_INVALID, "vbx_shard_plan: seg_start must ascend");
    }
    size_t lo = 0, hi = 0;
    int rc = vbx_shard_range(n_frames, world, rank, h_seg_start, n_segments, &lo, &hi);
    if (rc != VBX_SUCCESS) return rc;
    // does the utterance that holds frame `c` reach back further than a warm-up can cover exactly?
    auto continued = [&](size_t c) { return c > 0 && c < n_frames && c - seg_start_of(h_seg_start, n_segments, c) > (size_t)VBX_SHARD_WARM_FRAMES; };
    out->lo = lo; out->hi = hi;
    out->warm = 0; out->stop = 0; out->continues_prev = 0; out->continues_next = 0;
    if (hi <= lo) return VBX_SUCCESS;                // an empty shard (more ranks than frames): nothing to do, nothing to pass on
    const size_t back = lo - seg_start_of(h_seg_start, n_segments, lo);
    out->warm = back < (size_t)VBX_SHARD_WARM_FRAMES ? back : (size_t)VBX_SHARD_WARM_FRAMES;
    out->continues_prev = continued(lo) ? 1 : 0;
    out->continues_next = continued(hi) ? 1 : 0;
    const size_t next = seg_start_after(h_seg_start, n_segments, lo, n_frames);
    out->stop = ((next < hi) ? next : hi) - (lo - out->warm);
    return VBX_SUCCESS;
}

int vbx_shard_local_segments(const vbx_shard_plan_t *h_plan, const int64_t *h_seg_start, size_t n_segments,
                             int64_t *h_out, size_t cap, size_t *n_out) {
    if (!h_plan || !n_out) return fail(nullptr, VBX_E_INVALID, "vbx_shard_local_segments: null argument");
    const size_t first = h_plan->lo - h_plan->warm;
    size_t n = 0;
    if (h_out && n < cap) h_out[n] = 0;
    n++;
    if (h_seg_start) for (size_t i = 0; i < n_segments; i++) {
        const size_t b = (size_t)h_seg_start[i];
        if (b > first && b < h_plan->hi) { if (h_out && n < cap) h_out[n] = (int64_t)(b - first); n++; }
    }
    *n_out = n;
    if (h_out && n > cap) return fail(nullptr, VBX_E_INVALID, "vbx_shard_local_segments: output too small");
    return VBX_SUCCESS;
}

int vbx_shard_samples(size_t lo, size_t hi, size_t frame_len, size_t hop, size_t *s0, size_t *s1) {
    if (!s0 || !s1 || frame_len < 1 || hop < 1) return fail(nullptr, VBX_E_INVALID, "vbx_shard_samples: bad argument");
    *s0 = lo * hop;
    *s1 = (hi <= lo) ? lo * hop : (hi - 1) * hop + frame_len;     // includes the frame_len - hop halo
    return VBX_SUCCESS;
}

// Chunk c of a host-resident recording (vbx_analyze_host): the shard plan's arithmetic on cuts every chunk_frames frames.  Unlike
// vbx_shard_plan, continues_prev is set for EVERY cut inside an utterance, a short warm-up included: the previous chunk's rows are at
// hand on the same device, so the stitch always runs there (and finds nothing to redo when the warm-up began at the utterance's start).
int vbx_host_chunk_plan(size_t n_frames, size_t chunk_frames, size_t c, size_t frame_len, size_t stride,
                        const int64_t *h_seg_start, size_t n_segments, vbx_shard_plan_t *out, size_t *s0, size_t *s1) {
    if (!out || !s0 || !s1 || chunk_frames < 1 || frame_len < 1 || stride < 1) return fail(nullptr, VBX_E_INVALID, "vbx_host_chunk_plan: bad argument");
    if (h_seg_start && n_segments > 0) {
        if (h_seg_start[0] != 0) return fail(nullptr, VBX_E_INVALID, "vbx_host_chunk_plan: seg_start[0] must be 0");
        for (size_t i = 1; i < n_segments; i++)
            if (h_seg_start[i] < h_seg_start[i - 1]) return fail(nullptr, VBX_E_INVALID, "vbx_host_chunk_plan: seg_start must ascend");
    }
    if (c >= n_frames / chunk_frames + (n_frames % chunk_frames != 0)) return fail(nullptr, VBX_E_INVALID, "vbx_host_chunk_plan: no such chunk");
    const size_t lo = c * chunk_frames, hi = (n_frames - lo > chunk_frames) ? lo + chunk_frames : n_frames;
    auto inside = [&](size_t f) { return f > 0 && f < n_frames && seg_start_of(h_seg_start, n_segments, f) != f; };
    const size_t back = lo - seg_start_of(h_seg_start, n_segments, lo);
    out->lo = lo; out->hi = hi;
    out->warm = back < (size_t)VBX_SHARD_WARM_FRAMES ? back : (size_t)VBX_SHARD_WARM_FRAMES;
    out->continues_prev = inside(lo) ? 1 : 0;
    out->continues_next = inside(hi) ? 1 : 0;
    const size_t next = seg_start_after(h_seg_start, n_segments, lo, n_frames);
    out->stop = ((next < hi) ? next : hi) - (lo - out->warm);
    return vbx_shard_samples(lo - out->warm, hi, frame_len, stride, s0, s1);
}

// One push of a live session (vbx_session_push): the frames it completes, the warm-up before them, and what the carry must hold.
// The analysed range [lo - warm, hi) never reaches before utt_frame, so it lies in ONE utterance; keep_from is the earliest sample
// frame any later push can read (its lo is this hi, its warm-up at most WARM frames and never before utt_frame).
int vbx_session_plan(size_t consumed, size_t utt_frame, size_t n_new, size_t frame_len, size_t stride, vbx_session_plan_t *out) {
    if (!out || frame_len < 1 || stride < 1) return fail(nullptr, VBX_E_INVALID, "vbx_session_plan: bad argument");
    if (consumed + n_new < consumed) return fail(nullptr, VBX_E_INVALID, "vbx_session_plan: consumed + n_new overflows");
    const size_t W = (size_t)VBX_SHARD_WARM_FRAMES;
    const size_t lo = vbx_frame_count(consumed, frame_len, stride), hi = vbx_frame_count(consumed + n_new, frame_len, stride);
    if (utt_frame > lo) return fail(nullptr, VBX_E_INVALID, "vbx_session_plan: utt_frame lies beyond the frames consumed");
    out->lo = lo; out->hi = hi;
    out->warm = hi > lo ? (lo - utt_frame < W ? lo - utt_frame : W) : 0;
    out->continues_prev = (lo > utt_frame && hi > lo) ? 1 : 0;
    out->read_from = (lo - out->warm) * stride;
    const size_t back = hi - utt_frame < W ? hi - utt_frame : W;
    const size_t from = (hi - back) * stride;
    out->keep_from = from < consumed + n_new ? from : consumed + n_new;
    return VBX_SUCCESS;
}

// One push of a multi-channel session (vbx_session_push_channels): vbx_session_plan's arithmetic -- every channel shares it -- and
// the layout of the n_sel planes the one frame-loop call runs over.  A plane holds what the one-channel session's carry holds after
// the push: `len` elements from sample frame `base`.  Its pitch is a whole number of hops, plane_frames, so that frame
// k * plane_frames + j of the call is frame j of plane k; it covers the plane's elements and is rounded up until every plane base is a
// multiple of 256 bytes.
int vbx_session_channels_plan(size_t consumed, size_t utt_frame, size_t n_new, size_t frame_len, size_t stride, size_t elem_bytes,
                              size_t n_sel, vbx_session_channels_plan_t *out, int64_t *h_seg_start) {
    if (!out) return fail(nullptr, VBX_E_INVALID, "vbx_session_channels_plan: bad argument");
    if (!(elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8) || n_sel < 1 || n_sel > (size_t)VBX_HOST_MAX_CHANNELS)
        return fail(nullptr, VBX_E_INVALID, "vbx_session_channels_plan: elem_bytes must be 2, 4 or 8 and n_sel in [1, 64]");
    int rc = vbx_session_plan(consumed, utt_frame, n_new, frame_len, stride, &out->push);
    if (rc != VBX_SUCCESS) return fail(nullptr, rc, "vbx_session_channels_plan: bad argument");
    if (stride > ((size_t)1 << 40) || n_new > ((size_t)1 << 48) || frame_len > ((size_t)1 << 40))
        return fail(nullptr, VBX_E_INVALID, "vbx_session_channels_plan: n_new, frame_len or stride too large");
    const vbx_session_plan_t &p = out->push;
    const size_t nf = p.hi - p.lo, end = consumed + n_new;
    out->frames = nf ? p.warm + nf : 0;
    out->base = nf ? p.read_from : p.keep_from;           // (<= end: the last frame delivered ends inside the block)
    out->keep = out->base < consumed ? consumed - out->base : 0;
    out->len = end - out->base;
    size_t align = 256;                                   // plane_frames * stride * elem_bytes must be a multiple of 256
    const size_t hop_bytes = ((stride % 256) * elem_bytes) % 256;
    for (size_t g = 256; g >= 1; g /= 2) if (hop_bytes % g == 0) { align = 256 / g; break; }
    size_t q = out->len / stride + (out->len % stride != 0);
    if (q < 1) q = 1;
    q = (q + align - 1) / align * align;
    out->plane_frames = q;
    out->plane_ld = q * stride;
    out->call_frames = out->frames ? (n_sel - 1) * q + out->frames : 0;
    out->capacity = out->plane_ld;
    if (h_seg_start) for (size_t k = 0; k < n_sel; k++) h_seg_start[k] = (int64_t)(k * q);
    return VBX_SUCCESS;
}

// One tick of a session pool (vbx_pool_push): vbx_session_plan's arithmetic per entry -- every slot has its own timeline -- the
// entries' rows in the tick's outputs, and the layout of the one plane the tick's frame-loop call runs over.  An entry with frames
// analyses m = warm + n_rows of them from its stream's sample read_from on: a region of span = (m - 1) * stride + frame_len
// elements at element plane_frame * stride.  The next entry with frames starts ceil(span / stride) frames behind it (vbx_clips_plan's
// rule), so the gap between two regions is shorter than one hop and every frame of [plane_frame, plane_frame + m) reads its own
// entry's samples only.
int vbx_pool_plan(const size_t *h_consumed, const size_t *h_utt_frame, const size_t *h_n_new, size_t n_entries, size_t frame_len,
                  size_t stride, vbx_pool_plan_row *h_rows, size_t *h_total_rows, size_t *h_call_frames) {
    if (h_total_rows) *h_total_rows = 0;
    if (h_call_frames) *h_call_frames = 0;
    if (frame_len < 1 || stride < 1) return fail(nullptr, VBX_E_INVALID, "vbx_pool_plan: frame_len and stride must be >= 1");
    if (n_entries > 0 && (!h_consumed || !h_utt_frame || !h_n_new || !h_rows)) return fail(nullptr, VBX_E_INVALID, "vbx_pool_plan: null array");
    if (stride > ((size_t)1 << 40) || frame_len > ((size_t)1 << 40)) return fail(nullptr, VBX_E_INVALID, "vbx_pool_plan: frame_len or stride too large");
    // first: nothing is written for a tick that is refused
    size_t total = 0, next = 0, call = 0;
    for (size_t i = 0; i < n_entries; i++) {
        vbx_session_plan_t p{};
        if (h_n_new[i] > ((size_t)1 << 48)) return fail(nullptr, VBX_E_INVALID, "vbx_pool_plan: n_new too large");
        int rc = vbx_session_plan(h_consumed[i], h_utt_frame[i], h_n_new[i], frame_len, stride, &p);
        if (rc != VBX_SUCCESS) return fail(nullptr, rc, "vbx_pool_plan: bad entry (vbx_session_plan refuses it)");
        const size_t nf = p.hi - p.lo;
        if (nf == 0) continue;
        const size_t m = p.warm + nf, span = (m - 1) * stride + frame_len;
        if (nf > 0x7fffffffull - total || next + m > 0x7fffffffull) return fail(nullptr, VBX_E_INVALID, "vbx_pool_plan: more than 0x7fffffff frames in one call");
        total += nf;
        call = next + m;
        next += span / stride + (span % stride != 0);
    }
    size_t row = 0;
    next = 0;
    for (size_t i = 0; i < n_entries; i++) {
        vbx_pool_plan_row &r = h_rows[i];
        vbx_session_plan(h_consumed[i], h_utt_frame[i], h_n_new[i], frame_len, stride, &r.plan);
        const size_t nf = r.plan.hi - r.plan.lo;
        r.row_start = (int64_t)row; r.n_rows = (int64_t)nf; r.frames = 0; r.plane_frame = -1;
        if (nf == 0) continue;
        const size_t m = r.plan.warm + nf, span = (m - 1) * stride + frame_len;
        r.frames = (int64_t)m; r.plane_frame = (int64_t)next;
        next += span / stride + (span % stride != 0);
        row += nf;
    }
    if (h_total_rows) *h_total_rows = total;
    if (h_call_frames) *h_call_frames = call;
    return VBX_SUCCESS;
}

// The rows one slot's area of a bound pool's contour arrays needs (vbx_pool_path_bind): a tick's path launch never writes more for a
// slot than the frames it held pending, at most max_pending, plus the frames its block completes, at most ceil(n / stride) for a
// block of n samples.  0: stride == 0, or the sum does not fit.
size_t vbx_pool_path_slot_rows(size_t max_pending, size_t max_block_sample_frames, size_t stride) {
    if (stride == 0) return 0;
    const size_t done = max_block_sample_frames / stride + (max_block_sample_frames % stride != 0);
    return (max_pending > SIZE_MAX - done) ? 0 : max_pending + done;
}

// A batch of clips (vbx_analyze_clips): each clip's rows in the outputs, the group that analyses it and where it lies in that
// group's packed plane.  Groups are greedy runs of whole clips in order.  Inside a group clip b's sample 0 lies at element
// plane_frame_b * stride; the next clip with frames starts ceil(len_b / stride) frames behind it, so the gap between them is shorter
// than one hop and every frame of [plane_frame_b, plane_frame_b + n_rows_b) reads clip b's own samples only.  Frames longer than
// VBX_MAX_FRAME_LEN: every clip is a group by itself -- the long-frame kernels (k_long.hip) choose how they split a frame's sums
// from the frame count of the call, so only a call of the clip's own frame count gives the resident call's bits.
// the 256 values of a G.711 law, by the function the reader kernels run (vbx_sample8.hpp)
int vbx_g711_table(int format, int16_t *h_out) {
    if (format != VBX_SAMPLE_ULAW && format != VBX_SAMPLE_ALAW) return fail(nullptr, VBX_E_INVALID, "vbx_g711_table: format must be VBX_SAMPLE_ULAW or VBX_SAMPLE_ALAW");
    if (!h_out) return fail(nullptr, VBX_E_INVALID, "vbx_g711_table: null output");
    for (uint32_t b = 0; b < 256; b++) h_out[b] = format == VBX_SAMPLE_ULAW ? vbx::ulaw_value(b) : vbx::alaw_value(b);
    return VBX_SUCCESS;
}

int vbx_clips_plan(const size_t *h_len, size_t n_clips, size_t frame_len, size_t stride, size_t group_frames, vbx_clip_row *h_rows,
                   size_t *h_total_rows, size_t *h_n_groups) {
    if (h_total_rows) *h_total_rows = 0;
    if (h_n_groups) *h_n_groups = 0;
    if (frame_len < 1 || stride < 1) return fail(nullptr, VBX_E_INVALID, "vbx_clips_plan: frame_len and stride must be >= 1");
    if (n_clips > 0 && (!h_len || !h_rows)) return fail(nullptr, VBX_E_INVALID, "vbx_clips_plan: null array");
    if (group_frames != 0 && group_frames < (size_t)VBX_CLIPS_MIN_GROUP_FRAMES)
        return fail(nullptr, VBX_E_INVALID, "vbx_clips_plan: group_frames must be 0 or >= VBX_CLIPS_MIN_GROUP_FRAMES");
    size_t gf = group_frames;
    if (gf == 0) {                                        // the default: an f64 plane of at most VBX_CLIPS_PLANE_BYTES
        gf = (size_t)VBX_CLIPS_PLANE_BYTES / sizeof(double) / stride;
        if (gf > (size_t)VBX_HOST_DEFAULT_CHUNK_FRAMES) gf = (size_t)VBX_HOST_DEFAULT_CHUNK_FRAMES;
        if (gf < (size_t)VBX_CLIPS_MIN_GROUP_FRAMES) gf = (size_t)VBX_CLIPS_MIN_GROUP_FRAMES;
    }
    if (gf > 0x7fffffffull) gf = 0x7fffffffull;           // (a group is one frame-loop call)
    size_t total = 0;
    for (size_t b = 0; b < n_clips; b++) {                // first: nothing is written for a batch that is refused
        const size_t n = vbx_frame_count(h_len[b], frame_len, stride);
        if (n > 0x7fffffffull - total) return fail(nullptr, VBX_E_INVALID, "vbx_clips_plan: more than 0x7fffffff rows");
        total += n;
    }
    const bool alone = frame_len > (size_t)VBX_MAX_FRAME_LEN;
    size_t row = 0, groups = 0, next = 0;                 // next: the plane frame the next clip of the open group would start at
    for (size_t b = 0; b < n_clips; b++) {
        const size_t n = vbx_frame_count(h_len[b], frame_len, stride);
        vbx_clip_row &r = h_rows[b];
        r.row_start = (int64_t)row; r.n_rows = (int64_t)n; r.group = -1; r.plane_frame = 0;
        if (n == 0) continue;
        if (groups == 0 || alone || next + n > gf) { groups++; next = 0; }      // (a clip larger than gf on its own: a group by itself)
        r.group = (int64_t)(groups - 1); r.plane_frame = (int64_t)next;
        next += h_len[b] / stride + (h_len[b] % stride != 0);
        row += n;
    }
    if (h_total_rows) *h_total_rows = total;
    if (h_n_groups) *h_n_groups = groups;
    return VBX_SUCCESS;
}

}  // extern "C"

namespace vbx {

size_t session_carry_samples(size_t frame_len, size_t stride, size_t max_block) {
    return ((size_t)VBX_SHARD_WARM_FRAMES + 1) * stride + frame_len + max_block;
}

size_t session_max_frames(size_t stride, size_t max_block) { return max_block / stride + 1 + (size_t)VBX_SHARD_WARM_FRAMES; }

// keep_from >= (hi - WARM) * stride and consumed + n_new < hi * stride + frame_len (vbx_session_plan): the tail is shorter than
// WARM hops and a frame
size_t pool_carry_samples(size_t frame_len, size_t stride) { return (size_t)VBX_SHARD_WARM_FRAMES * stride + frame_len - 1; }

// An entry of n samples analyses m <= WARM + n / stride + 1 frames and takes m - 1 + ceil(frame_len / stride) frames of the plane
// (the last one: m, which is no more); at most min(max_streams, max_tick) entries hold a sample, their lengths sum to max_tick.
size_t pool_max_call_frames(size_t frame_len, size_t stride, size_t max_streams, size_t max_tick) {
    const size_t e = max_streams < max_tick ? max_streams : max_tick;
    return e * ((size_t)VBX_SHARD_WARM_FRAMES + frame_len / stride + (frame_len % stride != 0)) + max_tick / stride;
}

void launch_ranges_host(const int64_t *seg_start, size_t n_seg, size_t n_frames, size_t launch_frames,
                        std::vector<int64_t> &seg, std::vector<size_t> &off, std::vector<int64_t> &stitch) {
    seg.clear(); off.clear(); stitch.clear();
    if (launch_frames == 0) launch_frames = 1;
    if (seg_start == nullptr) n_seg = 0;
    size_t k = 0;                                            // the first start not yet passed
    for (size_t f0 = 0; f0 < n_frames; f0 += launch_frames) {
        const size_t f1 = (n_frames - f0 < launch_frames) ? n_frames : f0 + launch_frames;
        off.push_back(seg.size());
        seg.push_back(0);
        bool starts_here = (f0 == 0);
        while (k < n_seg && (size_t)seg_start[k] <= f0) { starts_here = starts_here || (size_t)seg_start[k] == f0; k++; }
        const size_t first_inside = seg.size();
        while (k < n_seg && (size_t)seg_start[k] < f1) seg.push_back(seg_start[k++] - (int64_t)f0);
        // rows that continue the utterance before the launch: up to the first start inside it, or all of them
        stitch.push_back(starts_here ? 0 : (first_inside < seg.size() ? seg[first_inside] : (int64_t)(f1 - f0)));
    }
    off.push_back(seg.size());
}

}  // namespace vbx
