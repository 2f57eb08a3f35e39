// vbx_table_cache.hpp -- every host-built device table of a context (vbx_ctx.hpp) in one cache.  A key is the table's kind and its
// parameters; an entry is ONE device allocation with the byte offsets of its sub-tables; one miss path sizes, builds on the host,
// allocates, uploads and inserts, and leaves nothing behind when a step fails.  The builders are plain host functions: vbx_host.cpp,
// or beside their kernels (spectral_fill_tab, mfcc_interp_fill, mfcc_czt_fill_tabs).
#pragma once

#include "../../include/voxbox_hip.h"
#include "vbx_host.hpp"
#include "vbx_kernels.hpp"

#include <hip/hip_runtime.h>

#include <array>
#include <cstring>
#include <initializer_list>
#include <map>
#include <type_traits>

namespace vbx {

// the key parameters of a kind are the arguments of its lookup below
enum table_kind_t : int { TABLE_WINDOW, TABLE_LAG_WINDOW_F32, TABLE_GOERTZEL, TABLE_DCT, TABLE_DFT2, TABLE_MFMA, TABLE_CZT, TABLE_BINS,
                          TABLE_SLOPES, TABLE_INTERP, TABLE_RESAMPLE, TABLE_SPECTRAL, TABLE_KINDS };
enum : uint32_t {
    TABLE_ABSENT = 1u,     // the parameters have no such table (remembered: the builder is not asked again); no allocation
    TABLE_LAG_RCP = 2u,    // the lag window's reciprocals may be used (window_dev_fill)
};

// doubles enter a key by bit pattern: a total order whatever the value (NaN included)
inline uint64_t table_key_word(double v) { uint64_t b; std::memcpy(&b, &v, sizeof b); return b; }
template <class T, class = std::enable_if_t<std::is_integral<T>::value>>
inline uint64_t table_key_word(T v) { return (uint64_t)(int64_t)v; }

struct table_key_t {
    int kind;
    std::array<uint64_t, 5> p;
    template <class... A> explicit table_key_t(int k, A... params) : kind(k), p{table_key_word(params)...} {}
    bool operator<(const table_key_t &o) const { return kind != o.kind ? kind < o.kind : p < o.p; }
};

struct table_entry_t {
    void *dev = nullptr;
    size_t bytes = 0, off[4] = {};            // the allocation and where its sub-tables begin
    uint32_t flags = 0;                       // TABLE_*
    int32_t aux[5] = {};                      // host-side words of the builder (TABLE_INTERP: the geometry mfcc_interp_fill reports)
    template <class T> const T *sub(int i) const { return reinterpret_cast<const T *>(static_cast<const char *>(dev) + off[i]); }
    // sub-tables one after the other, each on a 256-byte boundary (what hipMalloc gives a table of its own)
    static table_entry_t packed(std::initializer_list<size_t> sub_bytes) {
        table_entry_t t;
        int i = 0;
        for (size_t b : sub_bytes) { t.off[i++] = t.bytes; t.bytes = (t.bytes + b + 255) & ~(size_t)255; }
        return t;
    }
};

class table_cache_t {
public:
    // entries a kind may hold (0: no bound).  A miss at the bound drains the device (a queued kernel may still read a table) and drops
    // that kind's entries: a caller that sweeps frame lengths or bands makes one interpolation table (48-200 KB) per shape.
    size_t cap[TABLE_KINDS] = {};
    table_cache_t() { cap[TABLE_INTERP] = 64; }

    // t: the layout (table_entry_t::packed, or offsets of the builder's own).  build(h, t) fills the ZEROED host copy h of the allocation
    // and may set t.flags / t.aux; false: bad parameters (hipErrorInvalidValue, nothing inserted)
    template <class Build>
    hipError_t get(const table_key_t &key, table_entry_t t, Build &&build, const table_entry_t **out) {
        auto it = entries_.find(key);
        if (it == entries_.end()) {
            if (cap[key.kind] && count_[key.kind] >= cap[key.kind]) {
                hipError_t e = hipDeviceSynchronize();
                if (e != hipSuccess) return e;
                drop(key.kind);
            }
            std::vector<char> h(t.bytes, 0);
            if (!build(h.data(), t)) return hipErrorInvalidValue;
            if (!(t.flags & TABLE_ABSENT)) {
                hipError_t e = hipMalloc(&t.dev, t.bytes);
                if (e == hipSuccess && (e = hipMemcpy(t.dev, h.data(), t.bytes, hipMemcpyHostToDevice)) != hipSuccess) (void)hipFree(t.dev);
                if (e != hipSuccess) return e;
            }
            it = entries_.emplace(key, t).first;
            count_[key.kind]++;
        }
        *out = &it->second;
        return hipSuccess;
    }

    void drop(int kind) {
        auto lo = entries_.lower_bound(table_key_t(kind)), hi = entries_.lower_bound(table_key_t(kind + 1));
        for (auto it = lo; it != hi; ++it) if (it->second.dev) (void)hipFree(it->second.dev);
        entries_.erase(lo, hi);
        count_[kind] = 0;
    }

    void clear() { for (int k = 0; k < TABLE_KINDS; k++) drop(k); }

private:
    std::map<table_key_t, table_entry_t> entries_;
    size_t count_[TABLE_KINDS] = {};
};

// one lookup per kind
struct device_tables_t : table_cache_t {
    template <class T, class Build>            // a single table of `count` T
    hipError_t one(const table_key_t &key, size_t count, Build &&build, const T **out, uint32_t *flags = nullptr) {
        const table_entry_t *e = nullptr;
        hipError_t rc = get(key, table_entry_t::packed({count * sizeof(T)}), [&](char *h, table_entry_t &t) { return build(reinterpret_cast<T *>(h), t); }, &e);
        if (rc == hipSuccess) { *out = e->sub<T>(0); if (flags) *flags = e->flags; }
        return rc;
    }
    // a window as the kernels read it; *lag_rcp: the lag window's reciprocals (behind the table) may be used by the fused kernels' divide
    // (quotient_by_table, vbx_spectral.hpp)
    hipError_t window(int kind, size_t n, const double **out, bool *lag_rcp = nullptr) {
        uint32_t flags = 0;
        hipError_t rc = one(table_key_t(TABLE_WINDOW, kind, n), window_dev_doubles(kind, n), [&](double *h, table_entry_t &t) {
            bool usable = false;
            if (window_dev_fill(kind, n, h, &usable) != VBX_SUCCESS) return false;
            if (usable) t.flags |= TABLE_LAG_RCP;
            return true;
        }, out, &flags);
        if (lag_rcp) *lag_rcp = (flags & TABLE_LAG_RCP) != 0;
        return rc;
    }
    // w_lag as the f64 table of the reference's recurrence, each entry rounded to f32 (Pitched<f32, f32>)
    hipError_t lag_window_f32(size_t n, const float **out) {
        return one(table_key_t(TABLE_LAG_WINDOW_F32, n), n, [&](float *h, table_entry_t &) { return vbx_window_table_f32(VBX_WINDOW_HANNING_LAG, n, h) == VBX_SUCCESS; }, out);
    }
    hipError_t goertzel(size_t n, int b_lo, int nb, const double **out) {
        return one(table_key_t(TABLE_GOERTZEL, n, b_lo, nb), goertzel_doubles(nb), [&](double *h, table_entry_t &) { goertzel_fill(n, b_lo, nb, h); return true; }, out);
    }
    hipError_t dct(size_t k, const double **out) {
        return one(table_key_t(TABLE_DCT, k), dct_doubles(k), [&](double *h, table_entry_t &) { dct_fill(k, h); return true; }, out);
    }
    // twiddles of the fused spectral kernels (k_spectral.hip, k_spectral_pow2.hip), one table per plan
    hipError_t spectral(int plan, const double **out) {
        return one(table_key_t(TABLE_SPECTRAL, plan), 2 * (size_t)spectral_tab_complex(plan), [&](double *h, table_entry_t &) { spectral_fill_tab(plan, h); return true; }, out);
    }
    // the device copy of the mel bins (the callers compute the host bins on every call: they need them)
    hipError_t bins(size_t n, size_t k, double lo, double hi, double sr, const std::vector<int32_t> &hb, const int32_t **out) {
        return one(table_key_t(TABLE_BINS, n, k, lo, hi, sr), hb.size(), [&](int32_t *h, table_entry_t &) { std::memcpy(h, hb.data(), hb.size() * sizeof(int32_t)); return true; }, out);
    }
    hipError_t slopes(size_t n, size_t k, double lo, double hi, double sr, const std::vector<int32_t> &hb, const double **out) {
        return one(table_key_t(TABLE_SLOPES, n, k, lo, hi, sr), slopes_doubles(hb.data(), k), [&](double *h, table_entry_t &) { slopes_fill(hb.data(), k, h); return true; }, out);
    }
    // two-stage MFCC DFT (k_mfcc.hip), keyed (n, n1)
    hipError_t dft2(size_t n, const mfcc_plan_t &pl, const double **ctab, const double **twid) {
        const table_entry_t *e = nullptr;
        hipError_t rc = get(table_key_t(TABLE_DFT2, n, pl.n1), table_entry_t::packed({dft2_ctab_doubles(pl.n1, pl.nc) * 8, dft2_twid_doubles(n) * 8}),
                            [&](char *h, table_entry_t &t) { dft2_fill(n, pl.n1, pl.nc, (double *)h, (double *)(h + t.off[1])); return true; }, &e);
        if (rc == hipSuccess) { *ctab = e->sub<double>(0); *twid = e->sub<double>(1); }
        return rc;
    }
    // matrix-core MFCC kernel (k_mfcc_mfma.hip), keyed (n, n1, k2)
    hipError_t mfma(size_t n, const mfcc_mplan_t &pl, const double **ctab, const double **twd, const double **twm, const double **wm) {
        size_t d[4];
        mfma_doubles(pl.n1, pl.mt, pl.ntd, pl.ntm, d);
        const table_entry_t *e = nullptr;
        hipError_t rc = get(table_key_t(TABLE_MFMA, n, pl.n1, pl.k2), table_entry_t::packed({d[0] * 8, d[1] * 8, d[2] * 8, d[3] * 8}), [&](char *h, table_entry_t &t) {
            mfma_fill(n, pl.n1, pl.n2, pl.k2, pl.mt, pl.ntd, pl.ntm, pl.src0, pl.src1, (double *)h, (double *)(h + t.off[1]), (double *)(h + t.off[2]), (double *)(h + t.off[3]));
            return true;
        }, &e);
        if (rc == hipSuccess) { *ctab = e->sub<double>(0); *twd = e->sub<double>(1); *twm = e->sub<double>(2); *wm = e->sub<double>(3); }
        return rc;
    }
    // chirp-z MFCC kernel (k_mfcc_czt.hip): the chirp and the FFT of the chirp segment(s); n1: the split length or 0
    hipError_t czt(size_t n, int top, int L, int n1, const double **chirp, const double **bhat) {
        const size_t nblk = (n1 > 0 && (size_t)n1 < n) ? (n + n1 - 1) / n1 : 1;
        const table_entry_t *e = nullptr;
        hipError_t rc = get(table_key_t(TABLE_CZT, n, top, L, n1), table_entry_t::packed({2 * n * 8, 2 * (size_t)L * nblk * 8}),
                            [&](char *h, table_entry_t &t) { mfcc_czt_fill_tabs((int)n, top, L, n1, (double *)h, (double *)(h + t.off[1])); return true; }, &e);
        if (rc == hipSuccess) { *chirp = e->sub<double>(0); *bhat = e->sub<double>(1); }
        return rc;
    }
    // sample 0.10 Converter's source index and fraction of each of the m outputs, keyed (n, ratio)
    hipError_t resample(size_t n, double ratio, size_t m, const int32_t **index, const double **frac) {
        const table_entry_t *e = nullptr;
        hipError_t rc = get(table_key_t(TABLE_RESAMPLE, n, ratio), table_entry_t::packed({m * sizeof(int32_t), m * sizeof(double)}),
                            [&](char *h, table_entry_t &t) { resample_fill(m, ratio, (int32_t *)h, (double *)(h + t.off[1])); return true; }, &e);
        if (rc == hipSuccess) { *index = e->sub<int32_t>(0); *frac = e->sub<double>(1); }
        return rc;
    }
    // the MFCC bins interpolated inside the fused kernel (mfcc_interp_t): rot, coef, j0 where mfcc_interp_fill puts them; *ok = false: the
    // shape has no such form
    hipError_t interp(int plan, int n, int b_lo, int nb, mfcc_interp_t *out, bool *ok) {
        table_entry_t lay;
        lay.off[1] = mfcc_interp_coef_offset(plan); lay.off[2] = mfcc_interp_j0_offset(plan, nb); lay.bytes = mfcc_interp_table_bytes(plan, nb);
        const table_entry_t *e = nullptr;
        hipError_t rc = get(table_key_t(TABLE_INTERP, plan, n, b_lo, nb), lay, [&](char *h, table_entry_t &t) {
            mfcc_interp_t d{};
            if (!mfcc_interp_fill(plan, n, b_lo, nb, h, &d)) t.flags |= TABLE_ABSENT;
            t.aux[0] = d.jmin; t.aux[1] = d.jmax; t.aux[2] = d.taps; t.aux[3] = d.pu_off; t.aux[4] = d.lds_bytes;
            return true;
        }, &e);
        if (rc != hipSuccess) return rc;
        *ok = !(e->flags & TABLE_ABSENT);
        *out = mfcc_interp_t{nullptr, nullptr, nullptr, e->aux[0], e->aux[1], e->aux[2], e->aux[3], e->aux[4]};
        if (*ok) { out->rot = e->sub<double>(0); out->coef = e->sub<double>(1); out->j0 = e->sub<int32_t>(2); }
        return hipSuccess;
    }
};

}  // namespace vbx
