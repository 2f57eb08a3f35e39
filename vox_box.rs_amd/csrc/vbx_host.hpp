// vbx_host.hpp -- the library's host-only arithmetic (vbx_host.cpp): tables, bins and shard geometry that need no GPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace vbx {

// sample 0.10 window / HanningLag / periodic Hanning tables by the crate's own recurrences (VBX_WINDOW_* kinds)
int window_table_host(int kind, size_t n, double *out);
// mel filter bank bins, src/spectrum.rs:411-414 (Q14); overflow: a bin beyond any spectrum (the reference panics)
void mel_bins_host(size_t n, size_t k, double lo, double hi, double sr, std::vector<int32_t> &bins, bool &overflow);

// ---- the tables the context keeps on the device (vbx_table_cache.hpp), host side: a size function and a fill that writes
// into the caller's ZEROED buffers (what the packing rules call padding is never written).  Plain integers and doubles only.

// a window as the kernels read it: the table, and for the lag window its entries' reciprocals from element (n + 1) & ~1 on
// (each correctly rounded: one IEEE division); *rcp_usable: no zero, no entry whose reciprocal leaves the normal range
size_t window_dev_doubles(int kind, size_t n);
int window_dev_fill(int kind, size_t n, double *out, bool *rcp_usable);
// Goertzel-Reinsch constants of bins [b_lo, b_lo + nb) of an n-point DFT (k_mfcc.hip): [nb][2] kappa, sigma
size_t goertzel_doubles(int nb);
void goertzel_fill(size_t n, int b_lo, int nb, double *out);
// two-stage MFCC DFT (k_mfcc.hip, mfcc_plan_t): ctab[n1][nc] cos / sin columns of the n1-point DFT, twid[n][2]
size_t dft2_ctab_doubles(int n1, int nc);
size_t dft2_twid_doubles(size_t n);
void dft2_fill(size_t n, int n1, int nc, double *ctab, double *twid);
// matrix-core MFCC kernel (k_mfcc_mfma.hip, mfcc_mplan_t): ctab, twd, twm, wm; doubles[4] in that order
void mfma_doubles(int n1, int mt, int ntd, int ntm, size_t doubles[4]);
void mfma_fill(size_t n, int n1, int n2, int k2, int mt, int ntd, int ntm, int src0, int src1,
               double *ctab, double *twd, double *twm, double *wm);
// DCT-II table of src/spectrum.rs:395: [k][k]
size_t dct_doubles(size_t k);
void dct_fill(size_t k, double *out);
// slope factor of every bin of the k mel filters on bins[k + 2]: [max(nb, 1)][2] i / up, i / down (src/spectrum.rs:424,430)
size_t slopes_doubles(const int32_t *bins, size_t k);
void slopes_fill(const int32_t *bins, size_t k, double *out);
// sample 0.10 Converter's linear interpolation: left source index and fraction of each of the m outputs
void resample_fill(size_t m, double resample_ratio, int32_t *index, double *frac);

// ---- a live session's geometry (vbx_session_plan itself is an entry point: include/voxbox_hip.h, defined in vbx_host.cpp) ----
// samples a session's carry buffer holds: the kept tail never exceeds WARM hops and a frame, a push adds at most max_block
size_t session_carry_samples(size_t frame_len, size_t stride, size_t max_block);
// the most frames one push's frame-loop call covers: the frames max_block samples can complete, and the warm-up
size_t session_max_frames(size_t stride, size_t max_block);
// ---- a session pool's geometry (vbx_pool_plan is an entry point) ----
// elements a slot's carried tail never exceeds: VBX_SHARD_WARM_FRAMES hops and a frame less one sample
size_t pool_carry_samples(size_t frame_len, size_t stride);
// the most frames one tick's frame-loop call covers (vbx_pool_plan's call_frames), for ticks of at most max_tick samples in all
size_t pool_max_call_frames(size_t frame_len, size_t stride, size_t max_streams, size_t max_tick);

// ---- the fused frame loop cut into launches (analyze_frames with Burg's lag sums from the analyze kernel, vbx_api_frames.hip) ----
// Launch j covers frames [j L, min((j + 1) L, F)).  The tracker scans each launch's rows alone, as if an utterance began with the
// launch: seg[off[j] .. off[j + 1]) are the utterance starts of that scan, relative to the launch's first frame -- a 0, then every
// start of seg_start (null: one utterance) strictly inside the launch; stitch[j] is the number of rows from the launch's first that
// continue an utterance begun before it (0: an utterance starts with the launch) -- those are repaired from the row before them.
void launch_ranges_host(const int64_t *seg_start, size_t n_seg, size_t n_frames, size_t launch_frames,
                        std::vector<int64_t> &seg, std::vector<size_t> &off, std::vector<int64_t> &stitch);

// table kinds of vbx_internal_host_table (tests, tools/host_property_check.py)
enum { HOST_TABLE_WINDOW, HOST_TABLE_LAG_F32, HOST_TABLE_GOERTZEL, HOST_TABLE_DFT2, HOST_TABLE_MFMA, HOST_TABLE_DCT,
       HOST_TABLE_SLOPES, HOST_TABLE_RESAMPLE, HOST_TABLE_KINDS };

}  // namespace vbx
