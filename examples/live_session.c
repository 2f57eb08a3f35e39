/*
 * examples/live_session.c -- audio that ARRIVES, analysed as it comes: raw 16-bit little-endian mono PCM at 48 kHz on stdin, read in
 * hop-sized reads (480 samples = 10 ms) and pushed into a live session (vbx_session_*); pitch, F1-F4 and RMS of every frame are
 * printed as the frames complete.  The rows are those of the resident frame loop on the whole stream, bit for bit.
 *
 *   gcc -std=c11 -Iinclude examples/live_session.c -Lvox_box.rs_amd/lib -lvoxbox_hip \
 *       -Wl,-rpath,$PWD/vox_box.rs_amd/lib -o live_session
 *   arecord -t raw -f S16_LE -r 48000 -c 1 | ./live_session          (needs an MI355X)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "voxbox_hip.h"

#define CHECK(call)                                                                   \
    do {                                                                              \
        int rc_ = (call);                                                             \
        if (rc_ != VBX_SUCCESS) { fprintf(stderr, "%s: %s\n", #call, vbx_last_error(ctx)); return 1; } \
    } while (0)

int main(void) {
    const size_t frame_len = 1200, hop = 480;
    vbx_ctx *ctx = NULL;
    if (vbx_ctx_create(&ctx, 0, NULL) != VBX_SUCCESS) { fprintf(stderr, "no gfx950 device: %s\n", vbx_last_error(NULL)); return 2; }

    /* the frame loop of examples/formant_extraction: pitch, four formants tracked from the male estimates, and the frame's RMS */
    vbx_analysis_params p;
    memset(&p, 0, sizeof p);
    p.sample_rate = 48000.0;
    p.pitch_threshold = 0.2; p.pitch_fmin = 75.0; p.pitch_fmax = 600.0;
    p.formant_order = 12; p.n_est = 4;
    for (int e = 0; e < 4; e++) { p.est_init[e].frequency = VBX_MALE_FORMANT_ESTIMATES[e]; p.est_init[e].bandwidth = 1.0; }
    vbx_analysis_ext ext;
    memset(&ext, 0, sizeof ext);
    ext.rms = 1;
    vbx_host_audio fmt;
    memset(&fmt, 0, sizeof fmt);
    fmt.format = VBX_SAMPLE_PCM16; fmt.channels = 1; fmt.channel = 0;

    const size_t rec = vbx_record_doubles_ex(&p, &ext), ld = rec + (rec & 1);      /* [ pitch 2 | formants 8 | rms 1 ] */
    const size_t max_block = frame_len;                                            /* the largest read below */
    const size_t max_rows = max_block / hop + 1;
    vbx_session *s = NULL;
    CHECK(vbx_session_open(ctx, &fmt, frame_len, hop, &p, &ext, NULL, max_block, &s));

    void *h_block = NULL, *d_rec = NULL, *d_st = NULL;
    CHECK(vbx_malloc_host(ctx, &h_block, max_block * sizeof(int16_t)));            /* pinned: the upload runs beside the analysis */
    CHECK(vbx_malloc(ctx, &d_rec, max_rows * ld * sizeof(double)));
    CHECK(vbx_malloc(ctx, &d_st, 3 * max_rows * sizeof(int32_t)));
    double *h_rec = (double *)malloc(max_rows * ld * sizeof(double));
    int32_t *h_st = (int32_t *)malloc(3 * max_rows * sizeof(int32_t));

    size_t frame = 0, got;
    while ((got = fread(h_block, sizeof(int16_t), hop, stdin)) > 0) {              /* a short last read is pushed as it is */
        size_t n = 0;
        CHECK(vbx_session_push(s, h_block, got, (double *)d_rec, ld, (int32_t *)d_st, max_rows, NULL, &n));
        if (n == 0) continue;                                                      /* the block completed no frame */
        CHECK(vbx_memcpy_d2h(ctx, h_rec, d_rec, n * ld * sizeof(double)));         /* (waits for the push's kernels) */
        CHECK(vbx_memcpy_d2h(ctx, h_st, d_st, 3 * max_rows * sizeof(int32_t)));
        for (size_t k = 0; k < n; k++, frame++) {
            const double *r = h_rec + k * ld;
            printf("frame %zu  %8.2f Hz (%.3f)  F1-F4 %7.1f %7.1f %7.1f %7.1f  rms %.5f  status %d/%d\n", frame, r[0], r[1], r[2], r[4], r[6],
                   r[8], r[rec - 1], (int)h_st[k], (int)h_st[max_rows + k]);
        }
        fflush(stdout);
    }
    size_t consumed = 0, frames = 0, carried = 0;
    CHECK(vbx_session_info(s, &consumed, &frames, &carried));
    fprintf(stderr, "%zu samples, %zu frames, %zu samples still carried\n", consumed, frames, carried);

    vbx_session_close(s);
    vbx_free(ctx, d_rec); vbx_free(ctx, d_st);
    vbx_free_host(ctx, h_block);
    vbx_ctx_destroy(ctx);
    free(h_rec); free(h_st);
    return 0;
}
