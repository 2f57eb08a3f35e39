/*
 * examples/live_array.c -- BOTH channels of live stereo audio from ONE session: raw 16-bit little-endian stereo PCM at 48 kHz on
 * stdin, read in hop-sized reads (480 sample frames = 10 ms) and pushed into a multi-channel live session
 * (vbx_session_open_channels / vbx_session_push_channels).  Every push uploads the interleaved block once and runs one frame-loop
 * call over both channels; pitch and F1 of the left and the right channel are printed as the frames complete.  Per channel the rows
 * are those of a one-channel session on that channel -- the resident frame loop on the whole channel, bit for bit.
 *
 *   gcc -std=c11 -Iinclude examples/live_array.c -Lvox_box.rs_amd/lib -lvoxbox_hip \
 *       -Wl,-rpath,$PWD/vox_box.rs_amd/lib -o live_array
 *   arecord -t raw -f S16_LE -r 48000 -c 2 | ./live_array            (needs an MI355X)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "voxbox_hip.h"

#define CHANNELS 2

#define CHECK(call)                                                                   \
    do {                                                                              \
        int rc_ = (call);                                                             \
        if (rc_ != VBX_SUCCESS) { fprintf(stderr, "%s: %s\n", #call, vbx_last_error(ctx)); return 1; } \
    } while (0)

int main(void) {
    const size_t frame_len = 1200, hop = 480;
    vbx_ctx *ctx = NULL;
    if (vbx_ctx_create(&ctx, 0, NULL) != VBX_SUCCESS) { fprintf(stderr, "no gfx950 device: %s\n", vbx_last_error(NULL)); return 2; }

    /* pitch and four formants tracked from the male estimates: one parameter set for both channels */
    vbx_analysis_params p;
    memset(&p, 0, sizeof p);
    p.sample_rate = 48000.0;
    p.pitch_threshold = 0.2; p.pitch_fmin = 75.0; p.pitch_fmax = 600.0;
    p.formant_order = 12; p.n_est = 4;
    for (int e = 0; e < 4; e++) { p.est_init[e].frequency = VBX_MALE_FORMANT_ESTIMATES[e]; p.est_init[e].bandwidth = 1.0; }
    vbx_host_audio fmt;
    memset(&fmt, 0, sizeof fmt);
    fmt.format = VBX_SAMPLE_PCM16; fmt.channels = CHANNELS; fmt.channel = 0;        /* the selection is h_channels */
    const int32_t select[CHANNELS] = {0, 1};

    const size_t rec = vbx_record_doubles_ex(&p, NULL), ld = rec + (rec & 1);       /* [ pitch 2 | formants 8 ] */
    const size_t max_block = hop;                                                   /* the largest read below */
    const size_t max_rows = max_block / hop + 1;
    vbx_session *s = NULL;
    CHECK(vbx_session_open_channels(ctx, &fmt, select, CHANNELS, frame_len, hop, &p, NULL, NULL, max_block, &s));

    void *h_block = NULL;
    CHECK(vbx_malloc_host(ctx, &h_block, max_block * CHANNELS * sizeof(int16_t)));  /* pinned staging of the reads */
    vbx_channel_outputs out[CHANNELS];                                              /* entry k: where channel select[k]'s rows go */
    double *h_rec[CHANNELS];
    memset(out, 0, sizeof out);
    for (int k = 0; k < CHANNELS; k++) {
        void *d = NULL;
        CHECK(vbx_malloc(ctx, &d, max_rows * ld * sizeof(double)));
        out[k].records = (double *)d;
        h_rec[k] = (double *)malloc(max_rows * ld * sizeof(double));
    }

    size_t frame = 0, got;
    while ((got = fread(h_block, CHANNELS * sizeof(int16_t), hop, stdin)) > 0) {    /* a short last read is pushed as it is */
        size_t n = 0;
        CHECK(vbx_session_push_channels(s, h_block, got, out, ld, 0, &n));
        if (n == 0) continue;                                                       /* the block completed no frame */
        for (int k = 0; k < CHANNELS; k++)
            CHECK(vbx_memcpy_d2h(ctx, h_rec[k], out[k].records, n * ld * sizeof(double)));     /* (waits for the push's kernels) */
        for (size_t j = 0; j < n; j++, frame++) {
            const double *l = h_rec[0] + j * ld, *r = h_rec[1] + j * ld;
            printf("frame %zu  left %8.2f Hz (%.3f) F1 %7.1f   right %8.2f Hz (%.3f) F1 %7.1f\n", frame, l[0], l[1], l[2], r[0], r[1], r[2]);
        }
        fflush(stdout);
    }
    size_t consumed = 0, frames = 0, carried = 0;
    CHECK(vbx_session_info(s, &consumed, &frames, &carried));
    fprintf(stderr, "%zu sample frames, %zu frames per channel, %zu sample frames still carried\n", consumed, frames, carried);

    vbx_session_close(s);
    for (int k = 0; k < CHANNELS; k++) { vbx_free(ctx, out[k].records); free(h_rec[k]); }
    vbx_free_host(ctx, h_block);
    vbx_ctx_destroy(ctx);
    return 0;
}
