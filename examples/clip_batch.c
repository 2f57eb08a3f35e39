/*
 * examples/clip_batch.c -- a batch of variable-length clips from ONE call: a padded batch [B, Tmax] of 16-bit PCM at 48 kHz with
 * lengths[B], as a data loader hands it over, is uploaded once and analysed by vbx_analyze_clips.  Each clip's rows are those of
 * the resident frame loop on that clip alone, bit for bit; vbx_clips_plan says where they are.  Prints every clip's median pitch.
 *
 *   gcc -std=c11 -Iinclude examples/clip_batch.c -Lvox_box.rs_amd/lib -lvoxbox_hip \
 *       -Wl,-rpath,$PWD/vox_box.rs_amd/lib -lm -o clip_batch
 *   ./clip_batch            (needs an MI355X)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "voxbox_hip.h"

#define B 6
#define TMAX 48000

#define CHECK(call)                                                                   \
    do {                                                                              \
        int rc_ = (call);                                                             \
        if (rc_ != VBX_SUCCESS) { fprintf(stderr, "%s: %s\n", #call, vbx_last_error(ctx)); return 1; } \
    } while (0)

static int by_value(const void *a, const void *b) { const double x = *(const double *)a, y = *(const double *)b; return (x > y) - (x < y); }

int main(void) {
    const size_t frame_len = 1200, hop = 480;
    const size_t lengths[B] = {48000, 1199, 30001, 1200, 0, 17520};                 /* clips 1 and 4 are shorter than a frame */
    vbx_ctx *ctx = NULL;
    if (vbx_ctx_create(&ctx, 0, NULL) != VBX_SUCCESS) { fprintf(stderr, "no gfx950 device: %s\n", vbx_last_error(NULL)); return 2; }

    /* the padded batch: clip b is a sine of 100 + 40 b Hz, the padding behind it is never read */
    int16_t *h_batch = (int16_t *)calloc((size_t)B * TMAX, sizeof(int16_t));
    for (int b = 0; b < B; b++)
        for (size_t i = 0; i < lengths[b]; i++)
            h_batch[(size_t)b * TMAX + i] = (int16_t)lrint(12000.0 * sin(2.0 * 3.14159265358979323846 * (100.0 + 40.0 * b) * (double)i / 48000.0));
    void *d_batch = NULL;
    CHECK(vbx_malloc(ctx, &d_batch, (size_t)B * TMAX * sizeof(int16_t)));
    CHECK(vbx_memcpy_h2d(ctx, d_batch, h_batch, (size_t)B * TMAX * sizeof(int16_t)));
    const void *clips[B];                                                           /* device pointers, in host memory */
    for (int b = 0; b < B; b++) clips[b] = (const int16_t *)d_batch + (size_t)b * TMAX;

    vbx_analysis_params p;
    memset(&p, 0, sizeof p);
    p.sample_rate = 48000.0;
    p.pitch_threshold = 0.2; p.pitch_fmin = 75.0; p.pitch_fmax = 600.0;
    vbx_clip_format fmt;
    memset(&fmt, 0, sizeof fmt);
    fmt.format = VBX_SAMPLE_PCM16;                                                  /* group_frames 0: the library's default */

    vbx_clip_row rows[B];
    size_t total = 0, groups = 0;
    CHECK(vbx_clips_plan(lengths, B, frame_len, hop, fmt.group_frames, rows, &total, &groups));
    const size_t rec = vbx_record_doubles_ex(&p, NULL), ld = rec + (rec & 1);       /* [ pitch 2 ] */
    void *d_rec = NULL;
    CHECK(vbx_malloc(ctx, &d_rec, (total ? total : 1) * ld * sizeof(double)));
    CHECK(vbx_analyze_clips(ctx, clips, lengths, B, &fmt, frame_len, hop, &p, NULL, NULL, (double *)d_rec, ld, NULL, NULL));
    double *h_rec = (double *)malloc((total ? total : 1) * ld * sizeof(double));
    CHECK(vbx_memcpy_d2h(ctx, h_rec, d_rec, total * ld * sizeof(double)));          /* (waits for the call's kernels) */

    double *hz = (double *)malloc((total ? total : 1) * sizeof(double));
    for (int b = 0; b < B; b++) {
        if (rows[b].n_rows == 0) { printf("clip %d: %zu samples, no frame\n", b, lengths[b]); continue; }
        for (int64_t j = 0; j < rows[b].n_rows; j++) hz[j] = h_rec[(size_t)(rows[b].row_start + j) * ld];
        qsort(hz, (size_t)rows[b].n_rows, sizeof(double), by_value);
        printf("clip %d: %zu samples, rows [%lld, %lld), median pitch %.2f Hz\n", b, lengths[b], (long long)rows[b].row_start,
               (long long)(rows[b].row_start + rows[b].n_rows), hz[rows[b].n_rows / 2]);
    }
    printf("%zu rows from %zu group(s)\n", total, groups);

    free(hz); free(h_rec); free(h_batch);
    vbx_free(ctx, d_rec);
    vbx_free(ctx, d_batch);
    vbx_ctx_destroy(ctx);
    return 0;
}
