/*
 * examples/pitch_boersma.c -- a short glide (180 -> 240 Hz in one second) through vbx_pitch_boersma_f64 -> vbx_frame_peak_f64 ->
 * vbx_pitch_path_f64, the contour printed beside vbx_pitch_f64's: the crate's rows sit on integer lags (48000 / k), the Boersma
 * candidates follow the glide.
 *
 *   gcc -std=c11 -Iinclude examples/pitch_boersma.c -Lvox_box.rs_amd/lib -lvoxbox_hip \
 *       -Wl,-rpath,$PWD/vox_box.rs_amd/lib -lm -o pitch_boersma && ./pitch_boersma      (needs an MI355X)
 */
#define _USE_MATH_DEFINES
#define _GNU_SOURCE
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "voxbox_hip.h"

#define CHECK(call)                                                                   \
    do {                                                                              \
        int rc_ = (call);                                                             \
        if (rc_ != VBX_SUCCESS) { fprintf(stderr, "%s: %s\n", #call, vbx_last_error(ctx)); return 1; } \
    } while (0)

int main(void) {
    const double sample_rate = 48000.0, f_start = 180.0, f_end = 240.0;
    const size_t n_samples = 48000, bin = 1200, hop = 480, kmax = 15;
    double *h_audio = (double *)malloc(n_samples * sizeof(double));
    /* phase of a linear glide: 2 pi (f_start t + (f_end - f_start) t^2 / 2) over one second */
    for (size_t i = 0; i < n_samples; i++) {
        const double t = (double)i / sample_rate;
        h_audio[i] = 0.5 * sin(2.0 * M_PI * (f_start * t + 0.5 * (f_end - f_start) * t * t));
    }

    vbx_ctx *ctx = NULL;
    if (vbx_ctx_create(&ctx, 0, NULL) != VBX_SUCCESS) { fprintf(stderr, "no gfx950 device: %s\n", vbx_last_error(NULL)); return 2; }

    const size_t n_frames = vbx_frame_count(n_samples, bin, hop);
    double *h_win = (double *)malloc(bin * sizeof(double));
    CHECK(vbx_window_table_f64(VBX_WINDOW_HANNING, bin, h_win));

    void *d_audio = NULL, *d_win = NULL, *d_cand = NULL, *d_ref = NULL, *d_count = NULL, *d_status = NULL, *d_peak = NULL, *d_path = NULL;
    CHECK(vbx_malloc(ctx, &d_audio, n_samples * sizeof(double)));
    CHECK(vbx_malloc(ctx, &d_win, bin * sizeof(double)));
    CHECK(vbx_malloc(ctx, &d_cand, n_frames * kmax * sizeof(vbx_pitch)));
    CHECK(vbx_malloc(ctx, &d_ref, n_frames * sizeof(vbx_pitch)));
    CHECK(vbx_malloc(ctx, &d_count, n_frames * sizeof(int32_t)));
    CHECK(vbx_malloc(ctx, &d_status, n_frames * sizeof(int32_t)));
    CHECK(vbx_malloc(ctx, &d_peak, n_frames * sizeof(double)));
    CHECK(vbx_malloc(ctx, &d_path, n_frames * sizeof(vbx_pitch)));
    CHECK(vbx_memcpy_h2d(ctx, d_audio, h_audio, n_samples * sizeof(double)));
    CHECK(vbx_memcpy_h2d(ctx, d_win, h_win, bin * sizeof(double)));

    /* the crate's rows: PitchExtractor's output is entry 0 of every frame */
    vbx_pitch *h_ref = (vbx_pitch *)malloc(n_frames * sizeof(vbx_pitch));
    CHECK(vbx_pitch_f64(ctx, (const double *)d_audio, n_frames, bin, hop, (const double *)d_win, sample_rate, 0.2, 75.0, 600.0,
                        1, (vbx_pitch *)d_ref, (int32_t *)d_count, (int32_t *)d_status));
    CHECK(vbx_memcpy_d2h(ctx, h_ref, d_ref, n_frames * sizeof(vbx_pitch)));

    /* Boersma's candidates, the frames' peaks, the path over the lists: three launches on the context's stream */
    CHECK(vbx_pitch_boersma_f64(ctx, (const double *)d_audio, n_frames, bin, hop, (const double *)d_win, sample_rate, 0.2, 75.0, 600.0,
                                kmax, (vbx_pitch *)d_cand, (int32_t *)d_count, (int32_t *)d_status));
    CHECK(vbx_frame_peak_f64(ctx, (const double *)d_audio, n_frames, bin, hop, (double *)d_peak));
    vbx_pitch_path_params pp = {0.45, 0.03, 0.01, 0.35, 0.14, 600.0, (double)hop / sample_rate, 0};      /* Praat's "To Pitch (ac)" values */
    CHECK(vbx_pitch_path_f64(ctx, (const vbx_pitch *)d_cand, (const int32_t *)d_count, (const int32_t *)d_status, n_frames, kmax,
                             (const double *)d_peak, NULL, 0, &pp, (vbx_pitch *)d_path, NULL));
    vbx_pitch *h_path = (vbx_pitch *)malloc(n_frames * sizeof(vbx_pitch));
    CHECK(vbx_memcpy_d2h(ctx, h_path, d_path, n_frames * sizeof(vbx_pitch)));
    CHECK(vbx_sync(ctx));

    double worst = 0.0, worst_ref = 0.0;
    for (size_t t = 0; t < n_frames; t++) {
        /* the glide's frequency at the frame's centre */
        const double tc = ((double)(t * hop) + 0.5 * (double)bin) / sample_rate, truth = f_start + (f_end - f_start) * tc;
        const double e = fabs(h_path[t].frequency - truth) / truth, e_ref = fabs(h_ref[t].frequency - truth) / truth;
        if (e > worst) worst = e;
        if (e_ref > worst_ref) worst_ref = e_ref;
        if (t % 10 == 0)
            printf("frame %3zu: glide %8.3f Hz  boersma path %8.3f Hz  vbx_pitch_f64 %8.3f Hz\n", t, truth, h_path[t].frequency, h_ref[t].frequency);
    }
    printf("worst relative error: boersma %.3e  vbx_pitch_f64 %.3e\n", worst, worst_ref);

    vbx_free(ctx, d_audio); vbx_free(ctx, d_win); vbx_free(ctx, d_cand); vbx_free(ctx, d_ref); vbx_free(ctx, d_count);
    vbx_free(ctx, d_status); vbx_free(ctx, d_peak); vbx_free(ctx, d_path);
    vbx_ctx_destroy(ctx);
    free(h_audio); free(h_win); free(h_ref); free(h_path);
    return 0;
}
