/*
 * examples/live_pitch.c -- the pitch contour of audio that ARRIVES: raw 16-bit little-endian mono PCM at 48 kHz on stdin, read in
 * hop-sized reads (480 samples = 10 ms) and pushed into a tracked live session that is bound to an online pitch path
 * (vbx_session_path_bind).  Every push commits the frames of the contour whose state is decided; each committed stretch is printed
 * with its delay, the number of frames the audio is ahead of it.  Rows that are not flagged as forced are the rows of
 * vbx_pitch_path_f64 over the whole utterance, bit for bit.
 *
 *   gcc -std=c11 -Iinclude examples/live_pitch.c -Lvox_box.rs_amd/lib -lvoxbox_hip \
 *       -Wl,-rpath,$PWD/vox_box.rs_amd/lib -o live_pitch
 *   arecord -t raw -f S16_LE -r 48000 -c 1 | ./live_pitch          (needs an MI355X)
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

#define KMAX 15
#define MAX_PENDING 64

static vbx_ctx *ctx = NULL;
static void *d_path = NULL, *d_forced = NULL, *d_commit = NULL;
static vbx_pitch h_path[MAX_PENDING + 4];
static uint8_t h_forced[MAX_PENDING + 4];

/* what the last push (or mark) committed: rows [first, first + n) of the contour, `frames` frames of audio in */
static int print_commit(size_t frames) {
    vbx_path_commit c;
    CHECK(vbx_memcpy_d2h(ctx, &c, d_commit, sizeof c));                            /* (waits for the push's kernels) */
    if (c.n == 0) return 0;
    CHECK(vbx_memcpy_d2h(ctx, h_path, d_path, (size_t)c.n * sizeof(vbx_pitch)));
    CHECK(vbx_memcpy_d2h(ctx, h_forced, d_forced, (size_t)c.n));
    printf("frames %lld..%lld (delay %lld frames, %lld pending)", (long long)c.first, (long long)(c.first + c.n - 1),
           (long long)frames - (long long)c.first, (long long)c.pending);
    for (int64_t k = 0; k < c.n; k++) {
        if (h_path[k].frequency > 0.0) printf("  %.1f Hz%s", h_path[k].frequency, h_forced[k] ? "!" : "");
        else printf("  --%s", h_forced[k] ? "!" : "");
    }
    printf("\n");
    fflush(stdout);
    return 0;
}

int main(void) {
    const size_t frame_len = 1200, hop = 480;
    if (vbx_ctx_create(&ctx, 0, NULL) != VBX_SUCCESS) { fprintf(stderr, "no gfx950 device: %s\n", vbx_last_error(NULL)); return 2; }

    vbx_analysis_params p;
    memset(&p, 0, sizeof p);
    p.sample_rate = 48000.0;
    p.pitch_threshold = 0.2; p.pitch_fmin = 75.0; p.pitch_fmax = 600.0;            /* the pitch alone: no LPC, formants or MFCC */
    vbx_pitch_track_params track;
    memset(&track, 0, sizeof track);
    track.kmax = KMAX;
    track.path.voicing_threshold = 0.45; track.path.silence_threshold = 0.03;     /* Praat's "To Pitch (ac)" values */
    track.path.octave_cost = 0.01; track.path.octave_jump_cost = 0.35; track.path.voiced_unvoiced_cost = 0.14;
    track.path.ceiling_hz = 600.0;                                                 /* time_step 0: hop / sample_rate */
    vbx_host_audio fmt;
    memset(&fmt, 0, sizeof fmt);
    fmt.format = VBX_SAMPLE_PCM16; fmt.channels = 1; fmt.channel = 0;

    const size_t rec = vbx_record_doubles_ex(&p, NULL), ld = rec + (rec & 1);
    const size_t max_block = frame_len, max_rows = max_block / hop + 1;
    vbx_session *s = NULL;
    CHECK(vbx_session_open(ctx, &fmt, frame_len, hop, &p, NULL, &track, max_block, &s));

    /* the session's own outputs (the lists are the path's input; this example does not look at them) ... */
    void *h_block = NULL, *d_rec = NULL, *d_cand = NULL, *d_count = NULL, *d_peak = NULL, *d_index = NULL;
    CHECK(vbx_malloc_host(ctx, &h_block, max_block * sizeof(int16_t)));
    CHECK(vbx_malloc(ctx, &d_rec, max_rows * ld * sizeof(double)));
    CHECK(vbx_malloc(ctx, &d_cand, max_rows * KMAX * sizeof(vbx_pitch)));
    CHECK(vbx_malloc(ctx, &d_count, max_rows * sizeof(int32_t)));
    CHECK(vbx_malloc(ctx, &d_peak, max_rows * sizeof(double)));
    vbx_pitch_track_outputs out;
    memset(&out, 0, sizeof out);
    out.cand = (vbx_pitch *)d_cand; out.count = (int32_t *)d_count; out.peak = (double *)d_peak;
    /* ... and the contour's: MAX_PENDING + the frames of the largest push rows.  P of the silence term: full scale (PCM16 peaks
     * are max |s| / 32767) */
    const size_t path_rows = MAX_PENDING + max_rows;
    CHECK(vbx_malloc(ctx, &d_path, path_rows * sizeof(vbx_pitch)));
    CHECK(vbx_malloc(ctx, &d_index, path_rows * sizeof(int32_t)));
    CHECK(vbx_malloc(ctx, &d_forced, path_rows));
    CHECK(vbx_malloc(ctx, &d_commit, sizeof(vbx_path_commit)));
    CHECK(vbx_session_path_bind(s, 1.0, MAX_PENDING, (vbx_pitch *)d_path, 2, (int32_t *)d_index, (uint8_t *)d_forced,
                                (vbx_path_commit *)d_commit));

    size_t frames = 0, got;
    while ((got = fread(h_block, sizeof(int16_t), hop, stdin)) > 0) {
        size_t n = 0;
        CHECK(vbx_session_push(s, h_block, got, (double *)d_rec, ld, NULL, 0, &out, &n));
        frames += n;
        if (print_commit(frames)) return 1;
    }
    CHECK(vbx_session_mark_utterance(s));                                          /* the stream has ended: the rest, at once */
    if (print_commit(frames)) return 1;

    vbx_session_close(s);
    vbx_free(ctx, d_rec); vbx_free(ctx, d_cand); vbx_free(ctx, d_count); vbx_free(ctx, d_peak);
    vbx_free(ctx, d_path); vbx_free(ctx, d_index); vbx_free(ctx, d_forced); vbx_free(ctx, d_commit);
    vbx_free_host(ctx, h_block);
    vbx_ctx_destroy(ctx);
    return 0;
}
