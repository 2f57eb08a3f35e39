/*
 * examples/call_pool_pitch.c -- the TRACKED pitch contour of many calls while they run: a few G.711 mu-law calls of different lengths
 * deliver a 20 ms packet per tick to ONE session pool whose slots are bound to the online pitch path (vbx_pool_path_bind).  Every
 * tick costs one more launch, whatever the number of calls, and leaves in slot s's area of the bound arrays the rows of the contour
 * that are decided by now -- a few frames behind the audio -- with their count in d_commit[s].  At hang-up the slot is marked and
 * an EMPTY tick fetches the rest of the contour without audio.  Per call the rows are, bit for bit, those a one-channel vbx_session
 * bound with vbx_session_path_bind commits on the same packets.  Prints every call's frame count and its median voiced pitch.
 *
 *   gcc -std=c11 -Iinclude examples/call_pool_pitch.c -Lvox_box.rs_amd/lib -lvoxbox_hip -Wl,-rpath,$PWD/vox_box.rs_amd/lib -lm -o call_pool_pitch
 *   ./call_pool_pitch                                       (needs an MI355X)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "voxbox_hip.h"

#define CHECK(call)                                                                   \
    do {                                                                              \
        int rc_ = (call);                                                             \
        if (rc_ != VBX_SUCCESS) { fprintf(stderr, "%s: %s\n", #call, vbx_last_error(ctx)); return 1; } \
    } while (0)

#define CALLS 3                                          /* one slot each */
#define PACKET 160                                       /* 20 ms at 8 kHz */
#define KMAX 4
#define MAX_PENDING 64
#define MAX_FRAMES 400

static int by_value(const void *a, const void *b) { const double x = *(const double *)a, y = *(const double *)b; return (x > y) - (x < y); }

/* the mu-law code nearest to a 16-bit sample, by a search of the library's own table (no encoder definition needed) */
static unsigned char nearest_code(const int16_t *table, int s) {
    int best = 0;
    for (int b = 1; b < 256; b++) if (abs(table[b] - s) < abs(table[best] - s)) best = b;
    return (unsigned char)best;
}

int main(void) {
    const double rate = 8000.0;
    const size_t frame_len = 200, hop = 80;              /* 25 ms frames every 10 ms */
    const size_t length[CALLS] = {24000, 9000, 16000};   /* samples: 3 s, 1.1 s, 2 s */
    const double f0[CALLS] = {110.0, 180.0, 140.0};
    int16_t table[256];
    if (vbx_g711_table(VBX_SAMPLE_ULAW, table) != VBX_SUCCESS) return 2;
    unsigned char *codes[CALLS];
    for (int c = 0; c < CALLS; c++) {                    /* every call its own gliding tone */
        codes[c] = (unsigned char *)malloc(length[c]);
        double phase = 0.0;
        for (size_t i = 0; i < length[c]; i++) {
            phase += 2.0 * 3.14159265358979323846 * (f0[c] + 40.0 * (double)i / (double)length[c]) / rate;
            codes[c][i] = nearest_code(table, (int)lrint(9000.0 * sin(phase)));
        }
    }

    vbx_ctx *ctx = NULL;
    if (vbx_ctx_create(&ctx, 0, NULL) != VBX_SUCCESS) { fprintf(stderr, "no gfx950 device: %s\n", vbx_last_error(NULL)); return 2; }
    vbx_analysis_params p;
    memset(&p, 0, sizeof p);
    p.sample_rate = rate;
    p.pitch_threshold = 0.2; p.pitch_fmin = 75.0; p.pitch_fmax = 500.0;
    vbx_pitch_track_params track;
    memset(&track, 0, sizeof track);                     /* time_step 0: hop / sample_rate */
    track.kmax = KMAX;
    track.path.voicing_threshold = 0.45; track.path.silence_threshold = 0.03; track.path.octave_cost = 0.01;
    track.path.octave_jump_cost = 0.35; track.path.voiced_unvoiced_cost = 0.14; track.path.ceiling_hz = 600.0;
    vbx_host_audio fmt;
    memset(&fmt, 0, sizeof fmt);
    fmt.format = VBX_SAMPLE_ULAW; fmt.channels = 1;
    vbx_pool *pool = NULL;
    CHECK(vbx_pool_open(ctx, &fmt, frame_len, hop, &p, NULL, &track, CALLS, PACKET, CALLS * PACKET, &pool));

    /* the tick's own outputs (the tracked form delivers the lists; the contour does not read them) */
    const size_t rec = vbx_record_doubles_ex(&p, NULL), ld = rec + (rec & 1);
    const size_t tick_rows = CALLS * (PACKET / hop + 1);
    void *d_rec = NULL, *d_cand = NULL, *d_count = NULL, *d_peak = NULL;
    CHECK(vbx_malloc(ctx, &d_rec, tick_rows * ld * sizeof(double)));
    CHECK(vbx_malloc(ctx, &d_cand, tick_rows * KMAX * sizeof(vbx_pitch)));
    CHECK(vbx_malloc(ctx, &d_count, tick_rows * sizeof(int32_t)));
    CHECK(vbx_malloc(ctx, &d_peak, tick_rows * sizeof(double)));
    vbx_pitch_track_outputs lists;
    memset(&lists, 0, sizeof lists);
    lists.cand = (vbx_pitch *)d_cand; lists.count = (int32_t *)d_count; lists.peak = (double *)d_peak;

    /* the contours: slot s commits into rows [s * slot_rows, ...) and reports in d_commit[s]; P = the format's full scale */
    const size_t slot_rows = vbx_pool_path_slot_rows(MAX_PENDING, PACKET, hop);
    void *d_path = NULL, *d_commit = NULL;
    CHECK(vbx_malloc(ctx, &d_path, CALLS * slot_rows * sizeof(vbx_pitch)));
    CHECK(vbx_malloc(ctx, &d_commit, CALLS * sizeof(vbx_path_commit)));
    vbx_pool_path_outputs bound;
    memset(&bound, 0, sizeof bound);
    bound.out_path = (vbx_pitch *)d_path; bound.d_commit = (vbx_path_commit *)d_commit;
    CHECK(vbx_pool_path_bind(pool, 1.0, MAX_PENDING, &bound, 2, slot_rows));
    vbx_pitch *h_path = (vbx_pitch *)malloc(CALLS * slot_rows * sizeof(vbx_pitch));
    vbx_path_commit h_commit[CALLS];

    static double hz[CALLS][MAX_FRAMES];
    size_t frames[CALLS] = {0, 0, 0}, voiced[CALLS] = {0, 0, 0}, sent[CALLS] = {0, 0, 0};
    int hung_up[CALLS] = {0, 0, 0};

    for (int tick = 0;; tick++) {
        vbx_pool_entry entries[CALLS];
        int visited[CALLS] = {0, 0, 0};
        size_t n = 0, total = 0;
        for (int s = 0; s < CALLS; s++) {
            if (sent[s] == length[s]) {                  /* hang-up: the next tick ends the slot's contour, with or without audio */
                if (!hung_up[s]) { CHECK(vbx_pool_mark_utterance(pool, s)); hung_up[s] = visited[s] = 1; }
                continue;
            }
            const size_t take = length[s] - sent[s] < PACKET ? length[s] - sent[s] : PACKET;
            entries[n].stream = s; entries[n].block = codes[s] + sent[s]; entries[n].n_sample_frames = take;
            n++;
            sent[s] += take;
            visited[s] = 1;
        }
        if (!visited[0] && !visited[1] && !visited[2]) break;
        /* ONE tick: n calls' packets -- an EMPTY one (n == 0) when only the tails of calls that hung up are left to fetch */
        CHECK(vbx_pool_push(pool, entries, n, (double *)d_rec, ld, NULL, 0, &lists, NULL, &total));
        CHECK(vbx_memcpy_d2h(ctx, h_commit, d_commit, sizeof h_commit));
        CHECK(vbx_memcpy_d2h(ctx, h_path, d_path, CALLS * slot_rows * sizeof(vbx_pitch)));
        for (int s = 0; s < CALLS; s++) {
            if (!visited[s]) continue;                   /* an unvisited slot's record is the one of its last visit */
            for (int64_t j = 0; j < h_commit[s].n; j++) {
                const vbx_pitch row = h_path[(size_t)s * slot_rows + (size_t)j];
                frames[s]++;
                if (row.frequency > 0.0 && voiced[s] < MAX_FRAMES) hz[s][voiced[s]++] = row.frequency;
            }
        }
    }
    for (int c = 0; c < CALLS; c++) {
        qsort(hz[c], voiced[c], sizeof(double), by_value);
        printf("call %d: %zu samples, %zu contour rows, %zu voiced, median pitch %.2f Hz\n", c, length[c], frames[c], voiced[c],
               voiced[c] ? hz[c][voiced[c] / 2] : 0.0);
    }

    vbx_pool_close(pool);
    vbx_free(ctx, d_commit); vbx_free(ctx, d_path);
    vbx_free(ctx, d_peak); vbx_free(ctx, d_count); vbx_free(ctx, d_cand); vbx_free(ctx, d_rec);
    vbx_ctx_destroy(ctx);
    free(h_path);
    for (int c = 0; c < CALLS; c++) free(codes[c]);
    return 0;
}
