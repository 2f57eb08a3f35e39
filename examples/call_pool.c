/*
 * examples/call_pool.c -- a gateway's view of the library: a few G.711 mu-law calls of different lengths that deliver a 20 ms packet
 * per tick, analysed from ONE session pool (vbx_pool_*).  Every tick hands over the packets that arrived -- one (slot, block) entry
 * per live call -- and gets the rows of the frames they complete in one set of arrays, from one upload and a fixed number of kernel
 * launches whatever the number of calls.  One call ends early: its slot is reset and reused for a new call.  Per call the rows are,
 * bit for bit, those of a one-channel vbx_session fed the same packets.  Prints every call's frame count and median pitch.
 *
 *   gcc -std=c11 -Iinclude examples/call_pool.c -Lvox_box.rs_amd/lib -lvoxbox_hip -Wl,-rpath,$PWD/vox_box.rs_amd/lib -lm -o call_pool
 *   ./call_pool                                             (needs an MI355X)
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

#define SLOTS 3
#define CALLS 4                                          /* call 3 takes over slot 1 when call 1 has ended */
#define PACKET 160                                       /* 20 ms at 8 kHz */
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
    const size_t length[CALLS] = {24000, 9000, 16000, 12000};          /* samples: 3 s, 1.1 s, 2 s, 1.5 s */
    const double f0[CALLS] = {110.0, 180.0, 140.0, 220.0};
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
    vbx_host_audio fmt;
    memset(&fmt, 0, sizeof fmt);
    fmt.format = VBX_SAMPLE_ULAW; fmt.channels = 1;      /* the bytes are decoded inside the tick's own ingest kernel */
    vbx_pool *pool = NULL;
    CHECK(vbx_pool_open(ctx, &fmt, frame_len, hop, &p, NULL, NULL, SLOTS, PACKET, SLOTS * PACKET, &pool));

    const size_t rec = vbx_record_doubles_ex(&p, NULL), ld = rec + (rec & 1);       /* [ pitch 2 ] */
    const size_t tick_rows = SLOTS * (PACKET / hop + 1);                            /* no tick delivers more */
    void *d_rec = NULL;
    CHECK(vbx_malloc(ctx, &d_rec, tick_rows * ld * sizeof(double)));
    double *h_rec = (double *)malloc(tick_rows * ld * sizeof(double));
    static double hz[CALLS][MAX_FRAMES];
    size_t frames[CALLS] = {0, 0, 0, 0}, sent[CALLS] = {0, 0, 0, 0};
    int call_of_slot[SLOTS] = {0, 1, 2};

    for (int tick = 0;; tick++) {
        vbx_pool_entry entries[SLOTS];
        vbx_pool_rows rows[SLOTS];
        int call_of_entry[SLOTS];
        size_t n = 0, total = 0;
        for (int s = SLOTS - 1; s >= 0; s--) {           /* any order: here the slots backwards */
            int c = call_of_slot[s];
            if (c >= 0 && sent[c] == length[c]) {        /* the call has ended: the slot is free again */
                c = call_of_slot[s] = (s == 1 && c == 1) ? 3 : -1;
                if (c >= 0) CHECK(vbx_pool_reset_stream(pool, s));                  /* as a freshly opened slot */
            }
            if (c < 0) continue;
            const size_t take = length[c] - sent[c] < PACKET ? length[c] - sent[c] : PACKET;
            entries[n].stream = s; entries[n].block = codes[c] + sent[c]; entries[n].n_sample_frames = take;
            call_of_entry[n++] = c;
            sent[c] += take;
        }
        if (n == 0) break;
        CHECK(vbx_pool_push(pool, entries, n, (double *)d_rec, ld, NULL, 0, NULL, rows, &total));      /* ONE tick, n calls */
        if (total) CHECK(vbx_memcpy_d2h(ctx, h_rec, d_rec, total * ld * sizeof(double)));
        for (size_t i = 0; i < n; i++)
            for (int64_t j = 0; j < rows[i].n_rows; j++) {
                const int c = call_of_entry[i];
                if (frames[c] < MAX_FRAMES) hz[c][frames[c]++] = h_rec[(size_t)(rows[i].row_start + j) * ld];
            }
    }
    for (int c = 0; c < CALLS; c++) {
        qsort(hz[c], frames[c], sizeof(double), by_value);
        printf("call %d: %zu samples, %zu frames, median pitch %.2f Hz\n", c, length[c], frames[c], frames[c] ? hz[c][frames[c] / 2] : 0.0);
    }

    vbx_pool_close(pool);
    vbx_free(ctx, d_rec);
    vbx_ctx_destroy(ctx);
    free(h_rec);
    for (int c = 0; c < CALLS; c++) free(codes[c]);
    return 0;
}
