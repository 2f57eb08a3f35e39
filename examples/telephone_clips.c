/*
 * examples/telephone_clips.c -- a G.711 call recording analysed without a host decode: the WAV header is parsed here (container
 * parsing stays with the caller), the one-byte samples go to the device as they are, and vbx_analyze_clips reads them as
 * VBX_SAMPLE_ULAW or VBX_SAMPLE_ALAW -- the decode to 16-bit linear PCM happens inside the call's own pack kernel.  The recording is
 * cut into clips of a few seconds, as a corpus loader would hand them over; every clip's rows are those of the resident frame loop on
 * the decoded clip alone, bit for bit.  Prints every clip's median pitch.
 *
 *   WAV format tag 7 = mu-law -> VBX_SAMPLE_ULAW, 6 = A-law -> VBX_SAMPLE_ALAW (the tags are NOT the library's constants), tag 1 with
 *   8 bits per sample = unsigned PCM -> VBX_SAMPLE_U8.
 *
 *   gcc -std=c11 -Iinclude examples/telephone_clips.c -Lvox_box.rs_amd/lib -lvoxbox_hip \
 *       -Wl,-rpath,$PWD/vox_box.rs_amd/lib -lm -o telephone_clips
 *   ./telephone_clips call.wav [clip_seconds]            (needs an MI355X; without a file a synthetic mu-law call is analysed)
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

static int by_value(const void *a, const void *b) { const double x = *(const double *)a, y = *(const double *)b; return (x > y) - (x < y); }
static unsigned le16(const unsigned char *p) { return (unsigned)p[0] | ((unsigned)p[1] << 8); }
static unsigned long le32(const unsigned char *p) { return (unsigned long)le16(p) | ((unsigned long)le16(p + 2) << 16); }

/* a mono 8-bit WAV: its format constant, sample rate and samples (malloc'ed); 0 on success */
static int read_wav8(const char *path, int *format, double *rate, unsigned char **samples, size_t *n) {
    FILE *f = fopen(path, "rb");
    unsigned char h[12], c[8], fmt[16];
    int have_fmt = 0;
    if (!f) return 1;
    if (fread(h, 1, 12, f) != 12 || memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4)) { fclose(f); return 2; }
    while (fread(c, 1, 8, f) == 8) {
        const unsigned long len = le32(c + 4);
        if (!memcmp(c, "fmt ", 4) && len >= 16) {
            if (fread(fmt, 1, 16, f) != 16) break;
            const unsigned tag = le16(fmt), channels = le16(fmt + 2), bits = le16(fmt + 14);
            if (channels != 1 || bits != 8) { fclose(f); return 3; }
            if (tag == 7) *format = VBX_SAMPLE_ULAW; else if (tag == 6) *format = VBX_SAMPLE_ALAW; else if (tag == 1) *format = VBX_SAMPLE_U8;
            else { fclose(f); return 3; }
            *rate = (double)le32(fmt + 4);
            have_fmt = 1;
            fseek(f, (long)(len - 16 + (len & 1)), SEEK_CUR);
        } else if (!memcmp(c, "data", 4) && have_fmt) {
            *samples = (unsigned char *)malloc(len ? len : 1);
            *n = fread(*samples, 1, len, f);
            fclose(f);
            return 0;
        } else fseek(f, (long)(len + (len & 1)), SEEK_CUR);
    }
    fclose(f);
    return 2;
}

/* the mu-law code nearest to a 16-bit sample, by a search of the library's own table (no encoder definition needed) */
static unsigned char nearest_code(const int16_t *table, int s) {
    int best = 0;
    for (int b = 1; b < 256; b++) if (abs(table[b] - s) < abs(table[best] - s)) best = b;
    return (unsigned char)best;
}

int main(int argc, char **argv) {
    int format = VBX_SAMPLE_ULAW;
    double rate = 8000.0;
    unsigned char *h_codes = NULL;
    size_t n = 0;
    if (argc > 1) {
        const int e = read_wav8(argv[1], &format, &rate, &h_codes, &n);
        if (e) { fprintf(stderr, "%s: %s\n", argv[1], e == 1 ? "cannot open" : e == 2 ? "not a WAV file" : "need mono, 8 bits: mu-law, A-law or PCM"); return 2; }
    } else {                                             /* twelve seconds of a gliding tone, encoded with vbx_g711_table (host only) */
        int16_t table[256];
        if (vbx_g711_table(format, table) != VBX_SUCCESS) return 2;
        n = 96000;
        h_codes = (unsigned char *)malloc(n);
        double phase = 0.0;
        for (size_t i = 0; i < n; i++) {
            phase += 2.0 * 3.14159265358979323846 * (110.0 + 90.0 * (double)i / (double)n) / rate;
            h_codes[i] = nearest_code(table, (int)lrint(9000.0 * sin(phase)));
        }
    }
    const double clip_seconds = argc > 2 ? atof(argv[2]) : 2.5;
    const size_t clip_len = (size_t)(clip_seconds * rate) ? (size_t)(clip_seconds * rate) : 1;
    const size_t n_clips = (n + clip_len - 1) / clip_len;
    const size_t frame_len = (size_t)lrint(0.025 * rate), hop = (size_t)lrint(0.010 * rate);      /* 25 ms frames every 10 ms */

    vbx_ctx *ctx = NULL;
    if (vbx_ctx_create(&ctx, 0, NULL) != VBX_SUCCESS) { fprintf(stderr, "no gfx950 device: %s\n", vbx_last_error(NULL)); return 2; }
    void *d_codes = NULL;
    CHECK(vbx_malloc(ctx, &d_codes, n ? n : 1));                                    /* ONE byte per sample crosses the bus */
    CHECK(vbx_memcpy_h2d(ctx, d_codes, h_codes, n));
    const void **clips = (const void **)malloc((n_clips ? n_clips : 1) * sizeof(void *));
    size_t *lengths = (size_t *)malloc((n_clips ? n_clips : 1) * sizeof(size_t));
    for (size_t b = 0; b < n_clips; b++) {                                          /* an 8-bit clip may start at any byte address */
        clips[b] = (const unsigned char *)d_codes + b * clip_len;
        lengths[b] = b + 1 < n_clips ? clip_len : n - b * clip_len;
    }

    vbx_analysis_params p;
    memset(&p, 0, sizeof p);
    p.sample_rate = rate;
    p.pitch_threshold = 0.2; p.pitch_fmin = 75.0; p.pitch_fmax = 500.0;
    vbx_clip_format fmt;
    memset(&fmt, 0, sizeof fmt);
    fmt.format = format;                                                            /* group_frames 0: the library's default */

    vbx_clip_row *rows = (vbx_clip_row *)malloc((n_clips ? n_clips : 1) * sizeof(vbx_clip_row));
    size_t total = 0, groups = 0;
    CHECK(vbx_clips_plan(lengths, n_clips, frame_len, hop, fmt.group_frames, rows, &total, &groups));
    const size_t rec = vbx_record_doubles_ex(&p, NULL), ld = rec + (rec & 1);       /* [ pitch 2 ] */
    void *d_rec = NULL;
    CHECK(vbx_malloc(ctx, &d_rec, (total ? total : 1) * ld * sizeof(double)));
    CHECK(vbx_analyze_clips(ctx, clips, lengths, n_clips, &fmt, frame_len, hop, &p, NULL, NULL, (double *)d_rec, ld, NULL, NULL));
    double *h_rec = (double *)malloc((total ? total : 1) * ld * sizeof(double));
    CHECK(vbx_memcpy_d2h(ctx, h_rec, d_rec, total * ld * sizeof(double)));          /* (waits for the call's kernels) */

    double *hz = (double *)malloc((total ? total : 1) * sizeof(double));
    for (size_t b = 0; b < n_clips; b++) {
        if (rows[b].n_rows == 0) { printf("clip %zu: %zu samples, no frame\n", b, lengths[b]); continue; }
        for (int64_t j = 0; j < rows[b].n_rows; j++) hz[j] = h_rec[(size_t)(rows[b].row_start + j) * ld];
        qsort(hz, (size_t)rows[b].n_rows, sizeof(double), by_value);
        printf("clip %zu: %zu samples, %lld frames, median pitch %.2f Hz\n", b, lengths[b], (long long)rows[b].n_rows, hz[rows[b].n_rows / 2]);
    }
    printf("%s at %.0f Hz: %zu rows from %zu group(s)\n", format == VBX_SAMPLE_ULAW ? "mu-law" : format == VBX_SAMPLE_ALAW ? "A-law" : "unsigned 8-bit PCM",
           rate, total, groups);

    free(hz); free(h_rec); free(rows); free(lengths); free(clips); free(h_codes);
    vbx_free(ctx, d_rec);
    vbx_free(ctx, d_codes);
    vbx_ctx_destroy(ctx);
    return 0;
}
