/* CPU baseline of the NTT over G1 points (tools/bench_g1_ntt.py): the transform ark-poly's generic fft / ifft runs over a Vec<G1Projective>,
 * over the C oracle's point arithmetic (oracle/field.h, oracle/curve_tmpl.h: Jacobian doubling and addition, binary double-and-add), the
 * butterflies of a level shared among threads.  Independent of the library: its own in-place decimation in frequency and a bit reversal.
 *   g1_ntt_ref <in> <out>
 *   in:  u32 log_n, inverse, threads, 0; 2^(log_n - 1) twiddles w^e and then 1 / n, 32 B canonical integers; 2^log_n x 96 B affine points
 *   out: 2^log_n x 144 B Jacobian points, natural order; f64 seconds of the transform alone */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "../../oracle/field.h"

static inline fp fp_one(void) { return FP_ONE; }
#define FE fp
#define F(x) fp_##x
#define G(x) g1_##x
#include "../../oracle/curve_tmpl.h"

static void mul_jac(g1_jac *r, const g1_jac *p, const uint64_t *s) {
    g1_jac acc;
    g1_jac_set_inf(&acc);
    for (int i = 255; i >= 0; i--) {
        g1_jac_double(&acc, &acc);
        if ((s[i >> 6] >> (i & 63)) & 1) g1_jac_add(&acc, &acc, p);
    }
    *r = acc;
}

typedef struct {
    g1_jac *x;
    const uint64_t *tw, *ninv;
    size_t n, half, step, lo, hi;
    int scale;
} job;

static void *level_worker(void *arg) {
    job *jb = (job *)arg;
    for (size_t i = jb->lo; i < jb->hi; i++) {
        if (jb->scale) {   /* the factor 1 / n of the inverse direction: n multiplications, as ark-poly applies it */
            mul_jac(&jb->x[i], &jb->x[i], jb->ninv);
            continue;
        }
        const size_t j = i % jb->half, s = (i / jb->half) * 2 * jb->half;
        g1_jac a = jb->x[s + j], b = jb->x[s + j + jb->half], nb = b, d;
        fp_neg(&nb.y, &b.y);
        g1_jac_add(&jb->x[s + j], &a, &b);
        g1_jac_add(&d, &a, &nb);
        if (j != 0) mul_jac(&d, &d, jb->tw + 4 * (j * jb->step));
        jb->x[s + j + jb->half] = d;
    }
    return NULL;
}

static void run(job proto, size_t count, unsigned threads) {
    pthread_t th[64];
    job jobs[64];
    for (unsigned t = 0; t < threads; t++) {
        jobs[t] = proto;
        jobs[t].lo = count * t / threads;
        jobs[t].hi = count * (t + 1) / threads;
        pthread_create(&th[t], NULL, level_worker, &jobs[t]);
    }
    for (unsigned t = 0; t < threads; t++) pthread_join(th[t], NULL);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hd[4];
    if (fread(hd, sizeof hd, 1, f) != 1) return 2;
    const unsigned log_n = hd[0], inverse = hd[1], threads = hd[2];
    if (log_n < 1 || log_n > 20 || threads < 1 || threads > 64) return 2;
    const size_t n = (size_t)1 << log_n;
    uint64_t *tw = malloc((n / 2 + 1) * 32);
    g1_affine *in = malloc(n * sizeof(g1_affine));
    g1_jac *x = malloc(n * sizeof(g1_jac)), *y = malloc(n * sizeof(g1_jac));
    if (!tw || !in || !x || !y || fread(tw, 32, n / 2 + 1, f) != n / 2 + 1 || fread(in, sizeof(g1_affine), n, f) != n) return 2;
    fclose(f);
    for (size_t i = 0; i < n; i++) {
        if (g1_aff_is_inf(&in[i])) g1_jac_set_inf(&x[i]);
        else g1_jac_from_affine(&x[i], &in[i]);
    }
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    job proto = {x, tw, tw + 4 * (n / 2), n, 0, 0, 0, 0, 0};
    for (unsigned l = 0; l < log_n; l++) {
        proto.half = n >> (l + 1);
        proto.step = (size_t)1 << l;
        run(proto, n / 2, threads);
    }
    if (inverse) {
        proto.scale = 1;
        run(proto, n, threads);
    }
    for (size_t i = 0; i < n; i++) {   /* the levels above leave bit-reversed order */
        size_t r = 0;
        for (unsigned b = 0; b < log_n; b++) r |= ((i >> b) & 1) << (log_n - 1 - b);
        y[r] = x[i];
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double secs = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    FILE *g = fopen(argv[2], "wb");
    if (!g || fwrite(y, sizeof(g1_jac), n, g) != n || fwrite(&secs, 8, 1, g) != 1) return 2;
    fclose(g);
    return 0;
}
