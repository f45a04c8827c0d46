/* BOTS fft (bots/fft/fft.c) against the MI355X build: the driver's shape,
 *     fft_gpu <fixture> [cutoff [band]]
 * with fft()'s `fft_aux(n, in, out, factors, W, n)` in its finish replaced by
 * one call, hclib_hip_fft, which runs the same call tree on the device's
 * dynamic dataflow. The reference fills `in` with (1.0, 1.0) and computes W
 * with libm; here both come from a fixture file of in (n pairs), W (n + 1
 * pairs) and the reference's out (n pairs) as raw little-endian doubles (n
 * from the file's size), so that the result can be compared on the bits: the
 * reference's W is an input (its last bits are libm's, no formula's). Prints a
 * checksum (64-bit FNV-1a) of the result's bytes, the launch's counters on one
 * line of key=value pairs, and a verdict: the reference's test_correctness
 * tests a relative 1e-3, this one every bit.
 *
 * HClib: Copyright (c) 2013-2015, Rice University, BSD 3-clause license (the
 * reference repository's LICENSE file); this file is this project's. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hclib.h"
#include "hclib_hip.h"

static int g_argc;
static char **g_argv;
static int g_status = 1;

static uint64_t fnv1a(const void *p, size_t bytes) {
    const unsigned char *b = (const unsigned char *)p;
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 0x100000001b3ull;
    return h;
}

static void entrypoint(void *arg) {
    (void)arg;
    if (g_argc < 2 || g_argc > 4) {
        printf("Usage: ./fft_gpu <fixture> [cutoff [band]]\n");
        return;
    }
    int cutoff = g_argc > 2 ? atoi(g_argv[2]) : 0, band = g_argc > 3 ? atoi(g_argv[3]) : 0;
    FILE *f = fopen(g_argv[1], "rb");
    if (!f || fseek(f, 0, SEEK_END) != 0) {
        fprintf(stderr, "cannot read %s\n", g_argv[1]);
        return;
    }
    long bytes = ftell(f);
    rewind(f);
    /* 2 n + 2 (n + 1) + 2 n doubles */
    long n = (bytes / (long)sizeof(double) - 2) / 6;
    if (n < 1 || n > (1L << 26) || (6 * n + 2) * (long)sizeof(double) != bytes) {
        fprintf(stderr, "%s: %ld bytes are not in, W and out of one transform\n", g_argv[1], bytes);
        fclose(f);
        return;
    }
    size_t all = (size_t)(6 * n + 2);
    double *m = (double *)malloc((all + 2 * (size_t)n) * sizeof(double)); /* in, W, the reference's out, ours */
    if (!m || fread(m, sizeof(double), all, f) != all) {
        fprintf(stderr, "cannot read %s\n", g_argv[1]);
        fclose(f);
        free(m);
        return;
    }
    fclose(f);
    const double *in = m, *w = m + 2 * n, *ref = m + 4 * n + 2;
    double *out = m + all;
    hclib_hip_fft_result_t res;
    printf("Computing FFT (n=%ld) ", n);
    if (hclib_hip_fft(in, out, (int)n, w, cutoff, band, &res) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        free(m);
        return;
    }
    printf(" completed!\n");
    printf("checksum=%llu tasks=%llu leaves=%llu calls=%llu unsh_bands=%llu twid_bands=%llu finishes=%llu check_ins=%llu "
           "bytes_moved=%llu\n",
           (unsigned long long)fnv1a(out, 2 * (size_t)n * sizeof(double)), (unsigned long long)res.tasks,
           (unsigned long long)res.leaves, (unsigned long long)res.calls, (unsigned long long)res.unsh_bands,
           (unsigned long long)res.twid_bands, (unsigned long long)res.finishes, (unsigned long long)res.check_ins,
           (unsigned long long)res.bytes_moved);
    printf("The computation took %f seconds\n", res.kernel_ms * 1e-3);
    if (memcmp(ref, out, 2 * (size_t)n * sizeof(double)) == 0) {
        printf("OK\n");
        g_status = 0;
    } else {
        printf("FFT: Wrong answer!\n");
    }
    free(m);
}

int main(int argc, char **argv) {
    g_argc = argc;
    g_argv = argv;
    const char *deps[] = {"system", "hip"};
    hclib_launch(entrypoint, NULL, deps, 2);
    return g_status;
}
