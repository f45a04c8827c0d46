/* BOTS Strassen (bots/strassen/strassen.c) against the MI355X build: the
 * driver's shape,
 *     strassen_gpu <fixture> [cutoff [band_rows]]     (cutoff: 64 in BOTS; 0 = the default)
 * with strassen_main_par's OptimizedStrassenMultiply_par replaced by one call,
 * hclib_hip_strassen, which runs the same call tree on the device's dynamic
 * dataflow. The reference fills A and B from rand(); here they come from a
 * fixture file of A, then B, then the reference's C as raw little-endian
 * doubles (n from the file's size), so that the result can be compared on the
 * bits. The call is C = A x B: the reference's KERNEL_CALL passes (C, A, B)
 * to a function declared (A, B, C), which is not restated. Prints a checksum
 * (64-bit FNV-1a) of the result's bytes, the launch's counters on one line of
 * key=value pairs, and a verdict: the reference's compare_matrix tests a
 * relative 1e-6, this one every bit.
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
        printf("Usage: ./strassen_gpu <fixture> [cutoff [band_rows]]\n");
        return;
    }
    int cutoff = g_argc > 2 ? atoi(g_argv[2]) : 0, band_rows = g_argc > 3 ? atoi(g_argv[3]) : 0;
    FILE *f = fopen(g_argv[1], "rb");
    if (!f || fseek(f, 0, SEEK_END) != 0) {
        fprintf(stderr, "cannot read %s\n", g_argv[1]);
        return;
    }
    long bytes = ftell(f);
    rewind(f);
    int n = 1;
    while ((long)n * n * 3 * (long)sizeof(double) < bytes) n *= 2;
    if ((long)n * n * 3 * (long)sizeof(double) != bytes) {
        fprintf(stderr, "%s: %ld bytes are not three square matrices of a power-of-two size\n", g_argv[1], bytes);
        fclose(f);
        return;
    }
    size_t nn = (size_t)n * n;
    double *m = (double *)malloc(4 * nn * sizeof(double)); /* A, B, the reference's C, ours */
    if (!m || fread(m, sizeof(double), 3 * nn, f) != 3 * nn) {
        fprintf(stderr, "cannot read %s\n", g_argv[1]);
        fclose(f);
        free(m);
        return;
    }
    fclose(f);
    hclib_hip_strassen_result_t res;
    printf("Computing parallel Strassen algorithm (n=%d) ", n);
    if (hclib_hip_strassen(m, m + nn, m + 3 * nn, n, cutoff, band_rows, &res) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        free(m);
        return;
    }
    printf(" completed!\n");
    printf("checksum=%llu tasks=%llu splits=%llu base=%llu tiles=%llu pre_bands=%llu combine_bands=%llu finishes=%llu "
           "check_ins=%llu workspace_bytes=%llu\n",
           (unsigned long long)fnv1a(m + 3 * nn, nn * sizeof(double)), (unsigned long long)res.tasks,
           (unsigned long long)res.splits, (unsigned long long)res.base, (unsigned long long)res.tiles,
           (unsigned long long)res.pre_bands, (unsigned long long)res.combine_bands,
           (unsigned long long)res.finishes, (unsigned long long)res.check_ins,
           (unsigned long long)res.workspace_bytes);
    printf("The computation took %f seconds\n", res.kernel_ms * 1e-3);
    if (memcmp(m + 2 * nn, m + 3 * nn, nn * sizeof(double)) == 0) {
        printf("OK\n");
        g_status = 0;
    } else {
        printf("Strassen: Wrong answer!\n");
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
