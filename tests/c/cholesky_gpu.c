/* test/cholesky/cholesky.cpp against the MI355X build: the driver's shape,
 *     cholesky_gpu matrixSize tileSize fileName [mode]
 * with its k-loop (two finish scopes per step, :80-124) replaced by one call,
 * hclib_hip_cholesky, which runs the same tile program as one device promise
 * DAG. mode: "exact" (the default and the one mode). Writes cholesky.out in
 * the working directory like the reference.
 *
 * The argument checks, the input reader (:57-61) and the cholesky.out writer
 * (:129-147, here over the flat factor instead of the tile versions) restate
 * the reference's driver. HClib: Copyright (c) 2013-2015, Rice University,
 * BSD 3-clause license (the reference repository's LICENSE file); the rest of
 * this file is this project's. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hclib.h"
#include "hclib_hip.h"

static int g_argc;
static char **g_argv;
static int g_status = 1;

static void entrypoint(void *arg) {
    int i, j;
    (void)arg;
    if (g_argc != 4 && g_argc != 5) {
        printf("Usage: ./Cholesky matrixSize tileSize fileName [exact] (found %d args)\n", g_argc);
        return;
    }
    int matrixSize = atoi(g_argv[1]);
    int tileSize = atoi(g_argv[2]);
    if (matrixSize <= 0 || tileSize <= 0 || matrixSize % tileSize != 0) {
        printf("Incorrect tile size %d for the matrix of size %d \n", tileSize, matrixSize);
        return;
    }
    int mode = HCLIB_HIP_CHOL_EXACT;
    if (g_argc == 5 && strcmp(g_argv[4], "exact") != 0) {
        printf("Unknown mode %s\n", g_argv[4]);
        return;
    }
    FILE *in = fopen(g_argv[3], "r");
    if (!in) {
        printf("Cannot find file: %s\n", g_argv[3]);
        return;
    }
    double *A = (double *)malloc(sizeof(double) * matrixSize * matrixSize);
    for (i = 0; i < matrixSize; ++i) {
        for (j = 0; j < matrixSize - 1; ++j)
            if (fscanf(in, "%lf ", &A[(size_t)i * matrixSize + j]) != 1) goto bad_input;
        if (fscanf(in, "%lf\n", &A[(size_t)i * matrixSize + j]) != 1) goto bad_input;
    }
    fclose(in);

    hclib_hip_cholesky_result_t res;
    int rc = hclib_hip_cholesky(A, matrixSize, tileSize, mode, A, &res);
    if (rc != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        free(A);
        return;
    }
    printf("The computation took %f seconds\r\n", res.kernel_ms * 1e-3);
    printf("%llu tasks (%llu potrf, %llu trsm, %llu syrk, %llu gemm), %.1f GFLOP/s\n",
           (unsigned long long)res.tasks, (unsigned long long)res.potrf, (unsigned long long)res.trsm,
           (unsigned long long)res.syrk, (unsigned long long)res.gemm, res.gflops);

    FILE *out = fopen("cholesky.out", "w");
    if (!out) {
        printf("Cannot write cholesky.out\n");
        free(A);
        return;
    }
    for (i = 0; i < matrixSize; ++i)
        for (j = 0; j <= i; ++j) fprintf(out, "%lf ", A[(size_t)i * matrixSize + j]);
    fclose(out);
    free(A);
    g_status = 0;
    return;
bad_input:
    printf("Cannot read %d x %d numbers from %s\n", matrixSize, matrixSize, g_argv[3]);
    fclose(in);
    free(A);
}

int main(int argc, char **argv) {
    g_argc = argc;
    g_argv = argv;
    const char *deps[] = {"system", "hip"};
    hclib_launch(entrypoint, NULL, deps, 2);
    return g_status;
}
