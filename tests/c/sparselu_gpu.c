/* BOTS sparselu (sparselu_single / sparselu_for) against the MI355X build: the
 * driver's shape,
 *     sparselu_gpu [matrixSize [submatrixSize]]     (the reference's -n / -m; 50 and 100)
 * with sparselu_init's genmat as hclib_hip_sparselu_genmat and the kk loop of
 * sparselu_par_call (two finish scopes per step in the HClib port) replaced by
 * one call, hclib_hip_sparselu, which runs the same block program as one
 * device promise DAG. Prints the reference's print_structure picture of the
 * matrix before and after (sparselu.ref.c:137-149) and a checksum of the
 * result: the sum of the float32 bit patterns of its blocks, modulo 2^64.
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

/* one line per block row, 'x' for a present block and ' ' for an absent one,
 * under the heading the reference prints (its picture, sparselu.ref.c:137-149) */
static void show_structure(const uint8_t *mask, int S) {
    char *line = (char *)malloc((size_t)S + 2);
    printf("Structure for matrix benchmark\n");
    for (int r = 0; r < S; ++r) {
        for (int c = 0; c < S; ++c) line[c] = mask[(size_t)r * S + c] ? 'x' : ' ';
        line[S] = '\n';
        line[S + 1] = 0;
        fputs(line, stdout);
    }
    putchar('\n');
    free(line);
}

static void entrypoint(void *arg) {
    (void)arg;
    int S = g_argc > 1 ? atoi(g_argv[1]) : 50;
    int B = g_argc > 2 ? atoi(g_argv[2]) : 100;
    if (g_argc > 3 || S < 1 || B < 1) {
        printf("Usage: ./sparselu_gpu [matrixSize [submatrixSize]]\n");
        return;
    }
    uint8_t *mask = (uint8_t *)malloc((size_t)S * S), *mask_out = (uint8_t *)malloc((size_t)S * S);
    uint64_t counts[6];
    float *blocks = NULL, *out = NULL;
    if (hclib_hip_sparselu_genmat(S, B, mask, NULL) != HCLIB_HIP_OK ||
        hclib_hip_sparselu_plan(mask, S, NULL, counts, NULL, NULL, NULL) != HCLIB_HIP_OK)
        goto fail;
    blocks = (float *)malloc(counts[4] * (size_t)B * B * sizeof(float));
    out = (float *)malloc(counts[5] * (size_t)B * B * sizeof(float));
    if (hclib_hip_sparselu_genmat(S, B, mask, blocks) != HCLIB_HIP_OK) goto fail;
    show_structure(mask, S);

    printf("Computing SparseLU Factorization (%dx%d matrix with %dx%d blocks) ", S, S, B, B);
    hclib_hip_sparselu_result_t res;
    if (hclib_hip_sparselu(mask, blocks, S, B, mask_out, out, &res) != HCLIB_HIP_OK) goto fail;
    printf(" completed!\n");
    printf("The computation took %f seconds\n", res.kernel_ms * 1e-3);
    printf("%llu tasks (%llu lu0, %llu fwd, %llu bdiv, %llu bmod), %llu -> %llu blocks, %.1f GFLOP/s\n",
           (unsigned long long)res.tasks, (unsigned long long)res.lu0, (unsigned long long)res.fwd,
           (unsigned long long)res.bdiv, (unsigned long long)res.bmod, (unsigned long long)res.blocks_in,
           (unsigned long long)res.blocks_out, res.gflops);
    show_structure(mask_out, S);
    {
        uint64_t sum = 0;
        size_t e, n = (size_t)res.blocks_out * B * B;
        for (e = 0; e < n; ++e) {
            uint32_t bits;
            memcpy(&bits, &out[e], sizeof bits);
            sum += bits;
        }
        printf("checksum %llu\n", (unsigned long long)sum);
    }
    g_status = 0;
    goto done;
fail:
    fprintf(stderr, "%s\n", hclib_hip_last_error());
done:
    free(mask);
    free(mask_out);
    free(blocks);
    free(out);
}

int main(int argc, char **argv) {
    g_argc = argc;
    g_argv = argv;
    const char *deps[] = {"system", "hip"};
    hclib_launch(entrypoint, NULL, deps, 2);
    return g_status;
}
