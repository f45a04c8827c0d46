/* BOTS alignment (bots/alignment_for/alignment.c, alignment_single/alignment.c)
 * against the MI355X build: the driver's shape,
 *     alignment_gpu <sequence file> <matrix file> [cutoff]
 * with pairalign_init's readseqs and pairalign's hclib_start_finish around one
 * hclib_async per sequence pair replaced by three calls,
 * hclib_hip_alignment_read_input, hclib_hip_alignment_read_matrix and
 * hclib_hip_alignment, which aligns every pair in one launch of dynamic device
 * dataflow. Prints what the reference prints with its debug output on
 * (align_end, alignment.c: "Benchmark sequences (i:j) Aligned. Score: s" for
 * every non-zero entry of bench_output), then the launch's counters on one
 * line of key=value pairs.
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

static void entrypoint(void *arg) {
    (void)arg;
    hclib_hip_alignment_input_t in;
    static hclib_hip_alignment_matrix_t mat;
    hclib_hip_alignment_result_t res;
    uint64_t bounds[6];
    if (g_argc < 3 || g_argc > 4) {
        printf("Usage: ./alignment_gpu <sequence file> <matrix file> [cutoff]\n");
        return;
    }
    const int cutoff = g_argc == 4 ? atoi(g_argv[3]) : 0;
    if (hclib_hip_alignment_read_input(g_argv[1], &in) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        return;
    }
    if (hclib_hip_alignment_read_matrix(g_argv[2], &mat) != HCLIB_HIP_OK ||
        hclib_hip_alignment_bounds(&in, cutoff, bounds) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        hclib_hip_alignment_free_input(&in);
        return;
    }
    printf("Multiple Pairwise Alignment (%d sequences)\n", in.nseqs);
    memset(&res, 0, sizeof(res));
    res.scores = (int32_t *)calloc((size_t)in.nseqs * in.nseqs, sizeof(int32_t));
    hclib_hip_alignment_pair_t *pairs = (hclib_hip_alignment_pair_t *)calloc(bounds[0] ? bounds[0] : 1, sizeof(*pairs));
    if (res.scores && pairs && hclib_hip_alignment(&in, &mat, cutoff, &res, pairs) == HCLIB_HIP_OK) {
        for (int i = 0; i < in.nseqs; i++)
            for (int j = 0; j < in.nseqs; j++)
                if (res.scores[i * in.nseqs + j] != 0)
                    printf("Benchmark sequences (%d:%d) Aligned. Score: %d\n", i + 1, j + 1, res.scores[i * in.nseqs + j]);
        long long maxsum = 0;
        for (uint64_t p = 0; p < res.pairs; p++) maxsum += pairs[p].maxscore;
        printf("completed! pairs=%llu tasks=%llu created=%llu promises=%llu pair_tasks=%llu spawn_tasks=%llu "
               "leaf_tasks=%llu matches=%llu diff_calls=%llu type2=%llu ties=%llu cells=%llu cutoff=%d maxscore_sum=%lld\n",
               (unsigned long long)res.pairs, (unsigned long long)res.tasks, (unsigned long long)res.created,
               (unsigned long long)res.promises, (unsigned long long)res.pair_tasks, (unsigned long long)res.spawn_tasks,
               (unsigned long long)res.leaf_tasks, (unsigned long long)res.matches, (unsigned long long)res.diff_calls,
               (unsigned long long)res.type2, (unsigned long long)res.ties, (unsigned long long)res.cells, res.cutoff,
               maxsum);
        printf("The computation took %f seconds\n", res.kernel_ms * 1e-3);
        g_status = res.tasks <= bounds[1] && res.diff_calls <= bounds[3] ? 0 : 1;
    } else {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
    }
    free(res.scores);
    free(pairs);
    hclib_hip_alignment_free_input(&in);
}

int main(int argc, char **argv) {
    g_argc = argc;
    g_argv = argv;
    const char *deps[] = {"system", "hip"};
    hclib_launch(entrypoint, NULL, deps, 2);
    return g_status;
}
