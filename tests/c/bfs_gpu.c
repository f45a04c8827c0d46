/* Rodinia BFS (rodinia/bfs/bfs.cpp) against the MI355X build: the driver's
 * shape,
 *     bfs_gpu <input_file> [level|async]
 * with BFSGraph's fscanf sequence and its do / while of two forasync sweeps
 * per level replaced by two calls, hclib_hip_bfs_read_input and hclib_hip_bfs,
 * which runs the search as one launch of the device's work-stealing scheduler.
 * Prints the reference's three lines (bfs.ref.cpp:73, 133, 193), writes
 * result.txt into the working directory in the reference's format (:189-192),
 * and prints the launch's counters on one line of key=value pairs.
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
    const char *fname = g_argc > 2 ? g_argv[2] : "level";
    if (g_argc < 2 || g_argc > 3 || (strcmp(fname, "level") != 0 && strcmp(fname, "async") != 0)) {
        fprintf(stderr, "Usage: %s <input_file> [level|async]\n", g_argv[0]);
        return;
    }
    int form = strcmp(fname, "async") == 0 ? HCLIB_HIP_BFS_ASYNC : HCLIB_HIP_BFS_LEVEL;
    printf("Reading File\n");
    int64_t counts[3];
    if (hclib_hip_bfs_read_input(g_argv[1], NULL, NULL, NULL, counts) != HCLIB_HIP_OK) {
        printf("Error Reading graph file\n");
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        return;
    }
    size_t n = (size_t)counts[0], m = (size_t)counts[1];
    int32_t *starting = malloc(4 * (n + 1)), *degree = malloc(4 * (n + 1)), *edges = malloc(4 * (m + 1)),
            *cost = malloc(4 * (n + 1));
    if (!starting || !degree || !edges || !cost) return;
    if (hclib_hip_bfs_read_input(g_argv[1], starting, degree, edges, counts) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        return;
    }
    printf("Start traversing the tree\n");
    hclib_hip_bfs_result_t res;
    if (hclib_hip_bfs(starting, degree, (int)n, edges, (int)m, (int)counts[2], form, cost, &res, NULL, NULL) !=
        HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        return;
    }
    FILE *fpo = fopen("result.txt", "w");
    if (!fpo) return;
    for (size_t i = 0; i < n; i++) fprintf(fpo, "%d) cost:%d\n", (int)i, cost[i]);
    fclose(fpo);
    printf("Result stored in result.txt\n");
    printf("levels=%llu reached=%llu relaxed=%llu items=%llu chunks_pushed=%llu chunks_stolen=%llu\n",
           (unsigned long long)res.levels, (unsigned long long)res.reached, (unsigned long long)res.relaxed,
           (unsigned long long)res.items, (unsigned long long)res.chunks_pushed,
           (unsigned long long)res.chunks_stolen);
    printf("The computation took %f seconds\n", res.kernel_ms * 1e-3);
    free(starting);
    free(degree);
    free(edges);
    free(cost);
    g_status = 0;
}

int main(int argc, char **argv) {
    g_argc = argc;
    g_argv = argv;
    const char *deps[] = {"system", "hip"};
    hclib_launch(entrypoint, NULL, deps, 2);
    return g_status;
}
