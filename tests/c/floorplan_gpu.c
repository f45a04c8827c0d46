/* BOTS floorplan (bots/floorplan/floorplan.c) against the MI355X build: the
 * driver's shape,
 *     floorplan_gpu <cell description file> [noprune]
 * with floorplan_init's read_inputs and compute_floorplan's finish around
 * add_cell(1, ...) replaced by two calls, hclib_hip_floorplan_read_input and
 * hclib_hip_floorplan, which runs the same branch-and-bound search on the
 * device's work-stealing scheduler. Prints what the reference prints
 * (write_outputs, floorplan.c:198-210: the minimum area and the lettered
 * board inside the footprint), the launch's counters on one line of key=value
 * pairs, and the reference's verdict: floorplan_verify (:387-393) compares the
 * area with the file's trailing expected solution.
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
    static hclib_hip_floorplan_input_t in;
    static uint8_t board[64 * 64];
    hclib_hip_floorplan_result_t res;
    if (g_argc < 2 || g_argc > 3 || (g_argc == 3 && strcmp(g_argv[2], "noprune") != 0)) {
        printf("Usage: ./floorplan_gpu <cell description file> [noprune]\n");
        return;
    }
    if (hclib_hip_floorplan_read_input(g_argv[1], &in) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        return;
    }
    printf("Computing floorplan ");
    if (hclib_hip_floorplan(&in, g_argc == 3 ? HCLIB_HIP_FLOORPLAN_NOPRUNE : 0, &res, board, NULL) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        return;
    }
    printf(" completed!\n");
    printf("Minimum area = %d\n\n", res.min_area);
    for (int i = 0; i < res.footprint[0]; i++) {
        for (int j = 0; j < res.footprint[1]; j++) {
            if (board[i * 64 + j] == 0) printf(" ");
            else printf("%c", 'A' + board[i * 64 + j] - 1);
        }
        printf("\n");
    }
    printf("min_area=%d rows=%d cols=%d tasks=%llu items=%llu laid=%llu complete=%llu improvements=%llu "
           "chunks_pushed=%llu chunks_stolen=%llu\n",
           res.min_area, res.footprint[0], res.footprint[1], (unsigned long long)res.tasks,
           (unsigned long long)res.items, (unsigned long long)res.laid, (unsigned long long)res.complete,
           (unsigned long long)res.improvements, (unsigned long long)res.chunks_pushed,
           (unsigned long long)res.chunks_stolen);
    printf("The computation took %f seconds\n", res.kernel_ms * 1e-3);
    if (in.solution == -1) {
        printf("No expected solution in %s\n", g_argv[1]);
    } else if (res.min_area == in.solution) {
        printf("OK\n");
        g_status = 0;
    } else {
        printf("FAIL\n");
    }
}

int main(int argc, char **argv) {
    g_argc = argc;
    g_argv = argv;
    const char *deps[] = {"system", "hip"};
    hclib_launch(entrypoint, NULL, deps, 2);
    return g_status;
}
