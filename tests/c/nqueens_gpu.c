/* N-Queens (bots/nqueens/nqueens.c and full-apps/nqueens.cpp) against the
 * MI355X build: the drivers' shape,
 *     nqueens_gpu [size [form [task_depth]]]     (size: 14 in BOTS, 12 in nqueens.cpp;
 *                                                  form: bots or flat; task_depth: 0 = none)
 * with find_queens / the hclib::finish around nqueens_kernel replaced by one
 * call, hclib_hip_nqueens, which runs the same call tree on the device's
 * work-stealing scheduler. Prints the count, the launch's counters on one
 * line of key=value pairs, and the reference's verdict: verify_queens
 * (nqueens.cpp:62-67, nqueens.c:226-231) compares the count with the entry of
 * its solutions table.
 *
 * HClib: Copyright (c) 2013-2015, Rice University, BSD 3-clause license (the
 * reference repository's LICENSE file); this file is this project's. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hclib.h"
#include "hclib_hip.h"

/* the reference's table (nqueens.cpp:5-23) */
static const uint64_t solutions[16] = {1,   0,    0,     2,     10,     4,       40,      92,
                                       352, 724, 2680, 14200, 73712, 365596, 2279184, 14772512};

static int g_argc;
static char **g_argv;
static int g_status = 1;

static void entrypoint(void *arg) {
    (void)arg;
    int n = g_argc > 1 ? atoi(g_argv[1]) : 12;
    const char *fname = g_argc > 2 ? g_argv[2] : "bots";
    int depth = g_argc > 3 ? atoi(g_argv[3]) : 0;
    int form = strcmp(fname, "flat") == 0 ? HCLIB_HIP_NQUEENS_FLAT : HCLIB_HIP_NQUEENS_BOTS;
    if (g_argc > 4 || (strcmp(fname, "flat") != 0 && strcmp(fname, "bots") != 0)) {
        printf("Usage: ./nqueens_gpu [size [bots|flat [task_depth]]]\n");
        return;
    }
    hclib_hip_nqueens_result_t res;
    printf("Computing N-Queens algorithm (n=%d) ", n);
    if (hclib_hip_nqueens(n, form, depth, &res, NULL) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        return;
    }
    printf(" completed!\n");
    printf("Number of solutions = %llu\n", (unsigned long long)res.solutions);
    printf("solutions=%llu tasks=%llu items=%llu scopes=%llu joins=%llu chunks_pushed=%llu chunks_stolen=%llu\n",
           (unsigned long long)res.solutions, (unsigned long long)res.tasks, (unsigned long long)res.items,
           (unsigned long long)res.scopes, (unsigned long long)res.joins, (unsigned long long)res.chunks_pushed,
           (unsigned long long)res.chunks_stolen);
    printf("The computation took %f seconds\n", res.kernel_ms * 1e-3);
    if (n > 16) {
        printf("No table entry for n=%d\n", n);
    } else if (res.solutions == solutions[n - 1]) {
        printf("OK\n");
        g_status = 0;
    } else {
        printf("Incorrect Answer\n");
    }
}

int main(int argc, char **argv) {
    g_argc = argc;
    g_argv = argv;
    const char *deps[] = {"system", "hip"};
    hclib_launch(entrypoint, NULL, deps, 2);
    return g_status;
}
