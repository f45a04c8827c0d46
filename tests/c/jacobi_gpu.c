/* Kastors jacobi (kastors-1.1/jacobi/src/poisson.c) against the MI355X build:
 * the driver's shape,
 *     jacobi_gpu [n [block [niter [fuse]]]]
 * run() with its three steps kept: rhs() and the initial estimate (here one
 * call, hclib_hip_jacobi_rhs), `sweep(nx, ny, dx, dy, f, 0, niter, u, unew,
 * block_size)` replaced by one call, hclib_hip_jacobi, which runs all niter
 * iterations as one launch of the device promise DAG, and the check against
 * a sequential sweep on the host. The reference compares the RMS errors of
 * the two results to 1e-6; this one compares every bit as well. Prints a
 * checksum (64-bit FNV-1a) of unew's bytes, the launch's counters on one line
 * of key=value pairs, and a verdict. Compile with -ffp-contract=off: the
 * host's sweep must round every operation, as the device's does.
 *
 * HClib: Copyright (c) 2013-2015, Rice University, BSD 3-clause license (the
 * reference repository's LICENSE file); this file is this project's. */
#include <math.h>
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

/* niter iterations on the host: two grids in turn, a boundary cell is f */
static void host_sweep(int nx, int ny, double dx, double dy, const double *f, int niter, double *a, double *b) {
    for (int it = 0; it < niter; ++it) {
        const double *u = it & 1 ? b : a;
        double *un = it & 1 ? a : b;
        for (int i = 0; i < nx; ++i)
            for (int j = 0; j < ny; ++j) {
                const size_t at = (size_t)i * ny + j;
                if (i == 0 || j == 0 || i == nx - 1 || j == ny - 1) un[at] = f[at];
                else un[at] = 0.25 * (u[at - ny] + u[at + 1] + u[at - 1] + u[at + ny] + f[at] * dx * dy);
            }
    }
}

static double rms_error(int nx, int ny, const double *a) {
    const double pi = 3.141592653589793;
    double v = 0.0;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const double x = (double)i / (double)(nx - 1), y = (double)j / (double)(ny - 1);
            const double d = a[(size_t)i * ny + j] - sin(pi * x * y);
            v = v + d * d;
        }
    return sqrt(v / (double)(nx * ny));
}

static void entrypoint(void *arg) {
    (void)arg;
    if (g_argc > 5) {
        printf("Usage: ./jacobi_gpu [n [block [niter [fuse]]]]\n");
        return;
    }
    /* run()'s defaults, except the block: 128 is above what a task's LDS holds */
    int n = g_argc > 1 ? atoi(g_argv[1]) : 512, block = g_argc > 2 ? atoi(g_argv[2]) : 64;
    int niter = g_argc > 3 ? atoi(g_argv[3]) : 4, fuse = g_argc > 4 ? atoi(g_argv[4]) : 0;
    if (n <= 0) n = 512;
    if (niter <= 0) niter = 4;
    const int nx = n, ny = n;
    const size_t cells = (size_t)nx * ny;
    double *m = (double *)malloc(5 * cells * sizeof(double));
    if (!m) return;
    double *f = m, *unew0 = m + cells, *unew = m + 2 * cells, *a = m + 3 * cells, *b = m + 4 * cells;
    if (block > 0 && ((nx % block) || (ny % block))) {
        printf("*****ERROR: blocsize must divide NX and NY\n");
        free(m);
        return;
    }
    const double dx = 1.0 / (double)(nx - 1), dy = 1.0 / (double)(ny - 1);
    if (hclib_hip_jacobi_rhs(nx, ny, f, unew0) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        free(m);
        return;
    }
    hclib_hip_jacobi_result_t res;
    printf("Computing Jacobi (n=%d block=%d niter=%d) ", n, block, niter);
    if (hclib_hip_jacobi(f, unew0, nx, ny, dx, dy, block, niter, fuse, unew, &res) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        free(m);
        return;
    }
    printf(" completed!\n");
    printf("checksum=%llu tasks=%llu puts=%llu supersteps=%llu bytes_moved=%llu block=%d fuse=%d\n",
           (unsigned long long)fnv1a(unew, cells * sizeof(double)), (unsigned long long)res.tasks,
           (unsigned long long)res.puts, (unsigned long long)res.supersteps, (unsigned long long)res.bytes_moved, res.block,
           res.fuse);
    printf("The computation took %f seconds\n", res.kernel_ms * 1e-3);
    memcpy(a, unew0, cells * sizeof(double));
    host_sweep(nx, ny, dx, dy, f, niter, a, b);
    const double *seq = niter & 1 ? b : a;
    const double error = rms_error(nx, ny, unew), error1 = rms_error(nx, ny, seq);
    printf("RMS error %.17g, sequential %.17g\n", error, error1);
    if (fabs(error - error1) < 1.0E-6 && memcmp(seq, unew, cells * sizeof(double)) == 0) {
        printf("OK\n");
        g_status = 0;
    } else {
        printf("Jacobi: Wrong answer!\n");
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
