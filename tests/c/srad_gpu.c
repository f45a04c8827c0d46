/* srad_gpu.c — Rodinia srad's main (test/performance-regression/full-apps/
 * rodinia/srad/srad.cpp) over the C ABI of include/hclib_hip.h: the port's two
 * hclib_forasync_future sweeps, the hclib_future_wait after each and the sums
 * the host thread runs between them are one call of hclib_hip_srad.
 *
 *   srad_gpu <j0 file> <rows> <cols> <y1> <y2> <x1> <x2> <lamda> <no. of iter> <out file> [block [dag|phases]]
 *
 * <j0 file>: rows * cols little-endian floats, the image after the reference's
 * `J = (float)exp(I)`, or "-" for the reference's own random image
 * (hclib_hip_srad_image). <out file> receives J as rows * cols floats. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hclib_hip.h"

static void usage(const char *argv0) {
    fprintf(stderr,
            "Usage: %s <j0 file> <rows> <cols> <y1> <y2> <x1> <x2> <lamda> <no. of iter> <out file> [block "
            "[dag|phases]]\n",
            argv0);
    exit(1);
}

int main(int argc, char **argv) {
    if (argc < 11 || argc > 13) usage(argv[0]);
    const int rows = atoi(argv[2]), cols = atoi(argv[3]);
    const int r1 = atoi(argv[4]), r2 = atoi(argv[5]), c1 = atoi(argv[6]), c2 = atoi(argv[7]);
    const float lambda = (float)atof(argv[8]);
    const int niter = atoi(argv[9]);
    const int block = argc > 11 ? atoi(argv[11]) : 0;
    int form = HCLIB_HIP_SRAD_DAG;
    if (argc > 12) {
        if (!strcmp(argv[12], "phases")) form = HCLIB_HIP_SRAD_PHASES;
        else if (strcmp(argv[12], "dag")) {
            fprintf(stderr, "the form is dag or phases\n");
            return 1;
        }
    }
    if (rows < 1 || cols < 1 || (rows % 16 != 0) || (cols % 16 != 0)) {
        fprintf(stderr, "rows and cols must be multiples of 16\n");
        return 1;
    }
    const size_t size_I = (size_t)cols * rows;
    float *J0 = (float *)malloc(size_I * sizeof(float)), *J = (float *)malloc(size_I * sizeof(float));
    float *q = (float *)calloc(niter > 0 ? (size_t)niter : 1, sizeof(float));
    if (!J0 || !J || !q) return 1;
    if (!strcmp(argv[1], "-")) {
        printf("Randomizing the input matrix\n");
        if (hclib_hip_srad_image(rows, cols, J0)) {
            fprintf(stderr, "%s\n", hclib_hip_last_error());
            return 1;
        }
    } else {
        FILE *f = fopen(argv[1], "rb");
        if (!f || fread(J0, sizeof(float), size_I, f) != size_I) {
            fprintf(stderr, "cannot read %zu floats from %s\n", size_I, argv[1]);
            return 1;
        }
        fclose(f);
    }
    printf("Start the SRAD main loop\n");
    hclib_hip_srad_result_t res;
    if (hclib_hip_srad(J0, rows, cols, r1, r2, c1, c2, lambda, niter, block, form, J, q, &res)) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        return 1;
    }
    printf("tasks=%llu awaits=%llu puts=%llu releases=%llu iterations=%llu bytes_moved=%llu block=%d form=%d\n",
           (unsigned long long)res.tasks, (unsigned long long)res.awaits, (unsigned long long)res.puts,
           (unsigned long long)res.releases, (unsigned long long)res.iterations, (unsigned long long)res.bytes_moved,
           res.block, res.form);
    printf("kernel %.3f ms\n", res.kernel_ms);
    for (int it = 0; it < niter; it++) {
        unsigned int b;
        memcpy(&b, &q[it], 4);
        printf("q0sqr[%d] %08x %g\n", it, b, q[it]);
    }
    FILE *o = fopen(argv[10], "wb");
    if (!o || fwrite(J, sizeof(float), size_I, o) != size_I || fclose(o)) {
        fprintf(stderr, "cannot write %s\n", argv[10]);
        return 1;
    }
    printf("Computation Done\n");
    free(J0);
    free(J);
    free(q);
    return 0;
}
