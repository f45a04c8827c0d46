/* Rodinia CFD (rodinia/cfd/euler3d_cpu_double.cpp) against the MI355X build:
 * the reference's main in its shape,
 *     cfd_gpu <mesh file> [output directory [iterations [block [form]]]]
 * with its steps kept: the reader (:417-455, here hclib_hip_cfd_read_input,
 * called once for the sizes and once to fill), the far field as the initial
 * state (variables0 = NULL), the loop over iterations and Runge-Kutta stages
 * with its 41 sweeps and waits (:470-482) replaced by one call, hclib_hip_cfd,
 * which runs all of them as one launch of the device promise DAG, and dump()
 * (:84-111): density, momentum and density_energy in the output directory (the
 * current one by default), a number as an ostream prints a double by default,
 * which is %g. Prints the launch's counters on one line of key=value pairs.
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

static FILE *open_out(const char *dir, const char *name, int nel, int nelr) {
    char path[4096];
    snprintf(path, sizeof(path), "%s/%s", dir, name);
    FILE *f = fopen(path, "w");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", path);
        return NULL;
    }
    fprintf(f, "%d %d\n", nel, nelr);
    return f;
}

static int dump(const char *dir, const double *variables, int nel, int nelr) {
    FILE *f = open_out(dir, "density", nel, nelr);
    if (!f) return 1;
    for (int i = 0; i < nel; i++) fprintf(f, "%g\n", variables[i * 5 + 0]);
    fclose(f);
    if (!(f = open_out(dir, "momentum", nel, nelr))) return 1;
    for (int i = 0; i < nel; i++) {
        for (int j = 0; j != 3; j++) fprintf(f, "%g ", variables[i * 5 + (1 + j)]);
        fprintf(f, "\n");
    }
    fclose(f);
    if (!(f = open_out(dir, "density_energy", nel, nelr))) return 1;
    for (int i = 0; i < nel; i++) fprintf(f, "%g\n", variables[i * 5 + 4]);
    fclose(f);
    return 0;
}

static void entrypoint(void *arg) {
    (void)arg;
    if (g_argc < 2) {
        printf("specify data file name\n");
        return;
    }
    const char *data_file_name = g_argv[1], *dir = g_argc > 2 ? g_argv[2] : ".";
    const int iterations = g_argc > 3 ? atoi(g_argv[3]) : 5, block = g_argc > 4 ? atoi(g_argv[4]) : 0;
    int form = HCLIB_HIP_CFD_DAG;
    if (g_argc > 5) {
        if (!strcmp(g_argv[5], "phases")) form = HCLIB_HIP_CFD_PHASES;
        else if (strcmp(g_argv[5], "dag")) {
            printf("*****ERROR: the form is dag or phases\n");
            return;
        }
    }
    /* read in domain geometry */
    int64_t counts[2];
    if (hclib_hip_cfd_read_input(data_file_name, NULL, NULL, NULL, counts) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        return;
    }
    const int nel = (int)counts[0], nelr = (int)counts[1];
    double *areas = (double *)malloc((size_t)nelr * sizeof(double));
    int *elements_surrounding_elements = (int *)malloc((size_t)nelr * 4 * sizeof(int));
    double *normals = (double *)malloc((size_t)nelr * 12 * sizeof(double));
    double *variables = (double *)malloc((size_t)nelr * 5 * sizeof(double));
    if (areas && elements_surrounding_elements && normals && variables) {
        hclib_hip_cfd_result_t res;
        if (hclib_hip_cfd_read_input(data_file_name, areas, elements_surrounding_elements, normals, counts) != HCLIB_HIP_OK) {
            fprintf(stderr, "%s\n", hclib_hip_last_error());
        } else {
            printf("Starting...\n");
            if (hclib_hip_cfd(nel, areas, elements_surrounding_elements, normals, NULL, iterations, block, form, variables,
                              &res) != HCLIB_HIP_OK) {
                fprintf(stderr, "%s\n", hclib_hip_last_error());
            } else {
                printf("nel=%d nelr=%d tasks=%llu puts=%llu stages=%llu bytes_moved=%llu block=%d form=%d\n", nel, nelr,
                       (unsigned long long)res.tasks, (unsigned long long)res.puts, (unsigned long long)res.stages,
                       (unsigned long long)res.bytes_moved, res.block, res.form);
                printf("The computation took %f seconds\n", res.kernel_ms * 1e-3);
                printf("Saving solution...\n");
                if (dump(dir, variables, nel, nelr) == 0) {
                    printf("Saved solution...\n");
                    g_status = 0;
                }
            }
        }
    }
    printf("Cleaning up...\n");
    free(areas);
    free(elements_surrounding_elements);
    free(normals);
    free(variables);
    if (g_status == 0) printf("Done...\n");
}

int main(int argc, char **argv) {
    g_argc = argc;
    g_argv = argv;
    const char *deps[] = {"system", "hip"};
    hclib_launch(entrypoint, NULL, deps, 2);
    return g_status;
}
