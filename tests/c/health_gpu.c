/* BOTS Health (bots/health/health.c) against the MI355X build: the driver's
 * shape,
 *     health_gpu <input file>
 * with read_input_data's 19 numbers (ten settings, nine expected results),
 * sim_village_main_par's loop of sim_time rounds replaced by one call,
 * hclib_hip_health, which runs every round of the village tree on the device's
 * dynamic dataflow, and check_village's comparison and table. Prints the
 * reference's "Sim. Variables" table, the launch's counters on one line of
 * key=value pairs, and a verdict.
 *
 * HClib: Copyright (c) 2013-2015, Rice University, BSD 3-clause license (the
 * reference repository's LICENSE file); this file is this project's. */
#include <stdio.h>
#include <stdlib.h>

#include "hclib.h"
#include "hclib_hip.h"

static int g_argc;
static char **g_argv;
static int g_status = 1;

static void entrypoint(void *arg) {
    (void)arg;
    if (g_argc != 2) {
        printf("Usage: ./health_gpu <input file>\n");
        return;
    }
    FILE *fin = fopen(g_argv[1], "r");
    if (!fin) {
        fprintf(stderr, "Could not open sequence file (%s)\n", g_argv[1]);
        return;
    }
    hclib_hip_health_params_t p;
    long seed;
    int e[8];
    float avg_stay;
    int res = fscanf(fin, "%d %d %d %d %d %d %ld %f %f %f %d %d %d %d %d %d %d %d %f", &p.level, &p.cities,
                     &p.population_ratio, &p.sim_time, &p.assess_time, &p.convalescence_time, &seed, &p.get_sick_p,
                     &p.convalescence_p, &p.realloc_p, &e[0], &e[1], &e[2], &e[3], &e[4], &e[5], &e[6], &e[7], &avg_stay);
    fclose(fin);
    if (res != 19) {
        fprintf(stderr, "Bogus input file (%s)\n", g_argv[1]);
        return;
    }
    p.seed = (int32_t)(uint32_t)((unsigned long)seed & 0xfffffffful); /* the low 32 bits */
    printf("Number of levels    = %d\n", p.level);
    printf("Cities per level    = %d\n", p.cities);
    printf("Population ratio    = %d\n", p.population_ratio);
    printf("Simulation time     = %d\n", p.sim_time);
    printf("Assess time         = %d\n", p.assess_time);
    printf("Convalescence time  = %d\n", p.convalescence_time);
    printf("Initial seed        = %d\n", (int)p.seed);
    printf("Get sick prob.      = %f\n", p.get_sick_p);
    printf("Convalescence prob. = %f\n", p.convalescence_p);
    printf("Realloc prob.       = %f\n", p.realloc_p);

    hclib_hip_health_result_t r;
    if (hclib_hip_health(&p, &r, NULL) != HCLIB_HIP_OK) {
        fprintf(stderr, "%s\n", hclib_hip_last_error());
        return;
    }
    const int64_t got[8] = {r.population, r.hospitals, r.personnel, r.hosps_visited,
                            r.in_village, r.waiting, r.assess, r.inside};
    static const char *const name[8] = {"Total population   ", "Hospitals          ", "Personnel          ",
                                        "Check-in's         ", "In Villages        ", "In Waiting List    ",
                                        "In Assess          ", "Inside Hospital    "};
    int ok = 1;
    printf("\nSim. Variables      = expect / result\n");
    for (int k = 0; k < 8; ++k) {
        if (got[k] != e[k]) ok = 0;
        printf("%s = %6d / %6d people\n", name[k], e[k], (int)got[k]);
    }
    printf("Average Stay        = %6f / %6f u/time\n", avg_stay, (float)r.total_time / (float)r.population);
    printf("tasks=%llu finishes=%llu check_ins=%llu leaf_calls=%llu inner_calls=%llu posts=%llu\n",
           (unsigned long long)r.tasks, (unsigned long long)r.finishes, (unsigned long long)r.check_ins,
           (unsigned long long)r.leaf_calls, (unsigned long long)r.inner_calls, (unsigned long long)r.posts);
    printf("The computation took %f seconds\n", r.kernel_ms * 1e-3);
    if (ok) {
        printf("OK\n");
        g_status = 0;
    } else {
        printf("Health: Wrong answer!\n");
    }
}

int main(int argc, char **argv) {
    g_argc = argc;
    g_argv = argv;
    const char *deps[] = {"system", "hip"};
    hclib_launch(entrypoint, NULL, deps, 2);
    return g_status;
}
