/* The C surface of include/hclib_atomic.h (inc/hclib_atomic.h:6-69 of the
 * reference): create / init / update / gather over a 12-byte {sum, max,
 * flag} element with a non-zero start value, updated by 1000 asyncs inside
 * one finish. Prints "Check results: OK" (tests/test_atomic_host.py). */
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hclib.h"
#include "hclib_atomic.h"

#define N_ASYNC 1000

typedef struct {
    int sum, max, flag;
} ele_t;

typedef struct {
    hclib_atomic_t *atomic;
    int value;
} task_arg_t;

static int n_init_calls = 0;

static void ele_init(void *ele, void *user_data) {
    ele_t *e = (ele_t *)ele;
    e->sum = *(int *)user_data; /* a non-zero start */
    e->max = -1;
    e->flag = 0;
    n_init_calls++;
}

static void ele_update(void *ele, void *user_data) {
    ele_t *e = (ele_t *)ele;
    const int v = *(int *)user_data;
    e->sum += v;
    if (v > e->max) e->max = v;
    if (v == N_ASYNC) e->flag = 1;
}

static void ele_gather(void *a, void *b, void *user_data) {
    ele_t *x = (ele_t *)a;
    const ele_t *y = (const ele_t *)b;
    x->sum += y->sum;
    if (y->max > x->max) x->max = y->max;
    x->flag = x->flag || y->flag;
    ++*(int *)user_data;
}

static void task(void *arg) {
    task_arg_t *t = (task_arg_t *)arg;
    hclib_atomic_update(t->atomic, ele_update, &t->value);
}

static void check_layout(const hclib_atomic_t *a) {
    assert(a->vals != NULL);
    assert(a->nthreads == (size_t)hclib_get_num_workers());
    assert(a->val_size == sizeof(ele_t) && sizeof(ele_t) == 12);
    assert(a->padded_val_size % CACHE_LINE_LEN_IN_BYTES == 0);
    assert(a->padded_val_size >= a->val_size);
}

static void entrypoint(void *arg) {
    (void)arg;
    int start = 5, folds = 0;
    size_t w;
    int i;
    /* create: storage from the library */
    hclib_atomic_t *atomic = hclib_atomic_create(sizeof(ele_t), ele_init, &start);
    check_layout(atomic);
    assert((size_t)n_init_calls == atomic->nthreads);
    for (w = 0; w < atomic->nthreads; ++w) {
        const ele_t *e = (const ele_t *)(atomic->vals + w * atomic->padded_val_size);
        assert(e->sum == 5 && e->max == -1 && e->flag == 0);
    }
    /* init: storage of the program's own */
    hclib_atomic_t mine;
    hclib_atomic_init(&mine, sizeof(ele_t), ele_init, &start);
    check_layout(&mine);

    task_arg_t *args = (task_arg_t *)malloc(sizeof(task_arg_t) * N_ASYNC);
    hclib_start_finish();
    for (i = 0; i < N_ASYNC; ++i) {
        args[i].atomic = (i & 1) ? &mine : atomic;
        args[i].value = i + 1;
        hclib_async(task, &args[i], NULL, 0, NULL);
    }
    hclib_end_finish();

    /* odd values 1, 3, .. 999 went to `atomic`, even ones 2, .. 1000 to `mine` */
    ele_t *r = (ele_t *)hclib_atomic_gather(atomic, ele_gather, &folds);
    assert((size_t)folds == atomic->nthreads - 1);
    assert(r->sum == 5 * (int)atomic->nthreads + 500 * 500 && r->max == 999 && r->flag == 0);
    free(r);
    r = (ele_t *)hclib_atomic_gather(&mine, ele_gather, &folds);
    assert(r->sum == 5 * (int)mine.nthreads + 500 * 501 && r->max == 1000 && r->flag == 1);
    /* gather leaves the elements alone: a second one gives the same */
    ele_t *again = (ele_t *)hclib_atomic_gather(&mine, ele_gather, &folds);
    assert(memcmp(r, again, sizeof(ele_t)) == 0);
    free(r);
    free(again);
    free(args);
    free(mine.vals);
    free(atomic->vals);
    free(atomic);
    printf("Check results: OK\n");
}

int main(void) {
    const char *deps[] = {"system"};
    hclib_launch(entrypoint, NULL, deps, 1);
    return 0;
}
