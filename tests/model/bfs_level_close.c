/* bfs_level_close.c — the level-closing protocol of hclib_amd/csrc/bfs.hip
 * (BfsLevelKind: process, drain, renew) restated with C11 atomics and threads,
 * run by tests/test_bfs_model.py under ThreadSanitizer.
 *
 *   bfs_level_close <threads> <seeds>
 *
 * A thread stands for a wave: it runs items from a stack of its own, gives
 * half of them to a shared pool now and then (the chunk deques; the pool's
 * lock is the deques' hand-off and `outstanding` their termination count),
 * and when its stack runs empty it drains: the items it ran since its last
 * flush are added to the monotonic `done`, but only if there are any, and the
 * thread whose add lands on `target` opens the next level (renew) instead of
 * going idle. As in the kernel
 *   - cost and packed are atomics (relaxed), order entries are plain stores:
 *     what makes them visible to the threads that read them one level later
 *     is the release / acquire add on done, and ThreadSanitizer checks it;
 *   - target, level and lvl_off are written by the closing thread alone.
 * Checked: every level has exactly one closer; no item of level L runs before
 * level L - 1 has closed, and a level closes only after all its items ran;
 * the targets grow strictly; a drain with nothing pending adds nothing; cost,
 * the frontier sizes and order (level by level, as sets) equal a serial BFS;
 * every run terminates through `outstanding` alone (nothing spins on a
 * level). As a control the zero-sum flush is replayed with the add made: it
 * lands on the target a second time, which is why the kernel skips it. */
#include <pthread.h>
#include <sched.h>
#include <stdatomic.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAXN 400
#define MAXE (MAXN * 8)
#define SHIFT 40

typedef struct {
    uint32_t tag, a, b, c, k; /* LEVEL {L, off, n} child k / VERTEX {v, start, L} edge k */
} item_t;
enum { LEVEL = 0, VERTEX = 1 };

static int n_nodes, n_edges, source;
static int starting[MAXN], degree[MAXN], edges[MAXE];

static _Atomic int cost[MAXN];
static uint32_t order[MAXN]; /* plain on purpose */
static _Atomic uint64_t packed, done, target;
static _Atomic uint32_t level, lvl_off[MAXN + 2];

/* the checker's own books */
static _Atomic uint32_t closers[MAXN + 1], ran[MAXN + 1], closed_upto; /* closed_upto = levels closed */
static _Atomic uint32_t zero_drains, violations;
static uint64_t expect_items[MAXN + 1];

/* the pool: chunks in flight, and the termination count */
static pthread_mutex_t pool_mu = PTHREAD_MUTEX_INITIALIZER;
static item_t *pool;
static size_t pool_n, pool_cap;
/* pool_n's mirror, read before the lock is taken: an idle thread that finds
 * the pool empty takes no lock, so its probes order nothing (in the kernel a
 * probe of an empty deque is a relaxed load) */
static _Atomic size_t pool_seen;
/* threads that hold work + 1 per pooled item; relaxed throughout, so that it orders nothing either */
static _Atomic int outstanding;

/* the checker's counters are relaxed: they must not order what the protocol leaves unordered */
#define COUNT(p) atomic_fetch_add_explicit((p), 1, memory_order_relaxed)
#define READ(p) atomic_load_explicit((p), memory_order_relaxed)

#define VIOLATION(...)                        \
    do {                                      \
        COUNT(&violations);                   \
        fprintf(stderr, "VIOLATION: ");       \
        fprintf(stderr, __VA_ARGS__);         \
        fprintf(stderr, "\n");                \
    } while (0)

typedef struct {
    item_t *st;
    size_t n, cap;
    uint32_t pending, rng;
    int active, seed_root;
} worker_t;

static uint32_t rnd(uint32_t *s) {
    *s = *s * 1664525u + 1013904223u;
    return *s >> 8;
}

static void push(worker_t *w, item_t it) {
    if (w->n == w->cap) w->st = realloc(w->st, (w->cap = w->cap ? 2 * w->cap : 64) * sizeof(item_t));
    w->st[w->n++] = it;
}

static void push_template(worker_t *w, uint32_t tag, uint32_t a, uint32_t b, uint32_t c, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) push(w, (item_t){tag, a, b, c, k});
}

static void process(worker_t *w, item_t it) {
    const uint32_t L = it.tag == LEVEL ? it.a : it.c;
    if (READ(&closed_upto) < L) VIOLATION("an item of level %u ran before level %u closed", L, L - 1);
    if (READ(&closed_upto) > L) VIOLATION("an item of level %u ran after it closed", L);
    COUNT(&ran[L]);
    w->pending += 1;
    if (it.tag == LEVEL) {
        const uint32_t v = order[it.b + it.k]; /* plain read: ordered by the done chain */
        push_template(w, VERTEX, v, (uint32_t)starting[v], it.a, (uint32_t)degree[v]);
        return;
    }
    const int id = edges[it.b + it.k];
    int unset = -1;
    if (atomic_load_explicit(&cost[id], memory_order_relaxed) == -1 &&
        atomic_compare_exchange_strong_explicit(&cost[id], &unset, (int)it.c + 1, memory_order_relaxed,
                                                memory_order_relaxed)) {
        const uint64_t old =
            atomic_fetch_add_explicit(&packed, (1ull << SHIFT) + (uint64_t)degree[id], memory_order_relaxed);
        order[old >> SHIFT] = (uint32_t)id; /* plain store */
    }
}

/* drain: 1 if this thread's flush closed the open level */
static int drain(worker_t *w) {
    const uint32_t s = w->pending;
    w->pending = 0;
    if (s == 0) {
        COUNT(&zero_drains);
        return 0;
    }
    const uint64_t now = atomic_fetch_add_explicit(&done, s, memory_order_acq_rel) + s;
    return now == atomic_load_explicit(&target, memory_order_relaxed);
}

/* renew: the children of the next LEVEL template pushed, or 0 */
static uint32_t renew(worker_t *w) {
    const uint64_t p = atomic_load_explicit(&packed, memory_order_relaxed);
    const uint32_t reached = (uint32_t)(p >> SHIFT);
    const uint64_t degsum = p & ((1ull << SHIFT) - 1);
    const uint32_t L = atomic_load_explicit(&level, memory_order_relaxed);
    if (COUNT(&closers[L]) != 0) VIOLATION("level %u closed twice", L);
    if (READ(&ran[L]) != expect_items[L])
        VIOLATION("level %u closed after %u of %llu items", L, READ(&ran[L]), (unsigned long long)expect_items[L]);
    const uint32_t off = atomic_load_explicit(&lvl_off[L + 1], memory_order_relaxed);
    const uint32_t n = reached - off;
    atomic_store_explicit(&lvl_off[L + 2], reached, memory_order_relaxed);
    if (n) {
        const uint64_t t = reached + degsum;
        if (t <= atomic_load_explicit(&target, memory_order_relaxed)) VIOLATION("target does not grow at level %u", L);
        atomic_store_explicit(&target, t, memory_order_relaxed);
        atomic_store_explicit(&level, L + 1, memory_order_relaxed);
    }
    /* (the checker's: after the protocol's own stores) */
    atomic_store_explicit(&closed_upto, L + 1, memory_order_relaxed);
    push_template(w, LEVEL, L + 1, off, n, n);
    return n;
}

static pthread_barrier_t start_line; /* the threads start together, or thread 0 would be done before the last exists */
static _Atomic uint32_t stolen;

static void *worker(void *arg) {
    worker_t *w = arg;
    pthread_barrier_wait(&start_line);
    if (w->seed_root) {
        push_template(w, LEVEL, 0, 0, 1, 1);
        w->active = 1; /* outstanding starts at 1 for this thread */
    }
    for (;;) {
        if (w->n) {
            process(w, w->st[--w->n]);
            /* spill: half of a stack that has grown, on a whim */
            if (w->n >= 4 && rnd(&w->rng) % 8 == 0) {
                const size_t give = w->n / 2;
                pthread_mutex_lock(&pool_mu);
                if (pool_n + give > pool_cap) pool = realloc(pool, (pool_cap = 2 * (pool_n + give)) * sizeof(item_t));
                memcpy(pool + pool_n, w->st, give * sizeof(item_t));
                pool_n += give;
                atomic_store_explicit(&pool_seen, pool_n, memory_order_relaxed);
                atomic_fetch_add_explicit(&outstanding, (int)give, memory_order_relaxed);
                pthread_mutex_unlock(&pool_mu);
                memmove(w->st, w->st + give, (w->n - give) * sizeof(item_t));
                w->n -= give;
            }
            /* a drain with the stack not empty never happens; one with nothing
             * pending does (a thread that took an item another had already
             * counted cannot exist here, so it is provoked: drain twice) */
            continue;
        }
        if (w->active) {
            int hit = drain(w);
            if (rnd(&w->rng) % 4 == 0 && drain(w)) VIOLATION("a drain with nothing pending closed a level");
            if (hit && renew(w)) continue; /* stays active, keeps its unit */
            w->active = 0;
            atomic_fetch_sub_explicit(&outstanding, 1, memory_order_relaxed);
        }
        /* steal: up to 3 items; the taker inherits one unit and returns the rest */
        size_t take = 0;
        if (atomic_load_explicit(&pool_seen, memory_order_relaxed)) {
            pthread_mutex_lock(&pool_mu);
            take = pool_n < 3 ? pool_n : 3;
            for (size_t i = 0; i < take; ++i) push(w, pool[--pool_n]);
            atomic_store_explicit(&pool_seen, pool_n, memory_order_relaxed);
            pthread_mutex_unlock(&pool_mu);
        }
        if (take) {
            COUNT(&stolen);
            w->active = 1;
            if (take > 1) atomic_fetch_sub_explicit(&outstanding, (int)take - 1, memory_order_relaxed);
            continue;
        }
        if (atomic_load_explicit(&outstanding, memory_order_relaxed) == 0) return NULL;
        sched_yield();
    }
}

static void make_graph(uint32_t seed) {
    uint32_t s = seed * 2654435761u + 1;
    n_nodes = 1 + (int)(rnd(&s) % (seed % 3 == 0 ? 40 : MAXN));
    const int maxdeg = seed % 5 == 0 ? 1 : 1 + (int)(rnd(&s) % 8); /* maxdeg 1: chains, every level one vertex */
    n_edges = 0;
    for (int v = 0; v < n_nodes; ++v) {
        starting[v] = n_edges;
        degree[v] = (int)(rnd(&s) % (uint32_t)(maxdeg + 1));
        if (seed % 5 == 0) degree[v] = v + 1 < n_nodes ? 1 : 0;
        for (int i = 0; i < degree[v]; ++i)
            edges[n_edges++] = (seed % 5 == 0) ? v + 1 : (int)(rnd(&s) % (uint32_t)n_nodes);
    }
    source = seed % 5 == 0 ? 0 : (int)(rnd(&s) % (uint32_t)n_nodes);
}

static int ref_cost[MAXN], ref_levels;
static uint32_t ref_size[MAXN + 1];
static void serial_bfs(void) {
    static int q[MAXN];
    int head = 0, tail = 0;
    for (int v = 0; v < n_nodes; ++v) ref_cost[v] = -1;
    memset(ref_size, 0, sizeof(ref_size));
    memset(expect_items, 0, sizeof(expect_items));
    ref_cost[source] = 0;
    q[tail++] = source;
    ref_levels = 0;
    while (head < tail) {
        const int v = q[head++];
        ref_size[ref_cost[v]] += 1;
        expect_items[ref_cost[v]] += 1 + (uint64_t)degree[v];
        if (ref_cost[v] + 1 > ref_levels) ref_levels = ref_cost[v] + 1;
        for (int i = 0; i < degree[v]; ++i) {
            const int id = edges[starting[v] + i];
            if (ref_cost[id] < 0) ref_cost[id] = ref_cost[v] + 1, q[tail++] = id;
        }
    }
}

static int run(int threads, uint32_t seed) {
    make_graph(seed);
    serial_bfs();
    for (int v = 0; v < n_nodes; ++v) atomic_store(&cost[v], -1), order[v] = 0xffffffffu;
    for (int i = 0; i < MAXN + 2; ++i) atomic_store(&lvl_off[i], 0);
    for (int i = 0; i <= MAXN; ++i) atomic_store(&closers[i], 0), atomic_store(&ran[i], 0);
    atomic_store(&cost[source], 0);
    order[0] = (uint32_t)source;
    atomic_store(&lvl_off[1], 1);
    atomic_store(&packed, (1ull << SHIFT) + (uint64_t)degree[source]);
    atomic_store(&done, 0);
    atomic_store(&target, 1 + (uint64_t)degree[source]);
    atomic_store(&level, 0);
    atomic_store(&closed_upto, 0);
    atomic_store(&outstanding, 1);
    pool_n = 0;
    atomic_store(&pool_seen, 0);
    pthread_barrier_init(&start_line, NULL, (unsigned)threads);
    pthread_t th[64];
    worker_t w[64];
    memset(w, 0, sizeof(w));
    for (int t = 0; t < threads; ++t) {
        w[t].rng = seed * 977u + (uint32_t)t * 131u + 7u;
        w[t].seed_root = t == 0;
        pthread_create(&th[t], NULL, worker, &w[t]);
    }
    for (int t = 0; t < threads; ++t) pthread_join(th[t], NULL), free(w[t].st);
    pthread_barrier_destroy(&start_line);
    int bad = 0;
    for (int v = 0; v < n_nodes; ++v) bad += atomic_load(&cost[v]) != ref_cost[v];
    for (int l = 0; l <= MAXN; ++l) bad += atomic_load(&closers[l]) != (l < ref_levels ? 1u : 0u);
    for (int l = 0; l < ref_levels; ++l) {
        const uint32_t a = atomic_load(&lvl_off[l]), b = atomic_load(&lvl_off[l + 1]);
        bad += b - a != ref_size[l];
        for (uint32_t i = a; i < b && i < (uint32_t)n_nodes; ++i)
            bad += order[i] >= (uint32_t)n_nodes || ref_cost[order[i]] != l;
    }
    bad += atomic_load(&done) != atomic_load(&target) || atomic_load(&level) + 1 != (uint32_t)ref_levels;
    if (bad) fprintf(stderr, "seed %u: %d mismatches against the serial search\n", seed, bad);
    return bad;
}

/* the control: thread A's add lands on the target; before A's renew has moved
 * the target, thread B drains with nothing pending and makes the add anyway */
static int control_zero_add(void) {
    atomic_store(&done, 10);
    atomic_store(&target, 13);
    int closers_seen = 0;
    closers_seen += atomic_fetch_add(&done, 3) + 3 == atomic_load(&target); /* A: the close */
    closers_seen += atomic_fetch_add(&done, 0) + 0 == atomic_load(&target); /* B: zero sum, added */
    return closers_seen;
}

int main(int argc, char **argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 4, seeds = argc > 2 ? atoi(argv[2]) : 20;
    if (threads < 1 || threads > 64) return 2;
    int bad = 0;
    for (int s = 0; s < seeds; ++s) bad += run(threads, (uint32_t)s);
    printf("threads %d seeds %d mismatches %d violations %u steals %u zero_drains %u\n", threads, seeds, bad,
           atomic_load(&violations), atomic_load(&stolen), atomic_load(&zero_drains));
    printf("control: %d closers when a zero-sum flush is added\n", control_zero_add());
    if (bad == 0 && atomic_load(&violations) == 0) printf("MODEL OK\n");
    free(pool);
    return bad || atomic_load(&violations) ? 1 : 0;
}
