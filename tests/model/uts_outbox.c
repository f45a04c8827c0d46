/* CPU model of the hand-off wave's outbox protocol (include/hclib_hip/
 * hx_sched.h: Inbox, inbox_claim / inbox_fill, narrow_shed's and run_worker's
 * outbox puts, comm_wave, wave_goes_idle), restated in C11 atomics and
 * threads. One "workgroup": W worker threads with an inbox each, two
 * outboxes, one comm thread, one shared deque standing for the HBM deques.
 *
 * The device's rules, as modelled:
 *  - a box's state word: 0 empty, 2 being filled, 1 full, 3 closed. A claim is
 *    a CAS 0 -> 2; the filler writes the items (plain stores), takes the
 *    block's unit of `outstanding`, then stores n and state = 1 (one wave's
 *    LDS operations land in order: a release store here, an acquire load at
 *    the reader);
 *  - a worker holds one unit while it has work; the worker whose decrement
 *    takes `outstanding` to 0 sets `done`; idle workers leave on `done`, close
 *    their inbox (CAS 0 -> 3) and count themselves in `left`;
 *  - the comm thread serves full outboxes: to a sibling that is idle with an
 *    empty inbox (redirect; the unit travels with the block, no add), else to
 *    the deque with the unit already held. It leaves when left == W and both
 *    outboxes are empty, and never reads `outstanding`.
 *
 * Work is a random tree: an item is a node (seed, depth); running it counts
 * it and pushes its children. Every block that changes hands carries a
 * unique id. Checked per schedule: the nodes run equal a serial walk; every
 * block id is taken exactly once (none lost, none doubled); `outstanding`
 * reaches zero exactly once and ends at zero; blocks put into outboxes equal
 * blocks the comm thread passed on; every box ends empty or closed; the
 * deque ends empty. ThreadSanitizer checks that the plain item stores are
 * ordered by the state words alone.
 *
 *   uts_outbox <workers> <schedules> <users>    users: bits 1 give-away,
 *                                               2 shed, 4 redirect (0: no comm thread)
 */
#include <pthread.h>
#include <sched.h>
#include <stdatomic.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAXW 8
#define BLK 16      /* items per block at most */
#define STACK 4096  /* a worker's local stack */
#define DQ 4096     /* deque slots */
#define MAXBLOCKS (1 << 16)

typedef struct {
    uint32_t seed, depth;
} item_t;

typedef struct {
    _Atomic uint32_t state;
    _Atomic uint32_t idle;
    uint32_t n, id; /* plain: ordered by `state` */
    item_t w[BLK];
} box_t;

static int W, users;
static box_t inbox[MAXW], outbox[2];
static _Atomic uint32_t outstanding, done_flag, left, zero_hits, next_id, err;
static _Atomic uint32_t taken[MAXBLOCKS];
static _Atomic uint64_t nodes_run;
static _Atomic uint32_t c_out_main, c_out_shed, c_to_deque, c_to_sib, c_busy, c_sib_direct, c_dq_direct;

/* the deque: a mutex-protected FIFO of blocks (its own protocol is not under test) */
static pthread_mutex_t dq_mu = PTHREAD_MUTEX_INITIALIZER;
static struct {
    uint32_t n, id;
    item_t w[BLK];
} dq[DQ];
static uint32_t dq_head, dq_tail;

static uint32_t mix(uint32_t x) {
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}
/* children of a node: a BIN-like rule, m = 3 with probability ~ 0.36 down to depth 14 */
static uint32_t nchildren(item_t it) { return it.depth < 14 && mix(it.seed) % 100 < 36 ? 3u : 0u; }
static item_t child(item_t it, uint32_t k) {
    item_t c = {mix(it.seed * 0x9e3779b9u + k + 1u), it.depth + 1};
    return c;
}
static uint64_t serial(item_t it) {
    uint64_t n = 1;
    for (uint32_t k = 0, nc = nchildren(it); k < nc; ++k) n += serial(child(it, k));
    return n;
}

static void fail(const char *what) {
    fprintf(stderr, "VIOLATION: %s\n", what);
    atomic_store(&err, 1);
}

static void jitter(uint32_t *rng) {
    *rng = mix(*rng + 0x632be5abu);
    if ((*rng & 7) == 0) sched_yield();
}

/* inbox_claim + inbox_fill: the items, the unit, n, idle = 0, state = 1 */
static int box_put(box_t *b, const item_t *src, uint32_t n) {
    uint32_t z = 0;
    if (!atomic_compare_exchange_strong_explicit(&b->state, &z, 2, memory_order_acquire, memory_order_relaxed)) return 0;
    memcpy(b->w, src, n * sizeof(item_t));
    b->n = n;
    b->id = atomic_fetch_add(&next_id, 1);
    if (b->id >= MAXBLOCKS) fail("too many blocks for the model");
    atomic_fetch_add(&outstanding, 1); /* before the block becomes visible */
    atomic_store_explicit(&b->idle, 0, memory_order_relaxed);
    atomic_store_explicit(&b->state, 1, memory_order_release);
    return 1;
}

/* enqueue_chunk: held = the unit was taken at the fill */
static int dq_put(const item_t *src, uint32_t n, uint32_t id, int held) {
    pthread_mutex_lock(&dq_mu);
    if (dq_tail - dq_head >= DQ) {
        pthread_mutex_unlock(&dq_mu);
        return 0;
    }
    if (!held) atomic_fetch_add(&outstanding, 1);
    memcpy(dq[dq_tail % DQ].w, src, n * sizeof(item_t));
    dq[dq_tail % DQ].n = n;
    dq[dq_tail % DQ].id = id;
    ++dq_tail;
    pthread_mutex_unlock(&dq_mu);
    return 1;
}
static uint32_t dq_take(item_t *dst) {
    uint32_t n = 0;
    pthread_mutex_lock(&dq_mu);
    if (dq_tail != dq_head) {
        n = dq[dq_head % DQ].n;
        memcpy(dst, dq[dq_head % DQ].w, n * sizeof(item_t));
        if (atomic_fetch_add(&taken[dq[dq_head % DQ].id], 1) != 0) fail("a deque block was taken twice");
        ++dq_head;
    }
    pthread_mutex_unlock(&dq_mu);
    return n;
}

typedef struct {
    int wave;
    uint32_t rng;
    int root;
    item_t root_item;
} wk_t;

/* give `n` items away: an idle sibling, then (users & bit) an outbox, then the deque */
static int give(wk_t *me, const item_t *src, uint32_t n, int bit) {
    for (int a = 1; a < W; ++a) {
        box_t *b = &inbox[(me->wave + a) % W];
        if (atomic_load_explicit(&b->idle, memory_order_relaxed) == 1 &&
            atomic_load_explicit(&b->state, memory_order_relaxed) == 0 && box_put(b, src, n)) {
            atomic_fetch_add(&c_sib_direct, 1);
            return 1;
        }
    }
    if (users & bit) {
        for (int o = 0; o < 2; ++o)
            if (atomic_load_explicit(&outbox[o].state, memory_order_relaxed) == 0 && box_put(&outbox[o], src, n)) {
                atomic_fetch_add(bit == 1 ? &c_out_main : &c_out_shed, 1);
                return 1;
            }
        atomic_fetch_add(&c_busy, 1);
    }
    if (bit == 2) return 0; /* narrow_shed: what finds no box stays with the wave (the ring) */
    if (dq_put(src, n, atomic_fetch_add(&next_id, 1), 0)) {
        atomic_fetch_add(&c_dq_direct, 1);
        return 1;
    }
    return 0;
}

static void *worker(void *arg) {
    wk_t *me = (wk_t *)arg;
    static _Thread_local item_t st[STACK];
    uint32_t top = 0;
    int active = 0;
    box_t *mine = &inbox[me->wave];
    if (me->root) { /* the host set outstanding = 1 for this worker */
        st[top++] = me->root_item;
        active = 1;
    }
    uint64_t spins = 0;
    while (!atomic_load(&err)) {
        if (top == 0) {
            if (active) {
                active = 0;
                const uint32_t prev = atomic_fetch_sub_explicit(&outstanding, 1, memory_order_acq_rel);
                if (prev == 0) fail("outstanding underflow");
                if (prev == 1) {
                    atomic_fetch_add(&zero_hits, 1);
                    atomic_store_explicit(&done_flag, 1, memory_order_release);
                }
                atomic_store_explicit(&mine->idle, 1, memory_order_relaxed);
            }
            /* the inbox first, then the deque; both inherit the block's unit */
            if (atomic_load_explicit(&mine->state, memory_order_acquire) == 1) {
                top = mine->n;
                memcpy(st, mine->w, top * sizeof(item_t));
                if (atomic_fetch_add(&taken[mine->id], 1) != 0) fail("an inbox block was taken twice");
                atomic_store_explicit(&mine->state, 0, memory_order_release);
            } else {
                top = dq_take(st);
            }
            if (top) {
                atomic_store_explicit(&mine->idle, 0, memory_order_relaxed);
                active = 1;
                spins = 0;
                continue;
            }
            if (atomic_load_explicit(&done_flag, memory_order_acquire)) break;
            if (++spins > 200000000ull) {
                fail("a worker's idle spin timed out (no termination)");
                break;
            }
            sched_yield();
            continue;
        }
        /* one "batch": run the top item, push its children */
        jitter(&me->rng);
        const item_t it = st[--top];
        atomic_fetch_add_explicit(&nodes_run, 1, memory_order_relaxed);
        const uint32_t nc = nchildren(it);
        if (top + nc > STACK) {
            fail("local stack overflow");
            break;
        }
        for (uint32_t k = 0; k < nc; ++k) st[top++] = child(it, k);
        me->rng = mix(me->rng + it.seed);
        /* the narrow loop's overflow exit: several blocks at once, keeping some */
        if (top >= 6 && (me->rng & 3) == 0) {
            while (top > 3) {
                const uint32_t n = top - 3 < BLK ? top - 3 : BLK;
                if (!give(me, st + top - n, n, 2)) break;
                top -= n;
            }
        } else if (top >= 2 && (me->rng & 3) == 1) {
            /* the give-away loop: the oldest half as one block */
            uint32_t n = (top + 1) / 2;
            if (n > BLK) n = BLK;
            if (n < top && give(me, st, n, 1)) {
                memmove(st, st + n, (top - n) * sizeof(item_t));
                top -= n;
            }
        }
    }
    if (active) atomic_fetch_sub(&outstanding, 1); /* error exits only */
    /* close the inbox: nothing may be put there afterwards */
    atomic_store_explicit(&mine->idle, 0, memory_order_relaxed);
    uint32_t z = 0;
    atomic_compare_exchange_strong(&mine->state, &z, 3);
    atomic_fetch_add_explicit(&left, 1, memory_order_release);
    return NULL;
}

static void *comm(void *arg) {
    uint32_t rng = *(uint32_t *)arg;
    uint64_t spins = 0;
    while (!atomic_load(&err)) {
        int served = 0;
        for (int o = 0; o < 2; ++o) {
            box_t *b = &outbox[o];
            if (atomic_load_explicit(&b->state, memory_order_acquire) != 1) continue;
            served = 1;
            jitter(&rng);
            int placed = 0;
            if (users & 4) {
                for (int a = 0; a < W && !placed; ++a) {
                    box_t *to = &inbox[a];
                    uint32_t z = 0;
                    if (atomic_load_explicit(&to->idle, memory_order_relaxed) != 1 ||
                        atomic_load_explicit(&to->state, memory_order_relaxed) != 0 ||
                        !atomic_compare_exchange_strong_explicit(&to->state, &z, 2, memory_order_acquire,
                                                                 memory_order_relaxed))
                        continue;
                    /* LDS to LDS: the unit travels with the block, no second add */
                    memcpy(to->w, b->w, b->n * sizeof(item_t));
                    to->n = b->n;
                    to->id = b->id;
                    atomic_store_explicit(&to->idle, 0, memory_order_relaxed);
                    atomic_store_explicit(&to->state, 1, memory_order_release);
                    atomic_fetch_add(&c_to_sib, 1);
                    placed = 1;
                }
            }
            while (!placed && !atomic_load(&err)) {
                placed = dq_put(b->w, b->n, b->id, 1);
                if (placed) atomic_fetch_add(&c_to_deque, 1);
                else sched_yield();
            }
            atomic_store_explicit(&b->state, 0, memory_order_release);
        }
        if (served) {
            spins = 0;
            continue;
        }
        if (atomic_load_explicit(&left, memory_order_acquire) == (uint32_t)W &&
            atomic_load_explicit(&outbox[0].state, memory_order_acquire) == 0 &&
            atomic_load_explicit(&outbox[1].state, memory_order_acquire) == 0)
            break;
        if (++spins > 400000000ull) {
            fail("the comm thread's nap timed out");
            break;
        }
        sched_yield();
    }
    return NULL;
}

int main(int argc, char **argv) {
    W = argc > 1 ? atoi(argv[1]) : 4;
    const int schedules = argc > 2 ? atoi(argv[2]) : 20;
    users = argc > 3 ? atoi(argv[3]) : 7;
    if (W < 2 || W > MAXW || users < 0 || users > 7) {
        fprintf(stderr, "usage: uts_outbox <workers 2..8> <schedules> <users 0..7>\n");
        return 2;
    }
    uint64_t tot_nodes = 0, tot_out = 0, tot_sib = 0, tot_dq = 0, tot_busy = 0, tot_blocks = 0;
    int bad = 0;
    for (int s = 0; s < schedules && !bad; ++s) {
        memset(inbox, 0, sizeof(inbox));
        memset(outbox, 0, sizeof(outbox));
        memset(taken, 0, sizeof(taken));
        dq_head = dq_tail = 0;
        atomic_store(&outstanding, 1);
        atomic_store(&done_flag, 0);
        atomic_store(&left, 0);
        atomic_store(&zero_hits, 0);
        atomic_store(&next_id, 0);
        atomic_store(&nodes_run, 0);
        atomic_store(&c_out_main, 0), atomic_store(&c_out_shed, 0), atomic_store(&c_to_deque, 0);
        atomic_store(&c_to_sib, 0), atomic_store(&c_busy, 0), atomic_store(&c_sib_direct, 0);
        atomic_store(&c_dq_direct, 0);
        /* a root whose tree is neither trivial nor huge */
        item_t root = {mix(0x1234567u + 977u * (uint32_t)s), 0};
        uint64_t want = serial(root);
        for (uint32_t t = 1; want < 200 || want > 200000; ++t) {
            root.seed = mix(root.seed + t);
            want = serial(root);
        }
        pthread_t th[MAXW + 1];
        wk_t wk[MAXW];
        uint32_t crng = mix(0xc0ffeeu + (uint32_t)s);
        for (int w = 0; w < W; ++w) {
            wk[w] = (wk_t){w, mix(0xabcdu * (uint32_t)(w + 1) + (uint32_t)s), w == 0, root};
            pthread_create(&th[w], NULL, worker, &wk[w]);
        }
        if (users) pthread_create(&th[W], NULL, comm, &crng);
        for (int w = 0; w < W + (users ? 1 : 0); ++w) pthread_join(th[w], NULL);
        const uint32_t ids = atomic_load(&next_id);
        uint32_t lost = 0;
        for (uint32_t i = 0; i < ids && i < MAXBLOCKS; ++i) lost += atomic_load(&taken[i]) != 1;
        const uint32_t out = atomic_load(&c_out_main) + atomic_load(&c_out_shed);
        int ok = !atomic_load(&err);
        if (lost) fail("a block was lost or doubled"), ok = 0;
        if (atomic_load(&nodes_run) != want) fail("node count differs from the serial walk"), ok = 0;
        if (atomic_load(&zero_hits) != 1 || atomic_load(&outstanding) != 0)
            fail("outstanding did not reach zero exactly once"), ok = 0;
        if (out != atomic_load(&c_to_deque) + atomic_load(&c_to_sib)) fail("outbox blocks != to-deque + to-sibling"), ok = 0;
        if (!users && out) fail("an outbox was used without a comm thread"), ok = 0;
        if (dq_head != dq_tail) fail("the deque is not empty at the end"), ok = 0;
        for (int o = 0; o < 2; ++o)
            if (atomic_load(&outbox[o].state) != 0) fail("an outbox is not empty at the end"), ok = 0;
        for (int w = 0; w < W; ++w)
            if (atomic_load(&inbox[w].state) != 3) fail("an inbox is not closed at the end"), ok = 0;
        if (ids != out + atomic_load(&c_sib_direct) + atomic_load(&c_dq_direct)) fail("block ids do not add up"), ok = 0;
        if (!ok) bad = 1;
        tot_nodes += want, tot_out += out, tot_sib += atomic_load(&c_to_sib), tot_dq += atomic_load(&c_to_deque);
        tot_busy += atomic_load(&c_busy), tot_blocks += ids;
    }
    printf("schedules %d workers %d users %d nodes %llu blocks %llu outbox %llu to_sibling %llu to_deque %llu busy %llu "
           "violations %d\n", schedules, W, users, (unsigned long long)tot_nodes, (unsigned long long)tot_blocks,
           (unsigned long long)tot_out, (unsigned long long)tot_sib, (unsigned long long)tot_dq,
           (unsigned long long)tot_busy, bad);
    if (bad) return 1;
    printf("MODEL OK\n");
    return 0;
}
