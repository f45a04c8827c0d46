/*
 * hclib_atomic.h — privatised atomics of the HClib API (MI355X build).
 *
 * Mirrors the reference's inc/hclib_atomic.h, so programs written against it
 * compile unmodified:
 *   CACHE_LINE_LEN_IN_BYTES, the three callback types   inc/hclib_atomic.h:6-30
 *   hclib_atomic_t                                      inc/hclib_atomic.h:37-42
 *   hclib_atomic_create / init / update / gather        inc/hclib_atomic.h:47-69,
 *                                                       src/hclib_atomic.c:3-54
 *   hclib::atomic_t<T>                                  inc/hclib_atomic.h:81-137
 *   hclib::atomic_sum_t / atomic_max_t / atomic_or_t    inc/hclib_atomic.h:141-186
 *
 * An atomic keeps one padded element per HOST worker
 * (hclib_get_num_workers(); this build's host has one, include/hclib-rt.h);
 * a task updates the element of the worker it runs on
 * (hclib_get_current_worker()) with no synchronisation, and gather folds
 * elements 1 .. n-1 into a copy of element 0, in that order. As in the
 * reference, nothing may update an atomic while it is gathered.
 *
 * Differences from the reference, both invisible at a zero default: padding
 * rounds the element size UP to the next multiple of the line (an element
 * that already fills whole lines gets no extra one), and the C++ gather
 * starts from worker 0's element instead of folding the default value in
 * once more.
 *
 * Device code reduces through hx::AtomicView (include/hclib_hip/hx_atomic.h)
 * and hclib::hip::atomic_sum_t / atomic_max_t / atomic_or_t
 * (include/hclib_hip_cpp.h): the same design with a wave as the worker.
 */
#ifndef HCLIB_ATOMIC_H_
#define HCLIB_ATOMIC_H_

#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "hclib-rt.h"

#define CACHE_LINE_LEN_IN_BYTES 32

#ifdef __cplusplus
extern "C" {
#endif

/* set one element to the atomic's start value */
typedef void (*atomic_init_func)(void *atomic_ele, void *user_data);
/* change the calling worker's element in place */
typedef void (*atomic_update_func)(void *atomic_ele, void *user_data);
/* fold element b into element a */
typedef void (*atomic_gather_func)(void *a, void *b, void *user_data);

typedef struct _hclib_atomic_t {
    char *vals;             /* nthreads elements, padded_val_size bytes apart */
    size_t nthreads;        /* host workers when the atomic was initialised */
    size_t val_size;        /* bytes of one element as the program sees it */
    size_t padded_val_size; /* val_size rounded up to whole lines */
} hclib_atomic_t;

/* malloc an hclib_atomic_t and initialise it (the program frees both the
 * struct and its vals) */
hclib_atomic_t *hclib_atomic_create(const size_t ele_size_in_bytes, atomic_init_func init, void *user_data);
/* initialise caller-provided storage: allocates vals, calls init on each element */
void hclib_atomic_init(hclib_atomic_t *atomic, const size_t ele_size_in_bytes, atomic_init_func init,
                       void *user_data);
/* f(the calling worker's element, user_data) */
void hclib_atomic_update(hclib_atomic_t *atomic, atomic_update_func f, void *user_data);
/* a malloc'ed copy of element 0 with every other element folded in by
 * f(result, element, user_data); the caller frees it */
void *hclib_atomic_gather(hclib_atomic_t *atomic, atomic_gather_func f, void *user_data);

#ifdef __cplusplus
}

#include <functional>
#include <new>

namespace hclib {

template <class T>
class atomic_t {
  public:
    atomic_t(T set_default_value)
        : nthreads_((size_t)hclib_get_num_workers()), default_value_(set_default_value) {
        vals_ = alloc(nthreads_);
        for (size_t w = 0; w < nthreads_; ++w) new (&vals_[w].val) T(default_value_);
    }
    atomic_t(const atomic_t &other) : nthreads_(other.nthreads_), default_value_(other.default_value_) {
        vals_ = alloc(nthreads_);
        for (size_t w = 0; w < nthreads_; ++w) new (&vals_[w].val) T(other.vals_[w].val);
    }
    atomic_t &operator=(const atomic_t &other) {
        if (this != &other) {
            atomic_t copy(other);
            swap(copy);
        }
        return *this;
    }
    ~atomic_t() {
        for (size_t w = 0; w < nthreads_; ++w) vals_[w].val.~T();
        free(vals_);
    }

    // f(current) -> new value of the calling worker's element
    template <class F>
    void update(F f) {
        T &mine = vals_[(size_t)hclib_get_current_worker()].val;
        mine = f(mine);
    }

    // reduce(a, b) folded over the workers' elements, worker 0's first
    template <class F>
    T gather(F reduce) {
        T acc = vals_[0].val;
        for (size_t w = 1; w < nthreads_; ++w) acc = reduce(acc, vals_[w].val);
        return acc;
    }

  private:
    // one element per line(s): neighbours never share a line
    struct alignas(CACHE_LINE_LEN_IN_BYTES) padded_t {
        T val;
    };
    static padded_t *alloc(size_t n) {
        void *p = NULL;
        if (posix_memalign(&p, alignof(padded_t) < sizeof(void *) ? sizeof(void *) : alignof(padded_t),
                           n * sizeof(padded_t)) != 0) {
            fprintf(stderr, "hclib::atomic_t: out of memory\n");
            abort();
        }
        return (padded_t *)p;
    }
    void swap(atomic_t &o) {
        padded_t *v = vals_;
        vals_ = o.vals_;
        o.vals_ = v;
        const size_t n = nthreads_;
        nthreads_ = o.nthreads_;
        o.nthreads_ = n;
        const T d = default_value_;
        default_value_ = o.default_value_;
        o.default_value_ = d;
    }

    size_t nthreads_;
    padded_t *vals_;
    T default_value_;
};

template <class T>
class atomic_sum_t : private atomic_t<T> {
  public:
    atomic_sum_t(T set_default_value) : atomic_t<T>(set_default_value) {}
    atomic_sum_t &operator+=(T other) {
        atomic_t<T>::update([other](T cur) { return (T)(cur + other); });
        return *this;
    }
    T get() {
        return atomic_t<T>::gather([](T a, T b) { return (T)(a + b); });
    }
};

template <class T>
class atomic_max_t : private atomic_t<T> {
  public:
    atomic_max_t(T set_default_value) : atomic_t<T>(set_default_value) {}
    void update(T other) {
        atomic_t<T>::update([other](T cur) { return other > cur ? other : cur; });
    }
    T get() {
        return atomic_t<T>::gather([](T a, T b) { return b > a ? b : a; });
    }
};

// logical or (inc/hclib_atomic.h:172-186): get() returns 0 or 1
template <class T>
class atomic_or_t : private atomic_t<T> {
  public:
    atomic_or_t(T set_default_value) : atomic_t<T>(set_default_value) {}
    atomic_or_t &operator|=(T other) {
        atomic_t<T>::update([other](T cur) { return (T)(cur || other); });
        return *this;
    }
    T get() {
        const T v = atomic_t<T>::gather([](T a, T b) { return (T)(a || b); });
        return (T)(v ? 1 : 0);
    }
};

}  // namespace hclib
#endif /* __cplusplus */

#endif /* HCLIB_ATOMIC_H_ */
