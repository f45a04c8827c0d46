// The C++ surface of include/hclib_atomic.h (inc/hclib_atomic.h:81-186 of
// the reference): atomic_t<T> with update / gather lambdas and a copy
// constructor, atomic_sum_t, atomic_max_t, atomic_or_t, each updated by 1000
// asyncs inside one finish, with non-zero defaults. Prints
// "Check results: OK" (tests/test_atomic_host.py).
#include <assert.h>
#include <stdio.h>

#include "hclib_cpp.h"
#include "hclib_atomic.h"

#define N 1000

struct ele_t {  // 12 bytes
    int sum, max, flag;
};

int main() {
    const char *deps[] = {"system"};
    bool ok = false;
    hclib::launch(deps, 1, [&]() {
        static_assert(sizeof(ele_t) == 12, "12-byte element");
        hclib::atomic_t<ele_t> *ele = new hclib::atomic_t<ele_t>(ele_t{3, -1, 0});
        hclib::atomic_t<int> *plain = new hclib::atomic_t<int>(0);
        hclib::atomic_sum_t<long> *sum = new hclib::atomic_sum_t<long>(100);
        hclib::atomic_max_t<double> *max = new hclib::atomic_max_t<double>(-1.5);
        hclib::atomic_or_t<int> *none = new hclib::atomic_or_t<int>(0);
        hclib::atomic_or_t<int> *some = new hclib::atomic_or_t<int>(0);
        hclib::finish([=]() {
            for (int i = 1; i <= N; ++i) {
                hclib::async([=]() {
                    ele->update([i](ele_t e) {
                        e.sum += i;
                        e.max = i > e.max ? i : e.max;
                        e.flag = e.flag || i == N;
                        return e;
                    });
                    plain->update([](int cur) { return cur + 1; });
                    *sum += i;
                    max->update(0.25 * i);
                    *none |= 0;
                    *some |= (i == 777) ? 5 : 0;
                });
            }
        });
        auto fold = [](ele_t a, ele_t b) { return ele_t{a.sum + b.sum, a.max > b.max ? a.max : b.max, a.flag || b.flag}; };
        const int nw = hclib_get_num_workers();
        const ele_t e = ele->gather(fold);
        assert(e.sum == 3 * nw + N * (N + 1) / 2 && e.max == N && e.flag == 1);
        assert(plain->gather([](int a, int b) { return a + b; }) == N);
        assert(sum->get() == 100L * nw + (long)N * (N + 1) / 2);
        assert(max->get() == 0.25 * N);
        assert(none->get() == 0 && some->get() == 1);  // a logical or: 5 reads as 1

        // the copy constructor: an independent copy with the same contents
        hclib::atomic_t<ele_t> copy(*ele);
        hclib::atomic_sum_t<long> sum_copy(*sum);
        hclib::finish([&]() {
            hclib::async([&]() {
                copy.update([](ele_t c) {
                    c.sum += 1;
                    return c;
                });
                sum_copy += 1;
            });
        });
        assert(copy.gather(fold).sum == e.sum + 1 && ele->gather(fold).sum == e.sum);
        assert(sum_copy.get() == sum->get() + 1);
        delete ele;
        delete plain;
        delete sum;
        delete max;
        delete none;
        delete some;
        ok = true;
    });
    assert(ok);
    printf("Check results: OK\n");
    return 0;
}
