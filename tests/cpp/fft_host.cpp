// The host half of BOTS fft (hclib_amd/csrc/hx_fft_host.h) as a plain C++
// program, built with AddressSanitizer and UBSan by tests/test_fft_host.py: no
// HIP, no GPU.
//   fft_host factors N             the factor list
//   fft_host factors_range A B     one line per n in A .. B: n, then the list or EINVAL
//   fft_host twiddles N            the n + 1 pairs as hexadecimal bit patterns
//   fft_host bounds N CUTOFF BAND  tasks scopes nodes leaves bands bytes check_ins calls
// A refusal prints "EINVAL: <message>" and exits with 2.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hx_fft_host.h"

using namespace hx;

static int refuse(const std::string &err) {
    printf("EINVAL: %s\n", err.c_str());
    return 2;
}

int main(int argc, char **argv) {
    if (argc < 3) return 64;
    const std::string cmd = argv[1];
    std::string err;
    int fl[kFftMaxFactors];
    if (cmd == "factors" && argc == 3) {
        const int cnt = fft_factors(atoi(argv[2]), fl, err);
        if (cnt < 0) return refuse(err);
        for (int k = 0; k < cnt; ++k) printf("%d%c", fl[k], k + 1 < cnt ? ' ' : '\n');
        return 0;
    }
    if (cmd == "factors_range" && argc == 4) {
        for (int n = atoi(argv[2]); n <= atoi(argv[3]); ++n) {
            const int cnt = fft_factors(n, fl, err);
            printf("%d", n);
            if (cnt < 0) printf(" EINVAL");
            for (int k = 0; k < cnt; ++k) printf(" %d", fl[k]);
            printf("\n");
        }
        return 0;
    }
    if (cmd == "twiddles" && argc == 3) {
        const int n = atoi(argv[2]);
        if (fft_factors(n, fl, err) < 0) return refuse(err);
        std::vector<double> w(2 * ((size_t)n + 1));
        fft_twiddles(n, w.data());
        for (size_t k = 0; k < w.size(); ++k) {
            uint64_t b;
            memcpy(&b, &w[k], 8);
            printf("%016llx\n", (unsigned long long)b);
        }
        return 0;
    }
    if (cmd == "bounds" && argc == 5) {
        int cutoff = atoi(argv[3]), band = atoi(argv[4]);
        FftPlan p;
        if (fft_check_args(atoi(argv[2]), cutoff, band, err) || fft_plan(atoi(argv[2]), cutoff, band, p, err))
            return refuse(err);
        printf("%llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)p.tasks, (unsigned long long)p.scopes,
               (unsigned long long)p.nodes, (unsigned long long)p.leaves, (unsigned long long)p.bands,
               (unsigned long long)p.bytes, (unsigned long long)p.check_ins, (unsigned long long)p.calls);
        return 0;
    }
    return 64;
}
