// The host half of BOTS alignment (hclib_amd/csrc/hx_align_host.h) as a plain
// C++ program, built with AddressSanitizer and UBSan by
// tests/test_alignment_host.py: no HIP, no GPU.
//   alignment_host read FILE          the sequences as readseqs leaves them
//   alignment_host matrix FILE        avscore and a checksum of the 1024 scores
//   alignment_host bounds FILE CUTOFF WAVES
//   alignment_host pairs FILE AVSCORE the (si, sj, g, gh) table
//   alignment_host score COUNT LEN1 LEN2
// A refusal prints "EINVAL: <message>" and exits with 2.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hx_align_host.h"

using namespace hx;

static int refuse(const std::string &err) {
    printf("EINVAL: %s\n", err.c_str());
    return 2;
}

int main(int argc, char **argv) {
    if (argc < 3) return 64;
    const std::string cmd = argv[1];
    std::string err;
    if (cmd == "score" && argc == 5) {
        printf("%d\n", al_score(atoll(argv[2]), atoi(argv[3]), atoi(argv[4])));
        return 0;
    }
    if (cmd == "matrix") {
        AlMatrix m;
        if (al_read_matrix(argv[2], m, err)) return refuse(err);
        long long sum = 0;
        for (int i = 0; i < kAlCodes; ++i)
            for (int j = 0; j < kAlCodes; ++j) sum += (long long)m.score[i][j] * (i * kAlCodes + j + 1);
        printf("avscore %d checksum %lld\n", m.avscore, sum);
        return 0;
    }
    std::vector<AlSeq> seqs;
    if (al_read_input(argv[2], seqs, err)) return refuse(err);
    std::vector<int> len;
    for (const AlSeq &q : seqs) len.push_back((int)q.codes.size());
    if (cmd == "read") {
        printf("%zu\n", seqs.size());
        for (const AlSeq &q : seqs) {
            printf("%s\t%zu\t%d\t", q.name.c_str(), q.codes.size(), al_len(q.codes.data(), (int)q.codes.size()));
            for (uint8_t c : q.codes) printf("%d,", (int)c);
            printf("\n");
        }
        return 0;
    }
    if (cmd == "bounds" && argc == 5) {
        AlBounds b;
        if (al_bounds(len.data(), (int)len.size(), atoi(argv[3]), atoi(argv[4]), b, err)) return refuse(err);
        printf("pairs %llu tasks %llu spawns %llu diffs %llu arena_bytes %llu row_bytes %llu cells %llu longest %d\n", b.pairs,
               b.tasks, b.spawns, b.diffs, b.arena_bytes, b.row_bytes, b.cells, b.longest);
        return 0;
    }
    if (cmd == "pairs" && argc == 4) {
        for (size_t i = 0; i < seqs.size(); ++i)
            for (size_t j = i + 1; j < seqs.size(); ++j) {
                if (len[i] == 0 || len[j] == 0) continue;
                int g, gh;
                al_gaps(len[i], len[j], atoi(argv[3]), g, gh);
                printf("%zu %zu %d %d\n", i, j, g, gh);
            }
        return 0;
    }
    return 64;
}
