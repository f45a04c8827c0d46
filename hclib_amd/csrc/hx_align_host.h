// hx_align_host.h — the host half of BOTS alignment (alignment.hip) in plain
// C++: no HIP and no getenv, so a host program can check it under sanitizers
// (tests/cpp/alignment_host.cpp). The Pearson reader with the reference's
// behaviour (bots/alignment_for/sequence.c:120-186), the substitution-matrix
// reader (INTEGRATION.md has the format), the per-pair gap penalties and the
// score from a match count (alignment.ref.c:496-498, 448, 513-516), and the
// closed-form bounds every pool of a launch is sized from.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace hx {

// MAX_ALN_LENGTH is 5000 and forward_pass / reverse_pass index HH[0..m],
// DD[0..m] of int[MAX_ALN_LENGTH] (:207-213, :249-255), diff HH[0..N] ..
// SS[0..N] of the same size (:296-299, :334, :362): the second sequence of a
// pair may have 4999 residues. Every sequence but the first is the second of
// some pair, and displ[2 * MAX_ALN_LENGTH + 1] (:484) holds n + m + 1 entries,
// so the cap is on every sequence.
constexpr int kAlMaxLen = 4999;
constexpr int kAlCodes = 32;            // NUMRES
constexpr int kAlGap1 = 30, kAlGap2 = 31;  // gap_pos1, gap_pos2
constexpr int kAlMaxLine = 512;         // MAXLINE
constexpr int kAlMaxName = 30;          // MAXNAMES
constexpr int kAlDefaultCutoff = 16384; // cells: a diff of at most this many runs its whole recursion in one task
constexpr int kAlPairsPerSpawn = 64;    // pair tasks per dyn_async_await of the root
// Row arrays HH / DD / RR / SS of one wave, (longest + 1) ints each: in LDS
// while the longest sequence has at most kAlLdsCols residues (4 x 768 ints =
// 12 KB beside the 4 KB matrix and the stack; 8 workgroups are 133 KB of a
// CU's 160), else a slice per resident wave of the launch's arena.
constexpr int kAlLdsCols = 767;
constexpr int kAlMaxWaves = 256 * 8;    // resident waves a launch can have: 256 CUs, at most 8 waves each
constexpr int kAlRecWords = 16;         // a pair's record, one 64-byte line
constexpr int kAlClasses = 4;           // task classes: root, pair, spawning diff, leaf diff
constexpr int kAlEinval = -2;           // HCLIB_HIP_EINVAL

struct AlSeq {
    std::string name;
    std::vector<uint8_t> codes;  // 0..24 by "ABCDEFGHIKLMNPQRSTUVWXYZ-", '-' as 31
};

struct AlMatrix {
    int avscore = 0;
    int score[kAlCodes][kAlCodes] = {};
};

// readseqs / get_seq. The reference keeps the last line it read in a static
// buffer: a sequence ends at a '>' anywhere in a line, and the next header is
// that line only if the '>' is its first character. A character survives if
// chartab maps it to itself: the 24 upper-case letters of the code string and
// '-'; chartab maps a lower-case letter to its upper-case one, so the
// comparison rejects it (fill_chartab :65-75, get_seq :144). A name is what
// follows '>' and blanks up to the next blank, cut at MAXNAMES characters (the
// reference writes past names[i] beyond that) and without the line end.
// EINVAL where the reference reads uninitialised or NULL memory: no count
// line, a count below 1, fewer headers than the count, a last header with no
// line after it; and a sequence longer than kAlMaxLen.
inline int al_read_input(const char *path, std::vector<AlSeq> &seqs, std::string &err) {
    seqs.clear();
    FILE *f = path ? fopen(path, "r") : nullptr;
    if (!f) {
        err = std::string("cannot open sequence file ") + (path ? path : "(null)");
        return kAlEinval;
    }
    int count = 0, rc = 0;
    if (fscanf(f, "Number of sequences is %d", &count) != 1 || count < 1) {
        err = std::string(path) + ": no 'Number of sequences is <n>' line with n >= 1";
        rc = kAlEinval;
    }
    char line[kAlMaxLine + 1];
    line[0] = 0;
    for (int s = 0; !rc && s < count; ++s) {
        bool eof = false;
        while (line[0] != '>' && !(eof = fgets(line, kAlMaxLine + 1, f) == nullptr)) {
        }
        if (eof) {
            err = std::string(path) + ": truncated: " + std::to_string(s) + " of " + std::to_string(count) + " sequences";
            rc = kAlEinval;
            break;
        }
        const size_t len = strlen(line);
        size_t i = 1, j;
        while (i < len && line[i] == ' ') ++i;
        for (j = i; j < len && line[j] != ' '; ++j) {
        }
        AlSeq q;
        q.name.assign(line + i, j - i);
        while (!q.name.empty() && (q.name.back() == '\n' || q.name.back() == '\r')) q.name.pop_back();
        if (q.name.size() > (size_t)kAlMaxName) q.name.resize(kAlMaxName);
        bool any = false;
        line[0] = 0;
        while (fgets(line, kAlMaxLine + 1, f) != nullptr) {
            any = true;
            char c = 0;
            for (int k = 0; k <= kAlMaxLine; ++k) {
                c = line[k];
                if (c == '\n' || c == 0 || c == '>') break;
                if (c == '-') {
                    q.codes.push_back((uint8_t)kAlGap2);
                } else if (c >= 'A' && c <= 'Z' && c != 'J' && c != 'O') {
                    // the index in "ABCDEFGHIKLMNPQRSTUVWXYZ-" (encode :80-97): J and O are not in it
                    q.codes.push_back((uint8_t)(c - 'A' - (c > 'J' ? 1 : 0) - (c > 'O' ? 1 : 0)));
                }
            }
            if (c == '>') break;
        }
        if (!any) {
            err = std::string(path) + ": the last sequence has no line after its header";
            rc = kAlEinval;
        } else if (q.codes.size() > (size_t)kAlMaxLen) {
            err = std::string(path) + ": sequence " + std::to_string(s + 1) + " has " + std::to_string(q.codes.size()) +
                  " residues, the reference's arrays hold " + std::to_string(kAlMaxLen);
            rc = kAlEinval;
        } else {
            seqs.push_back(std::move(q));
        }
    }
    fclose(f);
    if (rc) seqs.clear();
    return rc;
}

// A matrix file: lines that start with '#' are comments; then `avscore <int>`
// (mat_avscore) and 32 x 32 integers, matrix[i][j] by residue code as
// get_matrix leaves it (:129-199).
inline int al_read_matrix(const char *path, AlMatrix &m, std::string &err) {
    FILE *f = path ? fopen(path, "r") : nullptr;
    if (!f) {
        err = std::string("cannot open matrix file ") + (path ? path : "(null)");
        return kAlEinval;
    }
    int c, rc = 0;
    // comment lines, at the head only
    while ((c = fgetc(f)) == '#')
        while ((c = fgetc(f)) != EOF && c != '\n') {
        }
    if (c != EOF) ungetc(c, f);
    char word[16] = {};
    if (fscanf(f, "%15s %d", word, &m.avscore) != 2 || strcmp(word, "avscore") != 0) rc = kAlEinval;
    for (int i = 0; !rc && i < kAlCodes * kAlCodes; ++i)
        if (fscanf(f, "%d", &m.score[i / kAlCodes][i % kAlCodes]) != 1) rc = kAlEinval;
    int extra;
    if (!rc && fscanf(f, "%d", &extra) == 1) rc = kAlEinval;
    fclose(f);
    if (rc) err = std::string(path) + ": not a substitution-matrix file ('avscore <int>', then 1024 integers)";
    return rc;
}

// gapOpen and gapExtend of a pair (:496-498, protein branch, gap_open_scale 1,
// pw_go_penalty 10.0, pw_ge_penalty 0.1), in double as the reference does.
inline void al_gaps(int n, int m, int avscore, int &g, int &gh) {
    const double gg = 10.0 + log((double)(n < m ? n : m));
    g = (int)((avscore <= 0) ? (2 * 100 * gg) : (2 * avscore * gg * 1.0));
    gh = (int)(100 * 0.1);
}

// residues that are no gap codes (:471-474, :487-490)
inline int al_len(const uint8_t *codes, int n) {
    int len = 0;
    for (int i = 0; i < n; ++i) len += codes[i] != kAlGap1 && codes[i] != kAlGap2;
    return len;
}

// tracepath's 100.0 * count over MIN(len1, len2), truncated (:448, :513-516)
inline int al_score(long long count, int len1, int len2) {
    if (len1 == 0 || len2 == 0) return 0;
    return (int)(100.0 * (double)count / (double)(len1 < len2 ? len1 : len2));
}

// What a launch uses at most, closed forms in the lengths and the cutoff.
//  diff calls of a pair (n, m): T(0) = T(1) = 1 and a call with M >= 2 rows
//    has children of floor(M / 2) and ceil(M / 2) rows (type 2: one fewer
//    each), so T(M) <= 2 M - 1; the root diff has M <= n.
//  spawning diffs (no base case, M * N > cutoff): at depth d a call has at
//    most r = ceil(n / 2^d) rows, the calls of one depth have disjoint column
//    ranges of m columns in all, and one that spawns has more than
//    cutoff / r columns: at most min(2^d, floor(m r / (cutoff + 1))) of them,
//    summed over the depths with r >= 2.
//  tasks: the root, a task per pair and two per spawning diff.
struct AlBounds {
    unsigned long long pairs = 0, tasks = 0, spawns = 0, diffs = 0, arena_bytes = 0, row_bytes = 0, cells = 0;
    int longest = 0;
};

inline unsigned long long al_spawn_bound(int n, int m, int cutoff) {
    unsigned long long s = 0;
    for (int d = 0; d < 31; ++d) {
        const unsigned long long r = ((unsigned long long)n + (1ull << d) - 1) >> d;
        if (r < 2) break;
        const unsigned long long by_cols = (unsigned long long)m * r / ((unsigned long long)cutoff + 1);
        s += by_cols < (1ull << d) ? by_cols : (1ull << d);
    }
    return s;
}

// bytes of the launch's arena ahead of the row slices: class counters, the
// matrix, a {offset, length} pair per sequence, the pair table (si, sj, g,
// gh), the pair records and the codes
inline unsigned long long al_fixed_bytes(unsigned long long nseqs, unsigned long long pairs, unsigned long long total) {
    return (unsigned long long)kAlClasses * 256 + kAlCodes * kAlCodes * 4 + ((nseqs * 8 + 255) & ~255ull) +
           ((pairs * 16 + 255) & ~255ull) + pairs * kAlRecWords * 4 + ((total + 64 + 255) & ~255ull);
}

inline int al_bounds(const int *lengths, int nseqs, int cutoff, int waves, AlBounds &b, std::string &err) {
    b = AlBounds();
    if (!lengths || nseqs < 1 || cutoff < 1 || waves < 1 || waves > kAlMaxWaves) {
        err = "alignment bounds: nseqs, cutoff and waves must be at least 1 (waves at most " +
              std::to_string(kAlMaxWaves) + ")";
        return kAlEinval;
    }
    unsigned long long total = 0;
    for (int i = 0; i < nseqs; ++i) {
        if (lengths[i] < 0 || lengths[i] > kAlMaxLen) {
            err = "alignment: sequence " + std::to_string(i + 1) + " has " + std::to_string(lengths[i]) +
                  " residues, the reference's arrays hold " + std::to_string(kAlMaxLen);
            return kAlEinval;
        }
        total += (unsigned long long)lengths[i];
        if (lengths[i] > b.longest) b.longest = lengths[i];
    }
    for (int i = 0; i < nseqs; ++i)
        for (int j = i + 1; j < nseqs; ++j) {
            const int n = lengths[i], m = lengths[j];
            if (n == 0 || m == 0) continue;
            b.pairs += 1;
            b.diffs += n > 1 ? 2ull * n - 1 : 1;
            b.spawns += al_spawn_bound(n, m, cutoff);
            b.cells += (unsigned long long)n * m;
        }
    b.tasks = 1 + b.pairs + 2 * b.spawns;
    if (b.tasks >= 0xfffffff0ull) {
        err = "alignment: " + std::to_string(b.tasks) + " tasks, more than a 32-bit index addresses";
        return kAlEinval;
    }
    b.row_bytes = b.longest > kAlLdsCols ? 4ull * ((unsigned long long)b.longest + 1) * 4 : 0;
    b.arena_bytes = al_fixed_bytes((unsigned long long)nseqs, b.pairs, total) + b.row_bytes * (unsigned long long)waves;
    return 0;
}

}  // namespace hx
