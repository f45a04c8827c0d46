"""BOTS alignment restated serially in Python, the oracle of the alignment tests
(bots/alignment_for/alignment.ref.c: forward_pass :204-241, reverse_pass
:246-286, diff :291-417, tracepath :422-449, pairalign :452-529; the reader
sequence.c:120-186). Integers only except the two places the reference uses
doubles: the gap-open penalty and the final percentage.

What `diff` writes into displ is not restated: the score needs only the count
of zeros whose two residues are equal, a zero comes only from the M == 1 base
case with midj > 0, and the residues it compares are seq1[A + 1] and
seq2[B + midj]. So `matches` is a sum over base cases.

Per pair the oracle gives g, gh, maxscore, se1, se2, sb1, sb2, matches,
diff_calls (every invocation of diff, base cases included), type2 (midpoints
of type 2), ties (times the `hh == midh && HH[j] != DD[j] && RR[j] == SS[j]`
branch of the midpoint scan was taken) and areas (M * N of every diff that is
no base case, from which the task count of any cutoff follows).
"""
import math
import re

CODES = "ABCDEFGHIKLMNPQRSTUVWXYZ-"
GAP1, GAP2 = 30, 31
MAXLINE = 512
MAX_LEN = 4999  # MAX_ALN_LENGTH - 1: HH[0..m] and DD[0..m] are int[5000]
RECORD = ("maxscore", "se1", "se2", "sb1", "sb2", "matches", "diff_calls", "type2", "ties")


def read_matrix(path):
    """(avscore, 32 x 32 rows) of a matrix file: '#' lines are comments, then
    'avscore <int>', then 1024 integers."""
    words = []
    for line in open(path):
        if not line.startswith("#"):
            words += line.split()
    if len(words) != 2 + 1024 or words[0] != "avscore":
        raise ValueError(f"{path}: not a substitution-matrix file")
    v = [int(w) for w in words[1:]]
    return v[0], [v[1 + 32 * i:33 + 32 * i] for i in range(32)]


def _lines(text):
    """fgets(line, MAXLINE + 1, f) over text: pieces of at most MAXLINE chars, each ending at a newline."""
    pos = 0
    while pos < len(text):
        nl = text.find("\n", pos, pos + MAXLINE)
        end = nl + 1 if nl >= 0 else min(len(text), pos + MAXLINE)
        yield text[pos:end]
        pos = end


def read_input(path):
    """[(name, codes)] of a Pearson file as readseqs leaves it: only the 25
    code characters survive (upper case: chartab maps a lower-case letter to
    its upper-case one, which the comparison c == chartab[c] then rejects),
    '-' becomes code 31."""
    text = open(path, "rb").read().decode("latin-1")
    m = re.match(r"Number\s*of\s*sequences\s*is\s*([+-]?\d+)", text)
    if not m or int(m.group(1)) < 1:
        raise ValueError(f"{path}: no 'Number of sequences is' line")
    it = _lines(text[m.end():])
    line, seqs = "", []
    for _ in range(int(m.group(1))):
        while not line.startswith(">"):
            line = next(it, None)
            if line is None:
                raise ValueError(f"{path}: truncated")
        i = 1
        while i < len(line) and line[i] == " ":
            i += 1
        j = i
        while j < len(line) and line[j] != " ":
            j += 1
        name, codes, any_line = line[i:j].rstrip("\r\n")[:30], [], False
        while True:
            line = next(it, None)
            if line is None:
                line = ""
                break
            any_line = True
            stop = False
            for c in line:
                if c in "\n\0>":
                    stop = c == ">"
                    break
                if c == "-":
                    codes.append(GAP2)
                elif c in CODES:
                    codes.append(CODES.index(c))
            if stop:
                break
        if not any_line:
            raise ValueError(f"{path}: the last sequence has no line")
        if len(codes) > MAX_LEN:
            raise ValueError(f"{path}: a sequence of {len(codes)} residues (at most {MAX_LEN})")
        seqs.append((name, codes))
    return seqs


def gap_penalties(n, m, avscore):
    """(g, gh) of a pair of lengths n, m (:496-498, the protein branch)."""
    gg = 10.0 + math.log(float(min(n, m)))
    g = int(2 * 100 * gg) if avscore <= 0 else int(2 * avscore * gg * 1.0)
    return g, int(100 * 0.1)


def forward_pass(mat, ia, ib, n, m, g, gh):
    """(maxscore, se1, se2, cells): the first cell in row-major order that attains the maximum, and how many attain it."""
    HH, DD = [0] * (m + 1), [-g] * (m + 1)
    maxscore = se1 = se2 = cells = 0
    for i in range(1, n + 1):
        hh = p = 0
        f = -g
        row = mat[ia[i]]
        for j in range(1, m + 1):
            f -= gh
            t = hh - g - gh
            if f < t:
                f = t
            d = DD[j] - gh
            t = HH[j] - g - gh
            if d < t:
                d = t
            DD[j] = d
            hh = p + row[ib[j]]
            if hh < f:
                hh = f
            if hh < d:
                hh = d
            if hh < 0:
                hh = 0
            p = HH[j]
            HH[j] = hh
            if hh > maxscore:
                maxscore, se1, se2, cells = hh, i, j, 1
            elif hh == maxscore and hh > 0:
                cells += 1
    return maxscore, se1, se2, cells


def reverse_pass(mat, ia, ib, se1, se2, maxscore, g, gh):
    cost, sb1, sb2 = 0, 1, 1
    HH, DD = [-1] * (se2 + 1), [-1] * (se2 + 1)
    for i in range(se1, 0, -1):
        hh = f = -1
        p = 0 if i == se1 else -1
        row = mat[ia[i]]
        for j in range(se2, 0, -1):
            f -= gh
            t = hh - g - gh
            if f < t:
                f = t
            d = DD[j] - gh
            t = HH[j] - g - gh
            if d < t:
                d = t
            DD[j] = d
            hh = p + row[ib[j]]
            if hh < f:
                hh = f
            if hh < d:
                hh = d
            p = HH[j]
            HH[j] = hh
            if hh > cost:
                cost, sb1, sb2 = hh, i, j
                if cost >= maxscore:
                    return sb1, sb2
    return sb1, sb2


def diff(mat, s1, s2, A, B, M, N, tb, te, g, gh, st):
    """The reference's diff without displ; st collects matches, diff_calls, type2, ties, areas."""
    stack = [(A, B, M, N, tb, te)]
    while stack:
        A, B, M, N, tb, te = stack.pop()
        st["diff_calls"] += 1
        if N <= 0 or M <= 0:
            continue

        def tbgap(k):
            return 0 if k <= 0 else tb + gh * k

        def tegap(k):
            return 0 if k <= 0 else te + gh * k

        if M == 1:
            midh = -(tb + gh) - tegap(N)
            hh = -(te + gh) - tbgap(N)
            if hh > midh:
                midh = hh
            midj = 0
            row = mat[s1[A + 1]]
            for j in range(1, N + 1):
                hh = row[s2[B + j]] - tegap(N - j) - tbgap(j - 1)
                if hh > midh:
                    midh, midj = hh, j
            if midj > 0:
                c1, c2 = s1[A + 1], s2[B + midj]
                if c1 != GAP1 and c1 != GAP2 and c1 == c2:
                    st["matches"] += 1
            continue
        st["areas"].append(M * N)
        midi = M // 2
        HH, DD = [0] * (N + 1), [0] * (N + 1)
        t = -tb
        for j in range(1, N + 1):
            HH[j] = t = t - gh
            DD[j] = t - g
        t = -tb
        for i in range(1, midi + 1):
            s = HH[0]
            HH[0] = hh = t = t - gh
            f = t - g
            row = mat[s1[A + i]]
            for j in range(1, N + 1):
                hh = hh - g - gh
                f = f - gh
                if hh > f:
                    f = hh
                hh = HH[j] - g - gh
                e = DD[j] - gh
                if hh > e:
                    e = hh
                hh = s + row[s2[B + j]]
                if f > hh:
                    hh = f
                if e > hh:
                    hh = e
                s = HH[j]
                HH[j] = hh
                DD[j] = e
        DD[0] = HH[0]
        RR, SS = [0] * (N + 1), [0] * (N + 1)
        t = -te
        for j in range(N - 1, -1, -1):
            RR[j] = t = t - gh
            SS[j] = t - g
        t = -te
        for i in range(M - 1, midi - 1, -1):
            s = RR[N]
            RR[N] = hh = t = t - gh
            f = t - g
            row = mat[s1[A + i + 1]]
            for j in range(N - 1, -1, -1):
                hh = hh - g - gh
                f = f - gh
                if hh > f:
                    f = hh
                hh = RR[j] - g - gh
                e = SS[j] - gh
                if hh > e:
                    e = hh
                hh = s + row[s2[B + j + 1]]
                if f > hh:
                    hh = f
                if e > hh:
                    hh = e
                s = RR[j]
                RR[j] = hh
                SS[j] = e
        SS[N] = RR[N]
        midh, midj, typ = HH[0] + RR[0], 0, 1
        for j in range(N + 1):
            hh = HH[j] + RR[j]
            if hh >= midh:
                if hh > midh:
                    midh, midj = hh, j
                elif HH[j] != DD[j] and RR[j] == SS[j]:
                    midh, midj = hh, j
                    st["ties"] += 1
        for j in range(N, -1, -1):
            hh = DD[j] + SS[j] + g
            if hh > midh:
                midh, midj, typ = hh, j, 2
        # (the second call first: the stack pops the first call first)
        if typ == 1:
            stack.append((A + midi, B + midj, M - midi, N - midj, g, te))
            stack.append((A, B, midi, midj, tb, g))
        else:
            st["type2"] += 1
            stack.append((A + midi + 1, B + midj, M - midi - 1, N - midj, 0, te))
            stack.append((A, B, midi - 1, midj, tb, 0))


def score_from_count(count, len1, len2):
    """(int)(100.0 * count / MIN(len1, len2)), 0 when a sequence has only gap codes (:513-516)."""
    if len1 == 0 or len2 == 0:
        return 0
    return int(100.0 * float(count) / float(min(len1, len2)))


def align(seqs, avscore, mat):
    """(scores, pairs): scores the nseqs x nseqs matrix as bench_output (row
    major list), pairs a list of dicts in (si, sj) order for the pairs whose
    two sequences are not empty."""
    ns = len(seqs)
    scores = [0] * (ns * ns)
    pairs = []
    for si in range(ns):
        s1 = [0] + seqs[si][1]
        n = len(s1) - 1
        len1 = sum(1 for c in s1[1:] if c not in (GAP1, GAP2))
        for sj in range(si + 1, ns):
            s2 = [0] + seqs[sj][1]
            m = len(s2) - 1
            if n == 0 or m == 0:
                scores[si * ns + sj] = 1
                continue
            len2 = sum(1 for c in s2[1:] if c not in (GAP1, GAP2))
            g, gh = gap_penalties(n, m, avscore)
            maxscore, se1, se2, cells = forward_pass(mat, s1, s2, n, m, g, gh)
            sb1, sb2 = reverse_pass(mat, s1, s2, se1, se2, maxscore, g, gh)
            st = {"matches": 0, "diff_calls": 0, "type2": 0, "ties": 0, "areas": []}
            diff(mat, s1, s2, sb1 - 1, sb2 - 1, se1 - sb1 + 1, se2 - sb2 + 1, 0, 0, g, gh, st)
            scores[si * ns + sj] = score_from_count(st["matches"], len1, len2)
            st["areas"].sort()
            pairs.append(dict(si=si, sj=sj, g=g, gh=gh, max_cells=cells, maxscore=maxscore, se1=se1, se2=se2, sb1=sb1, sb2=sb2, **st))
    return scores, pairs


def tasks(pairs, cutoff):
    """Tasks of a launch at `cutoff` cells: the root, one per pair, and two
    for every diff that is no base case and has M * N > cutoff (its children;
    a pair's root diff runs inside the pair task)."""
    return 1 + len(pairs) + 2 * sum(1 for p in pairs for a in p["areas"] if a > cutoff)
