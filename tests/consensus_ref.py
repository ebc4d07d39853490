"""One voting + emission round of the pile-up consensus, restated in plain Python (second reference beside
oracle/consensus.c; it calls none of the C code).

The contract, per overlap of the template that is enabled and whose tiles all have at most SEG_MAX B bases:
  * every trace tile (template columns up to the next multiple of the trace spacing, B bases as the trace says) is aligned
    with a full-matrix Needleman-Wunsch, unit mismatch and indel costs; the trace's diffs are not used;
  * the traceback starts at the bottom-right corner and steps to the smallest neighbour, preferring the diagonal, then the
    insertion (j - 1), then the deletion (i - 1);
  * a deleted column moves to the left across columns that hold the same template base and match it exactly, as long as
    nothing is inserted in front of the column it leaves; then a run of at most MAXINS equal inserted bases c moves to the
    left across exact matches of c with nothing inserted in front of them.  Both only inside the tile;
  * every column counts 4 base votes, 1 deletion vote, 1 cover count and MAXINS x 4 votes for the bases inserted in front
    of it: VOTE_STRIDE = 22 counters.
Emission walks the homopolymer runs of the template: the run changes its length by round(net / (cover + 1)), net = deletion
votes minus votes for inserted copies of the run's base (the slot behind the run included), at most MAXINS longer; columns
whose winning base (the template's own base has one vote more) differs are emitted in place unless deleted by a majority;
inserted bases other than the run's and the previous run's base are emitted by a majority of cover + 1.

`mutate` names one deliberate error, for showing that a set of cases tells a wrong implementation from a right one."""
import numpy as np

MAXINS = 4
SEG_MAX = 250
VOTE_STRIDE = 6 + 4 * MAXINS
DISABLED, COMP = 0x20, 0x1
MUTANTS = ("ins_before_diag", "no_canonical", "maxins3", "truncate", "no_own_vote", "keep_prev_base")


def nw_ops(ref, qry, ins_before_diag=False):
    """Ops front to back: 0 = pair, 1 = deletion (template column without a B base), 2 = insertion."""
    n, m = len(ref), len(qry)
    q = np.asarray(qry, dtype=np.int64)
    jj = np.arange(m + 1, dtype=np.int64)
    F = np.zeros((n + 1, m + 1), dtype=np.int64)
    F[0] = jj
    for i in range(1, n + 1):
        # F[i][j] = min(F[i-1][j-1] + (ref != qry), F[i-1][j] + 1, F[i][j-1] + 1); the last term chains along the row:
        # F[i][j] = min over k <= j of (t[k] + j - k) with t the minimum of the other two
        t = np.empty(m + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(F[i - 1, :-1] + (q != ref[i - 1]), F[i - 1, 1:] + 1)
        F[i] = np.minimum.accumulate(t - jj) + jj
    F = F.tolist()
    ops = []
    i, j = n, m
    while i > 0 and j > 0:
        ms, is_, ds = F[i - 1][j - 1], F[i][j - 1], F[i - 1][j]
        nx = min(ms, is_, ds)
        if ins_before_diag and nx == is_:
            ops.append(2)
            j -= 1
        elif nx == ms:
            ops.append(0)
            i -= 1
            j -= 1
        elif nx == is_:
            ops.append(2)
            j -= 1
        else:
            ops.append(1)
            i -= 1
    ops += [1] * i + [2] * j
    return ops[::-1]


def _revcomp(s):
    return [3 - c if c < 4 else c for c in s[::-1]]


def consensus(ref, reads, las, trace, aidx, tspace, mutate=None):
    """(consensus bases uint8, vote table uint32 [len(ref), 22]) of one round; arguments as oracle.pyoracle.consensus."""
    assert mutate is None or mutate in MUTANTS
    M = 3 if mutate == "maxins3" else MAXINS
    ref = [int(c) for c in ref]
    rlen = len(ref)
    v = [[0] * VOTE_STRIDE for _ in range(rlen + 1)]
    for la in las:
        if int(la["aread"]) != aidx or int(la["flags"]) & DISABLED:
            continue
        b = [int(c) for c in reads.seq(int(la["bread"]))]
        if int(la["flags"]) & COMP:
            b = _revcomp(b)
        tr = [int(x) for x in trace[int(la["toff"]):int(la["toff"]) + int(la["tlen"])]]
        if any(x > SEG_MAX for x in tr[1::2]):
            continue
        a0, b0, aepos = int(la["abpos"]), int(la["bbpos"]), int(la["aepos"])
        for e in range(len(tr) // 2):
            a1 = min((a0 // tspace + 1) * tspace, aepos)
            b1 = b0 + tr[2 * e + 1]
            w = a1 - a0
            col, ins = [], [[] for _ in range(w + 1)]   # aligned B base or 5 = deleted; bases inserted before the column
            y = b0
            for op in nw_ops(ref[a0:a1], b[b0:b1], mutate == "ins_before_diag"):
                if op == 0:
                    col.append(b[y])
                    y += 1
                elif op == 1:
                    col.append(5)
                else:
                    ins[len(col)].append(b[y])
                    y += 1
            assert len(col) == w and y == b1
            if mutate != "no_canonical":
                for x in range(w):
                    if col[x] != 5:
                        continue
                    c, st = ref[a0 + x], x
                    while st > 0 and col[st - 1] == c and ref[a0 + st - 1] == c and not ins[st]:
                        st -= 1
                    if st < x:
                        col[st], col[x] = 5, c
                for x in range(1, w + 1):
                    n = len(ins[x])
                    if n == 0 or n > M:
                        continue
                    c = ins[x][0]
                    if c >= 4 or any(t != c for t in ins[x]):
                        continue
                    st = x
                    while st > 0 and col[st - 1] == c and ref[a0 + st - 1] == c and not ins[st - 1]:
                        st -= 1
                    if st < x:
                        ins[st], ins[x] = ins[x], []
            for x in range(w + 1):
                cnt = v[a0 + x]
                for t, c in enumerate(ins[x][:M]):
                    if c < 4:
                        cnt[6 + 4 * t + c] += 1
                if x == w:
                    break
                if col[x] == 5:
                    cnt[4] += 1
                elif col[x] < 4:
                    cnt[col[x]] += 1
                cnt[5] += 1
            a0, b0 = a1, b1
    out = []
    own = 0 if mutate == "no_own_vote" else 1

    def winner(cnt, c):
        best = c if c < 4 else 0
        bv = [cnt[k] + (own if k == c else 0) for k in range(4)]
        for k in range(4):
            if bv[k] > bv[best]:
                best = k
        return best
    rs = 0
    while rs < rlen:
        re = rs + 1
        while re < rlen and ref[re] == ref[rs]:
            re += 1
        c = ref[rs]
        den = v[rs][5] + 1
        net = 0
        for x in range(rs, re):
            net += v[x][4]
            if c < 4:
                net -= sum(v[x][6 + 4 * t + c] for t in range(M))
        if c < 4 and re < rlen:
            net -= sum(v[re][6 + 4 * t + c] for t in range(M))
        if mutate == "truncate":
            adj = net // den if net >= 0 else -((-net) // den)
        else:
            adj = (2 * net + den) // (2 * den) if net >= 0 else -((2 * -net + den) // (2 * den))
        ncols = sum(1 for x in range(rs, re) if winner(v[x], c) == c)
        target = min(max(ncols - adj, 0), ncols + M)
        extra, keep = max(target - ncols, 0), min(target, ncols)
        for x in range(rs, re):
            cnt = v[x]
            cover = cnt[5]
            pc = ref[rs - 1] if (x == rs and rs > 0 and mutate != "keep_prev_base") else 255
            for t in range(M):
                iv = cnt[6 + 4 * t:10 + 4 * t]
                tot, best = 0, -1
                for k in range(4):
                    if k == c or k == pc:
                        continue
                    tot += iv[k]
                    if best < 0 or iv[k] > iv[best]:
                        best = k
                if best < 0 or 2 * tot <= cover + 1:
                    break
                out.append(best)
            best = winner(cnt, c)
            if best != c:
                if 2 * cnt[4] <= cover + 1:
                    out.append(best)
                continue
            if x == rs:
                out += [c] * extra
            if keep > 0:
                out.append(c)
                keep -= 1
        rs = re
    return np.asarray(out, dtype=np.uint8), np.asarray(v[:rlen], dtype=np.uint32).reshape(rlen, VOTE_STRIDE)
