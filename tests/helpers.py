"""Shared helpers for the parity tests (HIP path vs. CPU oracle)."""
import numpy as np

FIELDS = ("tlen", "diffs", "abpos", "bbpos", "aepos", "bepos", "flags", "aread", "bread")


def la_rows(las, trace):
    """Canonical python rows: tuple of record fields + the trace as a tuple."""
    rows = []
    for la in las:
        t = tuple(int(x) for x in trace[la["toff"]:la["toff"] + la["tlen"]])
        rows.append(tuple(int(la[f]) for f in FIELDS) + (t,))
    return rows


def assert_same_las(got, exp):
    """Bit-exact comparison of two (records, trace) results."""
    g, e = la_rows(*got), la_rows(*exp)
    assert len(g) == len(e), f"LA count differs: got {len(g)} expected {len(e)}"
    for i, (x, y) in enumerate(zip(g, e)):
        assert x == y, f"LA {i} differs:\n got {x}\n exp {y}"


def check_trace_invariants(las, trace, tspace):
    """base.d:434-458: sum(bbases) == bepos - bbpos, sum(diffs) == diffs, #tp from A interval."""
    for la in las:
        t = trace[la["toff"]:la["toff"] + la["tlen"]].astype(np.int64)
        assert t[1::2].sum() == la["bepos"] - la["bbpos"]
        assert t[0::2].sum() == la["diffs"]
        assert la["tlen"] // 2 == -(-int(la["aepos"]) // tspace) - int(la["abpos"]) // tspace


def plant_long_indels(w, rng):
    """Reads of the workload `w` that span a gap get a 2-5 kb insertion of foreign bases, or lose 2-5 kb of contig bases,
    1.5-3.5 kb away from the gap (every second eligible read): each then maps as two collinear records on that flank,
    ONE alignment chain (dazzler.d:1728-1758).  Returns (reads DB, indices of the changed reads)."""
    from dentist_amd import sim
    seqs = [w.reads.seq(i) for i in range(w.reads.n)]
    planted, eligible = [], 0
    for i, (s0, e0, strand) in enumerate(w.read_truth):
        for g in range(len(w.gap_begin)):
            gb, ge = int(w.gap_begin[g]), int(w.gap_end[g])
            if not (s0 + 1500 < gb and ge + 1500 < e0):
                continue
            left = gb - s0 >= e0 - ge          # the longer flank part of the read gets the indel
            if (gb - s0 if left else e0 - ge) < 7000:
                continue
            eligible += 1
            if eligible % 2:
                continue
            # a position 1.5-3.5 kb away from the gap, in read coordinates (reads are ~ (1 + ins - del) longer than the truth)
            d = int(rng.integers(1500, 3500))
            gpos = gb - d if left else ge + d
            scale = len(seqs[i]) / float(e0 - s0)
            at = int((gpos - s0) * scale) if not strand else int((e0 - gpos) * scale)
            ln = int(rng.integers(2000, 5000))
            s = seqs[i]
            if len(planted) % 2 == 0:    # foreign bases in the read
                seqs[i] = np.concatenate([s[:at], rng.integers(0, 4, ln).astype(np.uint8), s[at:]])
            else:                        # contig bases missing from the read: cut away from the gap
                lo, hi = (at - ln, at) if left != bool(strand) else (at, at + ln)
                if lo < 1000 or hi > len(s) - 1000:
                    continue
                seqs[i] = np.concatenate([s[:lo], s[hi:]])
            planted.append(i)
            break
    return sim.SeqDb.from_list(seqs), planted


def plant_gap_insertions(w, rng, ln=1500):
    """Every second read of the workload `w` that spans a gap gets `ln` foreign bases in the middle of the gap: in the
    pile-up all-vs-all it aligns with the other reads as TWO local alignments that no chain joins (indel above
    --max-indel 1000, chaining.d:434-475) -- two components of the pair.  Returns (reads DB, indices of the changed reads)."""
    from dentist_amd import sim
    seqs = [w.reads.seq(i) for i in range(w.reads.n)]
    planted, eligible = [], 0
    for i, (s0, e0, strand) in enumerate(w.read_truth):
        for g in range(len(w.gap_begin)):
            gb, ge = int(w.gap_begin[g]), int(w.gap_end[g])
            if not (s0 + 1500 < gb and ge + 1500 < e0):
                continue
            eligible += 1
            if eligible % 2:
                break
            mid = (gb + ge) // 2
            scale = len(seqs[i]) / float(e0 - s0)
            at = int((mid - s0) * scale) if not strand else int((e0 - mid) * scale)
            seqs[i] = np.concatenate([seqs[i][:at], rng.integers(0, 4, ln).astype(np.uint8), seqs[i][at:]])
            planted.append(i)
            break
    return sim.SeqDb.from_list(seqs), planted


def tandem_reads(seed=7, n=12):
    """Random reads, two of three with a tandem array planted: a unit of 24 .. 900 bases repeated so that the array spans
    at least 700 bases, every copy with 8 % errors.  Returns (SeqDb, [(read, array begin, array end, period)])."""
    from dentist_amd import sim
    rng = np.random.default_rng(seed)

    def mutate(u, err):
        out = []
        for b in u:
            x = rng.random()
            if x < err / 3:
                continue
            if x < 2 * err / 3:
                out.append(int(rng.integers(0, 4)))
            out.append(int(b) if x >= err else int(rng.integers(0, 4)))
        return np.array(out, dtype=np.uint8)
    seqs, truth = [], []
    periods = [24, 150, 400, 900, 60]
    for i in range(n):
        ln = int(rng.integers(6000, 12000))
        s = rng.integers(0, 4, ln).astype(np.uint8)
        if i % 3 != 2:
            per = periods[len(truth) % len(periods)]
            copies = max(int(rng.integers(4, 12)), 700 // per + 2)
            unit = rng.integers(0, 4, per).astype(np.uint8)
            arr = np.concatenate([mutate(unit, 0.08) for _ in range(copies)])
            at = int(rng.integers(1000, ln - 1000))
            s = np.concatenate([s[:at], arr, s[at:]])
            truth.append((i, at, at + len(arr), per))
        seqs.append(s)
    return sim.SeqDb.from_list(seqs), truth


# ---------------------------------------------------------------- scaffold-graph pile-ups of the oracle (oracle/scaffold.py)
def la_chains(las, contigs, reads, idx=None, contig_shift=0):
    """One oracle/scaffold.py chain per record (all of `las`, or the records `idx`): id = the record's index in `las`,
    contig ids 1-based after subtracting `contig_shift`."""
    from oracle import scaffold as sc
    idx = range(len(las)) if idx is None else idx
    out = []
    for i in idx:
        l = las[i]
        a, b = int(l["aread"]), int(l["bread"])
        out.append(sc.chain(int(i), a - contig_shift + 1, contigs.length(a), b + 1, reads.length(b), bool(l["flags"] & 1),
                            int(l["abpos"]), int(l["aepos"]), int(l["bbpos"]), int(l["bepos"]),
                            disabled=bool(l["flags"] & 0x20)))
    return out


def oracle_gap_entries(pile_ups):
    """{left contig (0-based): [(read, LA on the left contig or -1, LA on the right contig or -1)]} of the gap pile-ups
    between neighbouring contigs that oracle/scaffold.py:build returned, entries in the builder's order."""
    from oracle import scaffold as sc
    exp = {}
    for e, ras in pile_ups:
        (c0, p0), (c1, p1) = e["start"], e["end"]
        if not (p0 == sc.END and p1 == sc.BEGIN and c1 == c0 + 1):
            continue
        ent = []
        for ra in ras:
            if len(ra) == 2:
                a, b = sorted(ra, key=lambda s: s[0]["a_id"])
                ent.append((a[0]["b_id"] - 1, a[0]["id"], b[0]["id"]))
            elif ra[0][0]["a_id"] == c0:
                ent.append((ra[0][0]["b_id"] - 1, ra[0][0]["id"], -1))
            else:
                ent.append((ra[0][0]["b_id"] - 1, -1, ra[0][0]["id"]))
        exp[c0 - 1] = ent
    return exp


def batch_order(ent):
    """Entries in the order of the product's batch: by read; the halves of a spanning read that opens with an extension:
    left one first."""
    return sorted(ent, key=lambda t: (t[0], t[1] < 0))


def cap_entries(ent, las, max_reads):
    """The read cap of dh_pileups_select restated on entries in batch order: distinct reads first, reads that span the gap
    before extension entries, then the lowest error rate of the anchoring alignments."""
    if max_reads <= 0 or len(ent) <= max_reads:
        return ent

    def err(t):
        ln = sum(int(las[i]["aepos"] - las[i]["abpos"]) for i in t[1:] if i >= 0)
        df = sum(int(las[i]["diffs"]) for i in t[1:] if i >= 0)
        return df * 1000000 // max(ln, 1)
    second = [False] * len(ent)   # every entry of a read but its best one ranks behind all first entries
    x0 = 0
    while x0 < len(ent):
        x1 = x0
        while x1 < len(ent) and ent[x1][0] == ent[x0][0]:
            x1 += 1
        best = min(range(x0, x1), key=lambda x: (err(ent[x]), x))
        for x in range(x0, x1):
            second[x] = x != best
        x0 = x1
    ext = [t[1] < 0 or t[2] < 0 for t in ent]   # ... and extension entries behind the reads that span the gap
    order = sorted(range(len(ent)), key=lambda x: (2 * ext[x] + second[x], err(ent[x]), x))[:max_reads]
    return [ent[x] for x in sorted(order)]


def restricted_gap_entries(las, contigs, reads, g, min_spanning_reads=3, window=1):
    """Entries of the gap behind contig `g` from oracle/scaffold.py:build on the records of contigs g - window ..
    g + 1 + window only (build walks every node against every edge: the whole graph of 1 001 contigs is out of reach).
    Exact while no read of the pile-up has a record outside the window: a 15 kb read cannot touch more than two contigs
    when the gaps are at least 20 kb apart."""
    from oracle import scaffold as sc
    lo, hi = max(0, g - window), min(contigs.n - 1, g + 1 + window)
    idx = np.flatnonzero((las["aread"] >= lo) & (las["aread"] <= hi))
    chains = la_chains(las, contigs, reads, idx, contig_shift=lo)
    n = hi - lo + 1
    got = oracle_gap_entries(sc.build(n, chains, [(c, c + 1) for c in range(1, n)], min_spanning_reads=min_spanning_reads))
    return batch_order(got.get(g - lo, []))


# ---------------------------------------------------------------- samples of a full-size run
def sub_db(db, ids):
    """SeqDb of the sequences `ids` of `db`, in that order."""
    from dentist_amd import sim
    return sim.SeqDb.from_list([db.seq(int(i)) for i in ids])


def chunk_bounds(nreads, chunk_items=1 << 20):
    """[first read, end read) of every chunk of one mapping call by the rule of align_range (the chunk loop in dh_align.cpp; the
    chunk size is prepare_dbs', dh_align_prepare.cpp): chunks of `chunk_items` items, two items (strands) per read."""
    per = chunk_items // 2
    return [(r, min(r + per, nreads)) for r in range(0, nreads, per)]


def chunk_edge_reads(nreads, chunk_items=1 << 20, edge=64):
    """The first and the last `edge` reads of every chunk."""
    out = []
    for lo, hi in chunk_bounds(nreads, chunk_items):
        out += list(range(lo, min(lo + edge, hi))) + list(range(max(hi - edge, lo), hi))
    return np.unique(np.asarray(out, dtype=np.int64))


def offset_wrap_reads(off, chunk_items=1 << 20, wrap=1 << 32, span=8):
    """Reads whose bases hold a byte offset that is a multiple of `wrap`, counted from the start of the DB or from the
    start of the read's chunk (offset 0 itself is no wrap).  Returns (those reads, those and `span` reads on either side)."""
    off = np.asarray(off, dtype=np.int64)
    n = len(off) - 1
    hit = set()
    for lo, hi in [(0, n)] + chunk_bounds(n, chunk_items):
        m = int(off[lo]) + wrap
        while m < int(off[hi]):
            hit.add(int(np.searchsorted(off, m, side="right")) - 1)
            m += wrap
    hit = np.asarray(sorted(hit), dtype=np.int64)
    around = [np.arange(max(0, r - span), min(n, r + span + 1)) for r in hit]
    return hit, (np.unique(np.concatenate(around)) if around else hit)


def first_distinct(values, limit):
    out, seen = [], set()
    for v in values:
        v = int(v)
        if v not in seen:
            seen.add(v)
            out.append(v)
            if len(out) == limit:
                break
    return out


def contig_extreme_reads(w, las, near=32, overhang=64):
    """The `near` mapped reads closest to each end of the first and of the last contig, and the `overhang` mapped reads
    whose true origin (w.read_truth) reaches the furthest past a gap edge."""
    out = []
    for c in (0, w.contigs.n - 1):
        idx = np.flatnonzero(las["aread"] == c)
        out += first_distinct(las["bread"][idx[np.argsort(las["abpos"][idx], kind="stable")]], near)
        out += first_distinct(las["bread"][idx[np.argsort(-las["aepos"][idx].astype(np.int64), kind="stable")]], near)
    s, e = w.read_truth[:, 0], w.read_truth[:, 1]
    gb, ge = np.asarray(w.gap_begin, dtype=np.int64), np.asarray(w.gap_end, dtype=np.int64)
    over = np.zeros(len(s), dtype=np.int64)
    if len(gb):
        i = np.minimum(np.searchsorted(gb, s, side="right"), len(gb) - 1)    # the first gap that begins behind the read's start
        over = np.where((gb[i] > s) & (gb[i] < e), e - gb[i], 0)
        j = np.maximum(np.searchsorted(ge, e, side="left") - 1, 0)           # the last gap that ends before the read's end
        over = np.maximum(over, np.where((ge[j] > s) & (ge[j] < e), ge[j] - s, 0))
    mapped = np.zeros(len(s), dtype=bool)
    mapped[las["bread"]] = True
    over[~mapped] = 0
    far = np.argsort(-over, kind="stable")[:overhang]
    out += [int(r) for r in far if over[r] > 0]
    return np.unique(np.asarray(out, dtype=np.int64))


def record_count_reads(las, nreads, rng, most=100, none=200):
    """The `most` reads with the most records (ties: seeded random -- nearly every read has one or two, and the lower read
    numbers would all sit at the start of the DB) and up to `none` reads without a record."""
    cnt = np.bincount(las["bread"], minlength=nreads)
    top = np.lexsort((rng.permutation(nreads), -cnt))[:most]
    zero = np.flatnonzero(cnt == 0)
    if len(zero) > none:
        zero = rng.choice(zero, size=none, replace=False)
    return np.unique(np.concatenate([top[cnt[top] > 0], zero]).astype(np.int64))


STRATA = ("chunk edges", "offset wrap", "contig extremes", "record count", "pile-up members", "seeded random")


def fullsize_read_sample(w, las, rng, pile_reads=(), size=2000, chunk_items=1 << 20, wrap=1 << 32):
    """A sample of the reads of one mapping call, stratified by where the call's code changes with size -- see STRATA:
    `size` reads beyond the pile-up members.  `las`: the records of the run under test (strata 3 and 4 read them).
    Returns (sorted unique read numbers, {stratum: reads it added to the strata before it}, the reads that hold a
    multiple of `wrap`)."""
    n = w.reads.n
    wrapped, around = offset_wrap_reads(w.reads.off, chunk_items, wrap)
    pile_reads = np.unique(np.asarray(pile_reads, dtype=np.int64))
    strata = [chunk_edge_reads(n, chunk_items), around, contig_extreme_reads(w, las), record_count_reads(las, n, rng), pile_reads]
    taken = np.zeros(n, dtype=bool)
    counts = {}
    for name, ids in zip(STRATA, strata):
        counts[name] = int((~taken[ids]).sum())
        taken[ids] = True
    fill = max(0, size - (int(taken.sum()) - counts["pile-up members"]))
    rest = np.flatnonzero(~taken)
    extra = rng.choice(rest, size=min(fill, len(rest)), replace=False)
    counts["seeded random"] = len(extra)
    taken[extra] = True
    return np.flatnonzero(taken).astype(np.int64), counts, wrapped


def assert_same_las_of_reads(got, exp, ids):
    """Bit-exact comparison of the records of the reads `ids`: got = (records, trace) of a run over the whole DB, exp =
    (records, trace) of a run over sub_db(reads, ids) -- its `bread` counts within `ids` and is mapped back here.  The
    order of a read's records is kept; a read without records on one side must have none on the other.  Returns
    (records compared, trace values compared)."""
    ids = np.asarray(ids, dtype=np.int64)
    assert np.all(np.diff(ids) > 0), "read numbers must be sorted and unique"
    (glas, gtrace), (elas, etrace) = got, exp
    elas = elas.copy()
    elas["bread"] = ids[elas["bread"]]
    gsel = np.flatnonzero(np.isin(glas["bread"], ids))
    gsel = gsel[np.argsort(glas["bread"][gsel], kind="stable")]
    esel = np.argsort(elas["bread"], kind="stable")
    gb, eb = glas["bread"][gsel], elas["bread"][esel]
    nrec = ntr = 0
    for r in ids:
        g = glas[gsel[np.searchsorted(gb, r, side="left"):np.searchsorted(gb, r, side="right")]]
        e = elas[esel[np.searchsorted(eb, r, side="left"):np.searchsorted(eb, r, side="right")]]
        try:
            assert_same_las((g, gtrace), (e, etrace))
        except AssertionError as err:
            raise AssertionError(f"read {int(r)}: {err}") from None
        nrec += len(e)
        ntr += int(e["tlen"].sum())
    return nrec, ntr


# ---------------------------------------------------------------- pile-ups of a full-size batch
def process_part_cuts(counts, nparts=3):
    """First pile-up of every concurrent part of dh_process_pileups (plan_part_cuts of dh_batch.cpp: contiguous runs of the batch with
    equal shares of the sum of entries^2, none empty; fewer than 64 pile-ups run in one piece).  Returns [0, cut 1, ..., n]."""
    n = len(counts)
    if n < 64:
        return [0, n]
    nparts = min(nparts, n // 16)
    cost = [float(c) * float(c) for c in counts]
    total = 0.0
    for c in cost:
        total += c
    wcum = [0.0]
    for _ in range(nparts):
        wcum.append(wcum[-1] + 1.0 / float(nparts))
    cut, p, acc = [0], 0, 0.0
    for k in range(1, nparts):
        while p < n and acc + cost[p] <= total * wcum[k]:
            acc += cost[p]
            p += 1
        while p < cut[k - 1] + 1:
            acc += cost[p]
            p += 1
        p = min(p, n - (nparts - k))
        cut.append(p)
    return cut + [n]


def fullsize_pile_sample(counts, gap_len, rng, nparts=3, nrandom=2):
    """Positions in a batch of pile-ups where the process stage changes with size: {what: position} -- the ends of the batch,
    the extremes of entries and gap length (ties: the first), both sides of every cut between the concurrent parts, and
    `nrandom` seeded random ones that are none of those."""
    counts, gap_len = np.asarray(counts), np.asarray(gap_len)
    n = len(counts)
    out = {"first": 0, "last": n - 1, "most entries": int(np.argmax(counts)), "fewest entries": int(np.argmin(counts)),
           "longest gap": int(np.argmax(gap_len)), "shortest gap": int(np.argmin(gap_len))}
    for k, c in enumerate(process_part_cuts(counts, nparts)[1:-1], start=1):
        out[f"last of part {k}"] = c - 1
        out[f"first of part {k + 1}"] = c
    rest = np.setdiff1d(np.arange(n), np.asarray(sorted(set(out.values()))))
    for k, p in enumerate(rng.choice(rest, size=min(nrandom, len(rest)), replace=False)):
        out[f"random {k + 1}"] = int(p)
    return out


PROCESS_STATUS = {0: "ok", 1: "no common trace point", 2: "pile too small", 3: "empty pileup alignment after filtering"}


def assert_same_insertion(r, bases, exp):
    """One record of dh_process_pileups (with the consensus bases of the call) against oracle/process.py:process_pile:
    status, crop points, pile-up reads, reference read, every consensus base, splice coordinates, inserted bases.
    Returns the status by its name."""
    from dentist_amd import sim
    g = exp["gap"]
    if exp["status"] != "ok":
        assert r["status"] != 0, (g, exp["status"])
        if int(r["status"]) in PROCESS_STATUS:
            assert PROCESS_STATUS[int(r["status"])] == exp["status"], g
        return exp["status"]
    assert r["status"] == 0, (g, int(r["status"]))
    assert (r["crop_left"], r["crop_right"]) == (exp["cropL"], exp["cropR"]), g
    assert r["nreads"] == exp["pile"].n and r["ref_read"] == exp["ref_idx"], g
    assert r["ref_read_id"] == exp["read_ids"][exp["ref_idx"]], g
    cons = bases[r["cons_off"]:r["cons_off"] + r["cons_len"]]
    assert np.array_equal(cons, exp["consensus"]), f"gap {g}: consensus differs"
    assert (r["left_aepos"], r["right_abpos"], r["ins_begin"], r["ins_end"]) == \
           (exp["left_aepos"], exp["right_abpos"], exp["ins_begin"], exp["ins_end"]), g
    cseq = sim.revcomp(cons) if r["comp"] else cons
    assert np.array_equal(cseq[r["ins_begin"]:r["ins_end"]], exp["insertion"]), f"gap {g}: inserted bases differ"
    return "ok"
