"""The shapes of dh_output_db's tests: inputs of `dentist output` (contigs, scaffolds, insertions) small enough to be read, one
per way the formatter can go wrong -- every line width, a body of one base, bodies that end on a full line, an empty body, a
segment and an n run of one base, a scaffold walked from a contig END, a complemented insertion, highlight off, extensions, a
cycle, a header longer than the smallest chunk, 300 records that share lanes, a segment that spans many chunks.  Each case is
also written as an insertions.db (write_db) for the route through the file.  `python tests/outfmt_cases.py <file>` dumps the
plans for tests/native/outfmt_host_san."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dentist_amd  # noqa: E402

FRONT0, BACK1, EXT = 1, 2, 4
WIDTHS = (0, 1, 3, 7, 50)
CHUNKS = {"default": None, "64": 64, "112": 112}   # bytes; "record": chunk_at_record_boundary(plan)


def _rec(n):
    r = np.zeros(n, dtype=dentist_amd.INSERTION_DTYPE)
    r["contig_right"] = -1
    r["right_abpos"] = -1
    return r


def _gap(r, left, right, join, left_pos, right_pos, b, e, comp, cons_off, cons_len, ref=0):
    r["contig_left"], r["contig_right"], r["join"], r["left_aepos"], r["right_abpos"] = left, right, join, left_pos, right_pos
    r["ins_begin"], r["ins_end"], r["comp"], r["cons_off"], r["cons_len"], r["ref_read_id"] = b, e, comp, cons_off, cons_len, ref


def _ext(r, contig, front, pos, b, e, comp, cons_off, cons_len, ref=0):
    r["contig_left"], r["contig_right"], r["join"], r["left_aepos"], r["right_abpos"] = contig, -1, EXT | (FRONT0 if front else 0), pos, -1
    r["ins_begin"], r["ins_end"], r["comp"], r["cons_off"], r["cons_len"], r["ref_read_id"] = b, e, comp, cons_off, cons_len, ref


def _case(lens, scaffold_of, headers, gap_len, rec, cons_lens, seed, ids=None, **kw):
    rng = np.random.default_rng(seed)
    contigs = [rng.integers(0, 4, n).astype(np.uint8) for n in lens]
    cons = [rng.integers(0, 4, n).astype(np.uint8) for n in cons_lens]
    bases = np.concatenate(cons) if cons else np.zeros(0, np.uint8)
    if ids is None:   # read ids 0-based: two or three per insertion
        per = [sorted(rng.choice(40, 2 + i % 2, replace=False).tolist()) for i in range(len(rec))]
        ids = (np.asarray([x for p in per for x in p], np.int32), np.cumsum([0] + [len(p) for p in per]).astype(np.int64))
    opts = dict(line_width=50, highlight=True, join_policy="scaffoldGaps", only="spanning", min_extension_length=100)
    opts.update(kw)
    return dict(contigs=contigs, scaffold_of=list(scaffold_of), headers=list(headers), gap_len=list(gap_len), rec=rec, bases=bases, ids=ids,
                opts=opts)


def basic(width, highlight=True):
    # scaffold A = contigs 0-2 (gaps of 30 and of ONE n), scaffold B = contig 3, then one contig per scaffold of 1, 7, 21, 50 and 100
    # bases (a body of one base; bodies that are whole lines at widths 1, 3, 7 and 50).  Gap 0|1 closed forward, gap 1|2 failed (its
    # n stays), the join 2|3 between the scaffolds by a complemented consensus (policy scaffolds).
    lens = [120, 80, 60, 90, 1, 7, 21, 50, 100]
    r = _rec(3)
    _gap(r[0], 0, 1, 0, 110, 5, 10, 42, 0, 0, 50, ref=7)
    r[1]["contig_left"], r[1]["contig_right"], r[1]["status"] = 1, 2, 4
    _gap(r[2], 2, 3, 0, 55, 3, 4, 30, 1, 50, 40, ref=2)
    return _case(lens, [0, 0, 0, 1, 2, 3, 4, 5, 6], ["scafA\textra", "scafB", "one", "seven", "twentyone", "fifty", "hundred"],
                 [30, 1, 0, 0, 0, 0, 0, 0, 0], r, [50, 40], 3, line_width=width, highlight=highlight, join_policy="scaffolds")


def reversed_start():
    # an anti-parallel join of the BEGINs of contigs 0 and 1 (policy contigs): the scaffold starts at the END of contig 0 and walks
    # it reversed; contig 1 is kept from base 29 of 30 on: a slice of ONE base
    r = _rec(1)
    _gap(r[0], 0, 1, FRONT0, 4, 29, 6, 20, 0, 0, 25)
    return _case([40, 30, 17], [0, 1, 2], ["a", "b", "c"], [0, 0, 0], r, [25], 5, line_width=7, join_policy="contigs")


def extensions():
    # a front extension of contig 0 and a back extension of contig 1 (only = both); contig 2 stands alone with an empty front and an
    # empty back extension whose splice sites meet at base 20: an empty body
    r = _rec(4)
    _ext(r[0], 0, True, 3, 0, 25, 0, 0, 40)
    _ext(r[1], 1, False, 85, 10, 40, 0, 40, 40)
    _ext(r[2], 2, True, 20, 0, 0, 0, 80, 12)
    _ext(r[3], 2, False, 20, 12, 12, 0, 92, 12)
    return _case([100, 90, 40, 9], [0, 0, 1, 2], ["ext", "empty", "tail"], [15, 0, 0, 0], r, [40, 40, 12, 12], 7, line_width=3, only="both",
                 min_extension_length=0)


def extensions_complement():
    r = _rec(2)
    _ext(r[0], 0, True, 3, 0, 25, 1, 0, 40)
    _ext(r[1], 0, False, 85, 10, 40, 1, 40, 40)
    return _case([100], [0], ["extc"], [0], r, [40, 40], 8, line_width=50, only="extending", min_extension_length=10)


def cyclic():
    # contigs 0 and 1 joined end to begin twice: a cycle (the isCyclic header)
    r = _rec(2)
    _gap(r[0], 0, 1, 0, 70, 4, 3, 19, 0, 0, 22)
    _gap(r[1], 0, 1, FRONT0 | BACK1, 6, 55, 2, 18, 0, 22, 20)
    return _case([80, 60], [0, 1], ["ring", "other"], [0, 0], r, [22, 20], 9, line_width=50, join_policy="contigs")


def many_small():
    # a header longer than the smallest chunk, then 300 records of one contig of 1-5 bases each: many records inside one lane's 16 bytes
    rng = np.random.default_rng(11)
    lens = [33] + rng.integers(1, 6, 300).tolist()
    headers = ["long_" + "h" * 200 + "\tcomment"] + [f"s{i}" for i in range(300)]
    return _case(lens, list(range(301)), headers, [0] * 301, _rec(0), [], 11, line_width=3)


def big():
    # one contig of 70 000 bases (a segment that spans many chunks) joined to a second one
    r = _rec(1)
    _gap(r[0], 0, 1, 0, 69990, 12, 5, 300, 1, 0, 320)
    return _case([70000, 500], [0, 0], ["big"], [100, 0], r, [320], 13, line_width=50)


def build():
    cases = {f"basic_w{w}": basic(w) for w in WIDTHS}
    cases["nohighlight"] = basic(50, highlight=False)
    cases["reversed_start"] = reversed_start()
    cases["extensions"] = extensions()
    cases["extensions_complement"] = extensions_complement()
    cases["cyclic"] = cyclic()
    cases["many_small"] = many_small()
    cases["many_small_w0"] = dict(many_small(), opts=dict(many_small()["opts"], line_width=0))
    cases["big"] = big()
    return cases


ALL = build()


def seqdb(c):
    from dentist_amd import sim
    return sim.SeqDb.from_list(c["contigs"])


def plan_of(c):
    off = np.cumsum([0] + [len(x) for x in c["contigs"]])
    return dentist_amd.output_plan(off, c["scaffold_of"], c["headers"], c["gap_len"], c["rec"], len(c["bases"]), **c["opts"])


def host_fasta(c, path, rec=None, bases=None, ids=None, **files):
    """the host writer (dh_output_assembly) on the case: the oracle of every route"""
    return dentist_amd.output_assembly(path, seqdb(c), c["scaffold_of"], c["headers"], c["gap_len"], c["rec"] if rec is None else rec,
                                       c["bases"] if bases is None else bases, read_ids=c["ids"] if ids is None else ids,
                                       agp_dazzler=True, **files, **c["opts"])


def chunk_at_record_boundary(plan):
    """a chunk size (a multiple of 16, at least 64) at which a chunk ends exactly where a record ends; None if the case has none"""
    for q in plan["rec_off"][1:-1]:
        if q >= 64 and q % 16 == 0:
            return int(q)
    return None


def write_db(c, path, diffs=None):
    """the case's insertions as an insertions.db: per closed gap or extension the overlaps that dh_insertions_from_db turns back
    into the case's record (a front-seeded overlap runs from the splice site to the contig's end and to the consensus' end, a
    back-seeded one from both begins to the splice site).  diffs: {record index: (left, right)}."""
    ins, sa, la, bases, ids = [], [], [], [], []
    lens = [len(x) for x in c["contigs"]]
    for i, r in enumerate(c["rec"]):
        if r["status"] != 0:
            continue
        ext = bool(r["join"] & EXT)
        front = [bool(r["join"] & FRONT0), not (r["join"] & BACK1)]
        clen, lc = int(r["cons_len"]), int(r["comp"])
        q = np.zeros(1, dentist_amd.INSERTION_REC_DTYPE)[0]
        c0 = int(r["contig_left"])
        c1 = c0 if ext else int(r["contig_right"])
        q["start_contig"], q["end_contig"] = c0 + 1, c1 + 1
        if ext:
            q["start_part"], q["end_part"] = (0, 1) if front[0] else (2, 3)
        else:
            q["start_part"], q["end_part"] = (1 if front[0] else 2), (1 if front[1] else 2)
        my = sorted(int(x) + 1 for x in c["ids"][0][int(c["ids"][1][i]):int(c["ids"][1][i + 1])])
        q["seq_len"], q["noverlaps"], q["nread_ids"] = clen, 1 if ext else 2, len(my)
        ins.append(q)
        bases.append(c["bases"][int(r["cons_off"]):int(r["cons_off"]) + clen])
        ids += my
        if ext:
            sides = [(c0, front[0], lc, int(r["left_aepos"]), int(r["ins_end"]) if front[0] else int(r["ins_begin"]))]
        else:
            rc = lc if front[0] != front[1] else 1 - lc
            p0 = int(r["ins_end"]) if front[0] else int(r["ins_begin"])
            p1 = int(r["ins_begin"]) if front[0] else int(r["ins_end"])
            if rc != lc:
                p1 = clen - p1
            sides = [(c0, front[0], lc, int(r["left_aepos"]), p0), (c1, front[1], rc, int(r["right_abpos"]), p1)]
        for k, (cc, fr, comp, apos, bpos) in enumerate(sides):
            s = np.zeros(1, dentist_amd.SEEDED_DTYPE)[0]
            s["id"], s["contig_a_id"], s["contig_a_len"], s["contig_b_id"], s["contig_b_len"] = len(sa), cc + 1, lens[cc], 1, clen
            s["flags"], s["seed"], s["tspace"], s["nla"] = comp, 0 if fr else 1, 100, 1
            sa.append(s)
            a = np.zeros(1, dentist_amd.CHAIN_LA_DTYPE)[0]
            if fr:
                a["a_begin"], a["a_end"], a["b_begin"], a["b_end"] = apos, lens[cc], bpos, clen
            else:
                a["a_begin"], a["a_end"], a["b_begin"], a["b_end"] = 0, apos, 0, bpos
            a["diffs"] = diffs[i][k] if diffs and i in diffs else 0
            a["ntp"] = 0
            la.append(a)
    dentist_amd.insertiondb_write(path, np.asarray(ins, dentist_amd.INSERTION_REC_DTYPE),
                                  np.concatenate(bases) if bases else np.zeros(0, np.uint8), np.asarray(ids, np.uint32),
                                  np.asarray(sa, dentist_amd.SEEDED_DTYPE), np.asarray(la, dentist_amd.CHAIN_LA_DTYPE), np.zeros(0, np.uint16))


def dump_plans(path):
    with open(path, "wb") as f:
        f.write(np.int64(len(ALL)).tobytes())
        for c in ALL.values():
            p = plan_of(c)
            f.write(np.int64(p["width"]).tobytes())
            for name in ("rec_off", "hdr_off", "seg_first", "seg_base", "seg_src", "seg_flags", "hdr"):
                f.write(np.int64(len(p[name])).tobytes() + p[name].tobytes())
            cb = np.concatenate(c["contigs"])
            f.write(np.int64(len(cb)).tobytes() + cb.tobytes())
            f.write(np.int64(len(c["bases"])).tobytes() + c["bases"].tobytes())


if __name__ == "__main__":
    dump_plans(sys.argv[1])
