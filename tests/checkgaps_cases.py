"""Constructed scenes for dh_check_gaps, shared by the restatement's tests, the CPU harness and the GPU parity test.  A scene is a
true assembly, the input contigs as mapped intervals on it, a result assembly put together gap by gap (closed with a given or
mutated sequence, left open behind an N-run, partially filled on both sides of one) and the mappings of the cropped contigs that
follow from the construction; `tweak` then bends single mappings.  Each case is the smallest that can go wrong.  expected_of(name)
runs the restatement (tests/checkgaps_ref.py) once per case and process.  Not a test module.

`legal` is False for the scenes with a gap of 0 bases: dh_check_gaps refuses touching mapped intervals (the reference's mask would
merge them), so these run through the restatement and the lane code only, and through the call as refusals."""
import functools

import numpy as np

import checkgaps_ref as cr
from nw_ref import mutate

MAP_DTYPE = np.dtype([("ref_contig", "<i4"), ("ref_begin", "<i4"), ("ref_end", "<i4"), ("ref_contig_length", "<i4"), ("query_contig", "<i4"),
                      ("duplicate", "<i4"), ("complement", "<i4"), ("alignment_error", "<f4")])
SUMMARY_DTYPE = np.dtype([(f, "<i4") for f in cr.FIELDS])


def rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def closed(seq=None, div=0.0, run_of=0):
    """seq: None = the true gap sequence mutated at `div`; an array; or a function of (rng, true gap sequence).  run_of: instead, the
    true gap sequence behind that many copies of a base that neither neighbour is (the insertion can stand nowhere else)"""
    return {"kind": "closed", "seq": seq, "div": div, "run_of": run_of}


def unclosed(run=50):
    return {"kind": "unclosed", "run": run}


def partial(left, right, run=50):
    return {"kind": "partial", "left": left, "right": right, "run": run}


def build(seed, crop, contigs, dust=None, complement=(), tweak=None, first_contig=1, count=None, legal=True, scoring=None):
    """contigs: per true contig (length, [(begin, end) of its input contigs], [what became of the gap behind each but the last])"""
    rng = np.random.default_rng(seed)
    true_seqs, mapped, maps, result, result_gap = [], [], [], [], []
    for t, (length, ivs, gaps) in enumerate(contigs):
        true = rnd(rng, length)
        true_seqs.append(true)
        cur = []

        def finish(run):
            result.append(np.concatenate(cur).astype(np.uint8) if cur else np.zeros(0, np.uint8))
            result_gap.append(run)
            cur.clear()
        assert len(gaps) == len(ivs) - 1
        for k, (b, e) in enumerate(ivs):
            pos = sum(len(x) for x in cur)
            cur.append(true[b:e])
            mapped.append((t + 1, b, e))
            maps.append({"ref_contig": len(result) + 1, "ref_begin": pos + crop, "ref_end": max(pos + crop, pos + (e - b) - crop), "ref_contig_length": 0,
                         "query_contig": len(mapped), "duplicate": 0, "complement": 0})
            if k == len(gaps):
                break
            g, hole = gaps[k], true[e:ivs[k + 1][0]]
            if g["kind"] == "closed":
                s = g["seq"]
                if g["run_of"]:
                    s = np.concatenate([np.full(g["run_of"], next(x for x in range(4) if x != true[e - 1] and x != true[e]), np.uint8), hole])
                cur.append(mutate(rng, hole, g["div"]) if s is None else (s(rng, hole) if callable(s) else np.asarray(s, np.uint8)))
            elif g["kind"] == "unclosed":
                finish(g["run"])
            else:
                cur.append(hole[:g["left"]])
                finish(g["run"])
                cur.append(hole[len(hole) - g["right"]:])
        finish(0)
    for m in maps:
        m["ref_contig_length"] = len(result[m["ref_contig"] - 1])
    for c in complement:  # result contig c (1-based) comes out reversed
        result[c - 1] = cr.revcomp(result[c - 1])
        for m in maps:
            if m["ref_contig"] == c:
                m["ref_begin"], m["ref_end"], m["complement"] = len(result[c - 1]) - m["ref_end"], len(result[c - 1]) - m["ref_begin"], 1
    scene = {"true_seqs": true_seqs, "result_seqs": result, "mapped": mapped, "maps": maps, "result_gap": result_gap, "dust": dust, "crop": crop,
             "first_contig": first_contig, "count": len(mapped) - first_contig + 1 if count is None else count, "legal": legal,
             "scoring": scoring}
    if tweak:
        tweak(scene)
    return scene


def maps_array(maps):
    a = np.zeros(len(maps), MAP_DTYPE)
    for k, m in enumerate(maps):
        for f in MAP_DTYPE.names[:-1]:
            a[k][f] = m[f]
    return a


def dust_arrays(dust, n_true):
    """(ptr, iv) in the layout of dh_dazz_read_mask, or (None, None)"""
    if dust is None:
        return None, None
    ptr, iv = [0], []
    for t in range(1, n_true + 1):
        iv += [x for be in dust.get(t, []) for x in be]
        ptr.append(len(iv) // 2)
    return np.asarray(ptr, np.int64), np.asarray(iv + [0, 0], np.int32)


# ---------------------------------------------------------------------------------------------------------------- the scenes
def _states_tweak(s):
    m = s["maps"]
    of = lambda q: next(x for x in m if x["query_contig"] == q)
    last = len(s["result_seqs"])
    # contigs 1..12 on true contig 1: gaps closed, unclosed, partial, then the bent ones
    of(6).update(ref_contig=last, ref_contig_length=len(s["result_seqs"][-1]), ref_begin=0, ref_end=10)   # 5|6, 6|7 broken: far away
    m.remove(of(8))                                                   # contig 8 has no mapping: 7|8 and 8|9 unkown
    m.append(dict(of(10), ref_begin=of(10)["ref_begin"] + 1))         # contig 10 has two: 9|10 and 10|11 unkown
    m.insert(0, dict(of(1), duplicate=1, ref_begin=3))                # contig 1: a duplicate beside the good one does not count
    of(12)["duplicate"] = 1                                           # contig 12's only mapping is a duplicate: 11|12 unkown
    m.reverse()                                                       # (any order)


def states(crop):
    ivs = [(100 + 400 * k, 400 + 400 * k) for k in range(12)]
    gaps = [closed(div=0.06), unclosed(), partial(30, 25), closed(), closed(), closed(), closed(), closed(), closed(), closed(), closed()]
    second = (1500, [(50, 400), (500, 900), (1000, 1450)], [closed(div=0.1), partial(0, 40, run=17)])
    return build(11 + crop, crop, [(5000, ivs, gaps), second], tweak=_states_tweak)


def _flip_rhs_strand(s):
    s["maps"][1]["complement"] = 1


def _shift_ends(s):
    s["maps"][0]["ref_end"] -= 3     # the query starts 3 bases early and ends 3 late: insertions in the first and last columns
    s["maps"][1]["ref_begin"] += 3


def _insert_at(k, extra):
    """`extra` copies of a base that neither neighbour is, in front of base k of the gap: the insertion can stand nowhere else"""
    def f(rng, hole):
        b = next(x for x in range(4) if x != hole[k] and x != hole[k - 1])
        return np.concatenate([hole[:k], np.full(extra, b, np.uint8), hole[k:]])
    return f


def _reverse_scaffold(s):
    """the two result contigs, both reversed already, change places: the result holds the scaffold's other strand"""
    s["result_seqs"].reverse()
    for m in s["maps"]:
        m["ref_contig"] = 3 - m["ref_contig"]
        m["ref_contig_length"] = len(s["result_seqs"][m["ref_contig"] - 1])


def _columns(crop):
    lens = [63, 64, 65, 260, 127, 128, 129]
    ivs, at = [], 50
    for n in lens + [0]:
        ivs.append((at, at + 300))
        at += 300 + max(n - 2 * crop, 1)
    return build(5, crop, [(at + 50, ivs, [closed()] * len(lens))])


def _many(crop, n=70):
    ivs = [(20 + 100 * k, 20 + 100 * k + 60) for k in range(n + 1)]
    return build(9, crop, [(100 * (n + 2), ivs, [closed(div=0.08 if k % 3 else 0.0) for k in range(n)])])


ALL = {
    "states_crop_0": lambda: states(0),
    "states_crop_20": lambda: states(20),
    "complemented_contig": lambda: build(3, 15, [(3000, [(100, 600), (700, 1300), (1500, 2000)], [closed(div=0.05), closed(div=0.05)])], complement=(1,)),
    "complemented_partial": lambda: build(4, 10, [(2000, [(100, 600), (900, 1500)], [partial(40, 60)])], complement=(1, 2), tweak=_reverse_scaffold),
    "strands_differ": lambda: build(3, 0, [(2000, [(100, 600), (700, 1300)], [closed()])], tweak=_flip_rhs_strand),
    "query_all_n": lambda: build(6, 0, [(1500, [(100, 500), (560, 1000)], [closed(seq=np.full(45, 4, np.uint8))])]),
    "query_all_n_crop": lambda: build(6, 12, [(1500, [(100, 500), (560, 1000)], [closed(seq=np.full(45, 4, np.uint8))])]),
    "query_empty": lambda: build(6, 0, [(1500, [(100, 500), (560, 1000)], [closed(seq=np.zeros(0, np.uint8))])]),
    "query_with_n_inside": lambda: build(6, 8, [(1500, [(100, 500), (560, 1000)], [closed(seq=lambda rng, h: np.concatenate([h[:20], [4] * 7, h[27:]]))])]),
    "reference_empty_gap_0": lambda: build(7, 0, [(1500, [(100, 500), (500, 1000)], [closed(seq=lambda rng, h: rnd(rng, 5))])], legal=False),
    "gap_0_crop_insertions": lambda: build(7, 12, [(1500, [(100, 500), (500, 1000)], [closed(run_of=5)])], legal=False),
    "crop_is_the_whole_contig": lambda: build(8, 20, [(1500, [(100, 500), (560, 600), (700, 1100)], [closed(div=0.05), closed()])]),
    "crop_bounds_move": lambda: build(12, 10, [(1500, [(100, 500), (650, 1000)], [closed()])], tweak=_shift_ends),
    "columns_crop_0": lambda: _columns(0),
    "columns_crop_10": lambda: _columns(10),
    "many_gaps": lambda: _many(0),
    "many_gaps_crop_7": lambda: _many(7),
    "dust_edges": lambda: build(13, 10, [(3000, [(100, 500), (700, 1100), (1300, 1700), (1900, 2300)], [closed(seq=_insert_at(60, 4)), closed(div=0.1), closed(div=0.1)])],
                                dust={1: [(450, 510), (560, 580), (690, 700), (1100, 1101), (1299, 1300), (1650, 1720), (2400, 2500)]}),
    "dust_at_insertions": lambda: build(14, 5, [(2000, [(100, 500), (700, 1100), (1300, 1700)], [closed(seq=_insert_at(60, 4)), closed(seq=_insert_at(60, 4))])],
                                        dust={1: [(540, 560), (1160, 1180)]}),
    "dust_crop_0": lambda: build(14, 0, [(2000, [(100, 500), (700, 1100), (1300, 1700)], [closed(seq=_insert_at(60, 4)), closed(div=0.15)])],
                                 dust={1: [(500, 501), (559, 561), (699, 700), (1100, 1300)], 2: []}),
    "dust_but_partial": lambda: build(15, 5, [(2000, [(100, 500), (800, 1200)], [partial(50, 50)])], dust={1: [(500, 800)]}),
    "no_dust_mask": lambda: build(13, 10, [(1500, [(100, 500), (700, 1100)], [closed(div=0.1)])]),
    "band_and_length": lambda: build(16, 5, [(75000, [(100, 400), (500, 800), (3400, 3700), (3800, 4100), (70200, 70500), (70600, 70900)],
                                              [closed(div=0.05), closed(seq=lambda rng, h: rnd(rng, len(h))), closed(div=0.05), closed(seq=lambda rng, h: rnd(rng, 30)),
                                               closed(div=0.05)])]),
    "batch_in_the_middle": lambda: build(5, 4, [(3000, [(100 + 300 * k, 300 + 300 * k) for k in range(8)], [closed(div=0.05)] * 7)], first_contig=3, count=4),
    "last_contig_alone": lambda: build(5, 4, [(1000, [(100, 400), (500, 900)], [closed()])], first_contig=2, count=1),
    "other_scoring": lambda: build(17, 6, [(1500, [(100, 500), (700, 1100)], [closed(div=0.15)])], scoring=(1, -1, 2, 1)),
}
GAP_0 = [n for n in ALL if n.startswith(("reference_empty_gap_0", "gap_0_"))]


@functools.lru_cache(maxsize=None)
def scene(name):
    return ALL[name]()


@functools.lru_cache(maxsize=None)
def expected_of(name):
    """(summaries as a structured array, identity, ops per gap or None)"""
    s = scene(name)
    an = cr.Analyzer(s["true_seqs"], s["result_seqs"], s["mapped"], s["maps"], s["result_gap"], s["dust"], s["crop"],
                     s["scoring"] or cr.nwa_ref.DEFAULT)
    sums, ops = an.analyze(s["first_contig"], s["count"])
    arr = np.zeros(len(sums), SUMMARY_DTYPE)
    for k, x in enumerate(sums):
        for f in cr.FIELDS:
            arr[k][f] = x[f]
    return arr, np.asarray([x["identity"] for x in sums], np.float64), ops


def refusals():
    """(name, scene, words of the message)"""
    def bent(name, f, **kw):
        s = dict(scene(name))
        s["maps"] = [dict(m) for m in s["maps"]]
        s["mapped"] = list(s["mapped"])
        s.update(kw)
        if f:
            f(s)
        return s

    def setm(k, **kw):
        return lambda s: s["maps"][k].update(kw)

    def setmapped(k, v):
        return lambda s: s["mapped"].__setitem__(k, v)
    base = "no_dust_mask"
    return [
        ("negative_crop", bent(base, None, crop=-1), "bad argument"),
        ("negative_count", bent(base, None, count=-1), "bad argument"),
        ("first_contig_0", bent(base, None, first_contig=0), "leave the 2 input contigs"),
        ("batch_behind_the_end", bent(base, None, first_contig=2, count=2), "leave the 2 input contigs"),
        ("true_contig_out_of_range", bent(base, setmapped(1, (2, 700, 1100))), "input contig 2: true contig 2 out of range"),
        ("interval_outside", bent(base, setmapped(1, (1, 700, 1501))), "input contig 2: mapped interval [700, 1501) outside true contig 1"),
        ("intervals_overlap", bent(base, setmapped(1, (1, 499, 1100))), "input contig 2: mapped interval not behind the one before it"),
        ("intervals_touch", bent(base, setmapped(1, (1, 500, 1100))), "input contig 2: mapped interval not behind the one before it"),
        ("gap_0_scene", scene("gap_0_crop_insertions"), "input contig 2: mapped interval not behind the one before it"),
        ("true_interval_leaves", bent(base, setmapped(0, (1, 0, 5)), crop=10), "input contig 2: the true interval of the gap in front of it leaves true contig 1"),
        ("mapping_query_range", bent(base, setm(1, query_contig=3)), "mapping 1: input contig 3 out of range"),
        ("mapping_ref_range", bent(base, setm(0, ref_contig=2)), "mapping 0: result contig 2 out of range"),
        ("mapping_outside", bent(base, setm(1, ref_end=100000)), ", 100000) outside result contig 1"),
        ("mapping_length", bent(base, setm(1, ref_contig_length=7)), "mapping 1: ref_contig_length 7 is not the length of result contig 1"),
        ("dust_unsorted", bent(base, None, dust={1: [(600, 650), (500, 550)]}), "dust mask: interval 1 of true contig 1"),
        ("dust_outside", bent(base, None, dust={1: [(1400, 1501)]}), "dust mask: interval 0 of true contig 1"),
        ("scoring", bent(base, None, scoring=(1, 2, 3, 4)), "scoring refused"),
    ]
