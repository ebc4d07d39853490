"""The contract of dh_la_validate_regions restated around the literal window loop of the oracle
(oracle.maskcov.validate_region, validateRegions.d:325-512): per region the report, the weak intervals and the ids of the
spanning reads in record order, the regions in input order, and the command's mask (the union per contig, util/region.d:776-816).
Test infrastructure; results are cached per case object."""
import json

import numpy as np

import dentist_amd
from oracle import maskcov as mc

REPORT_DTYPE = np.dtype([("num_spanning_reads", "<i4"), ("weak_bp", "<i4"), ("is_valid", "<i4"), ("ctx_begin", "<i4"), ("ctx_end", "<i4")])
_cache = {}


def extended(region, contig_len, context):
    """(cb, ce) of validateRegions.d:178-190"""
    _, b, e = region
    return (b - context if b > context else 0), min(e + context, contig_len)


def merged_mask(weak, ncontigs):
    """(ptr int64[ncontigs + 1], iv int32[k, 2]): per contig sorted, intersecting or touching intervals merged"""
    ptr, iv = [0], []
    for c in range(ncontigs):
        first = len(iv)
        for b, e in sorted((b, e) for cc, b, e in weak if cc == c and e > b):
            if len(iv) > first and b <= iv[-1][1]:
                iv[-1] = (iv[-1][0], max(iv[-1][1], e))
            else:
                iv.append((b, e))
        ptr.append(len(iv))
    return np.asarray(ptr, dtype=np.int64), np.asarray(iv, dtype=np.int32).reshape(-1, 2)


def _pack(case, reports, weak, spans, pairs):
    rep = np.zeros(len(reports), dtype=REPORT_DTYPE)
    for r, row in enumerate(reports):
        rep[r] = row
    off = np.concatenate([[0], np.cumsum([len(s) for s in spans])]).astype(np.int64)
    ids = np.asarray([x for s in spans for x in s], dtype=np.int32)
    return dict(reports=rep, weak=np.asarray(weak, dtype=np.int32).reshape(-1, 3), span_off=off, span_ids=ids,
                mask=merged_mask(weak, len(case["contig_off"]) - 1), pairs=pairs)


def validate(case):
    """the literal restatement, region by region"""
    if id(case) in _cache:
        return _cache[id(case)][1]
    las, lens = case["las"], np.diff(case["contig_off"])
    reports, weak, spans, pairs = [], [], [], 0
    for c, b, e in case["regions"]:
        mine = las[las["aread"] == c]
        al = [(int(x), int(y)) for x, y in zip(mine["abpos"], mine["aepos"])]
        sp, wk, ok, (cb, ce) = mc.validate_region(al, (b, e), int(lens[c]), case["context"], case["window"], case["min_cov"], case["min_span"])
        if ce - cb <= 0:  # no window is considered (the contract; the literal loop would test one of no bases)
            wk, ok = [], sp >= case["min_span"]
        ids = [int(rd) for x, y, rd in zip(mine["abpos"], mine["aepos"], mine["bread"]) if x < cb and ce < y]
        assert len(ids) == sp
        pairs += sum(1 for x, y in al if x < ce and cb < y)
        reports.append((sp, sum(y - x for x, y in wk), int(ok), cb, ce))
        weak += [(c, x, y) for x, y in wk]
        spans.append(ids)
    out = _pack(case, reports, weak, spans, pairs)
    _cache[id(case)] = (case, out)
    return out


def from_host(case):
    """the same from the host function dh_validate_regions, which tests/test_maskcov.py pins to the literal loop; the spanning
    ids and the pairs by their definition"""
    if ("host", id(case)) in _cache:
        return _cache[("host", id(case))][1]
    las, lens = case["las"], np.diff(case["contig_off"])
    rep, weak = dentist_amd.validate_regions(las, case["contig_off"], case["regions"], case["min_cov"], min_spanning_reads=case["min_span"],
                                             region_context=case["context"], weak_coverage_window=case["window"])
    spans, pairs = [], 0
    for r, (c, b, e) in enumerate(case["regions"]):
        cb, ce = extended((c, b, e), int(lens[c]), case["context"])
        assert (cb, ce) == (rep[r]["ctx_begin"], rep[r]["ctx_end"])
        on = las["aread"] == c
        spans.append(las["bread"][on & (las["abpos"] < cb) & (ce < las["aepos"])].tolist())
        pairs += int(np.count_nonzero(on & (las["abpos"] < ce) & (cb < las["aepos"])))
    out = _pack(case, [tuple(int(x) for x in row) for row in rep.tolist()], [tuple(x) for x in weak.tolist()], spans, pairs)
    _cache[("host", id(case))] = (case, out)
    return out


def same(got, exp):
    """got: a ValidatedRegions or a dict of the same fields; every array equal, dtypes included"""
    g = got if isinstance(got, dict) else dict(reports=got.reports, weak=got.weak, span_off=got.span_off, span_ids=got.span_ids, mask=got.mask)
    for k in ("reports", "weak", "span_off", "span_ids"):
        if g[k].dtype != exp[k].dtype or g[k].shape != exp[k].shape or not np.array_equal(g[k], exp[k]):
            return False
    return all(g["mask"][k].dtype == exp["mask"][k].dtype and g["mask"][k].shape == exp["mask"][k].shape
               and np.array_equal(g["mask"][k], exp["mask"][k]) for k in (0, 1))


def json_lines(case, exp, report_all, first_contig=0, first_read=0):
    """the lines tools/validate-regions prints: ids 1-based"""
    out = []
    for r, (c, b, e) in enumerate(case["regions"]):
        rep = exp["reports"][r]
        if rep["is_valid"] and not report_all:
            continue
        ids = exp["span_ids"][exp["span_off"][r]:exp["span_off"][r + 1]]
        out.append(json.dumps({"region": {"contigId": c + first_contig + 1, "begin": b, "end": e},
                               "regionWithContext": {"contigId": c + first_contig + 1, "begin": int(rep["ctx_begin"]), "end": int(rep["ctx_end"])},
                               "isValid": bool(rep["is_valid"]), "numSpanningReads": int(rep["num_spanning_reads"]),
                               "spanningReadIds": [int(x) + first_read + 1 for x in ids], "weakCoverageMaskBps": int(rep["weak_bp"])},
                              separators=(",", ":")))
    return out
