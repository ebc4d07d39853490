"""The contract of dh_check_gaps restated line by line from commands/checkResults.d of the reference: analyzeGaps :822-907,
getGapState / isGap* :909-982, getInsertionMapping :984-1009, mappedIntervalOf :1011-1022, inputGapSize :1037-1046,
computeInsertionAlignment :1270-1291, resultSubseqString :1355-1385, addDustAnalysis :1387-1462,
StretcherAlignment.cropReference :1986-2011 and the early return of stretcher :2081-2089.  Plain Python, loops over the alignment
columns as the D code has them.  The alignment itself is dh_nw_affine_batch's contract: its ops, and whether the band policy gives
a pair up, come from tests/nwa_ref.py.  Not a test module.

Sequences are lists of base-code arrays (0..3).  A mapping is a dict with the fields of ContigMapping: ref_contig (result contig,
1-based), ref_begin, ref_end, ref_contig_length, query_contig (input contig, 1-based), duplicate, complement.  `mapped` is a list of
(true contig, begin, end); `dust` a dict true contig -> sorted list of (begin, end), or None.

getFastaLength, read literally (util/fasta.d:354-395): the FASTA files hold a header line and one sequence line, so the length is
that of the whole sequence, and 0 for an empty one.  At the early return the alignment has these two lengths, no lines and a NaN
identity.  computeInsertionAlignment then crops when crop > 0: cropReference on empty lines gives countUntil = -1 twice, the slice
[0, 0), both lengths counted again as 0 and 0 / 0 = NaN.  So: crop 0 -> (R, Q), crop > 0 -> (0, 0); the identity is NaN in both."""
import math

import numpy as np

import nwa_ref

UNKOWN, BROKEN, UNCLOSED, PARTIALLY_CLOSED, CLOSED, IGNORED = range(6)
STATE_NAMES = ["unkown", "broken", "unclosed", "partiallyClosed", "closed", "ignored"]
NONE, OK, EMPTY, BAND_EXCEEDED, TOO_LONG = range(5)
MAX_LEN, MAX_BAND = 65536, 2048
CHARS = "acgtn"
FIELDS = ["state", "gap_length", "lhs_map", "rhs_map", "align_status", "complement", "true_contig", "true_begin", "true_end",
          "result_begin_contig", "result_begin", "result_end_contig", "result_end", "col_begin", "col_end", "reference_length",
          "query_length", "matches", "dust_ops", "dust_matches", "none_dust_ops", "none_dust_matches"]


def is_base(c):
    return c in "acgtACGT"


def revcomp(codes):
    """--sreverse2: n stays n"""
    c = np.asarray(codes, dtype=np.uint8)[::-1]
    return np.where(c < 4, 3 - c, c).astype(np.uint8)


def lines_of(ref, qry, ops):
    """the three lines of the `pair` text, lower case, '-' for a gap and for an indel op"""
    rl, eo, ql = [], [], []
    i = j = 0
    for op in ops:
        op = int(op)
        if op == 2:
            rl.append("-")
        else:
            rl.append(CHARS[min(int(ref[i]), 4)])
            i += 1
        if op == 1:
            ql.append("-")
        else:
            ql.append(CHARS[min(int(qry[j]), 4)])
            j += 1
        eo.append("|" if op == 0 else ("." if op == 3 else "-"))
    assert i == len(ref) and j == len(qry)
    return "".join(rl), "".join(eo), "".join(ql)


def count_until(seq, crop):
    """cumulativeFold!((n, c) => n + isBase(c))(0).countUntil(crop)"""
    n = 0
    for k, c in enumerate(seq):
        n += is_base(c)
        if n == crop:
            return k
    return -1


def crop_reference(al, crop):
    """StretcherAlignment.cropReference (:1986-2011); the complement is not carried over, as there"""
    ref_line = al["referenceLine"]
    gap_begin = count_until(ref_line, crop) + 1
    gap_end = len(ref_line) - count_until(ref_line[::-1], crop) - 1
    out = {"complement": False, "gapBegin": gap_begin, "gapEnd": gap_end}
    for k in ("referenceLine", "editOps", "queryLine"):
        out[k] = al[k][gap_begin:gap_end]
    out["referenceLength"] = sum(1 for c in out["referenceLine"] if is_base(c))
    out["queryLength"] = sum(1 for c in out["queryLine"] if is_base(c))
    n = len(out["editOps"])
    out["matches"] = out["editOps"].count("|")
    out["percentIdentity"] = out["matches"] / n if n else math.nan
    return out


def stretcher(ref, qry, complement, scoring):
    """stretcher (:2060-2111) with dh_nw_affine_batch in EMBOSS's place; `status` says what became of the attempt"""
    al = {"referenceLength": len(ref), "queryLength": len(qry), "complement": bool(complement), "percentIdentity": math.nan,
          "referenceLine": "", "editOps": "", "queryLine": "", "gapBegin": 0, "gapEnd": 0, "matches": 0, "status": EMPTY, "ops": None}
    if len(ref) == 0 or len(qry) == 0 or all(int(b) >= 4 for b in qry):
        return al
    if len(ref) > MAX_LEN or len(qry) > MAX_LEN:
        al["status"] = TOO_LONG
        return al
    q = revcomp(qry) if complement else np.asarray(qry, dtype=np.uint8)
    _, cost, ops = nwa_ref.align(ref, q, scoring)
    if nwa_ref.expected_attempts(len(ref), len(q), cost, nwa_ref.costs(scoring)[1], MAX_BAND)[0] != 0:
        al["status"] = BAND_EXCEEDED
        return al
    al["status"], al["ops"] = OK, ops
    al["referenceLine"], al["editOps"], al["queryLine"] = lines_of(ref, q, ops)
    n = len(ops)
    al["matches"] = al["editOps"].count("|")
    al["percentIdentity"] = al["matches"] / n if n else math.nan
    al["gapEnd"] = n
    return al


class Analyzer:
    def __init__(self, true_seqs, result_seqs, mapped, maps, result_gap, dust, crop, scoring=nwa_ref.DEFAULT):
        self.true_seqs, self.result_seqs, self.mapped, self.result_gap = true_seqs, result_seqs, mapped, result_gap
        self.dust, self.crop, self.scoring = dust, crop, scoring
        self.maps = [dict(m, index=k) for k, m in enumerate(maps)]

    def mapped_interval_of(self, contig):
        if contig > len(self.mapped):
            return (0, 0, 0)
        return tuple(self.mapped[contig - 1])

    def is_gap(self, lhs, rhs):
        lc = self.mapped_interval_of(lhs)[0]
        return lc > 0 and lc == self.mapped_interval_of(rhs)[0]

    def result_gap_size(self, contig):
        return self.result_gap[contig - 1]

    def is_gap_closed(self, lhs, rhs, no_swap=False):
        if not no_swap and lhs["complement"]:
            return self.is_gap_closed(rhs, lhs, True)
        return lhs["ref_contig"] == rhs["ref_contig"] and lhs["complement"] == rhs["complement"] and lhs["ref_end"] <= rhs["ref_begin"]

    def is_gap_partially_closed(self, lhs, rhs, no_swap=False):
        if not no_swap and lhs["complement"]:
            return self.is_gap_partially_closed(rhs, lhs, True)
        return (lhs["ref_contig"] + 1 == rhs["ref_contig"] and lhs["complement"] == rhs["complement"] and
                (lhs["ref_end"] + self.crop < lhs["ref_contig_length"] or self.crop < rhs["ref_begin"]) and
                self.result_gap_size(lhs["ref_contig"]) > 0)

    def is_gap_unclosed(self, lhs, rhs, no_swap=False):
        if not no_swap and lhs["complement"]:
            return self.is_gap_unclosed(rhs, lhs, True)
        return (lhs["ref_contig"] + 1 == rhs["ref_contig"] and lhs["complement"] == rhs["complement"] and
                lhs["ref_end"] + self.crop == lhs["ref_contig_length"] and self.crop == rhs["ref_begin"] and
                self.result_gap_size(lhs["ref_contig"]) > 0)

    def gap_state(self, lhs, rhs):
        if not self.is_gap(lhs["query_contig"], rhs["query_contig"]):
            return IGNORED
        if self.is_gap_closed(lhs, rhs):
            return CLOSED
        if self.is_gap_partially_closed(lhs, rhs):
            return PARTIALLY_CLOSED
        if self.is_gap_unclosed(lhs, rhs):
            return UNCLOSED
        return BROKEN

    def insertion_mapping(self, lhs, rhs):
        lm, rm = self.mapped_interval_of(lhs["query_contig"]), self.mapped_interval_of(rhs["query_contig"])
        begin_of, end_of = (rhs if lhs["complement"] else lhs), (lhs if lhs["complement"] else rhs)
        return {"true": (lm[0], lm[2] - self.crop, rm[1] + self.crop), "begin": (begin_of["ref_contig"], begin_of["ref_end"]),
                "end": (end_of["ref_contig"], end_of["ref_begin"]), "complement": bool(lhs["complement"])}

    def result_subseq(self, begin, end):
        if begin[0] == end[0]:
            return np.asarray(self.result_seqs[begin[0] - 1][begin[1]:end[1]], dtype=np.uint8)
        left = self.result_seqs[begin[0] - 1][begin[1]:]
        right = self.result_seqs[end[0] - 1][:end[1]]
        return np.concatenate([left, np.full(self.result_gap_size(begin[0]), 4, np.uint8), right]).astype(np.uint8)

    def insertion_alignment(self, im):
        t = im["true"]
        true_seq = np.asarray(self.true_seqs[t[0] - 1][t[1]:t[2]], dtype=np.uint8)
        al = stretcher(true_seq, self.result_subseq(im["begin"], im["end"]), im["complement"], self.scoring)
        if self.crop > 0:
            status, ops = al["status"], al["ops"]
            al = crop_reference(al, self.crop)
            al["status"], al["ops"] = status, ops
        return al

    def dust_analysis(self, s, lhs_contig, al):
        lm, rm = self.mapped_interval_of(lhs_contig), self.mapped_interval_of(lhs_contig + 1)
        lo, hi = lm[2], rm[1]
        gap_dust = [(max(b, lo), min(e, hi)) for b, e in self.dust.get(lm[0], []) if max(b, lo) < min(e, hi)]
        inside = lambda p: any(b <= p < e for b, e in gap_dust)
        ref_pos = lo
        for ref_char, op, _ in zip(al["referenceLine"], al["editOps"], al["queryLine"]):
            if inside(ref_pos) or (ref_char == "-" and (inside(ref_pos - 1) or inside(ref_pos + 1))):
                if op == "|":
                    s["dust_matches"] += 1
                s["dust_ops"] += 1
            else:
                if op == "|":
                    s["none_dust_matches"] += 1
                s["none_dust_ops"] += 1
            if op in "|." or is_base(ref_char):
                ref_pos += 1

    def analyze(self, first_contig, count):
        """(summaries as dicts of FIELDS plus `identity`, ops per gap or None)"""
        out, all_ops = [], []
        for i in range(count):
            lhs, rhs = first_contig + i, first_contig + i + 1
            s = dict.fromkeys(FIELDS, 0)
            s["lhs_map"] = s["rhs_map"] = -1
            s["identity"] = math.nan
            out.append(s)
            all_ops.append(None)
            if not self.is_gap(lhs, rhs):
                s["state"] = IGNORED
                continue
            s["gap_length"] = self.mapped_interval_of(rhs)[1] - self.mapped_interval_of(lhs)[2]
            la = [m for m in self.maps if m["query_contig"] == lhs and not m["duplicate"]]
            ra = [m for m in self.maps if m["query_contig"] == rhs and not m["duplicate"]]
            if len(la) != 1 or len(ra) != 1:
                s["state"] = UNKOWN
                continue
            s["lhs_map"], s["rhs_map"] = la[0]["index"], ra[0]["index"]
            s["state"] = self.gap_state(la[0], ra[0])
            if s["state"] in (PARTIALLY_CLOSED, CLOSED):
                im = self.insertion_mapping(la[0], ra[0])
                al = self.insertion_alignment(im)
                s["align_status"], s["complement"] = al["status"], int(im["complement"])
                s["true_contig"], s["true_begin"], s["true_end"] = im["true"]
                s["result_begin_contig"], s["result_begin"] = im["begin"]
                s["result_end_contig"], s["result_end"] = im["end"]
                s["col_begin"], s["col_end"] = al["gapBegin"], al["gapEnd"]
                s["reference_length"], s["query_length"], s["matches"] = al["referenceLength"], al["queryLength"], al["matches"]
                s["identity"] = al["percentIdentity"]
                all_ops[-1] = al["ops"]
                if self.dust is not None and s["state"] == CLOSED:
                    self.dust_analysis(s, lhs, al)
        return out, all_ops
