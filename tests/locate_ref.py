"""Brute-force restatement of the exact-match locator's contract (the reference's external/fm-index.cpp as `dentist
check-results` calls it, commands/checkResults.d:511-565): the oracle of dh_exact_locate and of tools/fm-index.

Sequences are strings.  Per record the occurrences of a query are found by repeated str.find(q, p + 1), so overlapping
occurrences are all found and a match never spans two records by construction."""

COMPLEMENT = {"a": "t", "c": "g", "g": "c", "t": "a", "A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(q):
    return "".join(COMPLEMENT[c] for c in reversed(q))


def as_text(seq):
    """a base-code array (0..3) as a lower-case string; strings pass through"""
    return seq if isinstance(seq, str) else "".join("acgt"[int(c)] for c in seq)


def occurrences(record, q):
    out = []
    p = record.find(q)
    while p >= 0:
        out.append(p)
        p = record.find(q, p + 1)
    return out


def locate(refs, queries, both_strands=True):
    """hits as tuples (query, ref, begin, end, complement) in the order of the contract: per query (an empty one has no
    hits) the forward occurrences ascending by (ref, begin), then those of the reverse complement"""
    refs = [as_text(r) for r in refs]
    hits = []
    for qi, q in enumerate(queries):
        q = as_text(q)
        if not q:
            continue
        for comp, pat in ((0, q), (1, revcomp(q))) if both_strands else ((0, q),):
            for ri, rec in enumerate(refs):
                hits += [(qi, ri, p, p + len(pat), comp) for p in occurrences(rec, pat)]
    return hits


def records_of(reference_text):
    """the records of a reference file: one per line, empty lines count, a last line without a newline is a record"""
    lines = reference_text.split("\n")
    if lines[-1] == "":
        lines.pop()
    return lines


def tool_output(reference_text, sources, reverse):
    """stdout of `fm-index [-r] <reference> [<queries>...]`: sources is a list of (name, text) -- the queries files as given
    on the command line, or [("stdin", text)].  Empty query lines are skipped and do not advance the 0-based query id, which
    restarts for every source."""
    refs = records_of(reference_text)
    out = []
    for name, text in sources:
        queries = [q for q in text.split("\n") if q]
        for qi, ri, b, e, comp in locate(refs, queries, reverse):
            out.append(f"{name}\t{ri}\t{len(refs[ri])}\t{qi}\t{b}\t{e}\t{'yes' if comp else 'no'}\n")
    return "".join(out)
