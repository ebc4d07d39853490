"""The contract of dh_output_db's FASTA formatter restated in plain Python: a plan (the layout csrc/dh_outfmt.h states, as
dentist_amd.output_plan returns it) -> the bytes of the file.  Written record by record and segment by segment, with none of
the lane code's position arithmetic: the lanes (tests/native/outfmt_host.cpp) and the kernel are compared with this, and this
with the host writer (tests/test_outfmt_ref.py)."""

KIND, REV, UPPER = 3, 4, 8
CONTIG, NRUN, CONS = 0, 1, 2
LOWER_OF = bytes.maketrans(bytes(range(5)), b"acgtn")
UPPER_OF = bytes.maketrans(bytes(range(5)), b"ACGTN")


def segment_text(flags, src, n, contig, cons):
    kind = flags & KIND
    if kind == NRUN:
        codes = bytes([4]) * n
    else:
        buf = contig if kind == CONTIG else cons
        if flags & REV:
            lo = src - (n - 1)
            assert lo >= 0 and src < len(buf), "segment outside its buffer"
            codes = bytes(3 - b if b < 4 else 4 for b in reversed(bytes(buf[lo:src + 1])))
        else:
            assert src >= 0 and src + n <= len(buf), "segment outside its buffer"
            codes = bytes(min(b, 4) for b in bytes(buf[src:src + n]))
    return codes.translate(UPPER_OF if flags & UPPER else LOWER_OF)


def wrap(body, width):
    """LineWriter's rules (dh_output.cpp): a newline behind every `width` bases, a final one unless the body ended on a full
    line, none at all for an empty body; width <= 0: one line and always its newline."""
    if width <= 0:
        return body + b"\n"
    out = b"".join(body[i:i + width] + b"\n" for i in range(0, len(body), width))
    return out


def plan_bytes(plan, contig, cons):
    out = []
    nrec = len(plan["hdr_off"]) - 1
    hdr = bytes(plan["hdr"])
    at = 0
    for r in range(nrec):
        assert int(plan["rec_off"][r]) == at, f"record {r}: offset"
        h = hdr[int(plan["hdr_off"][r]):int(plan["hdr_off"][r + 1])]
        body = b"".join(segment_text(int(plan["seg_flags"][s]), int(plan["seg_src"][s]),
                                     int(plan["seg_base"][s + 1] - plan["seg_base"][s]), contig, cons)
                        for s in range(int(plan["seg_first"][r]), int(plan["seg_first"][r + 1])))
        rec = h + wrap(body, plan["width"])
        out.append(rec)
        at += len(rec)
    assert int(plan["rec_off"][nrec]) == at if nrec else True
    return b"".join(out)
