"""dh_output_db's plan against the host writer: on every case of tests/outfmt_cases.py the plain-Python restatement of plan ->
bytes (tests/outfmt_ref.py) equals the FASTA dentist_amd.output_assembly writes, and the cases hold the shapes they are there
for.  No GPU needed."""
import numpy as np
import pytest

import outfmt_cases as oc
import outfmt_ref as orf


@pytest.fixture(scope="module")
def plans():
    return {name: oc.plan_of(c) for name, c in oc.ALL.items()}


@pytest.mark.parametrize("name", list(oc.ALL))
def test_restatement_equals_the_host_writer(tmp_path, plans, name):
    c = oc.ALL[name]
    fa = str(tmp_path / "host.fasta")
    oc.host_fasta(c, fa)
    want = open(fa, "rb").read()
    got = orf.plan_bytes(plans[name], np.concatenate(c["contigs"]), c["bases"])
    assert got == want
    assert int(plans[name]["rec_off"][-1]) == len(want)


def bodies(p):
    """bases of every record's body"""
    return [int(p["seg_base"][p["seg_first"][r + 1]] - p["seg_base"][p["seg_first"][r]]) for r in range(len(p["hdr_off"]) - 1)]


def test_the_cases_hold_their_shapes(plans):
    seg_len = {n: np.diff(p["seg_base"]) for n, p in plans.items()}
    assert sorted({p["width"] for p in plans.values()}) == [0, 1, 3, 7, 50]
    for w in oc.WIDTHS:
        b = bodies(plans[f"basic_w{w}"])
        assert 1 in b                                          # a body of one base
        if w > 0:
            assert any(x > 0 and x % w == 0 for x in b)        # a body that ends on a full line
            assert w == 1 or any(x % w != 0 for x in b)
        fl, ln = plans[f"basic_w{w}"]["seg_flags"], seg_len[f"basic_w{w}"]
        assert any((f & 3) == orf.NRUN and n == 1 for f, n in zip(fl, ln))                    # an n run of one base
        assert any((f & 3) == orf.CONS and f & orf.REV and f & orf.UPPER for f in fl)         # a complemented insertion
    assert not any(f & orf.UPPER for f in plans["nohighlight"]["seg_flags"])
    assert 0 in bodies(plans["extensions"])                    # an empty body
    assert sum((f & 3) == orf.CONS for f in plans["extensions"]["seg_flags"]) == 2            # a front and a back extension
    p = plans["reversed_start"]
    assert (p["seg_flags"][0] & 3) == orf.CONTIG and p["seg_flags"][0] & orf.REV              # the scaffold starts at a contig END
    assert any((f & 3) == orf.CONTIG and n == 1 for f, n in zip(p["seg_flags"], seg_len["reversed_start"]))  # a slice of one base
    assert b"\tisCyclic\n" in bytes(plans["cyclic"]["hdr"])
    p = plans["many_small"]
    assert len(p["hdr_off"]) - 1 == 301 and int(p["hdr_off"][1]) > 64 and max(bodies(p)[1:]) <= 5
    assert int(seg_len["big"].max()) >= 69000
    assert any(int(p["rec_off"][-1]) % 16 for p in plans.values())
    assert any(oc.chunk_at_record_boundary(p) for p in plans.values())
