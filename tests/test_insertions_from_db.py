"""dh_insertions_from_db: insertions.db files written by hand (dentist_amd.insertiondb_write) against a Python restatement of
what `dentist output` reads from them -- getCroppingPosition!"contigA" / !"contigB" and getInfoForNewSequenceInsertion
(common/insertions.d:110-140, 228-284), the join of makeJoin (base.d:2680-2722) -- and every refused file with its message.
No GPU needed."""
import numpy as np
import pytest

import dentist_amd

PRE, BEGIN, END, POST = 0, 1, 2, 3
FRONT, BACK = 0, 1
LENS = [1000, 800, 600]
OFF = np.cumsum([0] + LENS).astype(np.int64)


def ov(contig, seed, comp, las, blen, alen=None):
    """an overlap: contig 1-based, las = (a_begin, a_end, b_begin, b_end, diffs) in chain order"""
    return dict(contig=contig, seed=seed, comp=comp, las=las, blen=blen, alen=LENS[contig - 1] if alen is None else alen)


def write(path, insertions):
    ins, sa, la, bases, ids = [], [], [], [], []
    rng = np.random.default_rng(1)
    for x in insertions:
        q = np.zeros(1, dentist_amd.INSERTION_REC_DTYPE)[0]
        (q["start_contig"], q["start_part"]), (q["end_contig"], q["end_part"]) = x["start"], x["end"]
        q["seq_len"], q["noverlaps"], q["nread_ids"] = x["seq_len"], len(x["overlaps"]), len(x["ids"])
        ins.append(q)
        bases.append(rng.integers(0, 4, x["seq_len"]).astype(np.uint8))
        ids += x["ids"]
        for o in x["overlaps"]:
            s = np.zeros(1, dentist_amd.SEEDED_DTYPE)[0]
            s["id"], s["contig_a_id"], s["contig_a_len"], s["contig_b_id"], s["contig_b_len"] = len(sa), o["contig"], o["alen"], 1, o["blen"]
            s["flags"], s["seed"], s["tspace"], s["nla"] = o["comp"], o["seed"], 100, len(o["las"])
            sa.append(s)
            for t in o["las"]:
                a = np.zeros(1, dentist_amd.CHAIN_LA_DTYPE)[0]
                a["a_begin"], a["a_end"], a["b_begin"], a["b_end"], a["diffs"] = t
                la.append(a)
    dentist_amd.insertiondb_write(path, np.asarray(ins, dentist_amd.INSERTION_REC_DTYPE), np.concatenate(bases), np.asarray(ids, np.uint32),
                                  np.asarray(sa, dentist_amd.SEEDED_DTYPE), np.asarray(la, dentist_amd.CHAIN_LA_DTYPE), np.zeros(0, np.uint16))
    return np.concatenate(bases)


# ---- the reference's rules, restated
def crop_a(o):   # insertions.d:110-119
    return o["las"][0][0] if o["seed"] == FRONT else o["las"][-1][1]


def crop_b(o):   # insertions.d:122-140
    coord = o["las"][0][2] if o["seed"] == FRONT else o["las"][-1][3]
    return o["blen"] - coord if o["comp"] else coord


def sequence_slice(x):   # insertions.d:244-271: the slice on the stored sequence
    ovs = x["overlaps"]
    b, e = 0, x["seq_len"]
    if len(ovs) == 1:
        # the part that EXTENDS the contig.  For a complement overlap the reference's letter (:253-263) selects the aligned part
        # instead; the writers of this project document that difference (dh_output.cpp, "Two differences from the reference's
        # letter") and dh_process_pileups makes its records the same way, so the file route has to agree with it.
        if (ovs[0]["seed"] == FRONT) != bool(ovs[0]["comp"]):
            e = crop_b(ovs[0])
        else:
            b = crop_b(ovs[0])
    else:
        b, e = crop_b(ovs[0]), crop_b(ovs[1])
        if e < b:
            b, e = e, b
    return b, e


def expected(x):
    """the record's fields: flank 0 is the node with the smaller contig id (the start node of the stored edge)"""
    (c0, p0), (c1, p1) = x["start"], x["end"]
    by_contig = {(o["contig"], o["seed"]): o for o in x["overlaps"]}
    if c0 == c1:   # extension: (pre, begin) front, (end, post) back
        front = p0 == PRE
        o0 = x["overlaps"][0]
        join, right, right_pos = 4 | (1 if front else 0), -1, -1
    else:
        o0 = by_contig[(c0, FRONT if p0 == BEGIN else BACK)]
        o1 = by_contig[(c1, FRONT if p1 == BEGIN else BACK)]
        join, right, right_pos = (1 if p0 == BEGIN else 0) | (2 if p1 == END else 0), c1 - 1, crop_a(o1)
    return dict(contig_left=c0 - 1, contig_right=right, join=join, left_aepos=crop_a(o0), right_abpos=right_pos, comp=o0["comp"],
                slice=sequence_slice(x), cons_len=x["seq_len"], left_diffs=sum(t[4] for t in o0["las"]),
                right_diffs=sum(t[4] for t in o1["las"]) if c0 != c1 else 0)


CASES = {
    # (contig 1, end) -> (contig 2, begin): the back of contig 1, the front of contig 2
    "plain_gap": dict(start=(1, END), end=(2, BEGIN), seq_len=300, ids=[4, 9, 17],
                      overlaps=[ov(1, BACK, 0, [(700, 960, 0, 250, 7)], 300), ov(2, FRONT, 0, [(30, 90, 240, 300, 3)], 300)]),
    # both BEGINs: seeds equal, so one of the overlaps is a complement one
    "antiparallel_begins": dict(start=(1, BEGIN), end=(2, BEGIN), seq_len=300, ids=[2],
                                overlaps=[ov(1, FRONT, 1, [(40, 200, 150, 300, 5)], 300), ov(2, FRONT, 0, [(25, 180, 140, 300, 6)], 300)]),
    "antiparallel_ends": dict(start=(2, END), end=(3, END), seq_len=200, ids=[5, 6],
                              overlaps=[ov(2, BACK, 0, [(600, 790, 0, 60, 2)], 200), ov(3, BACK, 1, [(400, 590, 0, 50, 1)], 200)]),
    # a plain gap seen from a read of the other strand: both overlaps complement
    "complement_gap": dict(start=(1, END), end=(2, BEGIN), seq_len=300, ids=[8],
                           overlaps=[ov(1, BACK, 1, [(700, 950, 0, 230, 4)], 300), ov(2, FRONT, 1, [(20, 90, 250, 300, 2)], 300)]),
    "front_extension": dict(start=(2, PRE), end=(2, BEGIN), seq_len=400, ids=[3, 12],
                            overlaps=[ov(2, FRONT, 0, [(10, 120, 290, 400, 9)], 400)]),
    "back_extension": dict(start=(3, END), end=(3, POST), seq_len=400, ids=[1],
                           overlaps=[ov(3, BACK, 1, [(480, 595, 0, 110, 4)], 400)]),
    # the overlaps are chains of two local alignments: the first one's begin and the last one's end differ from the other's
    "chained_overlaps": dict(start=(1, END), end=(2, BEGIN), seq_len=500, ids=[7, 30],
                             overlaps=[ov(1, BACK, 0, [(500, 700, 0, 190, 11), (720, 970, 205, 460, 13)], 500),
                                       ov(2, FRONT, 0, [(15, 60, 420, 466, 2), (75, 130, 470, 500, 3)], 500)]),
}


def check(rec, x):
    e = expected(x)
    for f in ("contig_left", "contig_right", "join", "left_aepos", "right_abpos", "comp", "cons_len", "left_diffs", "right_diffs"):
        assert int(rec[f]) == e[f], (f, int(rec[f]), e[f])
    # the writers take the slice in the frame of `comp` (dh_output.cpp: sb = comp ? cons_len - ins_end : ins_begin)
    clen, b, en = int(rec["cons_len"]), int(rec["ins_begin"]), int(rec["ins_end"])
    assert ((clen - en, clen - b) if rec["comp"] else (b, en)) == e["slice"]
    assert int(rec["status"]) == 0


@pytest.mark.parametrize("name", list(CASES))
def test_one_insertion(tmp_path, name):
    x = CASES[name]
    path = str(tmp_path / "insertions.db")
    bases = write(path, [x])
    rec, got_bases, (ids, ids_off) = dentist_amd.insertions_from_db(path, OFF)
    assert len(rec) == 1 and rec.dtype == dentist_amd.INSERTION_DTYPE
    check(rec[0], x)
    assert np.array_equal(got_bases, bases) and got_bases.dtype == np.uint8 and int(rec[0]["cons_off"]) == 0
    assert ids.tolist() == [i - 1 for i in x["ids"]] and ids_off.tolist() == [0, len(x["ids"])]


def test_the_first_and_the_last_of_a_chain_are_not_the_same():
    x = CASES["chained_overlaps"]
    e = expected(x)
    assert e["left_aepos"] == 970 and e["right_abpos"] == 15 and e["slice"] == (460, 420)[::-1] and e["left_diffs"] == 24


def test_a_file_of_all_cases_keeps_order_offsets_and_ids(tmp_path):
    xs = list(CASES.values())
    path = str(tmp_path / "insertions.db")
    bases = write(path, xs)
    rec, got_bases, (ids, ids_off) = dentist_amd.insertions_from_db(path, OFF)
    assert len(rec) == len(xs) and np.array_equal(got_bases, bases)
    at = 0
    for r, x in zip(rec, xs):
        check(r, x)
        assert int(r["cons_off"]) == at
        at += x["seq_len"]
    assert ids_off.tolist() == np.cumsum([0] + [len(x["ids"]) for x in xs]).tolist()
    assert ids.tolist() == [i - 1 for x in xs for i in x["ids"]]


def refused(base, **change):
    x = dict(base)
    x.update(change)
    return x


G = CASES["plain_gap"]
REFUSED = {
    "contig id outside [1, 3]": refused(G, end=(4, BEGIN)),
    "contig_a_len 801 contradicts the length of contig 2": refused(G, overlaps=[G["overlaps"][0], ov(2, FRONT, 0, [(30, 90, 240, 300, 3)], 300, alen=801)]),
    "more than two overlaps": refused(G, overlaps=G["overlaps"] + [G["overlaps"][1]]),
    "neither a gap join nor an extension": refused(G, start=(1, PRE), end=(2, BEGIN)),
    "contig_b_len 299 differs from the sequence length 300": refused(G, overlaps=[G["overlaps"][0], ov(2, FRONT, 0, [(30, 90, 240, 299, 3)], 299)]),
}


@pytest.mark.parametrize("message", list(REFUSED))
def test_refused_files_name_the_insertion(tmp_path, message):
    path = str(tmp_path / "bad.db")
    write(path, [CASES["front_extension"], REFUSED[message]])
    with pytest.raises(dentist_amd.DhError) as ei:
        dentist_amd.insertions_from_db(path, OFF)
    assert ei.value.code == -1 and message in str(ei.value) and "insertion 1 of" in str(ei.value)
