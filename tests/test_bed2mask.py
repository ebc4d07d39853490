"""BED -> mask (dh_bed_to_mask, tools/bed2mask; source/dentist/commands/bed2mask.d:70-333) on a .dam with a scaffold of three
contigs and one of a single contig: the interval rules, the data comments, the refusals, the tool with its two track extras,
and the BED lines `output --closed-gaps-bed` writes (tests/test_output.py) as inputs.  Host only."""
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
from test_output import case as output_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bed2mask")
# scafA: contigs [0, 100), [120, 200), [230, 290) with runs of n between them; scafB: [0, 90)
LENS, GAPS = (100, 80, 60), (20, 30)
EINVAL = -1


def random_bases(rng, n):
    return "".join("acgt"[x] for x in rng.integers(0, 4, n))


@pytest.fixture(scope="module")
def dam(tmp_path_factory):
    d = tmp_path_factory.mktemp("bed2mask")
    rng = np.random.default_rng(7)
    a = random_bases(rng, LENS[0]) + "n" * GAPS[0] + random_bases(rng, LENS[1]) + "n" * GAPS[1] + random_bases(rng, LENS[2])
    path = str(d / "ref.dam")
    dentist_amd.dazz_create_dam(path, f">scafA\tsome more words\n{a}\n>scafB\n{random_bases(rng, 90)}\n")
    dentist_amd.dazz_split(path, cutoff=20)
    dz = dentist_amd.DazzDb(path)
    assert dz.n == 4 and dz.fpulse.tolist() == [0, 120, 230, 0]
    return d, path, dz


def intervals(m):
    """[(contig, begin, end, [contig ids], [read ids])] of a BedMask, in its order"""
    out = []
    for c in range(len(m.ptr) - 1):
        for j in range(m.ptr[c], m.ptr[c + 1]):
            out.append((c, int(m.iv[2 * j]), int(m.iv[2 * j + 1]), m.contig_ids[j].tolist(), m.read_ids[m.read_off[j]:m.read_off[j + 1]].tolist()))
    assert len(out) == len(m.read_off) - 1 == len(m.iv) // 2
    return out


RULES_BED = ("scafA\t10\t50\tcontigs-1-2|reads-4-8\n"          # inside one contig
             "\n"
             "scafA\t90\t130\tcontigs-3-4|reads-7\n"              # across a gap: two clipped intervals with the line's ids
             "scafA\t150\t200\tcontigs-5-6|reads\n"               # ends exactly at the contig's end; reads without ids
             "scafA\t200\t235\tcontigs-7-8|reads-1|reads-2-3\n"   # begins at a contig's end: nothing there; the last reads part wins
             "\n\n"
             "scafA\t240\t250\tcontigs-9-10|colour-red|reads-5\n"  # an unknown part is ignored
             "scafB\t0\t90\tcontigs-11-12|reads-6\textra column\n")
RULES = [(0, 10, 50, [1, 2], [4, 8]), (0, 90, 100, [3, 4], [7]), (1, 0, 10, [3, 4], [7]), (1, 30, 80, [5, 6], []),
         (2, 0, 5, [7, 8], [2, 3]), (2, 10, 20, [9, 10], [5]), (3, 0, 90, [11, 12], [6])]


def test_interval_rules_and_data_comments(dam):
    _, _, dz = dam
    m = dentist_amd.bed_to_mask(dz, RULES_BED, "in.bed", data_comments=True)
    assert m.ptr.tolist() == [0, 2, 4, 6, 7] and intervals(m) == RULES
    # without data comments: the same intervals, no ids, column 4 is not looked at
    m = dentist_amd.bed_to_mask(dz, RULES_BED.replace("contigs-1-2|reads-4-8", "contigs-x|reads-y|"), "in.bed")
    assert intervals(m) == [(c, b, e, [0, 0], []) for c, b, e, _, _ in RULES]
    # no text at all and a last line without its newline
    assert intervals(dentist_amd.bed_to_mask(dz, "", "in.bed", data_comments=True)) == []
    assert intervals(dentist_amd.bed_to_mask(dz, "\nscafB\t1\t2\tcontigs-1-2", "in.bed", data_comments=True)) == [(3, 1, 2, [1, 2], [])]


def test_half_open_ends_and_all_contigs(dam):
    _, _, dz = dam
    one = lambda line: intervals(dentist_amd.bed_to_mask(dz, line + "\tcontigs-1-2|reads-9\n", "in.bed", data_comments=True))  # noqa: E731
    ids = ([1, 2], [9])
    assert one("scafA\t230\t240") == [(2, 0, 10, *ids)]                      # begins exactly where the next contig begins
    assert one("scafA\t120\t230") == [(1, 0, 80, *ids)]                      # ends where the next contig begins: not on it
    assert one("scafA\t199\t231") == [(1, 79, 80, *ids), (2, 0, 1, *ids)]
    assert one("scafA\t0\t290") == [(0, 0, 100, *ids), (1, 0, 80, *ids), (2, 0, 60, *ids)]   # all three contigs
    assert one("scafA\t50\t100000") == [(0, 50, 100, *ids), (1, 0, 80, *ids), (2, 0, 60, *ids)]
    assert one("scafA\t105\t125") == [(1, 0, 5, *ids)]                       # begins inside the gap


def test_all_errors_of_a_data_comment_come_together(dam):
    _, _, dz = dam
    bed = "scafA\t10\t50\tcontigs-1-2\n\nscafA\t60\t70\tcontigs-1|contigs-1-2-3|contigs-a-2|reads-1-x\n"
    with pytest.raises(dentist_amd.DhError) as ei:
        dentist_amd.bed_to_mask(dz, bed, "gaps.bed", data_comments=True)
    assert ei.value.code == EINVAL
    assert str(ei.value).endswith("ill-formatted data comment in BED file gaps.bed:3:\n"
                                  "  - contigs must have exactly two entries\n"
                                  "  - contigs must have exactly two entries\n"
                                  "  - could not parse uint in contigs\n"
                                  "  - could not parse uint in reads")
    for comment, err in (("contigs-1-", "could not parse uint in contigs"), ("contigs-+1-2", "could not parse uint in contigs"),
                         ("contigs-1-2|reads- 3", "could not parse uint in reads"), ("contigs-1-2|reads-4294967296", "could not parse uint in reads"),
                         ("contigs", "contigs must have exactly two entries")):
        with pytest.raises(dentist_amd.DhError, match=r"gaps.bed:1:\n  - " + err):
            dentist_amd.bed_to_mask(dz, f"scafA\t10\t50\t{comment}\n", "gaps.bed", data_comments=True)
    m = dentist_amd.bed_to_mask(dz, "scafA\t10\t50\tcontigs-1-4294967295|reads-0\n", "gaps.bed", data_comments=True)
    assert intervals(m) == [(0, 10, 50, [1, 4294967295], [0])]


REFUSALS = [("nowhere\t1\t2\tcontigs-1-2", "unknown scaffold nowhere"),
            ("scafA\textra\t1\t2\tcontigs-1-2", "decimal numbers"),                  # (the key is the header up to its first tab)
            ("scafA\t1", "fewer than three columns"),
            ("scafA", "fewer than three columns"),
            ("scafA\tx\t2\tcontigs-1-2", "decimal numbers"),
            ("scafA\t1\t\tcontigs-1-2", "decimal numbers"),
            ("scafA\t1\t-2\tcontigs-1-2", "decimal numbers"),
            ("scafA\t1\t2147483648\tcontigs-1-2", "decimal numbers"),
            ("scafA\t5\t4\tcontigs-1-2", "begin > end"),
            ("scafA\t100\t120\tcontigs-1-2", "overlaps no contig"),                     # inside the run of n
            ("scafA\t290\t300\tcontigs-1-2", "overlaps no contig"),                     # behind the scaffold
            ("scafA\t10\t20", "no contigs part"),
            ("scafA\t10\t20\treads-1-2", "no contigs part")]


@pytest.mark.parametrize("line,message", REFUSALS)
def test_refusals_name_file_and_line(dam, line, message):
    _, _, dz = dam
    with pytest.raises(dentist_amd.DhError, match=r"BED file some/dir/in\.bed:3: .*" + message) as ei:
        dentist_amd.bed_to_mask(dz, "scafA\t1\t2\tcontigs-1-2\n\n" + line + "\n", "some/dir/in.bed", data_comments=True)
    assert ei.value.code == EINVAL


def test_intervals_must_ascend_in_file_order(dam):
    _, _, dz = dam
    for bed, line in (("scafB\t1\t2\nscafA\t1\t2\n", 2), ("scafA\t130\t140\n\nscafA\t10\t20\n", 3), ("scafA\t30\t40\nscafA\t10\t20\n", 2),
                      ("scafA\t0\t290\nscafA\t10\t20\n", 2)):
        with pytest.raises(dentist_amd.DhError, match=rf"in\.bed:{line}: .*must ascend") as ei:
            dentist_amd.bed_to_mask(dz, bed, "in.bed")
        assert ei.value.code == EINVAL
    assert len(intervals(dentist_amd.bed_to_mask(dz, "scafA\t10\t20\nscafA\t10\t20\nscafA\t10\t30\n", "in.bed"))) == 3


# ---------------------------------------------------------------------------------- the tool
def run(d, *args, stdin=None):
    return subprocess.run([TOOL, *args], cwd=d, input=stdin, capture_output=True, text=True, timeout=60)


def decode_reads(extra):
    out, at = [], 0
    while at < len(extra):
        out.append(extra[at + 1:at + 1 + extra[at]].tolist())
        at += 1 + int(extra[at])
    return out


def test_tool_writes_the_mask_and_both_extras(dam):
    d, path, dz = dam
    (d / "in.bed").write_text(RULES_BED)
    r = run(d, "--data-comments", "--bed=in.bed", "ref.dam", "closed-gaps")
    assert r.returncode == 0 and r.stdout == "" and r.stderr == "", r.stderr
    ptr, iv = dz.read_mask("closed-gaps")
    assert ptr.tolist() == [0, 2, 4, 6, 7] and iv.reshape(-1, 2).tolist() == [[b, e] for _, b, e, _, _ in RULES]
    contigs = dentist_amd.read_mask_extra(path, "closed-gaps", "contigs", np.int64)
    reads = dentist_amd.read_mask_extra(path, "closed-gaps", "reads", np.int64)
    assert contigs.accum == reads.accum == "exact"
    assert contigs.data.reshape(-1, 2).tolist() == [c for _, _, _, c, _ in RULES]
    assert reads.data.tolist() == [2, 4, 8, 1, 7, 1, 7, 0, 2, 2, 3, 1, 5, 1, 6] and decode_reads(reads.data) == [x for _, _, _, _, x in RULES]
    # `contigs` is written first
    anno = open(d / ".ref.closed-gaps.anno", "rb").read()
    assert anno.index(b"contigs") < anno.index(b"reads")
    # standard input gives the same files; the options every sub-command takes are reported once
    r = run(d, "--data-comments", "--config=dentist.json", "-v", "-T4", "ref.dam", "from-stdin", stdin=RULES_BED)
    assert r.returncode == 0 and r.stderr == "bed2mask: --config, -v, --quiet, -T and --threads have no effect here\n"
    for ext in ("anno", "data"):
        assert open(d / f".ref.from-stdin.{ext}", "rb").read() == open(d / f".ref.closed-gaps.{ext}", "rb").read()


def test_tool_without_data_comments_writes_no_extras(dam):
    d, path, dz = dam
    r = run(d, "ref.dam", "plain", stdin="scafA\t10\t50\t\x01|contigs-|reads-x\nscafB\t0\t5\n")
    assert r.returncode == 0, r.stderr
    ptr, iv = dz.read_mask("plain")
    assert ptr.tolist() == [0, 1, 1, 1, 2] and iv.tolist() == [10, 50, 0, 5]
    assert os.path.getsize(d / ".ref.plain.anno") == 8 + 8 * 5
    assert dentist_amd.read_mask_extra(path, "plain", "contigs") is None and dentist_amd.read_mask_extra(path, "plain", "reads") is None


def test_tool_exit_codes(dam):
    d, _, _ = dam
    r = run(d, "--data-comment", "ref.dam", "m", stdin="")
    assert r.returncode == 1 and r.stderr.startswith("bed2mask: unknown or malformed option --data-comment\nusage: bed2mask")
    assert run(d, "ref.dam", stdin="").returncode == 1
    r = run(d, "--bed=absent.bed", "ref.dam", "m")
    assert r.returncode == 2 and r.stderr == "bed2mask: cannot open absent.bed\n"
    r = run(d, "absent.dam", "m", stdin="")
    assert r.returncode == 2 and "absent.dam" in r.stderr
    (d / "bad.bed").write_text("scafA\t1\t2\tcontigs-1-2\nscafA\t100\t120\tcontigs-1-2\n")
    r = run(d, "--data-comments", "--bed=bad.bed", "ref.dam", "m")
    assert r.returncode == 2 and r.stderr == "bed2mask: BED file bad.bed:2: the interval overlaps no contig of scafA\n"
    r = run(d, "--data-comments", "ref.dam", "m", stdin="scafA\t1\t2\tcontigs-1\n")
    assert r.returncode == 2 and r.stderr == "bed2mask: ill-formatted data comment in BED file -:1:\n  - contigs must have exactly two entries\n"
    assert not os.path.exists(d / ".ref.m.anno")    # nothing is written when the BED is refused


# ---------------------------------------------------------------------------------- producer and consumer
def closed_gaps_route(tmp_path, bed_line, **kw):
    """dh_output_assembly on the case of tests/test_output.py; its FASTA as a .dam, its BED through tools/bed2mask"""
    contigs, sof, hd, gl, rec, bases, ids, c, cons = output_case()
    if kw.pop("with_ids", True):
        kw["read_ids"] = ids
    fa, bed = str(tmp_path / "out.fasta"), str(tmp_path / "out.bed")
    dentist_amd.output_assembly(fa, contigs, sof, hd, gl, rec, bases, bed_path=bed, line_width=50, **kw)
    lines = open(bed).read().split("\n")
    assert bed_line in lines            # the literal line of tests/test_output.py
    path = str(tmp_path / "closed.dam")
    dentist_amd.dazz_create_dam(path, open(fa).read())
    dentist_amd.dazz_split(path, cutoff=20)
    r = run(tmp_path, "--data-comments", "--bed=out.bed", "closed.dam", "closed-gaps")
    assert r.returncode == 0, r.stderr
    dz = dentist_amd.DazzDb(path)
    ptr, iv = dz.read_mask("closed-gaps")
    k = lines.index(bed_line)
    pair = dentist_amd.read_mask_extra(path, "closed-gaps", "contigs").data.reshape(-1, 2)[k].tolist()
    reads = decode_reads(dentist_amd.read_mask_extra(path, "closed-gaps", "reads").data)[k]
    contig = int(np.searchsorted(ptr, k, side="right")) - 1
    return dz, contig, iv.reshape(-1, 2)[k].tolist(), pair, reads, c, cons


def test_the_bed_lines_of_output_as_inputs(tmp_path):
    for sub in ("a", "b", "c"):
        (tmp_path / sub).mkdir()
    # tests/test_output.py:42 -- the insertion and one base on either side of it, in the joined contig 1+2
    dz, contig, iv, pair, reads, c, cons = closed_gaps_route(tmp_path / "a", "scafA\t110\t143\tcontigs-1-2|reads-4-8-12", agp_dazzler=True)
    assert (contig, iv, pair, reads) == (0, [110, 143], [1, 2], [4, 8, 12])
    assert dz.n == 3 and sim.decode(dz.seq(0)[111:142]) == sim.decode(cons[0][10:42])[1:]
    # :67 -- join policy `scaffolds`: the second insertion lies behind the run of n that is left, on the second contig
    line = f"scafA\t{110 + 32 + 75 + 20 + 55}\t{110 + 32 + 75 + 20 + 55 + 26 + 1}\tcontigs-3-4|reads-3-10"
    dz, contig, iv, pair, reads, c, cons = closed_gaps_route(tmp_path / "b", line, join_policy="scaffolds")
    assert dz.n == 2 and dz.fpulse.tolist() == [0, 110 + 32 + 75 + 20]
    assert (contig, iv, pair, reads) == (1, [55, 55 + 26 + 1], [3, 4], [3, 10])
    # :78 -- without read ids the reference read stands alone
    dz, contig, iv, pair, reads, c, cons = closed_gaps_route(tmp_path / "c", "scafA\t110\t143\tcontigs-1-2|reads-8", with_ids=False)
    assert (contig, iv, pair, reads) == (0, [110, 143], [1, 2], [8])


# ---------------------------------------------------------------------------------- validate-regions and extras that do not fit
def test_validate_regions_refuses_extras_that_do_not_fit_the_mask(dam):
    """found after the mask is read and before a device is asked for, so this runs without one"""
    d, path, dz = dam
    dentist_amd.dazz_create_db(str(d / "reads.db"), ">sim/1/0_100 RQ=0.850\n" + random_bases(np.random.default_rng(1), 100) + "\n")
    dentist_amd.dazz_split(str(d / "reads.db"), cutoff=20)
    las = np.zeros(1, dtype=dentist_amd.LA_DTYPE)
    las[0]["aepos"], las[0]["bepos"], las[0]["tlen"] = 100, 100, 2
    dentist_amd.las_write(str(d / "one.las"), las, np.asarray([0, 100], np.uint16), 100)
    ptr, iv = np.asarray([0, 2, 2, 3, 3], np.int64), np.asarray([1, 5, 10, 20, 3, 4], np.int32)

    def refused(contigs, reads):
        dentist_amd.dazz_write_mask(path, "fit", ptr, iv)
        if contigs is not None:
            dentist_amd.write_mask_extra(path, "fit", "contigs", np.asarray(contigs, np.int64))
        if reads is not None:
            dentist_amd.write_mask_extra(path, "fit", "reads", np.asarray(reads, np.int64))
        r = subprocess.run([os.path.join(ROOT, "tools", "validate-regions"), "--min-coverage-reads=1", "ref.dam", "reads.db", "one.las", "fit"], cwd=d,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == ""
        return r.stderr
    assert "the extra `contigs` has 4 entries, not two for each of the 3 intervals" in refused([1, 2, 3, 4], None)
    assert "the extra `contigs` has 7 entries" in refused([1, 2, 3, 4, 5, 6, 7], [0, 0, 0])
    assert "the extra `reads` holds 2 lists, not one for each of the 3 intervals" in refused([1, 2, 3, 4, 5, 6], [1, 9, 0])
    assert "the extra `reads` holds 4 lists" in refused(None, [0, 0, 0, 0])
    assert "the extra `reads` ends inside a list of read ids" in refused([1, 2, 3, 4, 5, 6], [1, 9, 0, 2, 8])
    assert "the extra `reads` ends inside a list of read ids" in refused(None, [-1, 0, 0])
    dentist_amd.dazz_write_mask(path, "fit", ptr, iv)
    dentist_amd.write_mask_extra(path, "fit", "contigs", np.asarray([1, 2, 3, 4, 5, 6], np.float64))    # the wrong value type
    r = subprocess.run([os.path.join(ROOT, "tools", "validate-regions"), "--min-coverage-reads=1", "ref.dam", "reads.db", "one.las", "fit"], cwd=d,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "vtype does not match: expected 0 but got 1" in r.stderr
