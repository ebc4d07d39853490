"""The command-line surface of tools/process (also installed as process-pile-ups) and tools/show-pile-ups: grammar, messages
and exit codes of everything that ends before `process` asks for a device -- the usage exits (1), what fails behind the
options (2), --batch with `$`, reversed ranges, ranges outside the file and ranges that intersect -- and show-pile-ups in both
forms against pileupdb_read's counts.  CPU only."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dentist_amd
import test_pileups_from_db as world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def run(tool, *args):
    r = subprocess.run([os.path.join(TOOLS, tool)] + list(args), capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("process_cli")
    rng = np.random.default_rng(3)
    fasta = "".join(">contig%d\n%s\n" % (i, "".join("acgt"[c] for c in rng.integers(0, 4, n))) for i, n in enumerate(world.CONTIG_LEN))
    ref = str(d / "ref.dam")
    dentist_amd.dazz_create_dam(ref, fasta)
    ptr = np.array([0, 1, 1, 2, 2], np.int64)
    dentist_amd.dazz_write_mask(ref, "rep", ptr, np.array([100, 300, 50, 80], np.int32))
    dentist_amd.dazz_write_mask(ref, "tan", ptr, np.array([200, 400, 10, 60], np.int32))
    nodes, triples, las, trace = world.build_world()
    piles = str(d / "pile-ups.db")
    world.write_world(piles, nodes, triples, las, trace)
    empty = str(d / "empty.db")
    dentist_amd.pileupdb_write(empty, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, dentist_amd.SEEDED_DTYPE),
                               np.zeros(0, dentist_amd.CHAIN_LA_DTYPE), np.zeros(0, np.uint16))
    split = world.split_piles(piles)
    split[2][0][0][0]["contig_a_len"] += 1
    bad = str(d / "bad.db")
    world.write_piles(bad, split)
    return dict(dir=str(d), ref=ref, reads=str(d / "reads.db"), piles=piles, empty=empty, bad=bad, out=str(d / "insertions.db"))


def test_usage_exits(files):
    for args in ([], ["--mask=rep"], [files["ref"], files["reads"], files["piles"], files["out"]],   # no mask: at least one is required
                 ["--mask=rep", files["ref"], files["reads"], files["piles"]], ["--mask=rep", files["ref"], files["reads"], files["piles"], files["out"], "x"]):
        rc, out, err = run("process", *args)
        assert rc == 1 and out == "" and err.startswith("process: usage: process [--mask="), (args, err)
    for bad in ("--frobnicate", "--only=neither", "--only=", "-x3", "--mask="):
        rc, out, err = run("process", bad, "--mask=rep", files["ref"], files["reads"], files["piles"], files["out"])
        assert rc == 1 and err.startswith("process: unknown or malformed option " + bad + "\nusage: process "), (bad, err)
    assert not os.path.exists(files["out"])


def test_allow_single_reads_is_not_built(files):
    rc, out, err = run("process", "--allow-single-reads", "--mask=rep", files["ref"], files["reads"], files["piles"], files["out"])
    assert rc == 2 and "--allow-single-reads" in err and "not built" in err


@pytest.mark.parametrize("spec", ["1..", "a", "1...3", "$", "..3", "1..$x", "1,,2", "1..-3", "0x2", "1.5", "2..$,"])
def test_ill_formatted_batches(files, spec):
    for form in (["--batch=" + spec], ["-b", spec], ["-b" + spec]):
        rc, out, err = run("process", "--mask=rep", *form, files["ref"], files["reads"], files["piles"], files["out"])
        assert (rc, err) == (2, "process: ill-formatted batch range\n"), (form, err)


@pytest.mark.parametrize("spec", ["3..1", "2..2", "0..6", "5", "5..$", "7..9", "0..2,4..99"])
def test_batches_outside_the_file_and_reversed(files, spec):
    rc, out, err = run("process", "--mask=rep", "--batch=" + spec, files["ref"], files["reads"], files["piles"], files["out"])
    assert (rc, err) == (2, "process: invalid batch range; check that 0 <= <from> < <to> <= 5\n"), (spec, err)


def test_batches_that_intersect(files):
    for args, i, j in ((["--batch=0..3,2..4"], 0, 1), (["--batch=4", "-b", "0..2", "--batch=1..$"], 0, 2), (["--batch=4", "-b", "0..2", "--batch=1..3"], 1, 2), (["-b3", "--batch=0..$"], 0, 1)):
        rc, out, err = run("process", "--mask=rep", *args, files["ref"], files["reads"], files["piles"], files["out"])
        assert (rc, err) == (2, "process: invalid --batch: <idx-spec>'s at indices %d and %d intersect\n" % (i, j)), (args, err)


@pytest.mark.parametrize("batch", [[], ["--batch=0..$"], ["--batch=0..5"], ["--batch=4", "--batch=0..2,2..4"], ["-b", "1..$", "-b0"], ["--batch=0..1,1..$"]])
def test_good_batches_reach_the_masks(files, batch):
    """a well-formed --batch is passed: the run ends at the next thing that fails, a mask track that does not exist"""
    rc, out, err = run("process", "--mask=rep,nope", *batch, files["ref"], files["reads"], files["piles"], files["out"])
    assert rc == 2 and err.startswith("process: mask nope: "), err


def test_numbers_are_checked(files):
    tail = ["--mask=rep", files["ref"], files["reads"], files["piles"], files["out"]]
    for opt, msg in (("--max-alignment-error=0.5", "--max-alignment-error must lie in (0, 0.3]"), ("-e0", "--max-alignment-error must lie in (0, 0.3]"),
                     ("--max-insertion-error=1.5", "--max-insertion-error must lie in [0, 1]"), ("--bad-fraction=0.5", "--bad-fraction must be within [0, 0.5)"),
                     ("--min-relative-score=0", "--min-relative-score must lie in (0, 1]"), ("--min-reads-per-pile-up=0", "an option's value is out of range"),
                     ("--min-anchor-length=12x", "an option's value is not a number")):
        rc, out, err = run("process", opt, *tail)
        assert (rc, err) == (2, "process: " + msg + "\n"), (opt, err)


def test_files_that_fail_before_a_device(files):
    tail = [files["reads"], files["piles"], files["out"]]
    rc, out, err = run("process", "--mask=rep", os.path.join(files["dir"], "none.dam"), *tail)
    assert rc == 2 and "none.dam" in err
    rc, out, err = run("process", "--mask=rep", files["ref"], files["reads"], os.path.join(files["dir"], "none.db"), files["out"])
    assert rc == 2 and "none.db" in err
    rc, out, err = run("process", "-m", "rep", "-mtan", files["ref"], files["reads"], files["bad"], files["out"])
    assert rc == 2 and "dh_pileups_from_db: pile-up 2: contig 2 has 6000 bases, the file says 6001" in err
    # ... but only when the batch holds the pile-up that is wrong
    rc, out, err = run("process", "--mask=rep,nope", "--batch=0..2", files["ref"], files["reads"], files["bad"], files["out"])
    assert rc == 2 and err.startswith("process: mask nope: ")
    assert not os.path.exists(files["out"])
    for r in (err,):
        assert not re.search(r"HIP|hip|dh_ctx_create", r)


def test_ignored_options_are_reported_once(files):
    rc, out, err = run("process", "--config=x.json", "-v", "--quiet", "-T4", "--threads=4", "-A2", "--auxiliary-threads=2", "-P/tmp", "--tmpdir=/tmp",
                       "--keep-temp", "--daccord=-f", "--daligner-consensus=-k20", "--daligner-reads-vs-reads=-k20", "--daligner-self=-k20",
                       "--datander-ref=-k20", "--dust-reads=-w64", "--mask=rep,nope", files["ref"], files["reads"], files["piles"], files["out"])
    assert rc == 2 and err.count("have no effect here") == 1 and "mask nope" in err


def test_an_empty_file_gives_an_empty_insertions_db_without_a_device(files):
    for tool, batch in (("process", []), ("process-pile-ups", ["--batch=0..$"])):
        out_path = files["out"] + "." + tool
        rc, out, err = run(tool, "--mask=rep", "--mask=tan", *batch, files["ref"], files["reads"], files["empty"], out_path)
        assert (rc, out, err) == (0, "", ""), err
        assert len(dentist_amd.insertiondb_read(out_path)["insertions"]) == 0
    assert open(files["out"] + ".process", "rb").read() == open(files["out"] + ".process-pile-ups", "rb").read()
    rc, out, err = run("process", "--mask=rep", "--batch=0", files["ref"], files["reads"], files["empty"], files["out"])
    assert (rc, err) == (2, "process: invalid batch range; check that 0 <= <from> < <to> <= 0\n")


def test_both_names_are_one_tool(files):
    for args in ([], ["--frobnicate"], ["--mask=rep", "--batch=3..1", files["ref"], files["reads"], files["piles"], files["out"]]):
        assert run("process", *args) == run("process-pile-ups", *args)
    rc, out, err = run("process", "--tool", "nope")
    assert rc == 1 and err == "nope: unknown tool (expected process process-pile-ups show-pile-ups)\n"


def test_show_pile_ups_in_both_forms(files):
    back = dentist_amd.pileupdb_read(files["piles"])
    want = {"totalDbSize": os.path.getsize(files["piles"]), "numPileUps": len(back["pile_counts"]), "numReadAlignments": len(back["ra_counts"]),
            "numSeededAlignments": len(back["seeded"]), "numLocalAlignments": len(back["las"]), "numTracePoints": len(back["trace"]) // 2}
    assert want["numPileUps"] == 5 and want["numTracePoints"] > 0
    for flag in ("-j", "--json"):
        rc, out, err = run("show-pile-ups", flag, files["piles"])
        assert rc == 0 and err == "" and out.count("\n") == 1
        assert json.loads(out) == want and list(json.loads(out)) == list(want)
    rc, out, err = run("show-pile-ups", files["piles"])
    assert rc == 0 and err == ""
    width = len(str(max(want.values()) - 1)) if max(want.values()) > 1 else 0   # ceil(log10(max)): showPileUps.d:88-102
    lines = ["%-20s %*d%s" % (k + ":", width, v, " bytes" if k == "totalDbSize" else "") for k, v in want.items()]
    assert out == "\n".join(lines) + "\n"
    assert lines[1].startswith("numPileUps:          ") and lines[3].startswith("numSeededAlignments: ")
    # the empty file, the usage, a missing file
    rc, out, err = run("show-pile-ups", "-j", files["empty"])
    assert rc == 0 and json.loads(out)["numPileUps"] == 0 and json.loads(out)["totalDbSize"] == 48
    rc, out, err = run("show-pile-ups", files["empty"])
    assert rc == 0 and out.splitlines()[0] == "%-20s %2d bytes" % ("totalDbSize:", 48) and out.splitlines()[1] == "%-20s %2d" % ("numPileUps:", 0)
    assert run("show-pile-ups")[0] == 1 and run("show-pile-ups", "-x", files["piles"])[0] == 1 and run("show-pile-ups", files["piles"], files["piles"])[0] == 1
    rc, out, err = run("show-pile-ups", os.path.join(files["dir"], "none.db"))
    assert rc == 2 and "none.db" in err
