"""tools/output at its command line: the usage and the exit codes, --revert, the gap specs and their messages
(commandline.d:2428-2484, 2511-2604).  Everything here fails -- or is refused -- before a device is opened.  No GPU needed."""
import os
import subprocess

import pytest

import dentist_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*args, cwd=None):
    return subprocess.run([os.path.join(ROOT, "tools", "output"), *args], cwd=cwd, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def dbs(tmp_path_factory):
    """a .dam of three contigs in one scaffold and a reads .db; no insertions.db: every case ends before it is read"""
    d = tmp_path_factory.mktemp("cli")
    seq = "acgtgcatgactgactgactagctagctacgatcgatcagctagctagcta"
    dentist_amd.dazz_create_dam(str(d / "ref.dam"), ">scaf\n" + seq + "n" * 30 + seq[::-1] + "n" * 12 + seq + "\n")
    dentist_amd.dazz_split(str(d / "ref.dam"), cutoff=20)
    dentist_amd.dazz_create_db(str(d / "reads.db"), ">sim/1/0_51 RQ=0.850\n" + seq + "\n")
    dentist_amd.dazz_split(str(d / "reads.db"), cutoff=20)
    return d


def test_usage_and_unknown_options_exit_1():
    for args in ((), ("a.dam",), ("a.dam", "b.db"), ("a", "b", "c", "d", "e"), ("--no-such-option", "a", "b", "c"), ("--join-policy=all", "a", "b", "c"),
                 ("--only=none", "a", "b", "c")):
        r = run(*args)
        assert r.returncode == 1 and "usage: output [--agp=<f>]" in r.stderr and r.stdout == "", args


def test_scaffolding_is_refused_with_exit_2():
    r = run("--scaffolding=graph.db", "a", "b", "c")
    assert r.returncode == 2 and "--scaffolding" in r.stderr and "not built" in r.stderr


def test_ignored_options_are_reported_once(dbs):
    r = run("--config=x.yaml", "-v", "--quiet", "-T4", "--threads=2", "ref.dam", "reads.db", "missing.db", cwd=dbs)
    assert r.stderr.count("have no effect here") == 1
    assert r.returncode == 2 and "missing.db" in r.stderr     # the library's message: the file does not exist


def test_missing_databases_exit_2():
    r = run("no.dam", "no.db", "no-insertions.db")
    assert r.returncode == 2 and r.stderr.startswith("output: ")


def test_ill_formatted_gap_specs():
    for spec in ("1", "1-", "-2", "a-b", "1-2x", "1-2,", "1_2"):
        r = run(f"--skip-gaps={spec}", "a", "b", "c")
        bad = spec.split(",")[-1] if spec.endswith(",") else spec
        assert r.returncode == 2 and f"ill-formatted <gap-spec> ({bad}): should be <contigA>-<contigB>" in r.stderr, spec


def test_gap_specs_are_checked_against_the_reference_db(dbs):
    cases = {"0-2": "invalid <gap-spec>: <contigA> == 0 is out of bounds [1, 3]",
             "4-2": "invalid <gap-spec>: <contigA> == 4 is out of bounds [1, 3]",
             "1-7": "invalid <gap-spec>: <contigB> == 7 is out of bounds [1, 3]",
             "2-2": "invalid <gap-spec>: <contigA> mut not be equal to <contigB>",
             "1-2,3-3": "invalid <gap-spec>: <contigA> mut not be equal to <contigB>"}
    for spec, msg in cases.items():
        r = run(f"--skip-gaps={spec}", "ref.dam", "reads.db", "missing.db", cwd=dbs)
        assert r.returncode == 2 and msg in r.stderr, (spec, r.stderr)
    # well-formed pairs in either order pass the check: the run ends at the missing insertions.db
    r = run("--skip-gaps=2-1,2-3", "ref.dam", "reads.db", "missing.db", cwd=dbs)
    assert r.returncode == 2 and "gap-spec" not in r.stderr and "missing.db" in r.stderr


def test_skip_gaps_file(dbs):
    (dbs / "ok.txt").write_text("# comment\n\n1-2\n3-2\n")
    r = run("--skip-gaps-file=ok.txt", "ref.dam", "reads.db", "missing.db", cwd=dbs)
    assert r.returncode == 2 and "gap-spec" not in r.stderr and "missing.db" in r.stderr
    (dbs / "bad.txt").write_text("# comment\n1-2\n\n2+3\n")
    r = run("--skip-gaps-file=bad.txt", "ref.dam", "reads.db", "missing.db", cwd=dbs)
    assert r.returncode == 2 and "ill-formatted <gap-spec> (2+3) in bad.txt:4: should be <contigA>-<contigB>" in r.stderr
    (dbs / "range.txt").write_text("1-9\n")
    r = run("--skip-gaps-file=range.txt", "ref.dam", "reads.db", "missing.db", cwd=dbs)
    assert r.returncode == 2 and "<contigB> == 9 is out of bounds [1, 3]" in r.stderr
    r = run("--skip-gaps-file=none.txt", "ref.dam", "reads.db", "missing.db", cwd=dbs)
    assert r.returncode == 2 and "none.txt" in r.stderr


def test_revert(dbs):
    r = run("--revert=no-such", "a", "b", "c")
    assert r.returncode == 2 and "invalid value for --revert: unknown option --no-such" in r.stderr
    r = run("--revert=x", "a", "b", "c")
    assert r.returncode == 2 and "invalid value for --revert: unknown option -x" in r.stderr
    # a reverted option ends at its default whatever the command line gave it: the out-of-range pair is gone,
    # the bad error limit is the default again, and `scaffolding` is a known name
    r = run("--skip-gaps=1-9", "--max-insertion-error=7", "--revert=skip-gaps,max-insertion-error,scaffolding", "ref.dam", "reads.db", "missing.db", cwd=dbs)
    assert r.returncode == 2 and "gap-spec" not in r.stderr and "max-insertion-error" not in r.stderr and "missing.db" in r.stderr
    r = run("--revert=skip-gaps", "--skip-gaps=1-9", "ref.dam", "reads.db", "missing.db", cwd=dbs)   # the order on the line does not matter
    assert r.returncode == 2 and "gap-spec" not in r.stderr
    r = run("--max-insertion-error=7", "ref.dam", "reads.db", "missing.db", cwd=dbs)
    assert r.returncode == 2 and "--max-insertion-error must lie in [0, 1]" in r.stderr
    for name in ("agp", "agp-dazzler", "agp-skip-read-ids", "closed-gaps-bed", "fasta-line-width", "no-highlight-insertions", "join-policy", "only",
                 "min-extension-length", "skip-gaps-file"):
        r = run(f"--revert={name}", "ref.dam", "reads.db", "missing.db", cwd=dbs)
        assert r.returncode == 2 and "revert" not in r.stderr and "missing.db" in r.stderr, name
