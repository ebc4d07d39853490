"""tools/fm-index: the reference's external/fm-index.cpp as `dentist check-results` calls it
(commands/checkResults.d:511-565, 654-687) -- stdout byte for byte against tests/locate_ref.py, the .fm9 file, the exit
codes, and the pipeline shape of check-results on a .dam."""
import os
import subprocess

import numpy as np
import pytest

import locate_ref as lr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
FM = os.path.join(TOOLS, "fm-index")


def run(*args, cwd, stdin=None):
    kw = {"input": stdin} if stdin is not None else {"stdin": subprocess.DEVNULL}
    return subprocess.run([FM, *args], cwd=cwd, capture_output=True, text=True, timeout=300, **kw)


def rnd_text(rng, n, letters="acgt"):
    return "".join(letters[c] for c in rng.integers(0, 4, n))


@pytest.fixture(scope="module")
def texts():
    rng = np.random.default_rng(11)
    recs = [rnd_text(rng, 900), "", rnd_text(rng, 1), rnd_text(rng, 400), "a" * 100, rnd_text(rng, 2600)]
    ref = "".join(r + "\n" for r in recs)
    q1 = [recs[0][20:880], "", "a" * 40, lr.revcomp(recs[3][10:300]), recs[5], recs[0][-3:] + recs[3][:3], "acgtacgtgg" * 5, recs[5][7:8]]
    q2 = [recs[3][:64], "", "", recs[5][-257:]]
    return ref, "".join(q + "\n" for q in q1), "".join(q + "\n" for q in q2)


def test_output_equals_the_oracle(tmp_path, texts):
    ref, q1, q2 = texts
    (tmp_path / "ref.seq").write_text(ref)
    (tmp_path / "q.seq").write_text(q1)
    (tmp_path / "q2.seq").write_text(q2)
    # the index build of check-results: prints nothing, leaves the .fm9, writes no .idx
    res = run("ref.seq", cwd=tmp_path)
    assert (res.returncode, res.stdout) == (0, ""), res.stderr
    fm9 = tmp_path / "ref.seq.fm9"
    assert fm9.exists() and not (tmp_path / "ref.seq.idx").exists()
    assert "ref.seq.fm9" in res.stderr
    os.utime(fm9, ns=(10**18, 10**18))
    # queries from a file, both strands
    res = run("-r", "ref.seq", "q.seq", cwd=tmp_path)
    assert res.returncode == 0, res.stderr
    exp = lr.tool_output(ref, [("q.seq", q1)], True)
    assert exp.count("\n") > 100 and "\tyes\n" in exp and "\tno\n" in exp
    assert res.stdout == exp
    assert os.stat(fm9).st_mtime_ns == 10**18 and "fm9" not in res.stderr  # reused, not rewritten
    # forward only
    res = run("ref.seq", "q.seq", cwd=tmp_path)
    assert res.returncode == 0 and res.stdout == lr.tool_output(ref, [("q.seq", q1)], False)
    # queries on stdin, the way check-results pipes a slice of its list in
    res = run("-P" + str(tmp_path), "-r", "ref.seq", cwd=tmp_path, stdin=q1)
    assert res.returncode == 0 and res.stdout == lr.tool_output(ref, [("stdin", q1)], True)
    # two files: the ids restart; a file that does not exist is skipped with a warning
    res = run("-r", "ref.seq", "q.seq", "nothing.seq", "q2.seq", cwd=tmp_path)
    assert res.returncode == 0 and res.stdout == lr.tool_output(ref, [("q.seq", q1), ("q2.seq", q2)], True)
    assert "nothing.seq" in res.stderr and "\nq2.seq\t" in res.stdout
    # a corrupted magic: rewritten
    raw = fm9.read_bytes()
    fm9.write_bytes(b"X" + raw[1:])
    res = run("ref.seq", cwd=tmp_path)
    assert res.returncode == 0 and fm9.read_bytes() == raw and "ref.seq.fm9" in res.stderr


def test_fm9_follows_the_reference_file(tmp_path):
    (tmp_path / "r.seq").write_text("acgt\n\ncc\n")
    assert run("r.seq", cwd=tmp_path).returncode == 0
    raw = (tmp_path / "r.seq.fm9").read_bytes()
    head = np.frombuffer(raw[8:], dtype="<i8")
    assert raw[:5] == b"dhfm9" and head[:3].tolist() == [1, 9, 3] and head[3:].tolist() == [0, 5, 6, 9]
    (tmp_path / "r.seq").write_text("acgt\n\nccg\n")  # another size: rewritten
    assert run("r.seq", cwd=tmp_path).returncode == 0
    assert np.frombuffer((tmp_path / "r.seq.fm9").read_bytes()[8:], dtype="<i8")[:3].tolist() == [1, 10, 3]


def test_reference_without_a_final_newline(tmp_path):
    (tmp_path / "r.seq").write_text("acgtt\nggcat")
    res = run("-r", "r.seq", cwd=tmp_path, stdin="cat\nat\n")
    assert res.returncode == 0, res.stderr
    assert res.stdout == lr.tool_output("acgtt\nggcat", [("stdin", "cat\nat\n")], True)
    assert "stdin\t1\t5\t0\t2\t5\tno\n" in res.stdout


def test_upper_case_is_served_when_everything_is(tmp_path):
    (tmp_path / "r.seq").write_text("ACGTT\nGGCAT\n")
    res = run("-r", "r.seq", cwd=tmp_path, stdin="CAT\nAACG\n")
    assert res.returncode == 0 and res.stdout == lr.tool_output("ACGTT\nGGCAT\n", [("stdin", "CAT\nAACG\n")], True)
    assert res.stdout.count("\n") == 2


def test_error_paths(tmp_path):
    (tmp_path / "r.seq").write_text("acgtt\nggcat\n")
    (tmp_path / "q.seq").write_text("cat\n\nacnt\n")
    res = run("r.seq", "q.seq", cwd=tmp_path)
    assert res.returncode == 2 and res.stdout == "" and "q.seq: line 3" in res.stderr
    res = run("r.seq", cwd=tmp_path, stdin="cat\nCAT\n")
    assert res.returncode == 2 and res.stdout == "" and "stdin: line 2" in res.stderr and "case" in res.stderr
    (tmp_path / "R.seq").write_text("acgtt\nGGCAT\n")
    res = run("R.seq", cwd=tmp_path)
    assert res.returncode == 2 and "R.seq: line 2" in res.stderr
    res = run("-x", "r.seq", cwd=tmp_path)
    assert res.returncode == 1 and "Usage" in res.stderr
    res = run("-rx", "r.seq", cwd=tmp_path)
    assert res.returncode == 1 and "Usage" in res.stderr
    res = run("-P" + str(tmp_path / "no-such-dir"), "r.seq", cwd=tmp_path)
    assert res.returncode == 1 and "no-such-dir" in res.stderr
    res = run("-r", cwd=tmp_path)
    assert res.returncode == 1 and "Usage" in res.stderr
    res = run("missing.seq", cwd=tmp_path)
    assert res.returncode == 2
    res = run("r.seq", "nothing.seq", cwd=tmp_path)
    assert res.returncode == 0 and res.stdout == "" and "nothing.seq" in res.stderr


def test_check_results_pipeline_shape(tmp_path):
    """fasta2DAM, `DBdump -s | grep '^S' | cut -d' ' -f3`, the queries cropped by 20 bases per side as
    makeCroppedSequenceList does: exactly one forward hit per contig, at [20, len - 20)"""
    rng = np.random.default_rng(5)
    contigs = [rnd_text(rng, n) for n in (700, 1500, 333, 2100)]
    # two scaffolds; the second has a gap, so the .dam holds four contigs
    fasta = ">s1\n" + contigs[0] + "\n>s2\n" + contigs[1] + "n" * 50 + contigs[2] + "\n>s3\n" + contigs[3] + "\n"
    (tmp_path / "asm.fasta").write_text(fasta)
    subprocess.run([os.path.join(TOOLS, "fasta2DAM"), "asm.dam", "asm.fasta"], cwd=tmp_path, check=True, timeout=300)
    dump = subprocess.run([os.path.join(TOOLS, "DBdump"), "-s", "asm.dam"], cwd=tmp_path, check=True, capture_output=True, text=True,
                          timeout=300).stdout
    seqs = [line.split(" ")[2] for line in dump.split("\n") if line.startswith("S")]
    assert seqs == contigs
    (tmp_path / "asm.seq").write_text("".join(s + "\n" for s in seqs))
    queries = "".join(s[20:-20] + "\n" for s in seqs)
    assert run("asm.seq", cwd=tmp_path).returncode == 0 and (tmp_path / "asm.seq.fm9").exists()
    res = run("-P" + str(tmp_path), "-r", "asm.seq", cwd=tmp_path, stdin=queries)
    assert res.returncode == 0, res.stderr
    assert res.stdout == "".join(f"stdin\t{i}\t{len(s)}\t{i}\t20\t{len(s) - 20}\tno\n" for i, s in enumerate(seqs))
