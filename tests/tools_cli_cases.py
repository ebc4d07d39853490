"""The command-line surface of the tools, as a table: option grammar, message text, exit codes and the order in which
failures are found.  Every case ends before a tool creates a device context (options are parsed and files opened first), so
the table runs without a GPU.  `scripts/record_tools_cli.py` records it, `tests/test_tools_cli.py` replays it.

A case is (tool, argv, stdin): stdin is None, text, or "<name" for the bytes of the file `name` of the working directory.
All paths are relative to that directory, which `prepare` fills; no message contains a temporary path."""
import base64
import hashlib
import json
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

CONTIG = ["acgtacgttagcatcgatcgactagctagcatcgatcgatcagctacgatcgatcgactagc",
          "ttgacctagcatcgggatcctagcatgcatgcaagctagctagcatcgatgcatgctagcta",
          "ggatccatcgatgcatgcatcgtagctagcatgcatgcttagctagctagcatcgatcgat"]
READ = ["catcgatcgactagctagcatcgatcgatcagctacgatcgatcgactagcacgtacgttag",
        "cctagcatcgggatcctagcatgcatgcaagctagctagcatcgatgcatgctagctattga",
        "tccatcgatgcatgcatcgtagctagcatgcatgcttagctagctagcatcgatcgatgga",
        "gtgtctgctgttttttttcttttagtggacatacgatcgatcgatcgatgcatgcatgcat"]


def _run(tools, tool, args, cwd, stdin=None):
    p = subprocess.run([os.path.join(tools, tool), *args], input=stdin, cwd=cwd, capture_output=True, timeout=60)
    assert p.returncode == 0, (tool, args, p.stderr)


def prepare(tools, work):
    """ref.dam (a scaffold of two contigs and a single contig), reads.db (four reads), raw.db (not split); the masks `m`
    (one interval per contig and one more: four, as many as reads.db has reads), `m2` and `none` (empty) of ref.dam;
    small.las (ref.dam vs reads.db), empty.las, TAN.reads.las (self alignments); two FASTA files and the texts of fm-index."""
    import dentist_amd
    os.makedirs(work, exist_ok=True)
    ref = ">scaf_one\n%s%s%s\n>scaf_two\n%s\n" % (CONTIG[0], "n" * 30, CONTIG[1], CONTIG[2])
    reads = "".join(">Sim/%d/0_%d RQ=0.85%d\n%s\n" % (i + 1, len(s), i, s) for i, s in enumerate(READ))
    _run(tools, "fasta2DAM", ["-i", "ref.dam"], work, ref.encode())
    _run(tools, "fasta2DB", ["-i", "reads.db"], work, reads.encode())
    _run(tools, "fasta2DB", ["-i", "raw.db"], work, reads.encode())
    _run(tools, "DBsplit", ["-x20", "-a", "ref.dam"], work)
    _run(tools, "DBsplit", ["-x20", "-a", "reads.db"], work)
    dam = os.path.join(work, "ref.dam")
    dentist_amd.dazz_write_mask(dam, "m", [0, 2, 3, 4], [5, 20, 30, 50, 0, 40, 10, 61])
    dentist_amd.dazz_write_mask(dam, "m2", [0, 0, 1, 1], [20, 45])
    dentist_amd.dazz_write_mask(dam, "none", [0, 0, 0, 0], [0, 0])
    las = np.zeros(3, dtype=dentist_amd.LA_DTYPE)
    for i, (a, b) in enumerate([(0, 0), (1, 1), (2, 3)]):
        las[i]["aread"], las[i]["bread"] = a, b
        las[i]["abpos"], las[i]["aepos"], las[i]["bbpos"], las[i]["bepos"] = 10, 60, 0, 50
        las[i]["diffs"], las[i]["tlen"], las[i]["toff"] = 1, 2, 2 * i
    trace = np.asarray([1, 50] * 3, dtype=np.uint16)
    dentist_amd.las_write(os.path.join(work, "small.las"), las, trace, 100)
    dentist_amd.las_write(os.path.join(work, "empty.las"), las[:0], trace[:1], 100)
    las["bread"] = las["aread"]
    las["bbpos"], las["bepos"] = 2, 40
    dentist_amd.las_write(os.path.join(work, "TAN.reads.las"), las, trace, 100)
    for name, text in [("a.fasta", ">first one\n%s\n" % CONTIG[0]), ("b.fasta", ">second\n%s\n" % CONTIG[1]), ("plain.txt", "acgt\n"),
                       ("ref.seq", "acgtacgt\nttga\n"), ("withn.seq", "acgt\nacnt\n"), ("mixed.seq", "acgt\nACGT\n")]:
        with open(os.path.join(work, name), "w") as f:
            f.write(text)


IGNORED = ["-v", "--quiet", "--config=c.yaml", "-T8", "--threads=8"]
COLLECT_IGNORED = IGNORED + ["-A2", "--auxiliary-threads=2", "-Ptmp", "--tmpdir=tmp", "--damapper-ref-vs-reads=x.las"]


def _ignored(tool, rest, options=IGNORED):
    """every ignored option alone, in neighbouring pairs, all at once, and its malformed forms"""
    out = [(tool, [o] + rest, None) for o in options]
    out += [(tool, [a, b] + rest, None) for a, b in zip(options, options[1:])]
    out += [(tool, rest[:1] + options + rest[1:], None)]
    out += [(tool, [o] + rest, None) for o in ("-T", "--threads=", "--config=", "--config", "-vv", "--quiet=1")]
    return out


def _strict(tool, keys, rest):
    """the strict numbers: empty, not a number, trailing text, negative, too large, and the largest accepted"""
    return [(tool, ["--%s=%s" % (k, v)] + rest, None) for k in keys for v in ("", "x", "5x", "-1", "2147483648", "2147483647", " 7")]


def _lenient(tool, keys, rest):
    return [(tool, ["--%s=%s" % (k, v)] + rest, None) for k in keys for v in ("", "x", "5x", "1e", "0x10", " 7")]


def cases():
    c = []
    # ---- how a tool is chosen
    c += [("dazz_tools", [], None), ("dazz_tools", ["--tool"], None), ("dazz_tools", ["--tool", "nope"], None),
          ("dazz_tools", ["--tool", "nope", "x"], None), ("dazz_tools", ["--tool", "filter-mask"], None),
          ("dazz_tools", ["--tool", "DBshow", "-n", "ref.dam"], None), ("dazz_tools", ["--tool", "fasta2DAM"], None),
          ("dazz_tools", ["--tool", "DAScover"], None), ("dazz_tools", ["--tool", "computeintrinsicqv", "a"], None),
          ("filter-mask", ["--tool", "merge-masks"], None), ("dazz_tools", ["DBshow", "ref.dam"], None)]
    # ---- the DB tools
    for t in ("fasta2DB", "fasta2DAM"):
        c += [(t, [], None), (t, ["--bogus", "x.db"], None), (t, ["-Z", "x.db"], None), (t, ["-v"], None), (t, ["new.db", "absent.fasta"], None),
              (t, ["-v", "-i", "new"], ">Sim/1/0_8 RQ=0.850\nacgtacgt\n"), (t, ["-ifoo", "new"], ">x\nacgt\n"), (t, ["new", "a.fasta", "b.fasta"], None)]
    c += [("DBsplit", [], None), ("DBsplit", ["-Q", "x.db"], None), ("DBsplit", ["--bogus"], None), ("DBsplit", ["-a", "-f"], None),
          ("DBsplit", ["absent.db"], None), ("DBsplit", ["-x10", "-s1", "raw.db"], None), ("DBsplit", ["-x", "-s", "raw.db"], None),
          ("DBrm", [], None), ("DBrm", ["-v"], None), ("DBrm", ["absent.db"], None), ("DBrm", ["raw.db"], None)]
    c += [("DBdump", [], None), ("DBdump", ["-Z", "ref.dam"], None), ("DBdump", ["--bogus", "ref.dam"], None), ("DBdump", ["-rZ", "ref.dam"], None),
          ("DBdump", ["-r"], None), ("DBdump", ["absent.db"], None), ("DBdump", ["-r", "-h", "-s", "ref.dam"], None),
          ("DBdump", ["-rhsu", "reads.db", "2-3", "1"], None), ("DBdump", ["reads.db", "x"], None), ("DBdump", ["reads.db", "9"], None),
          ("DBdump", ["reads.db", "0"], None), ("DBdump", ["-i", "reads.db"], None), ("DBdump", ["-", "reads.db"], None),
          ("DBshow", [], None), ("DBshow", ["-Z", "ref.dam"], None), ("DBshow", ["--bogus", "ref.dam"], None), ("DBshow", ["-n"], None),
          ("DBshow", ["absent.dam"], None), ("DBshow", ["-n", "ref.dam"], None), ("DBshow", ["-w20", "-u", "reads.db", "2", "4"], None),
          ("DBshow", ["-w", "reads.db", "1"], None), ("DBshow", ["reads.db", "7"], None), ("DBshow", ["-q", "-U", "ref.dam", "1-2"], None)]
    c += [("DBdust", [], None), ("DBdust", ["-Z", "ref.dam"], None), ("DBdust", ["--bogus", "ref.dam"], None), ("DBdust", ["-w32", "ref.dam"], None),
          ("DBdust", ["-t2.5", "ref.dam"], None), ("DBdust", ["-m5", "ref.dam"], None), ("DBdust", ["-w64", "-t2.0", "-m10", "-b"], None),
          ("Catrack", [], None), ("Catrack", ["-Z", "ref.dam", "m"], None), ("Catrack", ["--bogus", "ref.dam", "m"], None),
          ("Catrack", ["ref.dam"], None), ("Catrack", ["ref.dam", "m", "x"], None), ("Catrack", ["absent.dam", "m"], None),
          ("Catrack", ["-v", "-f", "-d", "raw.db", "m"], None), ("Catrack", ["ref.dam", "absent"], None)]
    # ---- the .las tools
    c += [("LAmerge", [], None), ("LAmerge", ["-Z", "out", "small.las"], None), ("LAmerge", ["--bogus", "out", "small.las"], None),
          ("LAmerge", ["out"], None), ("LAmerge", ["-v", "-a", "-Ptmp"], None), ("LAmerge", ["out", "absent.las"], None),
          ("LAmerge", ["-v", "out", "small.las", "empty.las"], None), ("LAmerge", ["out.las", "empty.las"], None),
          ("LAsplit", [], None), ("LAsplit", ["-Z", "p.@", "2"], None), ("LAsplit", ["--bogus", "p.@", "2"], None), ("LAsplit", ["p.@"], None),
          ("LAsplit", ["p.@", "2", "3"], None), ("LAsplit", ["p", "2"], "<small.las"), ("LAsplit", ["p.@", "0"], "<small.las"),
          ("LAsplit", ["p.@", "x"], "<small.las"), ("LAsplit", ["p.@", "2"], "not a las"), ("LAsplit", ["-v", "p.@", "2"], "<small.las"),
          ("LAsplit", ["p.#.las", "1"], "<empty.las"), ("LAsplit", ["-", "2"], None),
          ("TANmask", [], None), ("TANmask", ["-Z", "reads.db", "TAN.reads.las"], None), ("TANmask", ["--bogus", "reads.db", "TAN.reads.las"], None),
          ("TANmask", ["-l", "reads.db", "TAN.reads.las"], None), ("TANmask", ["-n", "reads.db", "TAN.reads.las"], None),
          ("TANmask", ["reads.db"], None), ("TANmask", ["absent.db", "TAN.reads.las"], None), ("TANmask", ["reads.db", "absent.las"], None),
          ("TANmask", ["-v", "-l30", "reads.db", "TAN.reads"], None), ("TANmask", ["-l30", "-ntandem", "reads.db", "TAN.reads.las"], None),
          ("TANmask", ["-l30", "ref.dam", "small.las"], None), ("TANmask", ["-lx", "reads.db", "empty.las"], None)]
    for t in ("DAScover", "DASqv", "computeintrinsicqv"):
        c += [(t, [], None), (t, ["-Z", "reads.db", "small.las"], None), (t, ["--bogus", "reads.db", "small.las"], None), (t, ["-v", "reads.db"], None),
              (t, ["-c10", "-mdust", "-H5", "reads.db", "small.las", "x"], None)]
    c += [("DAScover", ["-v", "reads.db", "small.las"], None), ("DAScover", ["-d4", "absent.db", "absent.las"], None),
          ("daccord", [], None), ("daccord", ["-Z", "small.las", "reads.db"], None), ("daccord", ["--bogus", "small.las", "reads.db"], None),
          ("daccord", ["-Ix", "small.las", "reads.db"], None), ("daccord", ["-I1", "small.las", "reads.db"], None), ("daccord", ["small.las"], None),
          ("daccord", ["-t4", "-f", "-w1", "-a2", "-k8", "-m3", "-d9", "-V1", "--rounds=2", "small.las"], None),
          ("daccord", ["--rounds=", "small.las"], None), ("daccord", ["--eprofonly", "-I0,1", "small.las", "reads.db"], None),
          ("daccord", ["--eprofonly", "absent/small.las", "reads.db"], None),
          ("merge-insertions", [], None), ("merge-insertions", ["-Z", "out.db", "in.db"], None), ("merge-insertions", ["--bogus", "out.db", "in.db"], None),
          ("merge-insertions", ["-v", "-vv", "-vvv", "out.db"], None), ("merge-insertions", ["-vvvv", "out.db", "in.db"], None),
          ("merge-insertions", ["out.db", "absent.db"], None)]
    # ---- the alignment views
    c += [("LApaf", [], None), ("LApaf", ["-Z", "ref.dam", "small.las"], None), ("LApaf", ["--bogus", "ref.dam", "small.las"], None),
          ("LApaf", ["ref.dam"], None), ("LApaf", ["-a", "-c", "-w0", "ref.dam", "small.las"], None), ("LApaf", ["-wx", "ref.dam", "small.las"], None),
          ("LApaf", ["a", "b", "c", "d"], None), ("LApaf", ["a", "b", "c", "d", "1-2"], None),
          ("LApaf", ["ref.dam", "reads.db", "small.las", "-"], None),
          ("LAtranspose", [], None), ("LAtranspose", ["-Z", "a", "b", "c", "d"], None), ("LAtranspose", ["--bogus", "a", "b", "c", "d"], None),
          ("LAtranspose", ["-b", "a", "b", "c"], None), ("LAtranspose", ["a", "b", "c", "d", "e"], None),
          ("DBnw", [], None), ("DBnw", ["-Z", "ref.dam", "reads.db"], None), ("DBnw", ["--bogus", "ref.dam", "reads.db"], None), ("DBnw", ["ref.dam"], None),
          ("DBnw", ["-f", "-a", "-w0", "ref.dam", "reads.db"], None), ("DBnw", ["a", "b", "c"], None), ("DBnw", ["a", "b", "c", "1-2"], None)]
    pair = ["a.fasta", "absent.fasta"]
    c += [("stretcher", [], None), ("stretcher", ["--bogus"] + pair, None), ("stretcher", ["-Z"] + pair, None), ("stretcher", ["a.fasta"], None),
          ("stretcher", ["a.fasta", "b.fasta", "c.fasta"], None), ("stretcher", pair, None), ("stretcher", ["absent.fasta", "a.fasta"], None),
          ("stretcher", ["--auto", "--stdout", "--aformat=pair", "--awidth=4294967295", "--sreverse2"] + pair, None),
          ("stretcher", ["-auto", "-stdout", "-aformat=pair", "-awidth=60", "-sreverse2", "-gapopen=12", "-gapextend=2", "-outfile=o.txt"] + pair, None),
          ("stretcher", ["a.fasta", "plain.txt"], None), ("stretcher", ["-"] + pair, None)]
    c += [("stretcher", [o] + pair, None) for o in (
        "--auto=1", "--stdout=", "--sreverse2=x", "--aformat=srspair", "--aformat=", "--aformat", "--awidth=", "--awidth=x", "--awidth=0",
        "--awidth=-3", "--awidth", "--gapopen=", "--gapopen=x", "--gapopen=-1", "--gapopen=2147483648", "--gapopen=0", "--gapextend=",
        "--gapextend=1.5", "--gapextend=-2", "--outfile=", "--outfile")]
    c += [("fm-index", [], None), ("fm-index", ["-Z", "ref.seq"], None), ("fm-index", ["--bogus", "ref.seq"], None), ("fm-index", ["-P"], None),
          ("fm-index", ["-P", "ref.seq"], None), ("fm-index", ["-rx", "ref.seq"], None), ("fm-index", ["-r"], None), ("fm-index", ["-Pabsent", "ref.seq"], None),
          ("fm-index", ["-Pplain.txt", "-r", "ref.seq"], None), ("fm-index", ["-P."], None), ("fm-index", ["absent.seq"], None),
          ("fm-index", ["-r", "absent.seq", "plain.txt"], None), ("fm-index", ["withn.seq"], "acgt\n"), ("fm-index", ["mixed.seq"], "acgt\n"),
          ("fm-index", ["-"], None), ("fm-index", [""], None)]
    # ---- chain-local-alignments: its numbers are checked after the .las is read
    t, rest = "chain-local-alignments", ["ref.dam", "reads.db", "small.las", "out.las"]
    keys = ["max-indel", "max-chain-gap", "max-relative-overlap", "min-relative-score", "min-score"]
    c += [(t, [], None), (t, ["--bogus"] + rest, None), (t, ["-Z"] + rest, None), (t, ["-v"] + rest, None), (t, ["--max-indel"] + rest, None),
          (t, rest[:2], None), (t, rest + ["x"], None), (t, ["-"] + rest, None),
          (t, ["ref.dam", "reads.db", "absent.las", "out.las"], None), (t, ["--max-indel=x", "ref.dam", "reads.db", "absent.las", "out.las"], None),
          (t, ["--min-score=x", "absent.dam", "small.las", "out.las"], None), (t, ["absent.dam", "small.las", "out.las"], None),
          (t, ["ref.dam", "absent.db", "small.las", "out.las"], None), (t, ["absent.dam", "absent.db", "small.las", "out.las"], None),
          (t, ["--max-indel=5", "--max-chain-gap=7", "--max-relative-overlap=0.5", "--min-relative-score=.3", "--min-score=1",
               "ref.dam", "small.las", "out.las"], None),
          (t, ["reads.db", "ref.dam", "small.las", "out.las"], None), (t, ["--max-indel=1", "--max-indel=x", "ref.dam", "small.las", "out.las"], None)]
    c += _lenient(t, keys, ["ref.dam", "small.las", "out.las"])
    # ---- propagate-mask
    t, rest = "propagate-mask", ["-m", "m", "absent.dam", "reads.db", "small.las", "out"]
    c += [(t, [], None), (t, ["--bogus"] + rest, None), (t, ["-Z"] + rest, None), (t, ["ref.dam", "reads.db", "small.las", "out"], None),
          (t, ["ref.dam", "reads.db", "small.las", "out", "-m"], None), (t, ["--mask="] + rest, None), (t, ["--mask"] + rest, None),
          (t, ["-m", "m", "ref.dam", "out"], None), (t, ["-m", "m", "a", "b", "c", "d", "e"], None), (t, ["-m", "-v", "ref.dam", "small.las", "out"], None),
          (t, rest, None), (t, ["-mm", "ref.dam", "absent.db", "small.las", "out"], None), (t, ["--mask=m", "ref.dam", "reads.db", "absent.las", "out"], None),
          (t, ["-m", "m", "-mabsent", "--mask=m2", "ref.dam", "small.las", "out"], None), (t, ["--mask=m,m2", "ref.dam", "small.las", "out"], None),
          (t, ["-m", "absent", "ref.dam", "reads.db", "absent.las", "out"], None), (t, ["-mm", "--mask=m2", "-m", "none", "ref.dam", "absent.las", "out"], None)]
    c += _ignored(t, rest)
    # ---- validate-regions: its numbers are checked before anything is opened
    t, rest = "validate-regions", ["ref.dam", "reads.db", "absent.las", "m"]
    cov = ["--min-coverage-reads=2"]
    keys = ["min-coverage-reads", "read-coverage", "ploidy", "min-spanning-reads", "region-context", "weak-coverage-window"]
    c += [(t, [], None), (t, ["--bogus"] + rest, None), (t, ["-Z"] + rest, None), (t, cov + rest[:3], None), (t, cov + rest + ["x"], None),
          (t, rest, None), (t, cov + ["--read-coverage=20", "--ploidy=2"] + rest, None), (t, ["--read-coverage=20"] + rest, None),
          (t, ["--read-coverage=20", "--ploidy=0"] + rest, None), (t, ["--read-coverage=20", "--ploidy=-2"] + rest, None),
          (t, ["--ploidy=2"] + rest, None), (t, ["--read-coverage=20", "--ploidy=2"] + rest, None), (t, cov + rest, None),
          (t, ["--min-coverage-reads=x"] + rest, None), (t, ["--region-context=x", "--read-coverage=20"] + rest, None),
          (t, cov + ["--weak-coverage-mask="] + rest, None), (t, cov + ["--weak-coverage-mask=weak", "--report-all"] + rest, None),
          (t, cov + ["--report-all=1"] + rest, None), (t, cov + ["absent.dam", "reads.db", "small.las", "m"], None),
          (t, cov + ["ref.dam", "absent.db", "small.las", "m"], None), (t, cov + ["ref.dam", "reads.db", "empty.las", "m"], None),
          (t, cov + ["-v", "ref.dam", "reads.db", "empty.las", "absent"], None), (t, cov + ["ref.dam", "reads.db", "small.las", "absent"], None),
          (t, cov + ["--min-spanning-reads=1", "--region-context=10", "--weak-coverage-window=5", "ref.dam", "reads.db", "small.las", "absent"], None)]
    c += _lenient(t, keys, ["--min-coverage-reads=2"] + rest) + _ignored(t, cov + rest)
    # ---- collect: its numbers are checked after the .las is read
    t, rest = "collect", ["ref.dam", "reads.db", "small.las", "piles.db"]
    keys = ["max-alignment-error", "min-anchor-length", "proper-alignment-allowance", "min-spanning-reads", "best-pile-up-margin", "existing-gap-bonus"]
    c += [(t, [], None), (t, ["--bogus", "-mm"] + rest, None), (t, ["-Z", "-mm"] + rest, None), (t, rest, None), (t, rest + ["-m"], None),
          (t, rest + ["-e"], None), (t, ["--mask="] + rest, None), (t, ["--mask=,"] + rest, None), (t, ["--mask"] + rest, None), (t, ["--m=m"] + rest, None),
          (t, ["--e=0.2", "-mm"] + rest, None), (t, ["-mm"] + rest[:3], None), (t, ["-mm"] + rest + ["x"], None),
          (t, ["-m", "absent"] + rest, None), (t, ["-mabsent"] + rest, None), (t, ["--mask=absent"] + rest, None), (t, ["--mask=m,absent"] + rest, None),
          (t, ["--mask=m,,m2", "--mask=absent2,m"] + rest, None), (t, ["-m", "m,absent3"] + rest, None),
          (t, ["-mm", "-e", "0.5"] + rest, None), (t, ["-mm", "-e0.5"] + rest, None), (t, ["-mm", "--max-alignment-error=0.5"] + rest, None),
          (t, ["-mm", "-e", "0"] + rest, None), (t, ["-mm", "-e", "-0.1"] + rest, None), (t, ["-mm", "-e", "x"] + rest, None),
          (t, ["-mabsent", "-e", "0.3"] + rest, None), (t, ["-mabsent", "-e0.2", "--no-merge-extension"] + rest, None),
          (t, ["-mm", "--no-merge-extension=1"] + rest, None),
          (t, ["-mm", "ref.dam", "reads.db", "absent.las", "piles.db"], None), (t, ["-mm", "--min-anchor-length=x", "ref.dam", "reads.db", "absent.las", "piles.db"], None),
          (t, ["-mm", "-e", "0.5", "ref.dam", "reads.db", "empty.las", "piles.db"], None), (t, ["-mm", "--min-anchor-length=x", "ref.dam", "reads.db", "empty.las", "piles.db"], None),
          (t, ["-mm", "absent.dam", "reads.db", "small.las", "piles.db"], None), (t, ["-mm", "ref.dam", "absent.db", "small.las", "piles.db"], None),
          (t, ["-mabsent", "-e", "0.5", "absent.dam", "reads.db", "small.las", "piles.db"], None)]
    c += _lenient(t, keys, ["-mabsent"] + rest) + _ignored(t, ["-mabsent"] + rest, COLLECT_IGNORED)
    c += [(t, [o, "-mabsent"] + rest, None) for o in ("-A", "-P", "--auxiliary-threads=", "--tmpdir=", "--damapper-ref-vs-reads=", "--tmpdir", "--T8", "--A2", "--Ptmp")]
    # ---- mask-repetitive-regions
    t = "mask-repetitive-regions"
    self_case, reads_case = ["absent.dam", "small.las", "rep"], ["absent.dam", "reads.db", "small.las", "rep"]
    keys = ["max-coverage-reads", "max-improper-coverage-reads", "max-coverage-self", "proper-alignment-allowance"]
    c += [(t, [], None), (t, ["--bogus"] + self_case, None), (t, ["-Z"] + self_case, None), (t, self_case[:2], None), (t, reads_case + ["x"], None),
          (t, reads_case, None), (t, ["--max-coverage-reads=5"] + reads_case, None), (t, ["--max-improper-coverage-reads=5"] + reads_case, None),
          (t, ["--max-coverage-reads=5", "--read-coverage=20"] + reads_case, None), (t, ["--max-improper-coverage-reads=5", "--read-coverage=20"] + reads_case, None),
          (t, ["--max-coverage-reads=5", "--max-improper-coverage-reads=5"] + reads_case, None), (t, ["--read-coverage=20"] + reads_case, None),
          (t, ["--read-coverage=20"] + self_case, None), (t, ["--max-coverage-self=0"] + self_case, None), (t, ["--max-coverage-self=0", "--read-coverage=20"] + reads_case, None),
          (t, ["--max-coverage-self=1"] + self_case, None), (t, ["-v", "--max-coverage-self=0"] + self_case, None), (t, ["--debug-repeat-masks=1"] + self_case, None),
          (t, ["ref.dam", "absent.las", "rep"], None), (t, ["--read-coverage=20", "ref.dam", "absent.db", "small.las", "rep"], None),
          (t, ["ref.dam", "empty.las", "rep"], None), (t, ["--debug-repeat-masks", "ref.dam", "empty.las", "rep"], None),
          (t, ["--read-coverage=20", "ref.dam", "reads.db", "empty.las", "rep"], None),
          (t, ["--read-coverage=20", "--debug-repeat-masks", "--proper-alignment-allowance=3", "-T4", "ref.dam", "reads.db", "empty.las", "rep"], None)]
    c += [(t, ["--read-coverage=" + v] + reads_case, None) for v in ("", "x", "0", "-1", "1e", "2.5x", "nan", "0.5")]
    c += _strict(t, keys, self_case) + _ignored(t, self_case)
    # ---- merge-masks, filter-mask
    t, rest = "merge-masks", ["ref.dam", "out", "absent"]
    c += [(t, [], None), (t, ["--bogus"] + rest, None), (t, ["-Z"] + rest, None), (t, rest[:2], None), (t, ["absent.dam", "out", "m"], None), (t, rest, None),
          (t, ["ref.dam", "out", "m", "m2", "absent"], None), (t, ["ref.dam", "out", "1.absent"], None), (t, ["-"] + rest, None)]
    c += _ignored(t, rest)
    t, rest = "filter-mask", ["ref.dam", "none", "out"]
    c += [(t, [], None), (t, ["--bogus"] + rest, None), (t, ["-Z"] + rest, None), (t, rest[:2], None), (t, rest + ["x"], None), (t, ["absent.dam", "m", "out"], None),
          (t, ["ref.dam", "absent", "out"], None), (t, rest, None), (t, ["--min-gap-size=5", "--min-interval-size=9"] + rest, None),
          (t, ["--min-gap-size", "5"] + rest, None), (t, ["--min-gap-size=x", "absent.dam", "m", "out"], None)]
    c += _strict(t, ["min-gap-size", "min-interval-size"], rest) + _ignored(t, rest)
    # ---- check-results
    t, rest = "check-results", ["ref.dam", "m", "reads.db", "absent.db"]
    ok = ["ref.dam", "m", "reads.db", "raw.db"]
    c += [(t, [], None), (t, ["--bogus"] + rest, None), (t, ["-Z"] + rest, None), (t, rest[:3], None), (t, rest + ["x"], None), (t, rest, None),
          (t, ["absent.dam", "m", "reads.db", "raw.db"], None), (t, ["ref.dam", "m", "absent.db", "raw.db"], None),
          (t, ["--crop-alignment=101"] + rest, None), (t, ["--crop-alignment=5", "--crop-ambiguous=4"] + rest, None),
          (t, ["--crop-alignment=5", "--crop-ambiguous=5"] + rest, None), (t, ["--gap-details-context=1"] + rest, None),
          (t, ["--gap-details-context=0", "-j", "--json"] + rest, None), (t, ["--crop-alignment=101", "--gap-details-context=1", "-v"] + rest, None),
          (t, ["--dust="] + rest, None), (t, ["--gap-details="] + rest, None), (t, ["--dust", "m"] + rest, None), (t, ["--json=1"] + rest, None),
          (t, ok, None), (t, ["--crop-ambiguous=10"] + ok, None), (t, ["--crop-alignment=10", "--crop-ambiguous=10"] + ok, None),
          (t, ["--crop-ambiguous=0", "ref.dam", "absent", "reads.db", "raw.db"], None), (t, ["--crop-ambiguous=0", "ref.dam", "m2", "reads.db", "raw.db"], None),
          (t, ["--crop-ambiguous=0", "--dust=absent", "--gap-details=d.json"] + ok, None), (t, ["--crop-ambiguous=0", "ref.dam", "m", "ref.dam", "raw.db"], None)]
    c += _strict(t, ["crop-alignment", "crop-ambiguous", "gap-details-context"], rest) + _ignored(t, rest)
    # ---- the aligners: everything that is refused before a device is asked for
    for t in ("daligner", "damapper", "datander"):
        c += [(t, [], None), (t, ["-Z", "ref.dam", "reads.db"], None), (t, ["--bogus", "ref.dam", "reads.db"], None),
              (t, ["-e0.5", "ref.dam", "reads.db"], None), (t, ["-e1", "ref.dam", "reads.db"], None), (t, ["-B4", "-b", "-p", "-z", "-H100", "-v"], None),
              (t, ["--mode"], None), (t, ["-k14", "-w6", "-h35", "-t10", "-s100", "-l500", "-%3", "-A", "-I", "-C", "-mdust", "-T4", "-Ptmp", "-M16"], None)]
    c += [("daligner", ["ref.dam"], None), ("damapper", ["ref.dam"], None), ("damapper", ["-n2", "-e.7", "ref.dam", "reads.db"], None),
          ("daligner", ["--mode", "damapper", "-n-1", "ref.dam", "reads.db"], None), ("daligner", ["--mode", "datander"], None),
          ("datander", ["--mode", "daligner", "ref.dam"], None)]
    return c


def _snapshot(d):
    snap = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            with open(p, "rb") as h:
                snap[os.path.relpath(p, d)] = h.read()
    return snap


def run_cases(tools, work):
    """Every case in a fresh copy of the prepared directory: exit code, stdout, stderr, and the bytes of every file the
    case wrote, changed (base64) or removed (None)."""
    base = os.path.join(work, "base")
    prepare(tools, base)
    before = _snapshot(base)
    def one(item):
        k, (tool, argv, stdin) = item
        cwd = os.path.join(work, "case%d" % k)
        shutil.copytree(base, cwd)
        data = None if stdin is None else before[stdin[1:]] if stdin.startswith("<") else stdin.encode()
        p = subprocess.run([os.path.join(tools, tool), *argv], input=data, stdin=None if data is not None else subprocess.DEVNULL, cwd=cwd,
                           capture_output=True, timeout=60)
        after = _snapshot(cwd)
        shutil.rmtree(cwd)
        files = {n: base64.b64encode(b).decode() for n, b in sorted(after.items()) if before.get(n) != b}
        files.update({n: None for n in sorted(before) if n not in after})
        return {"case": "%d: %s %s" % (k, tool, " ".join(argv)), "exit": p.returncode, "stdout": p.stdout.decode("utf-8", "replace"),
                "stderr": p.stderr.decode("utf-8", "replace"), "files": files}

    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(one, enumerate(cases())))


def dump(results, path):
    """The golden file: most of a recording is the same usage text and the same small files over and over, so every distinct
    line (of stdout, of stderr, and each file's base64 text) is stored once in "strings", and a case is
    [exit, stdout, stderr, files] with lists of indices into it; the case names are kept as one digest."""
    strings, index = [], {}

    def ref(text):
        return [index.setdefault(ln, len(index)) for ln in text.split("\n")]

    rows = [[r["exit"], ref(r["stdout"]), ref(r["stderr"]), {n: None if b is None else ref(b) for n, b in r["files"].items()}] for r in results]
    strings = sorted(index, key=index.get)
    names = hashlib.sha256("\n".join(r["case"] for r in results).encode()).hexdigest()
    cells = [json.dumps(r, separators=(",", ":"), sort_keys=True) for r in rows]  # (eight cases to a line)
    with open(path, "w") as f:
        f.write('{"table_sha256": "%s",\n"strings": [\n%s\n],\n"cases": [\n%s\n]}\n' % (
            names, ",\n".join(json.dumps(x) for x in strings), ",\n".join(",".join(cells[k:k + 8]) for k in range(0, len(cells), 8))))


def load(path):
    """The recording of `dump`, as run_cases returns it, with the case names of the present table (after checking that it is
    the recorded one)."""
    with open(path) as f:
        g = json.load(f)
    names = ["%d: %s %s" % (k, tool, " ".join(argv)) for k, (tool, argv, _) in enumerate(cases())]
    assert hashlib.sha256("\n".join(names).encode()).hexdigest() == g["table_sha256"], "the case table is not the recorded one"

    def text(refs):
        return "\n".join(g["strings"][i] for i in refs)

    return [{"case": c, "exit": r[0], "stdout": text(r[1]), "stderr": text(r[2]), "files": {n: None if b is None else text(b) for n, b in r[3].items()}}
            for c, r in zip(names, g["cases"])]
