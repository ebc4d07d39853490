"""tools/propagate-mask: masks of a reference DAM carried to a reads DB through a .las and back through the transposed
records, as mask tracks on disk, against the restatement of the contract (tests/propagate_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
import propagate_cases as pc
import propagate_ref as pr
from test_tools_editpath_gpu import tool

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "propagate-mask")
NREF, NREADS, REF_LEN, READ_LEN, TS = 4, 12, 2400, 900, 100


def fasta(n, length, header, seed):
    rng = np.random.default_rng(seed)
    return "".join(f">{header(i)}\n{''.join('acgt'[c] for c in rng.integers(0, 4, length))}\n" for i in range(n))


def records(seed, na, alen, nb, blen):
    """random records of A sequences of alen bases against B sequences of blen bases, both strands"""
    rng = np.random.default_rng(seed)
    b = pc.Builder(TS)
    for i in range(40):
        tiles = int(rng.integers(1, 7))
        q = int(rng.integers(0, alen // TS - tiles))
        abpos, aepos = q * TS + int(rng.integers(0, TS // 2)), (q + tiles) * TS - int(rng.integers(0, TS // 2))
        bbases = rng.integers(TS - 10, TS + 11, tiles).tolist()
        b.record(int(rng.integers(0, na)), int(rng.integers(0, nb)), abpos, aepos, int(rng.integers(0, blen - sum(bbases))), bbases,
                 comp=bool(i & 1))
    case = b.case(ncontigs=na, nreads=nb)
    order = np.lexsort((case["las"]["abpos"], case["las"]["bread"], case["las"]["aread"]))
    return case["las"][order], case["trace"]


def random_mask(seed, n, length, per):
    rng = np.random.default_rng(seed)
    ptr, iv = [0], []
    for _ in range(n):
        cuts = np.sort(rng.choice(np.arange(0, length + 1), size=2 * per, replace=False))
        iv += [(int(x), int(y)) for x, y in cuts.reshape(-1, 2)]
        ptr.append(len(iv))
    return np.asarray(ptr, dtype=np.int64), np.asarray(iv, dtype=np.int32)


def united(masks, n):
    rows = pr.union([(c, int(b), int(e)) for ptr, iv in masks for c in range(n) for b, e in iv[ptr[c]:ptr[c + 1]]])
    return pr.arrays(rows, n)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pmask")
    tool("fasta2DAM", "-i", str(d / "ref.dam"), stdin=fasta(NREF, REF_LEN, lambda i: f"scaf{i}", 1))
    tool("fasta2DB", "-i", str(d / "reads.db"), stdin=fasta(NREADS, READ_LEN, lambda i: f"sim/{i + 1}/0_{READ_LEN} RQ=0.850", 2))
    tool("DBsplit", "-x20", str(d / "ref.dam"))
    tool("DBsplit", "-x20", str(d / "reads.db"))
    ma, mb = random_mask(3, NREF, REF_LEN, 5), random_mask(4, NREF, REF_LEN, 3)
    dentist_amd.dazz_write_mask(str(d / "ref.dam"), "a", *ma)
    dentist_amd.dazz_write_mask(str(d / "ref.dam"), "b", *mb)
    las, trace = records(5, NREF, REF_LEN, NREADS, READ_LEN)
    dentist_amd.las_write(str(d / "ref.reads.las"), las, trace, TS)
    return d, (ma, mb), las, trace


def read_mask(path, name):
    db = dentist_amd.DazzDb(str(path))
    ptr, iv = db.read_mask(name)
    return np.asarray(ptr), np.asarray(iv).reshape(-1, 2)


def test_reference_to_reads_and_back(files):
    d, masks, las, trace = files
    tool("propagate-mask", "-m", "a", "-m", "b", "ref.dam", "reads.db", "ref.reads.las", "a-reads", cwd=d)
    mask = united(masks, NREF)
    exp, stats = pr.propagate(las, trace, TS, mask[0], mask[1], [READ_LEN] * NREADS)
    eptr, eiv = pr.arrays(exp, NREADS)
    ptr, iv = read_mask(d / "reads.db", "a-reads")
    assert len(eiv) > 5 and np.array_equal(ptr, eptr) and np.array_equal(iv, eiv)
    # the reverse direction on a transposed record set: reads are the A side, the mask just written goes back to the reference
    back, btrace = records(6, NREADS, READ_LEN, NREF, REF_LEN)
    dentist_amd.las_write(str(d / "reads.ref.las"), back, btrace, TS)
    tool("propagate-mask", "--mask=a-reads", "-v", "-T4", "reads.db", "ref.dam", "reads.ref.las", "a-back", cwd=d)
    exp2, _ = pr.propagate(back, btrace, TS, eptr, eiv, [REF_LEN] * NREF)
    e2ptr, e2iv = pr.arrays(exp2, NREF)
    ptr2, iv2 = read_mask(d / "ref.dam", "a-back")
    assert len(e2iv) > 3 and np.array_equal(ptr2, e2ptr) and np.array_equal(iv2, e2iv)


def test_without_a_reads_db_the_reference_is_the_destination(files):
    d, masks, _, _ = files
    las, trace = records(7, NREF, REF_LEN, NREF, REF_LEN)
    dentist_amd.las_write(str(d / "ref.ref.las"), las, trace, TS)
    tool("propagate-mask", "-ma", "--quiet", "ref.dam", "ref.ref.las", "a-self", cwd=d)
    exp, _ = pr.propagate(las, trace, TS, masks[0][0], masks[0][1], [REF_LEN] * NREF)
    eptr, eiv = pr.arrays(exp, NREF)
    ptr, iv = read_mask(d / "ref.dam", "a-self")
    assert len(eiv) > 3 and np.array_equal(ptr, eptr) and np.array_equal(iv, eiv)


def test_unknown_option_and_missing_mask(files):
    d, _, _, _ = files
    r = subprocess.run([TOOL, "-m", "a", "--masks=b", "ref.dam", "reads.db", "ref.reads.las", "x"], cwd=d, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "usage" in r.stderr
    r = subprocess.run([TOOL, "-m", "absent", "ref.dam", "reads.db", "ref.reads.las", "x"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "absent" in r.stderr
