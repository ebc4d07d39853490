"""tools/check-results on a small .dam trio built with fasta2DAM from a scene of tests/checkgaps_cases.py (closed, unclosed and
partially closed gaps on two scaffolds, a dust mask): the JSON stats and the --gap-details lines, parsed, against the binding
(contig_mappings + Context.check_gaps) and against the stats' definitions written out here; the text form; the options that are
accepted and ignored; the refusals and their exit codes."""
import json
import os
import subprocess
import types

import numpy as np
import pytest

import dentist_amd
import checkgaps_cases as cc
import checkgaps_ref as cr
from test_tools_editpath_gpu import tool

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP = 10
DUST = {1: [(380, 420), (1190, 1230)], 2: [(450, 520)]}


def scene():
    first = (3000, [(100, 400), (500, 900), (1150, 1500), (1700, 2100), (2300, 2700)], [cc.closed(div=0.06), cc.closed(), cc.unclosed(33), cc.partial(40, 50, run=21)])
    second = (1500, [(50, 400), (520, 900), (1000, 1450)], [cc.closed(div=0.1), cc.closed(div=0.02)])
    return cc.build(21, CROP, [first, second], dust=DUST)


def text(codes):
    return "".join("acgt"[c] for c in codes)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("checkresults")
    s = scene()
    true_fa = "".join(f">true{t}\n{text(x)}\n" for t, x in enumerate(s["true_seqs"]))
    ref_fa = ""
    for t, x in enumerate(s["true_seqs"]):
        ivs = [(b, e) for c, b, e in s["mapped"] if c == t + 1]
        ref_fa += f">input{t}\n" + "".join(text(x[b:e]) + "n" * (ivs[k + 1][0] - e if k + 1 < len(ivs) else 0) for k, (b, e) in enumerate(ivs)) + "\n"
    res_fa, open_ = "", False
    for k, x in enumerate(s["result_seqs"]):
        res_fa += ("" if open_ else f">result{k}\n") + text(x) + "n" * s["result_gap"][k]
        open_ = s["result_gap"][k] > 0
        res_fa += "" if open_ else "\n"
    for name, fa, cutoff in (("true", true_fa, 20), ("ref", ref_fa, 250), ("result", res_fa, 20)):
        tool("fasta2DAM", "-i", str(d / f"{name}.dam"), stdin=fa)
        tool("DBsplit", f"-x{cutoff}", str(d / f"{name}.dam"))
    n_true = len(s["true_seqs"])
    ptr = np.zeros(n_true + 1, np.int64)
    for c, _, _ in s["mapped"]:
        ptr[c:] += 1
    dentist_amd.dazz_write_mask(str(d / "true.dam"), "mapped", ptr, np.asarray([x for _, b, e in s["mapped"] for x in (b, e)], np.int32))
    dp, di = cc.dust_arrays(DUST, n_true)
    dentist_amd.dazz_write_mask(str(d / "true.dam"), "lc", dp, di[:-2])
    return d, s


@pytest.fixture(scope="module")
def report(files, gpu_ctx):
    d, s = files
    ref_seqs = [s["true_seqs"][c - 1][b:e] for c, b, e in s["mapped"]]
    maps = dentist_amd.contig_mappings(gpu_ctx, ref_seqs, s["result_seqs"], CROP, 100)
    assert sorted((m["query_contig"], m["ref_contig"], m["ref_begin"], m["ref_end"], m["complement"]) for m in maps) == \
        sorted((m["query_contig"], m["ref_contig"], m["ref_begin"], m["ref_end"], m["complement"]) for m in s["maps"]) and not maps["duplicate"].any()

    def db(seqs):
        off = np.zeros(len(seqs) + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in seqs])
        return dentist_amd.Db(gpu_ctx, types.SimpleNamespace(bases=np.concatenate(seqs).astype(np.uint8), off=off))
    dp, di = cc.dust_arrays(DUST, len(s["true_seqs"]))
    return gpu_ctx.check_gaps(db(s["true_seqs"]), db(s["result_seqs"]), s["mapped"], maps, s["result_gap"], dust=(dp, di[:-2]), crop=CROP), maps


def run(d, *opts):
    return tool("check-results", *opts, "true.dam", "mapped", "ref.dam", "result.dam", cwd=d)


def test_json_stats_and_gap_details_against_the_binding(files, report):
    d, s = files
    rep, maps = report
    stats = json.loads(run(d, "--json", f"--crop-alignment={CROP}", "--dust=lc", "--gap-details=gaps.json"))
    g = rep.summaries
    live = g["state"] != cr.IGNORED
    closed = g["state"] == cr.CLOSED
    assert [cr.STATE_NAMES[x] for x in g["state"]] == ["closed", "closed", "unclosed", "partiallyClosed", "ignored", "closed", "closed", "ignored"]
    lens = np.asarray([e - b for _, b, e in s["mapped"]])
    scaffolds = [2700 - 100, 1450 - 50]

    def n50(v, total):
        cum = 0
        for x in sorted(v, reverse=True):
            cum += x
            if cum >= 0.5 * total:
                return x
        return 0
    exp = {"numContigsExpected": 8, "numMappedContigs": 8, "numClosedGaps": int(closed.sum()), "numPartiallyClosedGaps": 1,
           "numCorrectGaps": int((rep.identity[closed] >= 1.0).sum()), "numBpsExpected": sum(scaffolds), "numBpsKnown": int(lens.sum()),
           "numBpsResult": sum(len(x) for x in s["result_seqs"]), "numBpsInGaps": int(g["gap_length"][live].sum()),
           "maximumN50": n50(scaffolds, sum(scaffolds)), "inputN50": n50(lens, sum(scaffolds)),
           "resultN50": n50([len(x) for x in s["result_seqs"]], sum(scaffolds)), "gapMedian": int(sum(sorted(g["gap_length"][live])[2:4]) // 2),
           "closedGapMedian": int(sum(sorted(g["gap_length"][closed])[1:3]) // 2), "minClosedGap": int(g["gap_length"][closed].min()),
           "maxClosedGap": int(g["gap_length"][closed].max())}
    assert exp["numCorrectGaps"] >= 1 and live.sum() == 6 and closed.sum() == 4
    avg = stats.pop("averageInsertionError")
    assert stats == exp
    assert avg is None    # the unclosed gap's identity is NaN, and the weighted mean carries it (NaN has no JSON text)
    lines = [json.loads(x) for x in open(d / "gaps.json").read().splitlines()]
    assert [x["leftContig"] for x in lines] == [int(k) + 1 for k in np.flatnonzero(live)]
    for x in lines:
        k = x["leftContig"] - 1
        assert set(x) == {"leftContig", "rightContig", "state", "gapLength", "details", "sequence"} and x["sequence"] is None
        assert (x["rightContig"], x["state"], x["gapLength"]) == (k + 2, cr.STATE_NAMES[g["state"][k]], g["gap_length"][k])
        if g["state"][k] not in (cr.CLOSED, cr.PARTIALLY_CLOSED):
            assert x["details"] is None
            continue
        det = x["details"]
        assert set(det) == {"referenceLength", "queryLength", "complement", "percentIdentity", "dustPercentIdentity", "noneDustPercentIdentity", "alignment"}
        assert (det["referenceLength"], det["queryLength"], det["complement"]) == (g["reference_length"][k], g["query_length"][k], False)
        assert det["percentIdentity"] == rep.identity[k]
        if g["state"][k] == cr.CLOSED:
            assert det["dustPercentIdentity"] == (g["dust_matches"][k] / g["dust_ops"][k] if g["dust_ops"][k] else None)
            assert det["noneDustPercentIdentity"] == g["none_dust_matches"][k] / g["none_dust_ops"][k]
        else:
            assert det["dustPercentIdentity"] is None and det["noneDustPercentIdentity"] is None
        an = cr.Analyzer(s["true_seqs"], s["result_seqs"], s["mapped"], s["maps"], s["result_gap"], None, CROP)
        ref = s["true_seqs"][g["true_contig"][k] - 1][g["true_begin"][k]:g["true_end"][k]]
        qry = an.result_subseq((g["result_begin_contig"][k], g["result_begin"][k]), (g["result_end_contig"][k], g["result_end"][k]))
        assert det["alignment"] == [line[g["col_begin"][k]:g["col_end"][k]] for line in cr.lines_of(ref, qry, rep.ops_of(k))]
    assert any(x["details"] and x["details"]["dustPercentIdentity"] is not None for x in lines)


def test_text_form_and_ignored_options(files):
    d, _ = files
    out = run(d, f"--crop-alignment={CROP}", "--dust=lc", "-v", "-T4", "--config=none.yaml")
    rows = dict(line.split(":") for line in out.splitlines())
    assert int(rows["numClosedGaps"]) == 4 and int(rows["numContigsExpected"]) == 8 and rows["averageInsertionError"].strip() == "nan"
    # without --dust the default track `dust` is used when it exists; here it does not, and the call still succeeds
    assert json.loads(run(d, "--json"))["numClosedGaps"] == 4


@pytest.mark.parametrize("opts,code,words", [
    (["--frobnicate"], 1, "unknown option"), (["--gap-details-context=5"], 1, "only 0 is served"),
    (["--crop-alignment=120"], 1, "must be <= --crop-ambiguous"), (["--crop-ambiguous=125"], 2, "below the contig cutoff of 250"),
    (["--dust=missing"], 2, "missing")])
def test_refusals(files, opts, code, words):
    d, _ = files
    r = subprocess.run([os.path.join(ROOT, "tools", "check-results"), *opts, "true.dam", "mapped", "ref.dam", "result.dam"], cwd=d, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == code and words in r.stderr, r.stderr


def test_usage(files):
    d, _ = files
    r = subprocess.run([os.path.join(ROOT, "tools", "check-results"), "true.dam", "mapped"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "usage: check-results" in r.stderr
