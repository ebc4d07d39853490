"""What tests/seed_piletier_cases.py claims about its constructed ranges, checked on the oracle (no GPU): the candidate
lists worked out by hand are the oracle's, and nothing else has a candidate."""
import numpy as np

from oracle import pyoracle as oz
import seed_piletier_cases as pc
from test_parity_map_gpu import both_opts


def test_ranged_runs_are_what_the_oracle_finds():
    c = pc.ranged_runs()
    _, o = both_opts(**c["kw"])
    cand, ncand, nhits = oz.seed_candidates_all(c["A"], c["B"], o, with_nhits=True)
    assert sorted(np.flatnonzero(ncand).tolist()) == sorted(c["expect"])
    for it, want in c["expect"].items():
        got = [tuple(int(cand[it][j][f]) for f in ("score", "aseq", "apos", "bpos")) for j in range(ncand[it])]
        assert got == want, (it, got, want)
        # every hit of the item lies in the one range: 54 and 40 hits, both above the 16 of the serial walk
        assert nhits[it] == (54 if want[0][0] == 80 else 40), (it, int(nhits[it]))
