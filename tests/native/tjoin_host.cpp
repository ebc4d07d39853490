// The slot code of the per-group table join (dentist_amd/csrc/dh_tjoin.h: home slot, insert, probe walk, the -t cap rule)
// compiled for the CPU and checked against a plain scan of the entry list.  Test infrastructure (tests/test_tjoin_host.py;
// tjoin_host_main.cpp is the stand-alone program for a sanitizer build).
#include <stdint.h>

#include <algorithm>
#include <vector>

#define DH_TJOIN_SLOT_CODE_ONLY
#include "../../dentist_amd/csrc/dh_tjoin.h"

namespace {
struct Rng {
    uint64_t s;
    uint32_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 32);
    }
};
}  // namespace

// n entries (canonical k-mer of `kbits` bits, orientation) drawn from `ndistinct` keys -- copies of a key included, and
// keys forced into one home slot when clash != 0 -- go into the table; every key and as many absent ones are then looked
// up with every (orientation, palindrome) and compared with a scan of the list: the entry numbers seen, the run counts
// and what the cap and the strands leave of them.  Returns the number of disagreements, -1 for arguments out of range.
extern "C" int64_t tjoin_host_check(int32_t n, int32_t ndistinct, int32_t kbits, int32_t clash, int32_t tcap, int32_t strands,
                                    uint64_t seed)
{
    if (n < 0 || n > TJ_CAP || ndistinct < 1 || kbits < 2 || kbits > 32) return -1;
    Rng rng{seed * 2654435761ull + 1};
    const uint32_t kmask = kbits == 32 ? 0xFFFFFFFFu : ((1u << kbits) - 1u);
    std::vector<uint32_t> keys((size_t)ndistinct);
    for (int32_t i = 0; i < ndistinct; i++) {
        uint32_t c = rng.next() & kmask;
        if (clash && i > 0) {  // (search a key with the home slot of key 0: long probe runs, wrap-around at the table's end)
            for (int t = 0; t < 200000 && tj_home(c) != tj_home(keys[0]); t++) c = rng.next() & kmask;
        }
        keys[(size_t)i] = c;
    }
    std::vector<uint32_t> ecanon((size_t)n), eori((size_t)n);
    std::vector<uint64_t> tab((size_t)TJ_SLOTS, TJ_EMPTY);
    for (int32_t e = 0; e < n; e++) {
        ecanon[(size_t)e] = keys[rng.next() % (uint32_t)ndistinct];
        eori[(size_t)e] = rng.next() & 1u;
        tj_insert(tab.data(), tj_slot(ecanon[(size_t)e], eori[(size_t)e], (uint32_t)e), [](uint64_t *p, uint64_t v) {
            if (*p != TJ_EMPTY) return false;
            *p = v;
            return true;
        });
    }
    int64_t filled = 0, bad = 0;
    for (uint64_t s : tab) filled += s != TJ_EMPTY;
    if (filled != n) bad++;
    for (int32_t i = 0; i < 2 * ndistinct; i++) {
        const uint32_t c = i < ndistinct ? keys[(size_t)i] : (rng.next() & kmask);
        std::vector<uint32_t> want;
        for (int32_t e = 0; e < n; e++)
            if (ecanon[(size_t)e] == c) want.push_back((eori[(size_t)e] << 31) | (uint32_t)e);
        std::vector<uint32_t> got;
        tj_walk(tab.data(), c, [&](uint32_t lo) { got.push_back(lo); });
        std::sort(want.begin(), want.end());
        std::sort(got.begin(), got.end());
        if (want != got) bad++;
        for (uint32_t bori = 0; bori < 2; bori++)
            for (int pal = 0; pal < 2; pal++) {
                int32_t runf = 0, runr = 0;
                for (uint32_t lo : want) {
                    const bool same = (lo >> 31) == bori;
                    runf += (same || pal) ? 1 : 0;
                    runr += (!same || pal) ? 1 : 0;
                }
                const bool dof = runf > 0 && runf <= tcap && (strands & 1), dor = runr > 0 && runr <= tcap && (strands & 2);
                const TjMatch m = tj_match(tab.data(), c, bori, pal != 0, tcap, strands);
                if (m.emit != ((dof ? 1u : 0u) | (dor ? 2u : 0u)) || m.fwd != (dof ? runf : 0) || m.rev != (dor ? runr : 0)) bad++;
            }
    }
    return bad;
}
