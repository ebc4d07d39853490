// dh_locate.h -- lane code and host planning of dh_exact_locate (kernels: dh_locate.hip, driver: dh_locate.cpp): every exact
// occurrence of every query, and of its reverse complement, in a reference of many records -- what the reference's
// external/fm-index.cpp answers for `dentist check-results` (commands/checkResults.d:511-565).  Compiles for the host as
// well (tests/native/locate_host.cpp), so that the CPU tests run the very expressions the kernels run.
//
// Text: all records concatenated, 2 bits per base, base g in bits 2 (g & 31) of 64-bit word g >> 5, LOC_TEXT_PAD zero words
// behind the last one.  A record boundary is not in the text: the starts of the records are an int64 array of nref + 1
// entries, and a match is kept only when its first and last base lie in one record (same_record).
// Patterns: pattern e = 2 * query + strand (strand 1: the reverse complement); each starts at a word of its own in the
// pattern words, one zero word behind the last.  A pattern of 32 bases or more is found by its anchor, the first 32 bases as
// one word: the anchors are sorted, equal ones form a group of consecutive members, and an open-addressing table (linear
// probing, a power of two of slots, load <= 1/4) maps an anchor to its group.  A pattern of 1..31 bases is one masked word.
//
// Why a reference word is always two loads and a funnel shift: a match starts at any base, so the 32 bases at position p
// straddle words p >> 5 and (p >> 5) + 1.  Shift 0 takes the first word alone (a shift by 64 is undefined); the second word
// is loaded all the same, which is why the buffers are padded instead of the last word being a special case.
#ifndef DH_LOCATE_H
#define DH_LOCATE_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define LOC_HD __host__ __device__ __forceinline__
#else
#define LOC_HD inline
#endif

#define LOC_TEXT_PAD 16        /* zero words behind the packed text and behind the pattern words */
#define LOC_INLINE_BASES 224   /* bases behind the anchor the scan compares before it writes a candidate */
#define LOC_BITMAP_BITS (1 << 18) /* the pre-filter in front of the table: one bit per hash value, 32 KiB of LDS */
#define LOC_SEG_DEFAULT (1 << 20)
#define LOC_CAND_CAP_DEFAULT (1 << 20)

struct LocPat {     // one pattern; len 0: not searched (empty, longer than the longest record, or the strand is not asked for)
    int64_t woff;   // first word in the pattern words
    int64_t len;    // bases
};
struct LocSlot {    // one slot of the anchor table; count 0: empty
    uint64_t key;
    uint32_t first, count;  // members [first, first + count) of the member list
};
struct LocCand {    // a candidate of the scan: pattern `pat` at text position `pos`
    int64_t pos;
    uint32_t pat;
    uint32_t ok;    // 1 when written; a verify unit that meets a mismatch stores 0
};
struct LocUnit {    // one wavefront of k_locate_verify: segment `seg` of candidate `cand`
    uint32_t cand, seg;
};
struct LocShort {   // a pattern of 1..31 bases
    uint64_t word;
    uint32_t len, pat;
};

namespace loc {

LOC_HD uint64_t hash(uint64_t key) { return key * 0x9E3779B97F4A7C15ull; }
LOC_HD uint32_t bitmap_index(uint64_t h) { return (uint32_t)(h >> 24) & (LOC_BITMAP_BITS - 1); }

// the 32 bases that start 2 * sh bits into word a (sh = 2 * (pos & 31)); shift 0 must not become a shift by 64
LOC_HD uint64_t funnel(uint64_t a, uint64_t b, uint32_t sh) { return sh ? (a >> sh) | (b << (64u - sh)) : a; }
LOC_HD uint64_t window(const uint64_t *text, int64_t pos)
{
    const int64_t w = pos >> 5;
    return funnel(text[w], text[w + 1], 2u * (uint32_t)(pos & 31));
}
// the bits of the first n bases of a word (n >= 1)
LOC_HD uint64_t tail_mask(int64_t n) { return n >= 32 ? ~0ull : (1ull << (2 * n)) - 1ull; }

// the record that holds text position pos (0 <= pos < starts[nref]): the last one that starts at or before pos.  Empty
// records in front of it share its start and sort before it.
LOC_HD int64_t record_of(const int64_t *starts, int64_t nref, int64_t pos)
{
    int64_t lo = 0, hi = nref;  // starts[lo] <= pos < starts[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (starts[mid] <= pos)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}
LOC_HD bool same_record(const int64_t *starts, int64_t nref, int64_t pos, int64_t len)
{
    return pos + len <= starts[record_of(starts, nref, pos) + 1];
}

// the group of an anchor: the pre-filter (bitmap, may be NULL), then linear probing
template <typename BitmapPtr>
LOC_HD bool probe(const LocSlot *table, int32_t tbits, BitmapPtr bitmap, uint64_t key, uint32_t &first, uint32_t &count)
{
    const uint64_t h = hash(key);
    if (bitmap) {
        const uint32_t b = bitmap_index(h);
        if (!((bitmap[b >> 5] >> (b & 31)) & 1u)) return false;
    }
    const uint32_t mask = (1u << tbits) - 1u;
    uint32_t s = (uint32_t)(h >> (64 - tbits));
    for (uint32_t n = 0; n <= mask; n++, s = (s + 1) & mask) {  // load <= 1/4: an empty slot ends every walk
        const LocSlot e = table[s];
        if (e.count == 0) return false;
        if (e.key == key) {
            first = e.first;
            count = e.count;
            return true;
        }
    }
    return false;
}

// what the scan does with one member of a hit group at text position pos (the anchor is known to match): the record test
// first, then the bases [32, 32 + LOC_INLINE_BASES) of the pattern, so that a low-complexity anchor does not flood the list
LOC_HD bool scan_member(const uint64_t *text, int64_t nbases, const int64_t *starts, int64_t nref, const uint64_t *pw, LocPat p,
                        int64_t pos)
{
    if (p.len < 32 || pos + p.len > nbases || !same_record(starts, nref, pos, p.len)) return false;
    const int64_t end = p.len < 32 + LOC_INLINE_BASES ? p.len : 32 + LOC_INLINE_BASES;
    for (int64_t b = 32; b < end; b += 32)
        if ((window(text, pos + b) ^ pw[p.woff + (b >> 5)]) & tail_mask(end - b)) return false;
    return true;
}

// word w of the segment [base0, base0 + nb) of pattern p against the text at pos: the bits that differ
LOC_HD uint64_t verify_word(const uint64_t *text, const uint64_t *pw, LocPat p, int64_t pos, int64_t base0, int64_t nb, int64_t w)
{
    const int64_t b = base0 + 32 * w;
    return (window(text, pos + b) ^ pw[p.woff + (b >> 5)]) & tail_mask(nb - 32 * w);
}

// a short pattern at the window of a text position
LOC_HD bool short_match(uint64_t win, LocShort s) { return ((win ^ s.word) & tail_mask((int64_t)s.len)) == 0; }

}  // namespace loc

// ------------------------------------------------------------------------------------------------ host planning

namespace loc {

// 8 codes (one per byte, each <= 3) to 16 bits, first code lowest
inline uint64_t squeeze8(uint64_t x)
{
    x = (x | (x >> 6)) & 0x000F000F000F000Full;
    x = (x | (x >> 12)) & 0x000000FF000000FFull;
    return (x | (x >> 24)) & 0xFFFFull;
}
// bases [b0, b0 + 32 * nw) of a sequence of n codes as nw words (bases past n are zero); rc: of its reverse complement.
// false: a code above 3.
inline bool pack_words(const uint8_t *src, int64_t n, int64_t b0, int64_t nw, bool rc, uint64_t *dst)
{
    bool ok = true;
    for (int64_t w = 0; w < nw; w++) {
        uint64_t out = 0;
        for (int q = 0; q < 4; q++) {
            const int64_t b = b0 + 32 * w + 8 * q;
            uint64_t x = 0;
            if (b + 8 <= n) {
                if (rc) {
                    memcpy(&x, src + (n - 8 - b), 8);
                    if (x & 0xFCFCFCFCFCFCFCFCull) ok = false;
                    x = 0x0303030303030303ull - (__builtin_bswap64(x) & 0x0303030303030303ull);
                } else {
                    memcpy(&x, src + b, 8);
                    if (x & 0xFCFCFCFCFCFCFCFCull) ok = false;
                    x &= 0x0303030303030303ull;
                }
            } else {
                for (int u = 0; u < 8 && b + u < n; u++) {
                    const uint8_t c = rc ? src[n - 1 - (b + u)] : src[b + u];
                    if (c > 3) ok = false;
                    x |= (uint64_t)((rc ? 3 - c : c) & 3) << (8 * u);
                }
            }
            out |= squeeze8(x) << (16 * q);
        }
        dst[w] = out;
    }
    return ok;
}

struct Plan {
    std::vector<LocPat> pats;     // 2 * nqry
    std::vector<uint64_t> pw;     // the pattern words, LOC_TEXT_PAD zero words at the end
    std::vector<uint32_t> memb;   // patterns of >= 32 bases, sorted by (anchor, pattern)
    std::vector<LocSlot> table;
    int32_t tbits = 4;
    std::vector<uint32_t> bitmap; // LOC_BITMAP_BITS bits
    std::vector<LocShort> shorts;
    int64_t bad_query = -1;       // first query with a code above 3
};

// Par: par(n, fn(lo, hi)) runs fn over disjoint chunks of [0, n)
template <typename Par>
inline void build_plan(const uint8_t *qry, const int64_t *qry_off, int64_t nqry, bool both, int64_t longest_record, Par &&par, Plan &pl)
{
    pl.pats.assign((size_t)(2 * nqry), LocPat{0, 0});
    int64_t words = 0;
    for (int64_t q = 0; q < nqry; q++) {
        const int64_t len = qry_off[q + 1] - qry_off[q];
        const bool searched = len > 0 && len <= longest_record;
        for (int s = 0; s < 2; s++) {
            LocPat &p = pl.pats[(size_t)(2 * q + s)];
            p.woff = words;
            if (searched && (s == 0 || both)) {
                p.len = len;
                words += ((len + 31) >> 5) + 1;
            }
        }
    }
    pl.pw.assign((size_t)(words + LOC_TEXT_PAD), 0);
    // every query is packed (and so checked), searched or not: a code above 3 is refused wherever it is
    std::vector<int64_t> bad;
    par(nqry, [&](int64_t lo, int64_t hi) {
        std::vector<uint64_t> tmp;
        for (int64_t q = lo; q < hi; q++) {
            const int64_t len = qry_off[q + 1] - qry_off[q], nw = (len + 31) >> 5;
            const uint8_t *src = qry + qry_off[q];
            bool ok = true;
            if (pl.pats[(size_t)(2 * q)].len) {
                ok = pack_words(src, len, 0, nw, false, pl.pw.data() + pl.pats[(size_t)(2 * q)].woff);
                if (pl.pats[(size_t)(2 * q + 1)].len) pack_words(src, len, 0, nw, true, pl.pw.data() + pl.pats[(size_t)(2 * q + 1)].woff);
            } else {
                tmp.resize((size_t)nw + 1);
                ok = pack_words(src, len, 0, nw, false, tmp.data());
            }
            if (!ok) {  // the smallest such query, whichever thread meets it
                int64_t cur = __atomic_load_n(&pl.bad_query, __ATOMIC_RELAXED);
                while ((cur < 0 || q < cur) && !__atomic_compare_exchange_n(&pl.bad_query, &cur, q, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
            }
        }
    });
    if (pl.bad_query >= 0) return;
    for (size_t e = 0; e < pl.pats.size(); e++) {
        const LocPat &p = pl.pats[e];
        if (p.len >= 32)
            pl.memb.push_back((uint32_t)e);
        else if (p.len > 0)
            pl.shorts.push_back(LocShort{pl.pw[(size_t)p.woff], (uint32_t)p.len, (uint32_t)e});
    }
    auto anchor = [&](uint32_t e) { return pl.pw[(size_t)pl.pats[e].woff]; };
    std::sort(pl.memb.begin(), pl.memb.end(), [&](uint32_t a, uint32_t b) {
        const uint64_t ka = anchor(a), kb = anchor(b);
        return ka != kb ? ka < kb : a < b;
    });
    size_t ngroups = 0;
    for (size_t i = 0; i < pl.memb.size(); i++) ngroups += i == 0 || anchor(pl.memb[i]) != anchor(pl.memb[i - 1]);
    pl.tbits = 4;
    while (((size_t)1 << pl.tbits) < 4 * ngroups) pl.tbits++;
    pl.table.assign((size_t)1 << pl.tbits, LocSlot{0, 0, 0});
    pl.bitmap.assign(LOC_BITMAP_BITS / 32, 0);
    const uint32_t mask = (1u << pl.tbits) - 1u;
    for (size_t i = 0, j; i < pl.memb.size(); i = j) {
        const uint64_t key = anchor(pl.memb[i]);
        for (j = i + 1; j < pl.memb.size() && anchor(pl.memb[j]) == key; j++) {}
        const uint64_t h = hash(key);
        uint32_t s = (uint32_t)(h >> (64 - pl.tbits));
        while (pl.table[s].count) s = (s + 1) & mask;
        pl.table[s] = LocSlot{key, (uint32_t)i, (uint32_t)(j - i)};
        const uint32_t b = bitmap_index(h);
        pl.bitmap[b >> 5] |= 1u << (b & 31);
    }
}

struct Hit {  // dh_exact_hit's layout
    int32_t query, ref;
    int64_t begin, end;
    int32_t complement, pad_;
};

// the surviving candidates as hits in the order of the contract: by query, the forward strand first, by text position
inline void finish(std::vector<LocCand> &cands, const Plan &pl, const int64_t *starts, int64_t nref, std::vector<Hit> &hits)
{
    std::sort(cands.begin(), cands.end(), [](const LocCand &a, const LocCand &b) { return a.pat != b.pat ? a.pat < b.pat : a.pos < b.pos; });
    hits.clear();
    hits.reserve(cands.size());
    for (const LocCand &c : cands) {
        const int64_t r = record_of(starts, nref, c.pos), len = pl.pats[c.pat].len;
        hits.push_back(Hit{(int32_t)(c.pat >> 1), (int32_t)r, c.pos - starts[r], c.pos - starts[r] + len, (int32_t)(c.pat & 1), 0});
    }
}

// the verify units of candidates [0, n): none for a pattern the scan has compared whole
inline void make_units(const LocCand *cands, int64_t n, const Plan &pl, int64_t seg, std::vector<LocUnit> &units)
{
    units.clear();
    for (int64_t c = 0; c < n; c++) {
        const int64_t len = pl.pats[cands[c].pat].len;
        if (len <= 32 + LOC_INLINE_BASES) continue;
        for (int64_t s = 0; s * seg < len; s++) units.push_back(LocUnit{(uint32_t)c, (uint32_t)s});
    }
}

inline int64_t round_seg(int64_t seg) { return seg < 32 ? 32 : (seg + 31) & ~(int64_t)31; }

}  // namespace loc

#endif
