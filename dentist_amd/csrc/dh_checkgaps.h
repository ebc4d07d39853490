// dh_checkgaps.h -- the gap analysis of `dentist check-results` (dh_check_gaps; commands/checkResults.d:822-1046, :1270-1462,
// :1986-2011, :2081-2089): the lane code of its kernels and the checks of its driver, compiled for the device (dh_checkgaps.hip),
// for the driver (dh_checkgaps.cpp) and for the CPU harness (tests/native/checkgaps_host.cpp).  No HIP header is needed.
//
//   bind_gap     one lane per gap: the mapped intervals of both input contigs, two binary searches in the mappings sorted by
//                input contig, the state, the insertion mapping and the lengths of the pair to align.
//   ref_byte, qry_byte
//                byte k of a pair's two sequences, from the DBs' bases and reverse complements; code 4 is the N-run.
//   col_bits     what one alignment column is: which sides it consumes, which of them are bases, a match, whether the dust
//                analysis' refPos advances behind it.
//   dust_col     whether the dust analysis counts a column as dust: a binary search per probe in the true contig's dust intervals,
//                clipped to the gap.
//   The kernels and the harness carry the prefix counts from one chunk of 64 columns to the next (CgCarry) and reduce the
//   counters over the wavefront; nothing here depends on an order between wavefronts.
//
// States and statuses are the public header's (DH_GAP_*, DH_CG_*); the driver asserts the equalities.
#ifndef DH_CHECKGAPS_H
#define DH_CHECKGAPS_H

#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define CG_HD __host__ __device__ __forceinline__
#else
#define CG_HD inline
#endif

#define CG_MAX_LEN 65536  // DH_NWA_MAX_LEN
#define CG_OP_MATCH 0     // EP_OP_*
#define CG_OP_DEL 1       // a reference base without a query base
#define CG_OP_INS 2       // a query base without a reference base
#define CG_OP_MISMATCH 3
#define CG_N 4            // the code of n

enum { CG_UNKOWN = 0, CG_BROKEN = 1, CG_UNCLOSED = 2, CG_PARTIAL = 3, CG_CLOSED = 4, CG_IGNORED = 5 };
enum { CG_ST_NONE = 0, CG_ST_OK = 1, CG_ST_EMPTY = 2, CG_ST_BAND = 3, CG_ST_LONG = 4 };

struct CgMap {  // dh_contig_mapping with the caller's index in place of the error
    int32_t ref_contig, ref_begin, ref_end, ref_len, query, duplicate, complement, index;
};
struct CgSummary {  // dh_gap_summary
    int32_t state, gap_length, lhs_map, rhs_map, align_status, complement;
    int32_t true_contig, true_begin, true_end;
    int32_t rb_contig, rb, re_contig, re;
    int32_t col_begin, col_end;
    int32_t reference_length, query_length, matches;
    int32_t dust_ops, dust_matches, none_dust_ops, none_dust_matches;
};
struct CgStats {  // what k_cg_stats writes for an aligned gap
    int32_t col_begin, col_end, reference_length, query_length, matches, dust_ops, dust_matches, none_dust_ops, none_dust_matches;
};
struct CgEnv {
    const int32_t *mapped;  // 3 x n_input
    const CgMap *maps;      // sorted by query (stable)
    const int32_t *result_gap;
    const int64_t *result_off;  // offsets of the result DB's sequences
    int32_t n_input, nmaps, crop, first_contig;
};

namespace cg {

// the mappings of input contig `c` that are no duplicates: their number, *at = the last of them
CG_HD int32_t find_mapping(const CgMap *maps, int32_t nmaps, int32_t c, int32_t *at)
{
    int32_t lo = 0, hi = nmaps;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (maps[mid].query < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    int32_t cnt = 0;
    for (; lo < nmaps && maps[lo].query == c; lo++)
        if (!maps[lo].duplicate) {
            cnt++;
            *at = lo;
        }
    return cnt;
}

// getGapState behind the complement swap (a, b: lhs and rhs, exchanged when lhs is complemented)
CG_HD int32_t state_of(const CgMap &a, const CgMap &b, int32_t crop, int32_t run)
{
    const bool same_strand = a.complement == b.complement;
    if (a.ref_contig == b.ref_contig && same_strand && a.ref_end <= b.ref_begin) return CG_CLOSED;
    const bool next = a.ref_contig + 1 == b.ref_contig && same_strand && run > 0;
    if (next && ((int64_t)a.ref_end + crop < a.ref_len || crop < b.ref_begin)) return CG_PARTIAL;
    if (next && (int64_t)a.ref_end + crop == a.ref_len && crop == b.ref_begin) return CG_UNCLOSED;
    return CG_BROKEN;
}

// gap i of the call; *rl / *ql: the lengths of the pair to align, 0 / 0 when there is none
CG_HD void bind_gap(const CgEnv &e, int32_t i, CgSummary *out, int32_t *rl, int32_t *ql)
{
    CgSummary s = {CG_IGNORED, 0, -1, -1, CG_ST_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    *rl = *ql = 0;
    const int32_t lhs = e.first_contig + i, rhs = lhs + 1;
    const int32_t lc = e.mapped[3 * (lhs - 1)], lend = e.mapped[3 * (lhs - 1) + 2];
    const int32_t rc = rhs > e.n_input ? 0 : e.mapped[3 * (rhs - 1)], rbeg = rhs > e.n_input ? 0 : e.mapped[3 * (rhs - 1) + 1];
    if (!(lc > 0 && lc == rc)) {
        *out = s;
        return;
    }
    s.gap_length = rbeg - lend;
    int32_t la = 0, ra = 0;
    if (find_mapping(e.maps, e.nmaps, lhs, &la) != 1 || find_mapping(e.maps, e.nmaps, rhs, &ra) != 1) {
        s.state = CG_UNKOWN;
        *out = s;
        return;
    }
    const CgMap lm = e.maps[la], rm = e.maps[ra];
    s.lhs_map = lm.index, s.rhs_map = rm.index;
    const CgMap &a = lm.complement ? rm : lm, &b = lm.complement ? lm : rm;
    const int32_t run = e.result_gap[a.ref_contig - 1];
    s.state = state_of(a, b, e.crop, run);
    if (s.state == CG_CLOSED || s.state == CG_PARTIAL) {
        s.complement = lm.complement;
        s.true_contig = lc, s.true_begin = lend - e.crop, s.true_end = rbeg + e.crop;
        s.rb_contig = a.ref_contig, s.rb = a.ref_end, s.re_contig = b.ref_contig, s.re = b.ref_begin;
        const int64_t R = (int64_t)s.true_end - s.true_begin;
        int64_t Q;
        bool only_n = false;
        if (s.rb_contig == s.re_contig)
            Q = (int64_t)s.re - s.rb;
        else {
            const int64_t left = e.result_off[s.rb_contig] - e.result_off[s.rb_contig - 1] - s.rb;
            Q = left + run + s.re;
            only_n = left == 0 && s.re == 0;
        }
        if (R == 0 || Q == 0 || only_n)
            s.align_status = CG_ST_EMPTY;
        else if (R > CG_MAX_LEN || Q > CG_MAX_LEN)
            s.align_status = CG_ST_LONG;
        else {
            s.align_status = CG_ST_OK;
            *rl = (int32_t)R, *ql = (int32_t)Q;
        }
        // an alignment without lines: the lengths of the FASTA records, which cropReference (crop > 0 only) counts again -- as 0
        if (e.crop == 0) {
            s.reference_length = (int32_t)(R > INT32_MAX ? INT32_MAX : R);
            s.query_length = (int32_t)(Q > INT32_MAX ? INT32_MAX : Q);
        }
    }
    *out = s;
}

CG_HD uint8_t ref_byte(const CgSummary &s, const uint8_t *true_bases, const int64_t *true_off, int32_t k)
{
    return true_bases[true_off[s.true_contig - 1] + s.true_begin + k];
}

// the query: result[rb_contig][rb ..] (+ the N-run + result[re_contig][.. re)), reverse-complemented under `complement`
CG_HD uint8_t qry_byte(const CgSummary &s, int32_t ql, const uint8_t *res_bases, const uint8_t *res_rc, const int64_t *res_off,
                       const int32_t *result_gap, int32_t k)
{
    const int32_t p = s.complement ? ql - 1 - k : k;  // position in the forward query
    const int64_t ob = res_off[s.rb_contig - 1], lb = res_off[s.rb_contig] - ob;
    int32_t contig_off;  // position in its result contig
    int64_t o, len;
    if (s.rb_contig == s.re_contig) {
        o = ob, len = lb, contig_off = s.rb + p;
    } else {
        const int32_t left = (int32_t)(lb - s.rb), run = result_gap[s.rb_contig - 1];
        if (p < left)
            o = ob, len = lb, contig_off = s.rb + p;
        else if (p < left + run)
            return CG_N;
        else
            o = res_off[s.re_contig - 1], len = res_off[s.re_contig] - o, contig_off = p - left - run;
    }
    return s.complement ? res_rc[o + len - 1 - contig_off] : res_bases[o + contig_off];
}

enum { COL_REF = 1, COL_QRY = 2, COL_REF_BASE = 4, COL_QRY_BASE = 8, COL_MATCH = 16, COL_ADVANCE = 32 };
// rb / qb: the bytes the column consumes (ignored where it consumes none)
CG_HD int32_t col_bits(int32_t op, uint8_t rb, uint8_t qb)
{
    int32_t f = 0;
    if (op != CG_OP_INS) f |= COL_REF | (rb < CG_N ? COL_REF_BASE : 0);
    if (op != CG_OP_DEL) f |= COL_QRY | (qb < CG_N ? COL_QRY_BASE : 0);
    if (op == CG_OP_MATCH) f |= COL_MATCH;
    if (op == CG_OP_MATCH || op == CG_OP_MISMATCH || (f & COL_REF_BASE)) f |= COL_ADVANCE;
    return f;
}

// p in (dust & [lo, hi)); iv: the n sorted, disjoint intervals of the true contig
CG_HD bool in_dust(const int32_t *iv, int64_t n, int32_t lo, int32_t hi, int64_t p)
{
    if (p < lo || p >= hi) return false;
    int64_t a = 0, b = n;  // the first interval that ends behind p
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (iv[2 * mid + 1] <= p)
            a = mid + 1;
        else
            b = mid;
    }
    return a < n && iv[2 * a] <= p;
}
CG_HD bool dust_col(const int32_t *iv, int64_t n, int32_t lo, int32_t hi, int64_t ref_pos, bool insertion)
{
    return in_dust(iv, n, lo, hi, ref_pos) || (insertion && (in_dust(iv, n, lo, hi, ref_pos - 1) || in_dust(iv, n, lo, hi, ref_pos + 1)));
}

// ---------------------------------------------------------------------------------------------------- the driver's checks
// what dh_check_gaps refuses behind "bad argument": NULL when all is well, else the text in `msg`
inline const char *check(const int32_t *mapped, int32_t n_input, const CgMap *maps, int32_t nmaps, const int64_t *true_off, int32_t n_true,
                         const int64_t *res_off, int32_t n_res, const int64_t *dust_ptr, const int32_t *dust_iv, int32_t crop,
                         int32_t first_contig, int32_t count, char *msg, size_t cap)
{
    if (count > 0 && (first_contig < 1 || (int64_t)first_contig + count - 1 > n_input)) {
        snprintf(msg, cap, "gaps %d .. %lld leave the %d input contigs", first_contig, (long long)first_contig + count - 1, n_input);
        return msg;
    }
    for (int32_t c = 0; c < n_input; c++) {
        const int32_t t = mapped[3 * c], b = mapped[3 * c + 1], e = mapped[3 * c + 2];
        if (t < 0 || t > n_true) {
            snprintf(msg, cap, "input contig %d: true contig %d out of range", c + 1, t);
            return msg;
        }
        if (t == 0) continue;
        if (b < 0 || e < b || e > true_off[t] - true_off[t - 1]) {
            snprintf(msg, cap, "input contig %d: mapped interval [%d, %d) outside true contig %d", c + 1, b, e, t);
            return msg;
        }
        if (c > 0 && mapped[3 * (c - 1)] == t) {
            if (b <= mapped[3 * (c - 1) + 2]) {
                snprintf(msg, cap, "input contig %d: mapped interval not behind the one before it with a base between them", c + 1);
                return msg;
            }
            if ((int64_t)mapped[3 * (c - 1) + 2] - crop < 0 || (int64_t)b + crop > true_off[t] - true_off[t - 1]) {
                snprintf(msg, cap, "input contig %d: the true interval of the gap in front of it leaves true contig %d", c + 1, t);
                return msg;
            }
        }
    }
    for (int32_t k = 0; k < nmaps; k++) {
        const CgMap &m = maps[k];
        if (m.query < 1 || m.query > n_input) {
            snprintf(msg, cap, "mapping %d: input contig %d out of range", m.index, m.query);
            return msg;
        }
        if (m.ref_contig < 1 || m.ref_contig > n_res) {
            snprintf(msg, cap, "mapping %d: result contig %d out of range", m.index, m.ref_contig);
            return msg;
        }
        const int64_t len = res_off[m.ref_contig] - res_off[m.ref_contig - 1];
        if (m.ref_begin < 0 || m.ref_end < m.ref_begin || m.ref_end > len) {
            snprintf(msg, cap, "mapping %d: [%d, %d) outside result contig %d", m.index, m.ref_begin, m.ref_end, m.ref_contig);
            return msg;
        }
        if (m.ref_len != len) {
            snprintf(msg, cap, "mapping %d: ref_contig_length %d is not the length of result contig %d", m.index, m.ref_len, m.ref_contig);
            return msg;
        }
    }
    if (dust_ptr)
        for (int32_t t = 0; t < n_true; t++) {
            if (dust_ptr[t] < 0 || dust_ptr[t + 1] < dust_ptr[t]) {
                snprintf(msg, cap, "dust mask: offsets decrease at true contig %d", t + 1);
                return msg;
            }
            for (int64_t k = dust_ptr[t]; k < dust_ptr[t + 1]; k++)
                if (dust_iv[2 * k] < 0 || dust_iv[2 * k + 1] < dust_iv[2 * k] || dust_iv[2 * k + 1] > true_off[t + 1] - true_off[t] ||
                    (k > dust_ptr[t] && dust_iv[2 * k] < dust_iv[2 * k - 1])) {
                    snprintf(msg, cap, "dust mask: interval %lld of true contig %d is not sorted, disjoint and inside the contig",
                             (long long)(k - dust_ptr[t]), t + 1);
                    return msg;
                }
        }
    return nullptr;
}

}  // namespace cg

// what a wavefront carries from one chunk of 64 columns to the next
struct CgCarry {
    int32_t ref, qry;  // bytes consumed in front of the chunk
    int32_t bases;     // pass 1: reference bases seen; pass 2: advances of refPos
};

#endif
