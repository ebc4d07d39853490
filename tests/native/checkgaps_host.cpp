// The lane code of the gap analysis (dentist_amd/csrc/dh_checkgaps.h) compiled for the CPU and played as the kernels of
// dh_checkgaps.hip play it: cg::bind_gap one lane per gap, the gather with 64 lanes striding over a pair's bytes, and k_cg_stats as
// a 64-lane wavefront -- chunks of 64 columns, ballots as 64-bit words built lane by lane, prefix counts as population counts below
// the lane, the carried counts, the early exits of pass 1 and the reductions.  The alignment is not this harness's: the caller
// hands in the ops of every aligned gap (tests/nwa_ref.py's) and says which pairs the aligner gave up.  Every buffer a kernel
// would index is a heap block of exactly its size, so the sanitizers see an overrun (checkgaps_host_main.cpp).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../dentist_amd/csrc/dh_checkgaps.h"
#include "../../include/dentist_hip.h"

static_assert(sizeof(CgSummary) == sizeof(dh_gap_summary) && sizeof(CgMap) == sizeof(dh_contig_mapping), "layouts");

namespace {

template <class F>
uint64_t ballot(F pred)
{
    uint64_t m = 0;
    for (int lane = 0; lane < 64; lane++)
        if (pred(lane)) m |= (uint64_t)1 << lane;
    return m;
}
inline int32_t below(uint64_t m, int lane) { return __builtin_popcountll(m & (((uint64_t)1 << lane) - 1)); }
inline int32_t pop(uint64_t m) { return __builtin_popcountll(m); }

// k_cg_stats for one gap: ops[0, n), the pair's bytes ref[0, rl) / qry[0, ql)
CgStats stats_wave(const CgSummary &s, const uint8_t *ops, int32_t n, const uint8_t *ref, int32_t rl, const uint8_t *qry, const int64_t *dust_ptr,
                   const int32_t *dust_iv, int32_t crop)
{
    int32_t cb = 0, ce = n, r_cb = 0, q_cb = 0;
    int32_t op[64], ri[64], qi[64];
    bool cr[64], cq[64];
    if (crop > 0) {
        CgCarry c = {0, 0, 0};
        for (int32_t c0 = 0; c0 < n; c0 += 64) {
            for (int l = 0; l < 64; l++) {
                const int32_t k = c0 + l;
                op[l] = k < n ? ops[k] : -1;
                cr[l] = k < n && op[l] != CG_OP_INS, cq[l] = k < n && op[l] != CG_OP_DEL;
            }
            const uint64_t mr = ballot([&](int l) { return cr[l]; }), mq = ballot([&](int l) { return cq[l]; });
            for (int l = 0; l < 64; l++) ri[l] = c.ref + below(mr, l), qi[l] = c.qry + below(mq, l);
            const uint64_t mb = ballot([&](int l) { return cr[l] && (cg::col_bits(op[l], ref[ri[l]], 0) & cg::COL_REF_BASE); });
            const uint64_t hit = ballot([&](int l) { return ((mb >> l) & 1) && c.bases + below(mb, l) + 1 == crop; });
            if (hit) {
                const int L = __builtin_ffsll((long long)hit) - 1;
                cb = c0 + L + 1, r_cb = ri[L] + 1, q_cb = qi[L] + (cq[L] ? 1 : 0);
                break;
            }
            c.ref += pop(mr), c.qry += pop(mq), c.bases += pop(mb);
        }
        c = CgCarry{0, 0, 0};
        for (int32_t c0 = 0; c0 < n; c0 += 64) {
            for (int l = 0; l < 64; l++) {
                const int32_t k = n - 1 - (c0 + l);
                op[l] = k >= 0 ? ops[k] : -1;
                cr[l] = k >= 0 && op[l] != CG_OP_INS;
            }
            const uint64_t mr = ballot([&](int l) { return cr[l]; });
            for (int l = 0; l < 64; l++) ri[l] = rl - 1 - (c.ref + below(mr, l));
            const uint64_t mb = ballot([&](int l) { return cr[l] && (cg::col_bits(op[l], ref[ri[l]], 0) & cg::COL_REF_BASE); });
            const uint64_t hit = ballot([&](int l) { return ((mb >> l) & 1) && c.bases + below(mb, l) + 1 == crop; });
            if (hit) {
                ce = n - 1 - (c0 + (__builtin_ffsll((long long)hit) - 1));
                break;
            }
            c.ref += pop(mr), c.bases += pop(mb);
        }
        if (ce < cb) ce = cb;
    }
    const bool dusty = dust_ptr != nullptr && s.state == CG_CLOSED;
    const int32_t *iv = nullptr;
    int64_t niv = 0;
    if (dusty) {
        iv = dust_iv + 2 * dust_ptr[s.true_contig - 1];
        niv = dust_ptr[s.true_contig] - dust_ptr[s.true_contig - 1];
    }
    const int32_t gap_lo = s.true_begin + crop, gap_hi = s.true_end - crop;
    CgStats out = {cb, ce, 0, 0, 0, 0, 0, 0, 0};
    CgCarry c = {r_cb, q_cb, 0};
    int32_t bits[64];
    for (int32_t c0 = cb; c0 < ce; c0 += 64) {
        for (int l = 0; l < 64; l++) {
            const int32_t k = c0 + l;
            op[l] = k < ce ? ops[k] : -1;
            cr[l] = k < ce && op[l] != CG_OP_INS, cq[l] = k < ce && op[l] != CG_OP_DEL;
        }
        const uint64_t mr = ballot([&](int l) { return cr[l]; }), mq = ballot([&](int l) { return cq[l]; });
        for (int l = 0; l < 64; l++) {
            ri[l] = c.ref + below(mr, l), qi[l] = c.qry + below(mq, l);
            bits[l] = c0 + l < ce ? cg::col_bits(op[l], cr[l] ? ref[ri[l]] : 0, cq[l] ? qry[qi[l]] : 0) : 0;
        }
        const uint64_t ma = ballot([&](int l) { return (bits[l] & cg::COL_ADVANCE) != 0; });
        for (int l = 0; l < 64; l++) {  // (the per-lane sums, reduced over the wavefront)
            const bool valid = c0 + l < ce, match = (bits[l] & cg::COL_MATCH) != 0;
            const int64_t ref_pos = (int64_t)gap_lo + c.bases + below(ma, l);
            out.matches += match;
            out.reference_length += (bits[l] & cg::COL_REF_BASE) != 0;
            out.query_length += (bits[l] & cg::COL_QRY_BASE) != 0;
            if (dusty && valid) {
                const bool d = cg::dust_col(iv, niv, gap_lo, gap_hi, ref_pos, op[l] == CG_OP_INS);
                out.dust_ops += d, out.dust_matches += d && match, out.none_dust_ops += !d, out.none_dust_matches += !d && match;
            }
        }
        c.ref += pop(mr), c.qry += pop(mq), c.bases += pop(ma);
    }
    return out;
}

template <class T>
std::unique_ptr<T[]> exact_copy(const T *p, size_t n)
{
    std::unique_ptr<T[]> b(new T[n]);
    if (n) memcpy(b.get(), p, sizeof(T) * n);
    return b;
}

}  // namespace

// Returns 0, or -1 with the refusal in msg (run_check != 0: the driver's checks first).  given_up[g] != 0: the aligner answered
// DH_NW_BAND_EXCEEDED for gap g.  op_off / ops: the ops of the aligned gaps (count + 1 offsets).  out_ref / out_qry: the gathered
// pairs one after the other (cap bytes each; -2 when they do not fit), out_len: 2 x count lengths.
extern "C" int32_t checkgaps_host(const uint8_t *true_bases, const int64_t *true_off, int32_t n_true, const uint8_t *res_bases, const int64_t *res_off,
                                  int32_t n_res, const int32_t *mapped, int32_t n_input, const dh_contig_mapping *maps, int32_t nmaps,
                                  const int32_t *result_gap, const int64_t *dust_ptr, const int32_t *dust_iv, int32_t crop, int32_t first_contig,
                                  int32_t count, int32_t run_check, const uint8_t *given_up, const int64_t *op_off, const uint8_t *ops,
                                  dh_gap_summary *out, int32_t *out_len, uint8_t *out_ref, uint8_t *out_qry, int64_t cap, char *msg, int32_t msg_cap)
{
    std::vector<CgMap> sm((size_t)nmaps);
    for (int32_t k = 0; k < nmaps; k++)
        sm[(size_t)k] = CgMap{maps[k].ref_contig, maps[k].ref_begin, maps[k].ref_end, maps[k].ref_contig_length, maps[k].query_contig,
                              maps[k].duplicate != 0, maps[k].complement != 0, k};
    if (run_check && cg::check(mapped, n_input, sm.data(), nmaps, true_off, n_true, res_off, n_res, dust_ptr, dust_iv, crop, first_contig, count, msg,
                               (size_t)msg_cap))
        return -1;
    std::stable_sort(sm.begin(), sm.end(), [](const CgMap &a, const CgMap &b) { return a.query < b.query; });
    // the device copies, each exactly as long as its array; the reverse complement as dh_ensure_rc lays it out
    const size_t tb = (size_t)true_off[n_true], rb = (size_t)res_off[n_res];
    auto d_true = exact_copy(true_bases, tb), d_res = exact_copy(res_bases, rb);
    std::unique_ptr<uint8_t[]> d_rc(new uint8_t[rb]);
    for (int32_t c = 0; c < n_res; c++)
        for (int64_t k = res_off[c], e = res_off[c + 1]; k < e; k++) {
            const uint8_t b = res_bases[res_off[c] + (e - 1 - k)];
            d_rc[(size_t)k] = b < 4 ? (uint8_t)(3 - b) : b;
        }
    auto d_mapped = exact_copy(mapped, 3 * (size_t)n_input);
    auto d_maps = exact_copy(sm.data(), (size_t)nmaps);
    auto d_gap = exact_copy(result_gap, (size_t)n_res);
    auto d_toff = exact_copy(true_off, (size_t)n_true + 1), d_roff = exact_copy(res_off, (size_t)n_res + 1);
    const int64_t ndust = dust_ptr ? dust_ptr[n_true] : 0;
    auto d_dptr = exact_copy(dust_ptr, dust_ptr ? (size_t)n_true + 1 : 0);
    auto d_div = exact_copy(dust_iv, 2 * (size_t)ndust);
    const CgEnv env{d_mapped.get(), d_maps.get(), d_gap.get(), d_roff.get(), n_input, nmaps, crop, first_contig};
    std::vector<CgSummary> sum((size_t)count);
    int64_t rat = 0, qat = 0;
    for (int32_t g = 0; g < count; g++) {
        int32_t rl, ql;
        cg::bind_gap(env, g, &sum[(size_t)g], &rl, &ql);
        CgSummary &s = sum[(size_t)g];
        out_len[2 * g] = rl, out_len[2 * g + 1] = ql;
        if (rl == 0) continue;
        if (rat + rl > cap || qat + ql > cap) return -2;
        std::unique_ptr<uint8_t[]> ref(new uint8_t[(size_t)rl]), qry(new uint8_t[(size_t)ql]);
        bool base = false;
        for (int lane = 0; lane < 64; lane++) {
            for (int32_t k = lane; k < rl; k += 64) ref[(size_t)k] = cg::ref_byte(s, d_true.get(), d_toff.get(), k);
            for (int32_t k = lane; k < ql; k += 64) {
                qry[(size_t)k] = cg::qry_byte(s, ql, d_res.get(), d_rc.get(), d_roff.get(), d_gap.get(), k);
                base |= qry[(size_t)k] < CG_N;
            }
        }
        memcpy(out_ref + rat, ref.get(), (size_t)rl);
        memcpy(out_qry + qat, qry.get(), (size_t)ql);
        rat += rl, qat += ql;
        if (!base)
            s.align_status = CG_ST_EMPTY;
        else if (given_up[g])
            s.align_status = CG_ST_BAND;
        else {
            const int32_t n = (int32_t)(op_off[g + 1] - op_off[g]);
            auto d_ops = exact_copy(ops + op_off[g], (size_t)n);
            const CgStats x = stats_wave(s, d_ops.get(), n, ref.get(), rl, qry.get(), dust_ptr ? d_dptr.get() : nullptr, d_div.get(), crop);
            s.col_begin = x.col_begin, s.col_end = x.col_end, s.matches = x.matches;
            if (crop > 0) s.reference_length = x.reference_length, s.query_length = x.query_length;
            s.dust_ops = x.dust_ops, s.dust_matches = x.dust_matches, s.none_dust_ops = x.none_dust_ops, s.none_dust_matches = x.none_dust_matches;
        }
    }
    memcpy(out, sum.data(), sizeof(CgSummary) * (size_t)count);
    return 0;
}
