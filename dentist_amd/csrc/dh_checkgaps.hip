// dh_checkgaps.hip -- the kernels of dh_check_gaps (lane code and layouts: dh_checkgaps.h; driver: dh_checkgaps.cpp).  gfx950, wave64.
//
//   k_cg_bind     one lane per gap: state, insertion mapping, pair lengths (cg::bind_gap); lane `count` writes the 0 behind the last
//                 length, so that the exclusive scans (dhk_scan) leave count + 1 offsets.
//   k_cg_gather   one wavefront per pair: both sequences as byte codes, at their offsets behind NW_SEQ_PAD bytes, and whether the
//                 query has a base at all (a ballot).
//   k_cg_stats    one wavefront per aligned gap.  The ops go through in chunks of 64 columns; the bytes a column consumes are found
//                 by prefix counts over the wavefront (a ballot and a population count: the flags are single bits) on top of the
//                 counts carried from the chunks before.  Pass 1 (crop > 0) looks for the column of reference base #crop from the
//                 front, then from the back, and stops at the chunk that holds it; pass 2 counts matches, bases and the dust
//                 counters over the kept columns and reduces them over the wavefront.  Lane 0 writes the nine results.
//   No atomics; every gap is written by the one wavefront that owns it.
#include <hip/hip_runtime.h>

#include "dh_checkgaps.h"
#include "dh_nw.h"

#define CG_BLOCK 256
#define CG_WAVES (CG_BLOCK / 64)

__global__ __launch_bounds__(CG_BLOCK) void k_cg_bind(CgEnv e, int32_t count, CgSummary *sum, uint32_t *rlen, uint32_t *qlen)
{
    const int32_t i = (int32_t)(blockIdx.x * CG_BLOCK + threadIdx.x);
    if (i > count) return;
    if (i == count) {
        rlen[i] = qlen[i] = 0;
        return;
    }
    int32_t rl, ql;
    cg::bind_gap(e, i, sum + i, &rl, &ql);
    rlen[i] = (uint32_t)rl;
    qlen[i] = (uint32_t)ql;
}

__global__ __launch_bounds__(CG_BLOCK) void k_cg_gather(const CgSummary *__restrict__ sum, int32_t count, const uint32_t *__restrict__ roff,
                                                        const uint32_t *__restrict__ qoff, const uint8_t *__restrict__ true_bases,
                                                        const int64_t *__restrict__ true_off, const uint8_t *__restrict__ res_bases,
                                                        const uint8_t *__restrict__ res_rc, const int64_t *__restrict__ res_off,
                                                        const int32_t *__restrict__ result_gap, uint8_t *__restrict__ ref,
                                                        uint8_t *__restrict__ qry, uint32_t *__restrict__ has_base)
{
    const int32_t g = (int32_t)(blockIdx.x * CG_WAVES + (threadIdx.x >> 6)), lane = (int32_t)(threadIdx.x & 63);
    if (g >= count) return;
    const int32_t rl = (int32_t)(roff[g + 1] - roff[g]), ql = (int32_t)(qoff[g + 1] - qoff[g]);
    if (rl == 0) return;
    const CgSummary s = sum[g];
    uint8_t *r = ref + NW_SEQ_PAD + roff[g], *q = qry + NW_SEQ_PAD + qoff[g];
    for (int32_t k = lane; k < rl; k += 64) r[k] = cg::ref_byte(s, true_bases, true_off, k);
    bool base = false;  // the reference returns early from a query that is all n
    for (int32_t k = lane; k < ql; k += 64) {
        const uint8_t b = cg::qry_byte(s, ql, res_bases, res_rc, res_off, result_gap, k);
        q[k] = b;
        base |= b < CG_N;
    }
    const uint64_t any = __ballot(base);
    if (lane == 0) has_base[g] = any != 0;
}

__device__ __forceinline__ int32_t wave_sum(int32_t v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(CG_BLOCK) void k_cg_stats(const CgSummary *__restrict__ sum, int32_t count, const uint32_t *__restrict__ roff,
                                                       const uint32_t *__restrict__ qoff, const uint8_t *__restrict__ refs,
                                                       const uint8_t *__restrict__ qrys, const int64_t *__restrict__ op_off,
                                                       const uint8_t *__restrict__ all_ops, const int64_t *__restrict__ dust_ptr,
                                                       const int32_t *__restrict__ dust_iv, int32_t crop, CgStats *__restrict__ out)
{
    const int32_t g = (int32_t)(blockIdx.x * CG_WAVES + (threadIdx.x >> 6)), lane = (int32_t)(threadIdx.x & 63);
    if (g >= count) return;
    const int32_t n = (int32_t)(op_off[g + 1] - op_off[g]);
    if (n == 0) return;  // (the driver has answered the gap)
    const uint8_t *ops = all_ops + op_off[g], *ref = refs + NW_SEQ_PAD + roff[g], *qry = qrys + NW_SEQ_PAD + qoff[g];
    const int32_t rl = (int32_t)(roff[g + 1] - roff[g]);
    const CgSummary s = sum[g];
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    int32_t cb = 0, ce = n, r_cb = 0, q_cb = 0;
    if (crop > 0) {
        CgCarry c = {0, 0, 0};
        for (int32_t c0 = 0; c0 < n; c0 += 64) {
            const int32_t k = c0 + lane;
            const bool valid = k < n;
            const int32_t op = valid ? ops[k] : -1;
            const bool cr = valid && op != CG_OP_INS, cq = valid && op != CG_OP_DEL;
            const uint64_t mr = __ballot(cr), mq = __ballot(cq);
            const int32_t ri = c.ref + __popcll(mr & below), qi = c.qry + __popcll(mq & below);
            const bool base = cr && (cg::col_bits(op, ref[ri], 0) & cg::COL_REF_BASE);
            const uint64_t mb = __ballot(base);
            const uint64_t hit = __ballot(base && c.bases + __popcll(mb & below) + 1 == crop);
            if (hit) {
                const int32_t L = __ffsll((unsigned long long)hit) - 1;
                cb = c0 + L + 1;
                r_cb = __shfl(ri, L, 64) + 1;
                q_cb = __shfl(qi + (cq ? 1 : 0), L, 64);
                break;
            }
            c.ref += __popcll(mr), c.qry += __popcll(mq), c.bases += __popcll(mb);
        }
        c = CgCarry{0, 0, 0};
        for (int32_t c0 = 0; c0 < n; c0 += 64) {
            const int32_t k = n - 1 - (c0 + lane);
            const bool valid = k >= 0;
            const int32_t op = valid ? ops[k] : -1;
            const bool cr = valid && op != CG_OP_INS;
            const uint64_t mr = __ballot(cr);
            const int32_t ri = rl - 1 - (c.ref + __popcll(mr & below));
            const bool base = cr && (cg::col_bits(op, ref[ri], 0) & cg::COL_REF_BASE);
            const uint64_t mb = __ballot(base);
            const uint64_t hit = __ballot(base && c.bases + __popcll(mb & below) + 1 == crop);
            if (hit) {
                ce = n - 1 - (c0 + (__ffsll((unsigned long long)hit) - 1));
                break;
            }
            c.ref += __popcll(mr), c.bases += __popcll(mb);
        }
        if (ce < cb) ce = cb;  // (fewer than 2 crop bases: not with a reference of bases)
    }
    const bool dusty = dust_ptr != nullptr && s.state == CG_CLOSED;
    const int32_t *iv = nullptr;
    int64_t niv = 0;
    if (dusty) {
        iv = dust_iv + 2 * dust_ptr[s.true_contig - 1];
        niv = dust_ptr[s.true_contig] - dust_ptr[s.true_contig - 1];
    }
    const int32_t gap_lo = s.true_begin + crop, gap_hi = s.true_end - crop;
    int32_t matches = 0, rbases = 0, qbases = 0, d_ops = 0, d_m = 0, n_ops = 0, n_m = 0;
    CgCarry c = {r_cb, q_cb, 0};
    for (int32_t c0 = cb; c0 < ce; c0 += 64) {
        const int32_t k = c0 + lane;
        const bool valid = k < ce;
        const int32_t op = valid ? ops[k] : -1;
        const bool cr = valid && op != CG_OP_INS, cq = valid && op != CG_OP_DEL;
        const uint64_t mr = __ballot(cr), mq = __ballot(cq);
        const int32_t ri = c.ref + __popcll(mr & below), qi = c.qry + __popcll(mq & below);
        const int32_t bits = valid ? cg::col_bits(op, cr ? ref[ri] : 0, cq ? qry[qi] : 0) : 0;
        const uint64_t ma = __ballot((bits & cg::COL_ADVANCE) != 0);
        const int64_t ref_pos = (int64_t)gap_lo + c.bases + __popcll(ma & below);
        const bool match = (bits & cg::COL_MATCH) != 0;
        matches += match;
        rbases += (bits & cg::COL_REF_BASE) != 0;
        qbases += (bits & cg::COL_QRY_BASE) != 0;
        if (dusty && valid) {
            const bool d = cg::dust_col(iv, niv, gap_lo, gap_hi, ref_pos, op == CG_OP_INS);
            d_ops += d, d_m += d && match, n_ops += !d, n_m += !d && match;
        }
        c.ref += __popcll(mr), c.qry += __popcll(mq), c.bases += __popcll(ma);
    }
    matches = wave_sum(matches), rbases = wave_sum(rbases), qbases = wave_sum(qbases);
    d_ops = wave_sum(d_ops), d_m = wave_sum(d_m), n_ops = wave_sum(n_ops), n_m = wave_sum(n_m);
    if (lane == 0) out[g] = CgStats{cb, ce, rbases, qbases, matches, d_ops, d_m, n_ops, n_m};
}

extern "C" void dhk_cg_bind(hipStream_t st, CgEnv e, int32_t count, CgSummary *sum, uint32_t *rlen, uint32_t *qlen)
{
    hipLaunchKernelGGL(k_cg_bind, dim3((count + 1 + CG_BLOCK - 1) / CG_BLOCK), dim3(CG_BLOCK), 0, st, e, count, sum, rlen, qlen);
}

extern "C" void dhk_cg_gather(hipStream_t st, const CgSummary *sum, int32_t count, const uint32_t *roff, const uint32_t *qoff,
                              const uint8_t *true_bases, const int64_t *true_off, const uint8_t *res_bases, const uint8_t *res_rc,
                              const int64_t *res_off, const int32_t *result_gap, uint8_t *ref, uint8_t *qry, uint32_t *has_base)
{
    hipLaunchKernelGGL(k_cg_gather, dim3((count + CG_WAVES - 1) / CG_WAVES), dim3(CG_BLOCK), 0, st, sum, count, roff, qoff, true_bases, true_off,
                       res_bases, res_rc, res_off, result_gap, ref, qry, has_base);
}

extern "C" void dhk_cg_stats(hipStream_t st, const CgSummary *sum, int32_t count, const uint32_t *roff, const uint32_t *qoff, const uint8_t *refs,
                             const uint8_t *qrys, const int64_t *op_off, const uint8_t *ops, const int64_t *dust_ptr, const int32_t *dust_iv,
                             int32_t crop, void *out)
{
    hipLaunchKernelGGL(k_cg_stats, dim3((count + CG_WAVES - 1) / CG_WAVES), dim3(CG_BLOCK), 0, st, sum, count, roff, qoff, refs, qrys, op_off, ops,
                       dust_ptr, dust_iv, crop, (CgStats *)out);
}
