// dh_tjoin.h -- the seeds of a call "small grouped A against large grouped B" (the consensus re-alignment: the templates
// of every pile-up against all reads of the pile-ups, processPileUps/package.d:518-568) from a per-group k-mer table held
// in LDS instead of one dependent directory line per looked-up k-mer.
//
// Both DBs are grouped by pile-up and the index key carries the group, so a read only ever meets the index entries of
// its own group: a few thousand entries, one contiguous range of the entry array (the index lies in bucket order, the
// group is the top key bits).  k_tjoin (dh_tjoin.hip) works on units (group, run of consecutive reads of that group):
//
//   table build   the group's entries become 8-byte slots  canonical k-mer << 32 | orientation << 31 | entry number in the
//                 group  of an open-addressing table (linear probing, TJ_SLOTS slots).  Copies of a k-mer take separate
//                 slots of the same probe run: a lookup walks the run from the k-mer's home slot to the first empty slot
//                 and sees every entry with the key.  Built from the INDEX entries, so sampling, soft mask, N bases and the
//                 orientation bit of the A side are the index build's and not repeated here.
//   count pass    a wavefront per read, 512 consecutive k-mer starts per step, eight per lane from one packed word of
//                 the lane's 23 bases (tj_read, dh_tjoin.hip); which k-mers are looked up is decided as seed_item decides
//                 it (canonical choice, kmer_sampled, mask_touch on B, no base outside a, c, g, t = valid >= k).  A lane
//                 probes the table and counts the hits the directory lookups would emit: the -t cap per orientation class
//                 (runf / runr against tcap), a palindrome on both strands, o.strands.
//   reservation   ONE device-scope atomic per unit on the hit cursor; the cursor keeps counting when the buffer is full
//                 (DH_ST_TJ_HITCAP: the host reruns with the size the cursor reports; no hit is ever truncated).
//   write pass    the same walk again; a hit is  strand << 63 | D << HIT_QBITS | qs  with D = gv + sepv - qs and
//                 qs = strand ? blen - k - q : q  (ent.y is fetched only here, on a match); segtab[read - read0] =
//                 first hit << 24 | count: JoinView's gns == NULL form with ns_fixed = 1.
//   k_seed<.., JOIN>  the seed filter's back end unchanged: it gathers a read's hits from its segment.
//
// The multiset of hits a read gets is the one the directory lookups produce (same index entries, same rules), so the
// candidates and everything behind them are bit-identical; DH_NO_TJOIN=1 forces the directory path (tests compare the two).
// The directory path stays for k > 16, skip_self != 0, ungrouped DBs, and for a call in which a group has more entries
// than the table is planned for.
//
// The slot code (hash, insert, probe walk, the cap rule) compiles for the host as well: tests/native/tjoin_host.cpp
// checks it against a plain scan of the entry list.
#ifndef DH_TJOIN_H
#define DH_TJOIN_H
#include <stdint.h>

#if defined(__HIPCC__)
#define TJ_HD __host__ __device__ __forceinline__
#else
#define TJ_HD inline
#endif

#define TJ_SLOT_BITS 14
#define TJ_SLOTS (1 << TJ_SLOT_BITS)   /* slots of the table: 128 KB of LDS */
#define TJ_CAP 8192                    /* entries of a group the table is planned for (half of the slots) */
#define TJ_THREADS 1024
#define TJ_RUN (TJ_THREADS / 64)       /* reads per unit: a wavefront each */
#define TJ_QBATCH 4                    /* units per atomic on the work queue */
#define TJ_MAXK 16                     /* the canonical k-mer fits 32 bits */
#define TJ_EMPTY (~0ull)

#define DH_ST_TJ_HITCAP 0x80           /* the hit buffer was too small: the cursor holds the size needed, k_tjoin is rerun */
#define DH_ST_TJ_OVERFLOW 0x100        /* a read's segment does not fit the segment word: the call is redone by the directory */

TJ_HD uint32_t tj_home(uint32_t canon) { return (canon * 0x9E3779B1u) >> (32 - TJ_SLOT_BITS); }
TJ_HD uint64_t tj_slot(uint32_t canon, uint32_t ori, uint32_t idx) { return ((uint64_t)canon << 32) | (ori << 31) | idx; }

// claim(p, v): store v into *p iff *p is empty, true when it did (an atomic compare-and-swap on the device)
template <class Claim>
TJ_HD void tj_insert(uint64_t *tab, uint64_t v, Claim claim)
{
    uint32_t h = tj_home((uint32_t)(v >> 32));
    while (!claim(tab + h, v)) h = (h + 1) & (TJ_SLOTS - 1);
}

// every entry with the key: f(low word of its slot = orientation << 31 | entry number)
template <class F>
TJ_HD void tj_walk(const uint64_t *tab, uint32_t canon, F f)
{
    for (uint32_t h = tj_home(canon);; h = (h + 1) & (TJ_SLOTS - 1)) {
        const uint64_t s = tab[h];
        if (s == TJ_EMPTY) return;
        if ((uint32_t)(s >> 32) == canon) f((uint32_t)s);
    }
}

// the copies of a looked-up k-mer (orientation bori, palindrome pal) per orientation class and what the -t cap and
// o.strands leave of them: bit 0 = the forward-strand hits are emitted (fwd of them), bit 1 = the reverse-strand hits (rev)
struct TjMatch {
    int32_t fwd, rev;
    uint32_t emit;
};
TJ_HD TjMatch tj_match(const uint64_t *tab, uint32_t canon, uint32_t bori, bool pal, int32_t tcap, int32_t strands)
{
    int32_t runf = 0, runr = 0;
    tj_walk(tab, canon, [&](uint32_t lo) {
        const bool same = (lo >> 31) == bori;
        runf += (same || pal) ? 1 : 0;
        runr += (!same || pal) ? 1 : 0;
    });
    TjMatch m;
    m.emit = ((runf > 0 && runf <= tcap && (strands & 1)) ? 1u : 0u) | ((runr > 0 && runr <= tcap && (strands & 2)) ? 2u : 0u);
    m.fwd = (m.emit & 1u) ? runf : 0;
    m.rev = (m.emit & 2u) ? runr : 0;
    return m;
}

#ifndef DH_TJOIN_SLOT_CODE_ONLY /* (the host harness of the slot code stops here) */
#include "dh_device.h"
#include "dh_join.h"

struct TjView {
    const uint32_t *gent;    // [ngroups + 1] first index entry of group g of A
    int32_t ngroups;
    const int4 *units;       // (group, first read, end read, 0)
    int32_t nunits;
    int32_t read0;           // first read of the chunk: row 0 of segtab
    uint64_t *segtab;        // per read: first hit << 24 | count
    uint64_t *hits;
    int64_t hits_cap;
    unsigned long long *cursor;  // hits reserved so far
    uint32_t *queue;
    int32_t *status;
};

extern "C" {
/* first index entry of every group from the build's directory (dir[b] = end of bucket b, dir[-1] == 0): gent[g] = end of
 * the last bucket below group g's range, gent[ngroups] = n */
void dhk_tj_group_offsets(hipStream_t st, const uint32_t *dir, int32_t ngroups, int32_t k, int32_t shift, int64_t nb,
                          uint32_t *gent);
/* count, reserve, write (cursor and queue zeroed by the caller) */
void dhk_tjoin(hipStream_t st, DbView B, IndexView ix, DhOpts o, TjView t, int32_t ncu);
}
#endif
#endif
