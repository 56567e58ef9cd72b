/*
 * hs_report_passes.h — the report program of a block-mode corpus scan as
 * data-parallel passes over the scan's sorted records, one thread per record
 * (or candidate, or block).  The per-thread bodies are plain functors that
 * run as device code under report.hip's kernel wrapper and in serial loops on
 * the CPU (vsa_hs_report_records_emulated); run_passes, which sizes every
 * buffer and orders the passes, is one template over a backend that supplies
 * buffers, `each` (run a body for every index), an exclusive sum and a stable
 * pair sort -- hipcub on the device, <algorithm> / <numeric> on the CPU.
 *
 * Stages:
 *   lead       a record leads its end-group when the previous record has
 *              another end; the leader finds the block holding that end
 *   exhaustion every live occurrence of a keyed (SINGLEMATCH) pattern is a
 *              candidate, listed in delivery order; a stable sort by
 *              (block, key) brings a key's candidates of one block together
 *              and the first of each run is the one that reports
 *   count      report_group per leader with a counting emit
 *   offsets    exclusive sums: per record, then per caller block
 *   emit       report_group again, writing vsa_hs_match_t at the offsets
 *
 * Every offset, end and index is 64 bits wide.
 */
#ifndef VSA_HS_REPORT_PASSES_H
#define VSA_HS_REPORT_PASSES_H

#include <algorithm>
#include <vector>

#include "hs_report.h"

namespace vsa_report {

constexpr uint32_t NO_POS = ~0u;
constexpr uint32_t WG = 256; /* threads of a workgroup */
/* ends are shifted by END_SHIFT inside a 64-bit record key */
constexpr uint64_t MAX_END = 1ULL << (64 - END_SHIFT);
/* a grid's x dimension */
constexpr uint64_t MAX_GRID = 0x7fffffffULL;

/* workgroups for n threads, 0 when a grid cannot hold them */
inline uint64_t grid_for(uint64_t n) {
    const uint64_t g = n / WG + (n % WG != 0);
    return g <= MAX_GRID ? g : 0;
}

/* -------------------------------------------------------- block table -- */

/* the non-empty blocks sorted by offset (host side) */
struct BlockTable {
    std::vector<uint32_t> order;  /* position -> caller's block index */
    std::vector<uint64_t> so, se; /* [offset, end) in that order */
    /* every block the same length (the last may be shorter), back to back
     * from off0, none empty: the block of an end is (end - off0) / ulen */
    bool uniform = false;
    uint64_t off0 = 0, ulen = 0;
};

/* false: two non-empty blocks overlap, or a block ends past MAX_END */
inline bool build_block_table(const uint64_t *offsets, const uint64_t *lens, uint32_t nblocks,
                              BlockTable &bt) {
    bt = BlockTable();
    bool any_empty = false;
    for (uint32_t b = 0; b < nblocks; b++) {
        if (offsets[b] >= MAX_END || lens[b] >= MAX_END || offsets[b] + lens[b] >= MAX_END)
            return false;
        if (lens[b]) bt.order.push_back(b);
        else any_empty = true;
    }
    std::stable_sort(bt.order.begin(), bt.order.end(),
                     [&](uint32_t a, uint32_t b) { return offsets[a] < offsets[b]; });
    for (uint32_t b : bt.order) {
        if (!bt.so.empty() && offsets[b] < bt.se.back()) return false;
        bt.so.push_back(offsets[b]);
        bt.se.push_back(offsets[b] + lens[b]);
    }
    bt.uniform = nblocks > 0 && !any_empty;
    for (uint32_t b = 0; bt.uniform && b < nblocks; b++)
        bt.uniform = offsets[b] == offsets[0] + (uint64_t)b * lens[0] &&
                     (lens[b] == lens[0] || (b + 1 == nblocks && lens[b] < lens[0]));
    bt.off0 = nblocks ? offsets[0] : 0;
    bt.ulen = nblocks ? lens[0] : 0;
    return true;
}

/* the block table as the passes read it: every pointer in the memory the
 * bodies run in */
struct Blocks {
    const uint64_t *so, *se;      /* npos */
    const uint32_t *order;        /* npos */
    const uint64_t *offsets, *lens; /* nblocks, caller order */
    uint32_t npos, nblocks;
    uint32_t uniform;
    uint64_t off0, ulen;
};

/* position of the block holding end e, NO_POS when none does */
VSA_HD inline uint32_t block_pos(const Blocks &b, uint64_t e) {
    if (b.uniform) {
        if (e < b.off0) return NO_POS;
        const uint64_t p = (e - b.off0) / b.ulen;
        return p < b.npos && e < b.se[p] ? (uint32_t)p : NO_POS;
    }
    uint64_t lo = 0, hi = b.npos; /* first position whose offset is > e */
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (b.so[mid] <= e) lo = mid + 1;
        else hi = mid;
    }
    return lo && e < b.se[lo - 1] ? (uint32_t)(lo - 1) : NO_POS;
}

/* ------------------------------------------------------------- bodies -- */

/* what every body reads; the arrays are sized by run_passes */
struct Pass {
    Tables t;
    Blocks b;
    const uint8_t *data; /* the corpus */
    const uint64_t *keys;
    const uint32_t *ids;
    uint64_t n;          /* records */
    uint32_t has_keys;
    uint32_t *gpos;      /* n: a leader's block position, else NO_POS */
    uint64_t *cnt;       /* n + 1: per leader, candidates and later matches */
    uint64_t *coff;      /* n + 1: candidates before the group */
    uint64_t *moff;      /* n + 1: matches before the group, record order */
    uint64_t ncand;
    uint64_t *ckey, *cval, *skey, *sval; /* ncand: candidates, and sorted */
    uint8_t *flag;       /* ncand: this candidate reports */
    uint64_t *bcnt;      /* nblocks + 1: matches of the caller's block */
    uint64_t *bbase;     /* nblocks + 1: matches of the blocks before it */
    uint64_t *br0;       /* nblocks: its first record */
    vsa_hs_match_t *out;
    uint64_t cap;
};

struct Group {
    uint64_t k1, to, base;
    const uint8_t *blk;
    uint32_t pos;
};

/* the end-group led by record k; false when k leads none */
VSA_HD inline bool group_at(const Pass &p, uint64_t k, Group &g) {
    g.pos = p.gpos[k];
    if (g.pos == NO_POS) return false;
    const uint64_t end = p.keys[k] >> END_SHIFT;
    uint64_t k1 = k + 1;
    while (k1 < p.n && (p.keys[k1] >> END_SHIFT) == end) k1++;
    g.k1 = k1;
    g.base = p.b.so[g.pos];
    g.to = end - g.base + 1;
    g.blk = p.data ? p.data + g.base : nullptr;
    return true;
}

struct NoEmit {
    VSA_HD void operator()(uint32_t, uint64_t, uint64_t) {}
};
struct CountEmit {
    uint64_t n;
    VSA_HD void operator()(uint32_t, uint64_t, uint64_t) { n++; }
};
struct WriteEmit {
    vsa_hs_match_t *out;
    uint64_t cap, slot;
    uint32_t block;
    VSA_HD void operator()(uint32_t id, uint64_t from, uint64_t to) {
        if (slot < cap) {
            vsa_hs_match_t m;
            m.id = id;
            m.block = block;
            m.from = from;
            m.to = to;
            out[slot] = m;
        }
        slot++;
    }
};

/* report_group calls test() once per live keyed occurrence, in delivery
 * order: the j-th call of a group is candidate coff[leader] + j.  Every
 * occurrence counts as exhausted here, so nothing keyed is emitted. */
struct CandCountEx {
    uint64_t n;
    VSA_HD bool test(uint32_t) {
        n++;
        return true;
    }
    VSA_HD void set(uint32_t) {}
};
struct CandWriteEx {
    uint64_t *ckey, *cval;
    uint64_t at, hi; /* hi = block position << END_SHIFT */
    VSA_HD bool test(uint32_t e) {
        ckey[at] = hi | e;
        cval[at] = at;
        at++;
        return true;
    }
    VSA_HD void set(uint32_t) {}
};
/* an occurrence is exhausted unless it is its key's first in the block */
struct FlagEx {
    const uint8_t *flag; /* NULL: a database without keys */
    uint64_t at;
    VSA_HD bool test(uint32_t) { return !flag[at++]; }
    VSA_HD void set(uint32_t) {}
};

struct LeadBody {
    Pass p;
    VSA_HD void operator()(uint64_t k) const {
        const uint64_t e = p.keys[k] >> END_SHIFT;
        const bool lead = k == 0 || (p.keys[k - 1] >> END_SHIFT) != e;
        p.gpos[k] = lead ? block_pos(p.b, e) : NO_POS;
    }
};

/* n + 1 indices: the last one closes the sum */
struct CandCountBody {
    Pass p;
    VSA_HD void operator()(uint64_t k) const {
        Group g;
        CandCountEx ex{0};
        if (k < p.n && group_at(p, k, g)) {
            NoEmit em;
            report_group(p.t, p.ids, k, g.k1, g.blk, g.to, ex, em);
        }
        p.cnt[k] = ex.n;
    }
};

struct CandWriteBody {
    Pass p;
    VSA_HD void operator()(uint64_t k) const {
        Group g;
        if (!group_at(p, k, g)) return;
        CandWriteEx ex{p.ckey, p.cval, p.coff[k], (uint64_t)g.pos << END_SHIFT};
        NoEmit em;
        report_group(p.t, p.ids, k, g.k1, g.blk, g.to, ex, em);
    }
};

/* over the sorted candidates: the first of each (block, key) run reports */
struct FlagBody {
    Pass p;
    VSA_HD void operator()(uint64_t i) const {
        p.flag[p.sval[i]] = i == 0 || p.skey[i - 1] != p.skey[i];
    }
};

/* n + 1 indices */
struct CountBody {
    Pass p;
    VSA_HD void operator()(uint64_t k) const {
        Group g;
        CountEmit em{0};
        if (k < p.n && group_at(p, k, g)) {
            FlagEx ex{p.flag, p.has_keys ? p.coff[k] : 0};
            report_group(p.t, p.ids, k, g.k1, g.blk, g.to, ex, em);
        }
        p.cnt[k] = em.n;
    }
};

/* nblocks + 1 indices: a block's records are those whose end lies in it */
struct BlockCountBody {
    Pass p;
    VSA_HD void operator()(uint64_t b) const {
        uint64_t c = 0;
        if (b < p.b.nblocks) {
            uint64_t r0 = 0;
            if (p.b.lens[b]) {
                const uint64_t off = p.b.offsets[b];
                r0 = lower_bound_key(p.keys, p.n, off << END_SHIFT);
                const uint64_t r1 =
                    lower_bound_key(p.keys, p.n, (off + p.b.lens[b]) << END_SHIFT);
                c = p.moff[r1] - p.moff[r0];
            }
            p.br0[b] = r0;
        }
        p.bcnt[b] = c;
    }
};

/* the caller's blocks in index order, each one's matches in delivery order */
struct EmitBody {
    Pass p;
    VSA_HD void operator()(uint64_t k) const {
        Group g;
        if (!group_at(p, k, g)) return;
        const uint32_t b = p.b.order[g.pos];
        FlagEx ex{p.flag, p.has_keys ? p.coff[k] : 0};
        WriteEmit em{p.out, p.cap, p.bbase[b] + (p.moff[k] - p.moff[p.br0[b]]), b};
        report_group(p.t, p.ids, k, g.k1, g.blk, g.to, ex, em);
    }
};

/* ------------------------------------------------------------ the plan -- */

/* buffers of a backend, grown on demand and kept between passes */
enum Slot {
    S_GPOS, S_CNT, S_COFF, S_MOFF, S_CKEY, S_CVAL, S_SKEY, S_SVAL, S_FLAG, S_BCNT, S_BBASE,
    S_BR0, S_OUT, S_COUNT
};

/* run_passes tells the backend which stage the work queued next belongs to
 * (per-stage times); ST_N closes the last one */
enum Stage { ST_LEAD, ST_EXHAUST, ST_COUNT, ST_EMIT, ST_N };

/* bits of the candidate sort key: a key below 1 << END_SHIFT, above it a
 * block position below npos */
inline int cand_key_bits(uint32_t npos) {
    int bits = END_SHIFT;
    while (bits < 64 && ((uint64_t)npos >> (bits - END_SHIFT))) bits++;
    return bits;
}

/* One scan's records through the passes.  `p` arrives with t, b, data, keys,
 * ids and n set, in the backend's memory.  Afterwards p.out holds *total
 * matches (the backend's S_OUT buffer, sized from that total), p.bcnt the
 * per-block counts and p.bbase their exclusive sum.  Returns 0, or the
 * backend's error.
 *
 * Backend:
 *   template <class T> int buf(Slot, uint64_t count, T **)
 *   template <class F> int each(uint64_t n, const F &)
 *   int exclusive_sum(const uint64_t *in, uint64_t *out, uint64_t n)
 *   int sort_pairs(kin, kout, vin, vout, n, end_bit)   stable, ascending
 *   int read_u64(const uint64_t *src, uint64_t *dst)
 *   void stage(Stage) */
template <class Backend>
int run_passes(Backend &be, Pass &p, uint64_t *total) {
    int rc;
    const uint64_t n = p.n, nb = p.b.nblocks;
    p.has_keys = p.t.n_ekeys != 0;
    p.ncand = 0;
    p.flag = nullptr;
    p.ckey = p.cval = p.skey = p.sval = nullptr;
    p.out = nullptr;
    p.cap = 0;
    if ((rc = be.buf(S_GPOS, n, &p.gpos))) return rc;
    if ((rc = be.buf(S_CNT, n + 1, &p.cnt))) return rc;
    if ((rc = be.buf(S_COFF, p.has_keys ? n + 1 : 0, &p.coff))) return rc;
    if ((rc = be.buf(S_MOFF, n + 1, &p.moff))) return rc;
    if ((rc = be.buf(S_BCNT, nb + 1, &p.bcnt))) return rc;
    if ((rc = be.buf(S_BBASE, nb + 1, &p.bbase))) return rc;
    if ((rc = be.buf(S_BR0, nb, &p.br0))) return rc;
    be.stage(ST_LEAD);
    if ((rc = be.each(n, LeadBody{p}))) return rc;
    if (p.has_keys) {
        be.stage(ST_EXHAUST);
        if ((rc = be.each(n + 1, CandCountBody{p}))) return rc;
        if ((rc = be.exclusive_sum(p.cnt, p.coff, n + 1))) return rc;
        if ((rc = be.read_u64(p.coff + n, &p.ncand))) return rc;
        if ((rc = be.buf(S_CKEY, p.ncand, &p.ckey))) return rc;
        if ((rc = be.buf(S_CVAL, p.ncand, &p.cval))) return rc;
        if ((rc = be.buf(S_SKEY, p.ncand, &p.skey))) return rc;
        if ((rc = be.buf(S_SVAL, p.ncand, &p.sval))) return rc;
        if ((rc = be.buf(S_FLAG, p.ncand, &p.flag))) return rc;
        if (p.ncand) {
            if ((rc = be.each(n, CandWriteBody{p}))) return rc;
            if ((rc = be.sort_pairs(p.ckey, p.skey, p.cval, p.sval, p.ncand,
                                    cand_key_bits(p.b.npos))))
                return rc;
            if ((rc = be.each(p.ncand, FlagBody{p}))) return rc;
        }
    }
    be.stage(ST_COUNT);
    if ((rc = be.each(n + 1, CountBody{p}))) return rc;
    if ((rc = be.exclusive_sum(p.cnt, p.moff, n + 1))) return rc;
    if ((rc = be.each(nb + 1, BlockCountBody{p}))) return rc;
    if ((rc = be.exclusive_sum(p.bcnt, p.bbase, nb + 1))) return rc;
    if ((rc = be.read_u64(p.moff + n, total))) return rc;
    be.stage(ST_EMIT);
    if ((rc = be.buf(S_OUT, *total, &p.out))) return rc;
    p.cap = *total;
    if (*total && (rc = be.each(n, EmitBody{p}))) return rc;
    be.stage(ST_N);
    return 0;
}

} // namespace vsa_report

#endif
