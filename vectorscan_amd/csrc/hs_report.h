/*
 * hs_report.h — the report program of a pure-literal database (hs_lit.cpp
 * on_fragment / long_ok / flush_som and the pure-literal subset of
 * dropin.hip replay_lit) as one function over sorted HWLM records, run by
 * vsa_hs_report_records_host.
 *
 * The unit of work is an end-group: the records of one block with the same
 * end, i.e. everything delivered at one `to`.  What happens inside a group
 * (compile order of a fragment's patterns, the long-literal check, the
 * dedupe of an id at one offset, the SOM log and its flush in id order) is
 * local to the group and is computed here without any state carried between
 * groups.  Only exhaustion crosses groups; the caller supplies it as `Ex`
 * and resolves it in record order.
 *
 * replay_lit's NOREPEAT step (a record is skipped when its fragment is
 * NOREPEAT and the previous record of the block carries the same fragment)
 * needs no counterpart in block mode: a NOREPEAT fragment holds only
 * single-match patterns of at most 8 bytes, so after any record of it every
 * one of its patterns has its exhaustion key set (each either was exhausted
 * already or reported and set it), and the repeated record reports nothing
 * whether it is skipped or walked.  Such patterns are never in the SOM log
 * and never share an id with a pattern without a key, so they do not enter
 * the dedupe or the flush either.
 */
#ifndef VSA_HS_REPORT_H
#define VSA_HS_REPORT_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/vectorscan_amd_hs.h"

/* the functions below also run as device code (report.hip) */
#if defined(__HIP__)
#define VSA_HD __host__ __device__
#else
#define VSA_HD
#endif

namespace vsa_report {

constexpr uint32_t NO_EKEY = ~0u;
constexpr uint32_t SHORT_LEN = 8; /* ROSE_SHORT_LITERAL_LEN_MAX: the HWLM tail */
constexpr int END_SHIFT = 24;     /* record key: end << 24 | order */

enum : uint32_t { PAT_CASELESS = 1, PAT_SOM = 2, PAT_SOM_DEDUPE = 4 };

struct Pat {
    uint32_t id, ekey, len, flags;
    uint32_t pre; /* offset in the pool of the len - 8 bytes before the tail */
};

/* a database flattened */
struct Tables {
    const uint32_t *frag_off;   /* fragment -> [first, last) pattern, n_frags + 1 */
    const Pat *pats;            /* in compile order within a fragment */
    const uint8_t *pool;        /* prefixes of the patterns longer than 8 bytes */
    uint32_t n_frags, n_pats, n_ekeys;
    uint32_t dedupe;            /* some id has several patterns */
};

/* first record of keys[0, n) whose key is >= key */
VSA_HD inline uint64_t lower_bound_key(const uint64_t *keys, uint64_t n, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* CHECK_LONG_LIT for a pattern ending at `to` of the block at blk: `to` is
 * tested against the length before any byte is loaded, and only bytes of
 * [blk, blk + to) are read */
VSA_HD inline bool pat_live(const Tables &t, const Pat &p, const uint8_t *blk, uint64_t to) {
    if (p.len <= SHORT_LEN) return true;
    if (to < p.len) return false;
    const uint8_t *s = blk + (to - p.len);
    const uint8_t *w = t.pool + p.pre;
    const uint32_t n = p.len - SHORT_LEN;
    const bool nocase = p.flags & PAT_CASELESS;
    for (uint32_t k = 0; k < n; k++) {
        uint8_t b = s[k];
        if (nocase && b >= 'a' && b <= 'z') b = (uint8_t)(b - 32);
        if (b != w[k]) return false;
    }
    return true;
}

/* The reports of one end-group: records [k0, k1) of a block, all ending at
 * `to` (relative to the block, blk = its first
 * byte).  emit(id, from, to) is called in delivery order: the fragments in
 * record order, each one's patterns in compile order, then the SOM log of
 * this offset in ascending id order (flushStoredSomMatches).
 *
 * The dedupe of an id at one offset needs no list: an id with an exhaustion
 * key is already stopped by that key after its first report, and any other
 * id was reported before iff an earlier pattern of the group has that id,
 * reports directly (no SOM log) and passes its long-literal check. */
template <class Ex, class Emit>
VSA_HD inline void report_group(const Tables &t, const uint32_t *ids, uint64_t k0, uint64_t k1,
                         const uint8_t *blk, uint64_t to, Ex &ex, Emit &emit) {
    bool som_logged = false;
    for (uint64_t k = k0; k < k1; k++) {
        const uint32_t f = ids[k];
        for (uint32_t pi = t.frag_off[f]; pi < t.frag_off[f + 1]; pi++) {
            const Pat p = t.pats[pi];
            if (!pat_live(t, p, blk, to)) continue;
            if (p.ekey != NO_EKEY && ex.test(p.ekey)) continue;
            if (p.flags & PAT_SOM_DEDUPE) {
                som_logged = true;
                continue;
            }
            if (t.dedupe && p.ekey == NO_EKEY) {
                bool seen = false;
                for (uint64_t j = k0; j <= k && !seen; j++) {
                    const uint32_t g = ids[j];
                    const uint32_t q1 = j == k ? pi : t.frag_off[g + 1];
                    for (uint32_t qi = t.frag_off[g]; qi < q1; qi++) {
                        const Pat q = t.pats[qi];
                        if (q.id == p.id && !(q.flags & PAT_SOM_DEDUPE) &&
                            pat_live(t, q, blk, to)) {
                            seen = true;
                            break;
                        }
                    }
                }
                if (seen) continue;
            }
            if (p.ekey != NO_EKEY) ex.set(p.ekey);
            emit(p.id, (p.flags & PAT_SOM) ? to - p.len : 0, to);
        }
    }
    if (!som_logged) return;
    /* the SOM log: per id the leftmost start, ids ascending.  No exhaustion
     * test here: SINGLEMATCH with SOM_LEFTMOST is refused at compile, so a
     * pattern of the log never has a key */
    uint64_t lo = 0; /* ids below lo are flushed */
    for (;;) {
        uint64_t best = ~0ULL;
        uint32_t best_len = 0;
        for (uint64_t k = k0; k < k1; k++) {
            const uint32_t f = ids[k];
            for (uint32_t pi = t.frag_off[f]; pi < t.frag_off[f + 1]; pi++) {
                const Pat p = t.pats[pi];
                if (!(p.flags & PAT_SOM_DEDUPE) || p.id < lo || p.id > best) continue;
                if (p.id == best && p.len <= best_len) continue;
                if (!pat_live(t, p, blk, to)) continue;
                best = p.id;
                best_len = p.len;
            }
        }
        if (best == ~0ULL) break;
        emit((uint32_t)best, to - best_len, to);
        lo = best + 1;
    }
}

} // namespace vsa_report

#endif
