"""The report program restated per end-group (vectorscan_amd/csrc/hs_report.h
report_group: no state between groups but the exhaustion keys) through
vsa_hs_report_records_host, over the oracle's HWLM records: every block's
callback sequence equals the oracle's pure-literal run and, as a set, the
engine-free brute force."""
import functools

import numpy as np

import oracle
from oracle import hs_lit as ohs
import vectorscan_amd as vsa
from vectorscan_amd import hs, hsbench

from test_hsbench import make_case, make_corpus

ORACLE_CAP = 4096  # oracle.hs_lit.scan stops at this many HWLM records per block


def oracle_db(exprs, flags, ids):
    odb = ohs.compile_lit_multi(exprs, flags, ids)
    blob = vsa.hwlm_build([vsa.HwlmLiteral(t, nc, f, noruns=nr)
                           for t, nc, f, nr in odb.hwlm_literals()])
    return odb, blob


def block_records(blob, image, offs, lens):
    """(keys, ids) of the blocks' HWLM records, keys = end << 24 | order with
    the end relative to `image`, sorted; every block under the oracle's cap"""
    keys, ids = [], []
    for o, ln in sorted(zip(map(int, offs), map(int, lens))):
        if not ln:
            continue
        _, recs = oracle.hwlm_exec(blob.ptr, image[o:o + ln].copy(), cap=ORACLE_CAP)
        assert len(recs) < ORACLE_CAP, "block at %d: the oracle's record cap is reached" % o
        for k, (end, frag) in enumerate(recs):
            keys.append(((o + end) << 24) | k)
            ids.append(frag)
    return np.array(keys, np.uint64), np.array(ids, np.uint32)


def split_blocks(matches, counts):
    """per-block [(id, from, to)] of a vsa_hs_match_t array laid out block
    after block"""
    out, pos = [], 0
    for b, c in enumerate(counts):
        m = matches[pos:pos + int(c)]
        assert (m["block"] == b).all()
        out.append(list(zip(m["id"].tolist(), m["from"].tolist(), m["to"].tolist())))
        pos += int(c)
    assert pos == len(matches)
    return out


@functools.lru_cache(maxsize=None)
def ragged_case():
    """the third set of test_hsbench.CASES (300 literals of 2-24 bytes, mixed
    flags, shared ids) over 60 ragged chunks of 1-3000 bytes, with each
    block's oracle sequence, computed once"""
    rng, exprs, flags, ids, alpha = make_case(2, 1)
    chunks = make_corpus(rng, exprs, 7, 60, 1, 3000, alpha)
    blocks = [(i, s, d) for i, (s, d) in enumerate(chunks)]
    image, offs, lens, _ = hsbench.layout(blocks, hs.MODE_BLOCK)
    odb, blob = oracle_db(exprs, flags, ids)
    want = [ohs.scan(odb, blob.ptr, image[int(o):int(o + ln)].copy())
            for o, ln in zip(offs, lens)]
    return exprs, flags, ids, image, offs, lens, odb, blob, want


def test_report_records_host_ragged():
    exprs, flags, ids, image, offs, lens, odb, blob, want = ragged_case()
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    assert db.hwlm_bytes() == blob.tobytes()
    keys, rids = block_records(blob, image, offs, lens)
    rc, total, counts, digests, matches = hs.report_records_host(db, keys, rids, image, offs,
                                                                 lens)
    assert rc == hs.SUCCESS
    got = split_blocks(matches, counts)
    assert sum(len(w) for w in want) > 500
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, "block %d" % b
        assert int(digests[b]) == hs.seq_digest(w)
        o, ln = int(offs[b]), int(lens[b])
        assert sorted(g) == sorted(ohs.brute_force(odb, image[o:o + ln])), "block %d" % b
    assert total == sum(len(w) for w in want) == len(matches)
    # a short list: nothing past cap, the total still reported
    rc, total2, _, _, m2 = hs.report_records_host(db, keys, rids, image, offs, lens, cap=7)
    assert rc == hs.SUCCESS and total2 == total and len(m2) == 7
    assert (m2 == matches[:7]).all()


def test_report_records_host_edges():
    """long literals at block starts (prefix in the previous block), a
    caseless long literal, exhaustion per block, two patterns of one id at
    one offset with and without SOM, the SOM flush in id order, gaps"""
    som = hs.FLAG_SOM_LEFTMOST
    exprs = [b"abcdefghijk", b"XyZabcdefghijkl", b"hij", b"bc", b"abc", b"c", b"zbc", b"yzbc",
             b"bc"]
    flags = [0, hs.FLAG_CASELESS, hs.FLAG_SINGLEMATCH, 0, 0, som, som, som, som]
    ids = [1, 2, 3, 4, 4, 9, 9, 8, 8]  # ids 8 and 9 go through the SOM log
    text = (b"abcdefghijk" + b"..xyzABCDEFGHIJKL.." + b"hijhijhij" + b"--abc--yzbc" +
            b"abcdefghijk")
    image = np.frombuffer(text, np.uint8)
    # blocks: [0, 11) exact fit; [11, 30); [30, 39) x2 halves; a gap; the tail
    # block starts inside the last literal (prefix outside the block)
    offs = [0, 11, 30, 34, 39, len(text) - 8, 5]
    lens = [11, 19, 4, 5, 11, 8, 0]
    odb, blob = oracle_db(exprs, flags, ids)
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    keys, rids = block_records(blob, image, offs, lens)
    rc, total, counts, digests, matches = hs.report_records_host(db, keys, rids, image, offs,
                                                                 lens)
    assert rc == hs.SUCCESS
    got = split_blocks(matches, counts)
    for b, (o, ln) in enumerate(zip(offs, lens)):
        w = ohs.scan(odb, blob.ptr, image[o:o + ln].copy()) if ln else []
        assert got[b] == w, "block %d" % b
        assert sorted(w) == sorted(ohs.brute_force(odb, image[o:o + ln]))
    assert (1, 0, 11) in got[0] and not any(i == 1 for i, _, _ in got[5])
    assert [m for m in got[1] if m[0] == 2] == [(2, 0, 17)]
    assert [m for m in got[2] + got[3] if m[0] == 3] == [(3, 0, 3), (3, 0, 5)]
    assert [m for m in got[4] if m[2] == 5] == [(4, 0, 5), (8, 3, 5), (9, 4, 5)]
    assert [m for m in got[4] if m[2] == 11] == [(4, 0, 11), (8, 7, 11), (9, 8, 11)]
    stream_db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_STREAM |
                                     hs.MODE_SOM_HORIZON_LARGE)
    assert hs.report_records_host(stream_db, keys, rids, image, offs, lens)[0] == \
        hs.DB_MODE_ERROR


def check_exact(exprs, flags, ids, image, offs, lens):
    """the host walk's matches and digests == the oracle's sequence per
    block, which is checked as a set against the brute force"""
    image = np.ascontiguousarray(image, np.uint8)
    odb, blob = oracle_db(exprs, flags, ids)
    want = []
    for o, ln in zip(offs, lens):
        blk = np.ascontiguousarray(image[int(o):int(o + ln)])
        seq = ohs.scan(odb, blob.ptr, blk.copy()) if ln else []
        assert sorted(seq) == sorted(ohs.brute_force(odb, blk))
        want.append(seq)
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    keys, rids = block_records(blob, image, offs, lens)
    rc, total, counts, digests, matches = hs.report_records_host(db, keys, rids, image, offs,
                                                                 lens)
    assert rc == hs.SUCCESS and total == sum(len(w) for w in want)
    for b, (g, w) in enumerate(zip(split_blocks(matches, counts), want)):
        assert g == w, "block %d" % b
        assert int(digests[b]) == hs.seq_digest(w)
    return want


def test_long_literals_bound_check():
    """an 11-byte and a 300-byte literal; blocks behind a guard that holds
    the long literals' prefixes, so a missing `to >= len` check shows as a
    false match: a tail at a block's start with its prefix in the guard or in
    the previous block, a literal exactly filling a block, a caseless long
    literal in mixed case, a block shorter than every pattern, length-0
    blocks, a gap with planted matches, no blocks at all"""
    rng = np.random.default_rng(3)
    l11 = b"hello_world"
    l300 = bytes(rng.integers(0x41, 0x5B, 300, dtype=np.uint8))
    image = rng.integers(0x61, 0x7B, 6000, dtype=np.uint8)
    for p, s in [(10, l11), (700, l300), (1500, l11), (2990, l300), (5689, l11), (5700, l300)]:
        image[p:p + len(s)] = np.frombuffer(s, np.uint8)
    image[3500:3500 + 299] = np.frombuffer(l300[1:], np.uint8)  # all but its first byte
    # the second 300-byte literal is cut by a block boundary
    want = check_exact([l11, l300, b"wor"], [0, 0, 0], [1, 2, 3], image, [0, 3000, 3290],
                       [3000, 290, 2710])
    assert [len([m for m in w if m[0] == 2]) for w in want] == [1, 0, 1]
    assert [len([m for m in w if m[0] == 1]) for w in want] == [2, 0, 1]

    long_a, long_b = b"0123456789abcdefgh", b"QRSTUVWXyzyzyzyz"
    exprs = [long_a, long_b, b"tail", b"wxyzyzyzyz"]
    flags = [0, hs.FLAG_CASELESS, 0, hs.FLAG_CASELESS]
    guard = ((long_a[:10] + long_b[:8].lower()) * 40)[:502] + long_a[:10]
    parts = [long_a[10:] + b".....",   # 0: a tail at its start, the prefix ends the guard
             long_a,                   # 1: exactly the literal
             b"..0123456789",          # 2: ends with the prefix
             long_a[10:] + b"qrsTUVwxYZyzYzyZ" + b"..tail",  # 3: tail at start, prefix in 2
             b"tai",                   # 4: shorter than every pattern
             long_a + b"tail",         # a gap with planted matches
             b"xx" + long_a]           # 5: after the gap
    image = np.frombuffer(guard + b"".join(parts), np.uint8)
    starts = [len(guard) + sum(len(p) for p in parts[:k]) for k in range(len(parts))]
    offs = [starts[0], starts[1], starts[1], starts[2], starts[3], starts[4], starts[0] + 5,
            starts[6]]
    lens = [13, 18, 0, 12, 30, 3, 0, 20]
    assert offs[7] + lens[7] == len(image)
    want = check_exact(exprs, flags, [1, 2, 3, 4], image, offs, lens)
    assert want[0] == [] and want[1] == [(1, 0, 18)] and want[3] == []
    assert want[4] == [(2, 0, 24), (4, 0, 24), (3, 0, 30)]
    assert want[5] == [] and want[7] == [(1, 0, 20)]
    assert check_exact(exprs, flags, [1, 2, 3, 4], image, [], []) == []


def test_state_between_groups():
    """exhaustion per block (a SINGLEMATCH literal three times in each of two
    adjacent blocks), a NOREPEAT fragment in a 300-byte run, two patterns of
    one id ending together with and without SOM, two SOM-deduped ids at one
    offset flushed in id order, the flush at the block's end"""
    som, single = hs.FLAG_SOM_LEFTMOST, hs.FLAG_SINGLEMATCH
    exprs = [b"once", b"r", b"bc", b"abc", b"yz", b"xyz", b"z", b"wxyz", b"pq", b"opq"]
    flags = [single, single, 0, 0, som, som, som, som, som, som]
    ids = [1, 2, 3, 3, 8, 8, 5, 5, 9, 9]
    blk = b"once.once.once" + b"r" * 300 + b".abc.wxyz.."
    last = b"..opq"  # the SOM log flushed by the end of the block
    image = np.frombuffer(blk + blk + last, np.uint8)
    offs, lens = [0, len(blk), 2 * len(blk)], [len(blk), len(blk), len(last)]
    want = check_exact(exprs, flags, ids, image, offs, lens)
    for w in want[:2]:
        assert [m for m in w if m[0] == 1] == [(1, 0, 4)]
        assert [m for m in w if m[0] == 2] == [(2, 0, 15)]
        assert [m for m in w if m[0] == 3] == [(3, 0, 318)]
        assert [m for m in w if m[2] == 323] == [(5, 319, 323), (8, 320, 323)]
    assert want[2] == [(9, 2, 5)]
    # a NOREPEAT fragment beside a caseless twin that is not
    check_exact([b"r", b"R", b"bc", b"abc"], [single, hs.FLAG_CASELESS, 0, 0], [2, 6, 3, 3],
                image, offs, lens)


def test_engines():
    """Teddy (40 literals), noodle (one literal: no NOREPEAT step), FDR (the
    10k mixed set)"""
    import test_hsbench
    rng, exprs, flags, ids, alpha = make_case(0, 1)
    chunks = make_corpus(rng, exprs, 7, 30, 1, 3000, alpha)
    image, offs, lens, _ = hsbench.layout([(i, s, d) for i, (s, d) in enumerate(chunks)],
                                          hs.MODE_BLOCK)
    check_exact(exprs, flags, ids, image, offs, lens)
    text = np.frombuffer(b"..aaaaaa..aa.." * 40, np.uint8)
    for fl in (0, hs.FLAG_SINGLEMATCH, hs.FLAG_SOM_LEFTMOST | hs.FLAG_CASELESS):
        check_exact([b"aa"], [fl], [7], text, [0, 100, 300], [100, 200, 260])
    check_exact([b"aaaaaaaaaa"], [0], [7], np.frombuffer(b"a" * 64 + b"b" + b"a" * 12, np.uint8),
                [0, 64], [64, 13])
    exprs, flags, ids, blocks = test_hsbench.cfg5_case(256 << 10)
    image, offs, lens, _ = hsbench.layout(blocks, hs.MODE_BLOCK)
    check_exact(exprs, flags, ids, image, offs, lens)


def test_repeated_norepeat_records_report_nothing():
    """the oracle's records come with NOREPEAT applied; a scan's records do
    not.  Unfiltered repeats of a NOREPEAT fragment (a single-match literal
    of at most 8 bytes) report once per block all the same, with and without
    a second fragment in the database (FDR / Teddy against noodle)"""
    image = np.frombuffer(b"r" * 10 + b"zz" + b"r" * 4, np.uint8)
    keys = np.array([(e << 24) | k for k, e in enumerate(list(range(10)) + [12, 13, 14, 15])],
                    np.uint64)
    rids = np.zeros(len(keys), np.uint32)
    for exprs, flags, ids in (([b"r"], [hs.FLAG_SINGLEMATCH], [5]),
                              ([b"r", b"zz"], [hs.FLAG_SINGLEMATCH, 0], [5, 6])):
        db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
        rc, total, counts, _, m = hs.report_records_host(db, keys, rids, image, [0, 12], [12, 4])
        assert rc == hs.SUCCESS and total == 2 and list(counts) == [1, 1]
        assert m.tolist() == [(5, 0, 0, 1), (5, 1, 0, 1)]
