"""vsa_hs_report_records_emulated: the report program as the device runs it
(the passes of vectorscan_amd/csrc/hs_report_passes.h: lead, exhaustion by a
stable sort of the keyed candidates, count, exclusive sums, emit) in serial
loops on the CPU, held to vsa_hs_report_records_host field for field on the
inputs of test_device_report_host.py, whose own assertions (the oracle's
sequences, the brute force, the specific sequences) then run on the emulated
results."""
import numpy as np
import pytest

from vectorscan_amd import hs

import test_device_report_host as host_tests


def same(a, b):
    """(rc, total, counts, digests, matches) equal field for field"""
    assert a[0] == b[0], (a[0], b[0])
    assert a[1] == b[1], (a[1], b[1])
    assert np.array_equal(a[2], b[2])
    assert np.array_equal(a[3], b[3])
    assert a[4].dtype == b[4].dtype == hs.MATCH_DTYPE
    assert np.array_equal(a[4], b[4])


@pytest.fixture
def emulated(monkeypatch):
    """test_device_report_host's calls of hs.report_records_host answered by
    the emulated passes, after comparing them with the host walk; yields the
    list of compared calls"""
    calls = []
    host = hs.report_records_host

    def both(db, keys, ids, data, offsets, lens, cap=None):
        a = host(db, keys, ids, data, offsets, lens, cap)
        b = hs.report_records_emulated(db, keys, ids, data, offsets, lens, cap)
        same(a, b)
        calls.append(b[1])
        return b
    monkeypatch.setattr(host_tests.hs, "report_records_host", both)
    return calls


def test_ragged(emulated):
    host_tests.test_report_records_host_ragged()
    assert len(emulated) == 2 and emulated[0] > 500


def test_edges(emulated):
    host_tests.test_report_records_host_edges()
    assert len(emulated) == 2  # the block database and the refused stream database


def test_long_literals(emulated):
    host_tests.test_long_literals_bound_check()
    assert len(emulated) == 3 and emulated[2] == 0  # the last: no blocks at all


def test_state_between_groups(emulated):
    host_tests.test_state_between_groups()
    assert len(emulated) == 2


def test_engines(emulated):
    host_tests.test_engines()
    assert len(emulated) == 6


def test_norepeat(emulated):
    host_tests.test_repeated_norepeat_records_report_nothing()
    assert len(emulated) == 2


def test_winner_flags_span_many_groups():
    """3 blocks of 1,200 end-groups each; every group holds a SINGLEMATCH
    literal (so a candidate per group and more, over 3,600 in the exhaustion
    sort) and two patterns of one plain id; the SINGLEMATCH id 7 has two
    patterns on one key, id 9 is a second key.  Exactly one report per key and
    block survives: the first."""
    single = hs.FLAG_SINGLEMATCH
    exprs = [b"a", b"ba", b"a", b"xa", b"a"]
    flags = [single, single, 0, single, 0]
    ids = [7, 7, 3, 9, 3]
    groups = 1200
    blk = b"xa" + b"ba" * groups
    image = np.frombuffer(blk * 3, np.uint8)
    offs = [0, len(blk), 2 * len(blk)]
    lens = [len(blk)] * 3
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    odb, blob = host_tests.oracle_db(exprs, flags, ids)
    assert db.hwlm_bytes() == blob.tobytes()
    keys, rids = host_tests.block_records(blob, image, offs, lens)
    ends = keys >> np.uint64(24)
    for o, ln in zip(offs, lens):
        assert len(np.unique(ends[(ends >= o) & (ends < o + ln)])) > 1000
    a = hs.report_records_host(db, keys, rids, image, offs, lens)
    b = hs.report_records_emulated(db, keys, rids, image, offs, lens)
    same(a, b)
    rc, total, counts, digests, matches = b
    assert rc == hs.SUCCESS
    got = host_tests.split_blocks(matches, counts)
    assert got[0] == host_tests.ohs.scan(odb, blob.ptr, image[:len(blk)].copy())
    for blk_matches in got:
        # "a" and "xa" first end at 2, "ba" (the key of id 7 again) at 4
        assert [m for m in blk_matches if m[0] == 7] == [(7, 0, 2)]
        assert [m for m in blk_matches if m[0] == 9] == [(9, 0, 2)]
        # the shared plain id reports once per offset, not once per pattern
        threes = [m for m in blk_matches if m[0] == 3]
        assert len(threes) == len(set(threes)) > 1000
    # out of order and with an empty block between: matches in index order
    offs2, lens2 = [offs[2], 5, offs[0], offs[1]], [lens[2], 0, lens[0], lens[1]]
    same(hs.report_records_host(db, keys, rids, image, offs2, lens2),
         hs.report_records_emulated(db, keys, rids, image, offs2, lens2))
    same(hs.report_records_host(db, keys, rids, image, offs2, lens2, cap=5),
         hs.report_records_emulated(db, keys, rids, image, offs2, lens2, cap=5))


def test_overlapping_blocks_are_refused():
    db = hs.compile_lit_multi([b"ab"], [0], [1], hs.MODE_BLOCK)
    image = np.frombuffer(b"abababab", np.uint8)
    keys = np.array([(e << 24) for e in (1, 3, 5, 7)], np.uint64)
    rids = np.zeros(4, np.uint32)
    assert hs.report_records_emulated(db, keys, rids, image, [0, 3], [4, 5])[0] == hs.INVALID
    # a zero-length block may lie anywhere
    rc, total, counts, _, _ = hs.report_records_emulated(db, keys, rids, image, [0, 2, 4],
                                                         [4, 0, 4])
    assert rc == hs.SUCCESS and total == 4 and list(counts) == [2, 0, 2]
