"""The report program on the device (vsa_hs_corpus_prepare_device /
_scan_device / _scan_matches / _matches_device, vectorscan_amd/csrc/report.hip)
on corpora that live only in HBM: every block's match sequence equals the
oracle's, in order, with counts, total and sequence digests.  No host copy of
the corpus is passed anywhere."""
import numpy as np
import pytest

import vectorscan_amd as vsa
from vectorscan_amd import hs

import test_device_report_host as host_tests
from test_device_report_host import oracle_db, ohs, split_blocks

pytestmark = pytest.mark.gpu


class DeviceCorpus:
    """`data` uploaded at d_base + at (a fresh allocation of its size by
    default) and prepared for the device report: no host copy"""

    def __init__(self, db, data, offs, lens, d_base=None, at=0, ctx=None):
        data = np.ascontiguousarray(data, np.uint8)
        self.scratch = hs.Scratch(db)
        self.ctx = ctx or vsa.Context(0)
        self.own_ctx = ctx is None
        self.d = None
        self.corpus = None
        try:
            if d_base is None:
                self.d = d_base = self.ctx.malloc(max(1, len(data)))
            if len(data):
                self.ctx.h2d(d_base + at, data)
            self.corpus = hs.Corpus(db, self.scratch, d_base, offs, lens, device_report=True)
        except Exception:
            self.close()
            raise

    def close(self):
        if self.corpus:
            self.corpus.close()
        if self.d:
            self.ctx.free(self.d)
        if self.own_ctx:
            self.ctx.close()
        self.scratch.close()


def device_report(db, keys, ids, data, offs, lens, cap=None):
    """hs.report_records_host's arguments and results, computed by a device
    corpus from the bytes alone (the records are the scan's own)"""
    try:
        dc = DeviceCorpus(db, data, offs, lens)
    except hs.HsError as e:
        n = len(offs)
        return e.code, 0, np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(0, hs.MATCH_DTYPE)
    try:
        return dc.corpus.scan_matches(cap, counts=True, digests=cap is None)
    finally:
        dc.close()


@pytest.fixture
def on_device(monkeypatch):
    """test_device_report_host's cases with hs.report_records_host answered
    by the device: their assertions (the oracle's sequence per block, digests,
    the specific sequences) then hold the device path"""
    calls = []

    def run(*a, **kw):
        r = device_report(*a, **kw)
        calls.append(r[1])
        return r
    monkeypatch.setattr(host_tests.hs, "report_records_host", run)
    return calls


def test_ragged(on_device):
    exprs, flags, ids, image, offs, lens, odb, blob, want = host_tests.ragged_case()
    host_tests.test_report_records_host_ragged()
    assert len(on_device) == 2 and on_device[0] > 500
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    rc, total, counts, digests, matches = device_report(db, None, None, image, offs, lens)
    assert rc == hs.SUCCESS and total == sum(len(w) for w in want)
    shortest = {}
    for e, i in zip(exprs, ids):
        shortest[i] = min(len(e), shortest.get(i, len(e)))
    # an id all of whose patterns are longer than 8 bytes was matched
    assert any(shortest[int(i)] > 8 for i in np.unique(matches["id"]))


def test_edges(on_device):
    host_tests.test_report_records_host_edges()
    assert len(on_device) == 2 and on_device[0] > 0


def test_long_literals(on_device):
    host_tests.test_long_literals_bound_check()
    assert len(on_device) == 3 and on_device[2] == 0  # the last: an empty corpus


def test_state_between_groups(on_device):
    host_tests.test_state_between_groups()
    assert len(on_device) == 2


def mixed_corpus(n_lits, nbytes, corpus_seed, plant_every, **kw):
    import bench
    exprs, flags, ids = bench.make_mixed_set(n_lits, **kw)
    lits = [vsa.HwlmLiteral(e, False, i) for i, e in enumerate(exprs)]
    return exprs, flags, ids, lits, bench.make_corpus(nbytes, lits, seed=corpus_seed,
                                                      plant_every=plant_every)


def test_rescan_and_repeats():
    """more than 65,536 records: the first pass outgrows the output and
    rescans before the passes read the records; against the host replay of a
    second corpus that has the host copy; three device scans agree"""
    exprs, flags, ids, _, data = mixed_corpus(2000, 16 << 20, 17, 96)
    bl = 4 << 20
    offs, lens = [i * bl for i in range(4)], [bl, bl, bl, bl - 3]
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    dc = DeviceCorpus(db, data, offs, lens)
    try:
        rc, total, counts, digests, matches = dc.corpus.scan_matches(counts=True, digests=True)
        assert rc == hs.SUCCESS and total > 65536 and len(matches) == total
        scratch2 = hs.Scratch(db)
        ref = hs.Corpus(db, scratch2, dc.d, offs, lens, h_data=data)
        try:
            rc2, total2, counts2, digests2 = ref.scan(True, 16, digests=True)
        finally:
            ref.close()
            scratch2.close()
        assert rc2 == hs.SUCCESS and total == total2
        assert np.array_equal(counts, counts2) and np.array_equal(digests, digests2)
        assert (np.diff(matches["block"].astype(np.int64)) >= 0).all()
        for _ in range(2):
            rc3, total3, counts3 = dc.corpus.scan_device(counts=True)
            assert rc3 == hs.SUCCESS and total3 == total and np.array_equal(counts3, counts)
            rc4, d_ptr, n = dc.corpus.matches_device()
            assert rc4 == hs.SUCCESS and n == total
            again = np.zeros(n, hs.MATCH_DTYPE)
            dc.ctx.d2h(again, d_ptr)
            assert np.array_equal(again, matches)
    finally:
        dc.close()


def test_high_offsets():
    """a 4 GiB allocation of which two 64 KiB regions are written: one block
    straddles offset 2^31 (a long literal lies across it), one ends at 2^32;
    32-bit arithmetic on an offset, an end or a `to` shows here"""
    region = 64 << 10
    exprs, flags, ids, lits, a = mixed_corpus(60, region, 31, 256, seed=3, maxlen=24)
    b = mixed_corpus(60, region, 32, 256, seed=3, maxlen=24)[4]
    long_plain = [e for e, f in zip(exprs, flags) if len(e) > 12 and f == 0]
    assert long_plain
    for buf, at in ((a, region // 2 - 6), (b, region - len(long_plain[0])), (b, 100)):
        buf[at:at + len(long_plain[0])] = np.frombuffer(long_plain[0], np.uint8)
    offs = [(1 << 31) - region // 2, (1 << 32) - region]
    lens = [region, region]
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    odb, blob = oracle_db(exprs, flags, ids)
    want = [ohs.scan(odb, blob.ptr, x.copy()) for x in (a, b)]
    long_id = ids[exprs.index(long_plain[0])]
    assert (long_id, 0, region // 2 - 6 + len(long_plain[0])) in want[0]
    assert (long_id, 0, region) in want[1]
    ctx = vsa.Context(0)
    d = ctx.malloc(1 << 32)
    try:
        ctx.h2d(d + offs[1], b)
        dc = DeviceCorpus(db, a, offs, lens, d_base=d, at=offs[0], ctx=ctx)
        try:
            rc, total, counts, digests, matches = dc.corpus.scan_matches(counts=True,
                                                                        digests=True)
        finally:
            dc.close()
    finally:
        ctx.free(d)
        ctx.close()
    assert rc == hs.SUCCESS and total == len(want[0]) + len(want[1])
    got = split_blocks(matches, counts)
    for k in range(2):
        assert got[k] == want[k], "block %d" % k
        assert int(digests[k]) == hs.seq_digest(want[k])
        assert len(want[k]) > 100


def test_matches_device_pointer():
    exprs, flags, ids, image, offs, lens, odb, blob, want = host_tests.ragged_case()
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    dc = DeviceCorpus(db, image, offs, lens)
    try:
        rc, total, _, _, matches = dc.corpus.scan_matches()
        assert rc == hs.SUCCESS and total == len(matches) > 500
        rc, d_ptr, n = dc.corpus.matches_device()
        assert rc == hs.SUCCESS and n == total and d_ptr
        copy = np.zeros(n, hs.MATCH_DTYPE)
        dc.ctx.d2h(copy, d_ptr)
        assert np.array_equal(copy, matches)
    finally:
        dc.close()


def test_error_returns():
    image = np.frombuffer(b"0123456789abcdefgh..0123456789abcdefgh..", np.uint8)
    exprs, flags, ids = [b"0123456789abcdefgh", b"89ab"], [0, 0], [1, 2]
    stream_db = hs.compile_lit_multi(exprs, flags, ids,
                                     hs.MODE_STREAM | hs.MODE_SOM_HORIZON_LARGE)
    with pytest.raises(hs.HsError) as e:
        DeviceCorpus(stream_db, image, [0, 20], [20, 20])
    assert e.value.code == hs.DB_MODE_ERROR
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    with pytest.raises(hs.HsError) as e:
        DeviceCorpus(db, image, [0, 19], [20, 21])  # one byte shared
    assert e.value.code == hs.INVALID
    # zero-length blocks may lie anywhere
    dc = DeviceCorpus(db, image, [0, 10, 20, 40], [20, 0, 20, 0])
    try:
        rc, total, counts, digests, matches = dc.corpus.scan_matches(counts=True, digests=True)
        assert rc == hs.SUCCESS and total == 4 and list(counts) == [2, 0, 2, 0]
        assert matches.tolist() == [(2, 0, 0, 12), (1, 0, 0, 18), (2, 2, 0, 12), (1, 2, 0, 18)]
        # digests are folded from the copied matches: a short cap has none
        rc = dc.corpus.scan_matches(cap=3, digests=True)[0]
        assert rc == hs.INVALID
        rc, total, _, _, m = dc.corpus.scan_matches(cap=3)
        assert rc == hs.SUCCESS and total == 4 and np.array_equal(m, matches[:3])
        # the host replay has no bytes for the long literal's prefix
        assert dc.corpus.scan(True)[0] == hs.INVALID
        assert dc.corpus.scan_repeats(2)[0] == hs.INVALID
    finally:
        dc.close()
    # short literals only: the existing calls work on a device-prepared corpus
    short_db = hs.compile_lit_multi([b"89ab"], [0], [2], hs.MODE_BLOCK)
    dc = DeviceCorpus(short_db, image, [0, 20], [20, 20])
    try:
        rc, total, counts = dc.corpus.scan(True)
        assert rc == hs.SUCCESS and total == 2 and list(counts) == [1, 1]
        assert dc.corpus.scan_device(True)[1] == 2
    finally:
        dc.close()


def test_hsbench_device_report(tmp_path, capsys):
    """python -m vectorscan_amd.hsbench -N --device-report: the same totals
    and the same --echo-matches lines as the callback path, with literals
    longer than 8 bytes and no host copy kept for the corpus"""
    import json
    from vectorscan_amd import hsbench
    from test_hsbench import make_corpus
    import random
    rng = random.Random(11)
    alpha = b"abcdefgh"
    exprs = [bytes(rng.choice(alpha) for _ in range(rng.randint(3, 20))) for _ in range(80)]
    chunks = make_corpus(rng, exprs, 3, 12, 100, 2000, alpha)
    corpus = str(tmp_path / "corpus.db")
    hsbench.write_corpus(corpus, chunks)
    sig = tmp_path / "sigs"
    sig.write_text("".join("%d:/%s/%s\n" % (i, e.decode(), "H" if i % 7 == 0 else "")
                           for i, e in enumerate(exprs)))
    argv = ["-e", str(sig), "-c", corpus, "-n", "2", "-N", "--literal-on", "--json",
            "--echo-matches"]
    outs = []
    for extra in ([], ["--device-report"]):
        assert hsbench.main(argv + extra) == 0
        out = capsys.readouterr().out
        assert "WARNING" not in out
        res = json.loads(out.strip().splitlines()[-1])
        outs.append((res["matches"], [ln for ln in out.splitlines() if ln.startswith("Match @")]))
        assert res["device_report"] == bool(extra)
    assert outs[0] == outs[1] and outs[0][0] == len(outs[0][1]) > 20
    assert hsbench.main(argv[:4] + ["--literal-on", "--device-report"]) == 1  # streaming
    assert "--device-report needs block mode" in capsys.readouterr().out
