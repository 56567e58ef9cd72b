#!/usr/bin/env python3
"""bench.py — GB/s scanned, hsbench block mode, FDR 5k-literal database
(BASELINE.json configs[3], the north star's headline workload).

The corpus is ONE 4 GiB synthetic corpus made of 4 x 1 GiB blocks (each
block one hs_scan / hwlmExec call: hs_scan takes a 32-bit length,
src/hs_runtime.h:479).  One step = one pass of the hot path over the whole
corpus: every rank scans its stripe of it (one device launch), its confirmed
matches are sorted on the device into the reference callback order and their
count is read back; with N > 1 ranks the step ends with the RCCL gather of
every rank's match records to rank 0, merged in end order (where the
sequential host replay would run).  Inputs are resident in HBM before the
timed region.

Multi-GPU: one process per GPU.  `--gpus N` without a torchrun
environment spawns the N rank processes itself (before any GPU call); under
torchrun (WORLD_SIZE set) it checks N against WORLD_SIZE.  The corpus's end
positions are cut into N contiguous ranges (vectorscan_amd/stripe.py
plan_corpus_stripes): rank r holds its range plus the 7 bytes before it and
scans one window per block it overlaps, reporting only its own ends, so the
union over ranks is exactly the single-GPU match set (strong scaling: total
work fixed).  The timed region is bracketed by barrier + synchronize and the
max over ranks is reported.

A plain run (`--gpus N --steps K --warmup W`) sets up, settles the clock,
runs the W warmup and the K timed steps and prints the result line; with
`--dump-outputs DIR` it also writes the last timed step's records to
DIR/*.npy (dump_outputs below).  Everything else is a side leg behind
`--full`: the read-ceiling probe, parity, the CPU baseline and the two
end-to-end lines (their fields are null in a plain run's line).

Parity (`--full`): rank 0 checks the TIMED step's gathered records, per
block, against the oracle (oracle/oracle.c, the scalar restatement) over all
4 GiB, order-exact: the block's (end, id) sequence as sorted on the device
equals the oracle's callback sequence element for element (`parity_bytes` =
bytes checked).  The end_to_end line's delivered (id, from, to) sequences are
checked per block against oracle/hs_lit.py (digest + count).

Extra JSON fields: roofline (rank 0's scan kernel from hipEvents vs the 8 TB/s
MI355X peak; PMC traffic from profiles/; with `--full` the measured read
ceiling beside it), and with `--full` cpu_baseline (the SSE2 port of
the reference FDR main loop over the same 4 GiB, one pinned thread per
physical core the process may use, capped by the cgroup CPU quota, its match
set checked too).
"""
import argparse
import json
import os
import random
import socket
import sys
import time

import numpy as np

# Kernel arguments in device memory, not host memory: the scan kernel reads
# its ~600-byte argument block at start, and from host memory that is a
# PCIe round trip per dependent read (measured 2.6 us off the 512 MiB rank
# step, profiles/r06/r06n_gap_knobs.jsonl).  A runtime setting read when
# HIP initializes, so set before any GPU call; an explicit setting wins.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PRINTABLE = np.arange(0x20, 0x7F, dtype=np.uint8)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip table (spec)
CHUNK = 64 << 20       # corpus generation unit (position-addressable)


def make_literals(n, seed=12, minlen=4, maxlen=8, nocase_frac=0.02):
    """cfg 4 literal set: printable, length 4-8, 2% nocase."""
    import vectorscan_amd as vsa
    r = random.Random(seed)
    lits = []
    for i in range(n):
        ln = r.randint(minlen, maxlen)
        s = bytes(r.randint(0x20, 0x7E) for _ in range(ln))
        lits.append(vsa.HwlmLiteral(s, r.random() < nocase_frac, i))
    return lits


def make_mixed_set(n, seed=21, minlen=4, maxlen=16, shared_ids=True):
    """cfg-5-shaped pure-literal database (the regex mix of cfg 5 needs the
    reference's full compiler, out of scope): n printable literals of length
    minlen-maxlen (the ones past 8 bytes confirmed on the host), flags mixed
    70 % plain / 10 % CASELESS / 10 % SINGLEMATCH / 10 % SOM_LEFTMOST, ~10 %
    of ids shared by two patterns (SINGLEMATCH and SOM made consistent per
    id, as hs_compile requires; hsbench expression files need unique ids:
    shared_ids=False).  Returns (exprs, flags, ids)."""
    from vectorscan_amd import hs
    r = random.Random(seed)
    mix = [0] * 7 + [hs.FLAG_CASELESS, hs.FLAG_SINGLEMATCH, hs.FLAG_SOM_LEFTMOST]
    exprs, flags, ids = [], [], []
    single, som = {}, {}
    for i in range(n):
        ln = r.randint(minlen, maxlen)
        exprs.append(bytes(r.randint(0x20, 0x7E) for _ in range(ln)))
        ident = r.randrange(i) if i and r.random() < 0.1 and shared_ids else i
        f = r.choice(mix)
        s = single.setdefault(ident, bool(f & hs.FLAG_SINGLEMATCH))
        f = ((f | hs.FLAG_SINGLEMATCH) & ~hs.FLAG_SOM_LEFTMOST) if s else \
            (f & ~hs.FLAG_SINGLEMATCH)
        m = som.setdefault(ident, bool(f & hs.FLAG_SOM_LEFTMOST))
        flags.append((f | hs.FLAG_SOM_LEFTMOST) if m else (f & ~hs.FLAG_SOM_LEFTMOST))
        ids.append(ident)
    return exprs, flags, ids


def plant_plan(n, lits, seed, plant_every):
    """positions + literal bytes planted once per `plant_every` bytes."""
    r = np.random.default_rng(seed + 1)
    k = n // plant_every
    which = r.integers(0, len(lits), k)
    pos = np.arange(k, dtype=np.int64) * plant_every + r.integers(0, plant_every - 8, k)
    idx, val = [], []
    for p, w in zip(pos.tolist(), which.tolist()):
        s = lits[w].s
        idx.extend(range(p, p + len(s)))
        val.extend(s)
    return np.array(idx, np.int64), np.array(val, np.uint8)


def make_corpus(n, lits, seed=5, plant_every=64 << 10):
    """numpy version (tests): uniform printable bytes + planted literals."""
    r = np.random.default_rng(seed)
    data = PRINTABLE[r.integers(0, len(PRINTABLE), n, dtype=np.int64)]
    idx, val = plant_plan(n, lits, seed, plant_every)
    data[idx] = val
    return data


def make_corpus_device(torch, lo, hi, total, lits, seed, plant_every, device, plan=None):
    """Bytes [lo, hi) of the synthetic corpus of `total` bytes, generated on
    the GPU (torch is plumbing here).  Position-addressable: 64 MiB chunk k
    comes from its own generator, so every rank builds exactly its stripe of
    the same global corpus."""
    out = torch.empty(hi - lo, dtype=torch.uint8, device=device)
    g = torch.Generator(device=device)
    for k in range(lo // CHUNK, (hi - 1) // CHUNK + 1 if hi > lo else 0):
        g.manual_seed(seed * 1000003 + k)
        c = torch.randint(0x20, 0x7F, (CHUNK,), dtype=torch.uint8, device=device, generator=g)
        a, b = max(lo, k * CHUNK), min(hi, (k + 1) * CHUNK)
        out[a - lo:b - lo] = c[a - k * CHUNK:b - k * CHUNK]
    idx, val = plan if plan is not None else plant_plan(total, lits, seed, plant_every)
    sel = (idx >= lo) & (idx < hi)
    if sel.any():
        out[torch.from_numpy(idx[sel] - lo).to(device)] = torch.from_numpy(val[sel]).to(device)
    return out


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawned(rank, world, port, args):
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    run(args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--gib", type=float, default=4.0, help="corpus GiB (whole job)")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--lits", type=int, default=5000)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (what scan_wait / results hand "
                         "a caller) as DIR/<name>.npy, float64")
    ap.add_argument("--full", action="store_true",
                    help="also run the side legs around the timed steps: the read-ceiling "
                         "probe, full-corpus parity against the oracle, the CPU baseline, the "
                         "end-to-end and cfg-5-proxy lines (each has a --no-* switch below)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline timing")
    ap.add_argument("--no-e2e", action="store_true",
                    help="skip the end-to-end (matches delivered to the host) line")
    ap.add_argument("--no-cfg5", action="store_true",
                    help="skip the cfg-5-shaped hsbench pass (end_to_end_cfg5proxy)")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="one scan context: each step completed before the next is queued")
    ap.add_argument("--no-settle", action="store_true",
                    help="skip the clock-settle launches before the warmup steps")
    ap.add_argument("--dist", action="store_true",
                    help="run the N > 1 exchange (process group, PackedGather collectives) "
                         "even at N = 1: the RCCL path on a one-GPU box")
    ap.add_argument("--no-ceiling", action="store_true",
                    help="skip the streaming-read ceiling probe (roofline.peak_measured)")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="host threads for the oracle / cpu_baseline (default min(16, cpus))")
    args = ap.parse_args()
    env_world = int(os.environ.get("WORLD_SIZE", "0"))
    if env_world:
        if args.gpus not in (1, env_world):
            raise SystemExit("bench: --gpus %d but WORLD_SIZE=%d" % (args.gpus, env_world))
        args.gpus = env_world
        run(args)
    elif args.gpus > 1:
        # one process per GPU, started before this process touches the GPU
        import torch.multiprocessing as mp
        mp.spawn(_spawned, args=(args.gpus, _free_port(), args), nprocs=args.gpus, join=True)
    else:
        run(args)


def run(args):
    import torch
    import vectorscan_amd as vsa
    from vectorscan_amd import stripe

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    # VSA_BENCH_BACKEND=gloo rehearses the N > 1 path on fewer GPUs than
    # ranks (ranks share devices round-robin); the driver's runs use RCCL
    backend = os.environ.get("VSA_BENCH_BACKEND", "nccl")
    dev = torch.device("cuda", local % max(1, torch.cuda.device_count())
                       if backend != "nccl" else local)
    torch.cuda.set_device(dev)
    if world > 1 or args.dist:
        import torch.distributed as dist
        if world == 1:
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(_free_port()))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    ctx = vsa.Context(dev.index)
    lits = make_literals(args.lits, seed=12)
    blob = vsa.hwlm_build(lits)
    db = vsa.Database(ctx, blob)

    total = int(args.gib * (1 << 30))
    bl = (total + args.blocks - 1) // args.blocks
    nblocks = (total + bl - 1) // bl
    plant_every = 64 << 10
    pplan = plant_plan(total, lits, 5, plant_every)
    cuts, plan = stripe.plan_corpus_stripes(total, bl, world)
    wins = plan[rank]
    # this rank's bytes: its windows (own range + 7-byte halo), from g0
    g0 = min((w.wlo for w in wins), default=cuts[rank]) & ~1023
    g1 = cuts[rank + 1]
    data = make_corpus_device(torch, g0, g1, total, lits, 5, plant_every, dev, pplan)
    torch.cuda.synchronize()
    # the rank's buffer holds corpus bytes [g0, g1): blocks are addressed in
    # corpus coordinates from data_ptr - g0, so the match keys come out as
    # global end offsets.  g0 is 1 KiB-aligned like the kernel's segment
    # origins, so no read falls below the buffer.
    dptr = data.data_ptr() - g0
    offs = [w.wlo for w in wins]
    lens = [w.wlen for w in wins]
    rlos = [w.rlo for w in wins]
    local_bytes = g1 - cuts[rank]

    # Steps are pipelined over two scan contexts (own plan, counters and
    # output buffers each; one stream and the database shared, so scans run
    # one at a time in queue order and each kernel time is its own): step
    # k's scan is queued
    # before step k-1 is completed on the host, so its sort, count readback
    # and host turnaround run while step k's scan is on the GPU instead of
    # between two scans.  Every step still scans the whole corpus, sorts its
    # records in HBM and has its count read (all timed counts are checked);
    # the timed region ends after the last step is complete.  --no-pipeline:
    # one context, each step completed before the next is queued.
    #
    # N > 1 (stripe.PackedGather): a rank's sorted records are packed on the
    # device behind its asynchronous scan (vsa_scan_pack: the count rides in
    # the header, no host read), then ONE RCCL all-gather of the 8-byte
    # headers and ONE gather of the packed records to rank 0 over xGMI; the
    # host reads the headers only when the step is completed.  Rank 0
    # concatenates the ranks' records = global end order (keys are corpus
    # offsets).
    st = {"keys": None, "ids": None}
    nslot = 1 if args.no_pipeline else 2
    ctxs = [ctx] + [vsa.Context(share_stream_with=ctx) for _ in range(nslot - 1)]
    # the rank's windows as one launch plan per context (block table +
    # segment map on the device, built once: vsa_plan_create)
    plans = [c.plan(dptr, offs, lens, None, None, rlos) for c in ctxs]
    slots = []
    for c, pl in zip(ctxs, plans):
        sl = {"ctx": c, "plan": pl}
        if dist is not None:
            # the context's stream: the collectives wait for the pack on the GPU
            cs = torch.cuda.ExternalStream(c.stream, device=dev)
            sl["pg"] = stripe.PackedGather(dist, world, dev)
            sl["pack"] = (lambda c_: lambda buf, cap: c_.scan_pack(buf.data_ptr(), cap))(c)
            sl["wait"] = (lambda s_: lambda: torch.cuda.current_stream().wait_stream(s_))(cs)
        slots.append(sl)
    kms = []

    def issue(k):
        sl = slots[k % nslot]
        if dist is None:
            sl["ctx"].scan_plan(db, sl["plan"], asynchronous=True)
        else:
            # the scan's binned sort writes the records straight into this
            # slot's collective buffer (vsa_scan_plan_pack: no pack launch);
            # a rescan is repacked by finish() through scan_pack
            pg = sl["pg"]
            sl["ctx"].scan_plan_pack(db, sl["plan"], pg.pk_dev.data_ptr(), pg.cap)
            pg.start(None, sl["wait"])

    def complete(k):
        sl = slots[k % nslot]
        c = sl["ctx"]
        if dist is None:
            n = c.scan_wait()
        else:
            cl = sl["pg"].finish(sl["pack"], sl["wait"], c.scan_wait)
            if rank == 0:
                st["keys"], st["ids"] = sl["pg"].merged(cl)
            n = int(sum(cl))
        km = c.kernel_ms()
        if km >= 0:  # a timed launch (vsa_ctx_set_timing)
            kms.append(km)
        return n

    def run_steps(k_steps):
        """k_steps steps, pipelined nslot deep; their counts in step order"""
        counts = []
        for k in range(k_steps):
            issue(k)
            if k >= nslot - 1:
                counts.append(complete(k - nslot + 1))
        for k in range(max(0, k_steps - nslot + 1), k_steps):
            counts.append(complete(k))
        return counts

    # Clock settle (untimed, before the W warmup steps): after an idle
    # period the GPU's power management takes ~30-40 launches (~40 ms of
    # this load) to settle -- launch 2 runs ~1.4 ms, launch 30 ~0.94 ms, and
    # the same ramp reappears after 0.5 s idle (profiles/r03_ramp.jsonl,
    # tools/exp_ramp.py).  Scanning until the kernel time is stable makes the
    # timed steps the steady state whatever W is; how many launches that
    # took is reported ("settle").
    settle_n, t_settle = 0, time.perf_counter()
    if not args.no_settle:
        hist = []
        while settle_n < 400 and time.perf_counter() - t_settle < 3.0:
            # the rank's own scan only: ranks settle independently, no collective
            ctx.scan_plan(db, plans[0])
            settle_n += 1
            hist.append(ctx.kernel_ms())
            if settle_n >= 40 and max(hist[-8:]) <= 1.02 * min(hist[-8:]):
                break
    t_settle = time.perf_counter() - t_settle
    # the box's streaming-read ceiling over this rank's own corpus buffer
    # (untimed; a plain 16-byte-load kernel, vsa_read_ceiling): the HBM rate
    # a scan could reach here, beside the 8 TB/s spec peak
    ceiling = None
    if args.full and not args.no_ceiling:
        ceiling = ctx.read_ceiling(data.data_ptr(), data.numel(), 5)
    if dist is not None:
        dist.barrier()
    # from here on only every 4th launch of a context carries the timing
    # events (they cost ~4 us per dispatch at 512 MiB: a rank's step is
    # timed by the wall clock, the kernel average by the sampled launches)
    every = max(1, min(4, args.steps // 4))
    for sl in slots:
        sl["ctx"].timing(every)
    run_steps(args.warmup)

    def barrier():
        if dist is not None:
            dist.barrier()

    kms.clear()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counts = run_steps(args.steps)
    torch.cuda.synchronize()
    barrier()
    t1 = time.perf_counter()
    el = t1 - t0
    nm = counts[-1]
    last = slots[(args.steps - 1) % nslot]["ctx"]
    ncand = int(last.candidates())  # rank 0, last timed step
    if dist is not None:
        tt = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        el = float(tt.item())
    ms_step = el / args.steps * 1e3
    gbs = total / (el / args.steps) / 1e9

    # records of the last timed step, global offsets (rank 0): read back
    # only for the parity check and --dump-outputs
    full = args.full
    if rank == 0 and ((full and not args.no_parity) or args.dump_outputs):
        if dist is None:
            res = last.results(nm)
            keys, ids = res["key"], res["id"].astype(np.uint64)
        else:
            keys = st["keys"].cpu().numpy().view(np.uint64)
            ids = st["ids"].cpu().numpy().astype(np.uint64)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, keys, ids, counts)
    kavg = float(np.mean(kms))
    e2e = None
    if world == 1 and full and not args.no_e2e:
        try:
            e2e = end_to_end(lits, data.data_ptr(), bl, nblocks, total, nm, args.steps)
        except Exception as e:  # a side measurement never voids the bench line
            e2e = {"error": repr(e)}
    del data
    torch.cuda.empty_cache()
    cfg5 = None
    if world == 1 and full and not args.no_cfg5:
        try:
            cfg5 = cfg5_proxy(torch, dev, args.steps, args.no_parity, args.cpu_threads)
        except Exception as e:  # a side measurement never voids the bench line
            cfg5 = {"error": repr(e)}
        torch.cuda.empty_cache()

    out = None
    # the CPU baseline is timed at N = 1 only (on rank 0); N > 1 runs check
    # parity alone
    with_cpu = not args.no_cpu and world == 1
    parity, parity_bytes, cpu = None, 0, None
    if rank == 0 and full:
        import oracle
        # one pinned thread per physical core the process may use
        # (all physical host cores), capped by the cgroup CPU
        # quota: the GPU box shows 128 physical cores but grants 16 CPUs, and
        # past the quota the threads are throttled -- short best-of-3 runs
        # burst above it (profiles/r04e_cpu_threads.jsonl: 16 / 128 threads
        # 21 / 66 GB/s on 1 GiB), but over the whole 4 GiB corpus 128 threads
        # gave 12.7 GB/s against 25-30 GB/s for 16 (profiles/r04f_bench.json,
        # r04d_bench.json)
        pins, quota, visible, phys = host_cpu_share()
        cap = len(pins) if quota is None else max(1, min(len(pins), int(quota + 0.5)))
        threads = args.cpu_threads or cap
        oracle.set_pin(pins)
        eng = vsa.engine_blob(blob)
        if not args.no_parity:
            # order-exact: the timed step's (end, id) sequence of every block,
            # in the order the device sort put it (end, bucket, LitInfo chain =
            # the reference's callback order, fdr.c:299-333), equal element
            # for element to the oracle's callback sequence of that block
            ends = keys >> np.uint64(24)
            blk = ends // np.uint64(bl)
            bad, t_cpu, cpu_ok = [], 0.0, True
            n_want = 0
            e2e_chk = e2e is not None and "_digests" in e2e
            if e2e_chk:
                # the end-to-end line's delivered sequences vs oracle/hs_lit.py:
                # the same patterns compiled by the restatement, their HWLM
                # blob from the product builder (byte-identical to the hs
                # database's, tests/test_hs_lit.py), its records through the
                # restated report program, per block
                import oracle.hs_lit as ohl
                from vectorscan_amd import hs
                odb = ohl.compile_lit_multi([l.s for l in lits],
                                            [ohl.CASELESS if l.nocase else 0 for l in lits],
                                            [l.id for l in lits])
                oblob = vsa.hwlm_build([vsa.HwlmLiteral(t, nc, f, noruns=nr)
                                        for t, nc, f, nr in odb.hwlm_literals()])
                oeng = vsa.engine_blob(oblob)
                e2e_bad = []
            for b in range(nblocks):
                lo, hi = b * bl, min(total, (b + 1) * bl)
                host = make_corpus_device(torch, lo, hi, total, lits, 5, plant_every, dev,
                                          pplan).cpu().numpy()
                if e2e_chk:
                    he, hi_ = oracle.records_mt(oeng, host, threads, nood=oblob.is_noodle)
                    seq = ohl.scan_records(odb, host, zip(he.tolist(), hi_.tolist()))
                    if (hs.seq_digest(seq) != e2e["_digests"][b] or
                            len(seq) != e2e["_counts"][b]):
                        e2e_bad.append(b)
                oe, oi = oracle.records_mt(eng, host, threads)
                n_want += len(oe)
                sel = blk == np.uint64(b)
                ge, gi = ends[sel] - np.uint64(lo), ids[sel]
                # the block's records are one contiguous run of the sequence
                run = np.flatnonzero(sel)
                contiguous = len(run) == 0 or run[-1] - run[0] + 1 == len(run)
                if not (contiguous and len(ge) == len(oe) and np.array_equal(ge, oe) and
                        np.array_equal(gi.astype(np.uint32), oi)):
                    bad.append(b)
                if with_cpu:
                    # CPU baseline: the SSE2 port of fdr.c's main loop
                    # (get_conf_stride_1 :145-213 + confirm), same bytes,
                    # same host threads; its match set must equal the oracle's
                    tc = time.perf_counter()
                    d = oracle.digest_mt(eng, host, threads, simd=True)
                    t_cpu += time.perf_counter() - tc
                    cpu_ok = cpu_ok and d == oracle.digest_of(oe, oi)
                parity_bytes += hi - lo
                del host
            parity = (not bad and n_want == nm and len(keys) == nm and
                      all(c == nm for c in counts))
            if not parity:
                print("bench: PARITY FAILURE in blocks %s (records %d, oracle %d)" %
                      (bad, nm, n_want), file=sys.stderr, flush=True)
            if e2e_chk:
                e2e["parity"] = not e2e_bad
                e2e["parity_kind"] = ("order-exact: per-block digest of the delivered "
                                      "(id, from, to) callback sequence and its count vs "
                                      "oracle/hs_lit.py over all %d bytes" % parity_bytes)
                if e2e_bad:
                    print("bench: END-TO-END PARITY FAILURE in blocks %s" % e2e_bad,
                          file=sys.stderr, flush=True)
        if e2e is not None:
            e2e.pop("_digests", None)
            e2e.pop("_counts", None)
            if with_cpu:
                cpu = {"value": round(parity_bytes / t_cpu / 1e9, 4), "unit": "GB/s",
                       "cores": threads, "kind": "port", "match_set_equal": cpu_ok,
                       "pinned": "one thread per physical core, as many as the cgroup CPU quota "
                                 "grants", "physical_cores": phys,
                       "cpus_visible": visible, "cpu_quota": quota,
                       "sample": "the whole %d-byte corpus, 4 x 1 GiB blocks: oracle/oracle.c "
                                 "SSE2 port of the reference FDR main loop (fdr.c:145-333, "
                                 "m128 state, flood checks) over the FDR bytecode this "
                                 "repository builds (csrc/compile.cpp, the restated "
                                 "fdr_compile.cpp; byte identity with a reference-built blob "
                                 "unpinned), its own domain-%d table, %d threads over "
                                 "contiguous stripes (7-byte halo); host: %s" % (parity_bytes, blob_domain(blob), threads,
                                                     _cpu_model())}
    if rank == 0:
        alg_bytes = local_bytes + 16 * nm // world  # rank 0's input + its share of records
        achieved = alg_bytes / (kavg * 1e-3) / 1e9
        traffic = None
        pmc = os.path.join(ROOT, "profiles", "pmc_fdr5k_4gib.json")
        if world == 1 and os.path.exists(pmc):
            try:
                traffic = json.load(open(pmc)).get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        out = {
            "metric": "GB/s scanned (hsbench block mode), FDR 5k literals",
            "value": round(gbs, 3),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_step, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic (uniform printable 0x20-0x7E, 1 planted literal / 64 KiB)",
            "config": {"workload": "cfg4: FDR %d literals len 4-8 (2%% nocase), one %.0f GiB "
                                   "corpus as %d blocks striped over %d GPU(s), engine id %s" %
                                   (args.lits, args.gib, nblocks, world, blob.engine_id),
                       "global_bytes": total, "parallelism": "stripe%d" % world,
                       "exchange": ("rccl" if dist is not None and backend == "nccl" else
                                    backend if dist is not None else None)},
            "matches": nm,
            "confirm_candidates": ncand,
            "parity": parity,
            "parity_bytes": parity_bytes,
            "parity_kind": "order-exact: every block's (end, id) sequence equal element for "
                           "element to the oracle's callback sequence",
            "roofline": {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "traffic": traffic, "kernel_ms": round(kavg, 4),
                         "peak_measured": round(ceiling[0], 1) if ceiling else None,
                         "frac_of_measured": round(achieved / ceiling[0], 4) if ceiling else None,
                         "peak_measured_how": "vsa_read_ceiling: plain 16-byte-load read of "
                                              "%d bytes of this rank's corpus buffer, best of 5, "
                                              "untimed setup" % ceiling[2] if ceiling else None,
                         "scope": "rank 0 scan kernel (%d input bytes)" % local_bytes},
            "cpu_baseline": cpu,
            "pipeline": nslot,
            "full": full,
            "end_to_end": e2e,
            "end_to_end_cfg5proxy": cfg5,
            "settle": {"launches": settle_n, "s": round(t_settle, 3),
                       "why": "GPU clock ramp after idle (profiles/r03_ramp.jsonl): untimed "
                              "scans until the kernel time is stable, before the warmup"},
        }
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    for pl in plans:
        pl.close()
    db.close()
    for c in ctxs:
        c.close()


DUMP_CAP_BYTES = 48 << 20  # --dump-outputs: all files together stay well under 64 MB


def dump_outputs(out_dir, keys, ids, counts):
    """--dump-outputs: what the timed path handed its caller in the last
    timed step, as float64 .npy files (every value is an integer below 2^53,
    so float64 holds it exactly):
      match_end.npy      end offset of every record in the corpus, in the
                         order the device sort delivered them (key >> 24)
      match_order.npy    the key's low 24 bits (the sort's tie-break within
                         one end offset: bucket and LitInfo chain position)
      match_id.npy       the record's literal id
      step_counts.npy    the match count every timed step returned
      sample_index.npy   the positions in the record sequence the three
                         match_* files hold: all of them, or past the size
                         cap a fixed seeded sample in ascending order
    The inputs are seeded, so two builds run with the same arguments can be
    compared file for file."""
    os.makedirs(out_dir, exist_ok=True)
    n = len(keys)
    rows = DUMP_CAP_BYTES // (4 * 8)
    if n > rows:
        sel = np.sort(np.random.default_rng(20240607).choice(n, rows, replace=False))
    else:
        sel = np.arange(n)
    k = np.asarray(keys, np.uint64)[sel]
    arrays = {
        "match_end": k >> np.uint64(24),
        "match_order": k & np.uint64(0xFFFFFF),
        "match_id": np.asarray(ids)[sel],
        "step_counts": np.asarray(counts),
        "sample_index": sel,
    }
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float64))


def end_to_end(lits, d_data, bl, nblocks, total, hwlm_records, reps):
    """hsbench block mode end to end (tools/hsbench/main.cpp:487-511), beside
    `value` (which stops at the sorted records in HBM): the same literals as
    a pure-literal hs database (id = literal index, nocase -> CASELESS), the
    same bytes as `nblocks` hs_scan blocks, every match delivered to the host
    through the report program and counted; `reps` passes pipelined
    (vsa_hs_corpus_scan_repeats: pass k + 1 scans on the GPU while the host
    replays pass k), after 60 untimed passes (compiling the database idles
    the GPU long enough for its clock to drop: the same settle as `value`).
    Every pass replays every record through the report program into a
    callback (the per-block sequence digests ask for it; without them a
    one-record-one-match database only counts on the GPU); the last pass's
    per-block digests of the delivered (id, from, to) sequences are returned
    under "_digests" for the parity check against oracle/hs_lit.py."""
    from vectorscan_amd import hs
    db = hs.compile_lit_multi([l.s for l in lits],
                              [hs.FLAG_CASELESS if l.nocase else 0 for l in lits],
                              [l.id for l in lits], hs.MODE_BLOCK)
    scratch = hs.Scratch(db)
    offs = [b * bl for b in range(nblocks)]
    lens = [min(total, (b + 1) * bl) - b * bl for b in range(nblocks)]
    corpus = hs.Corpus(db, scratch, d_data, offs, lens)
    try:
        for _ in range(2):
            rc, _, _, _ = corpus.scan_repeats(30, digests=True)
            if rc:
                return {"error": rc}
        t0 = time.perf_counter()
        rc, tot, cnt, dg = corpus.scan_repeats(reps, counts=True, digests=True)
        el = time.perf_counter() - t0
        if rc:
            return {"error": rc}
        return {"value": round(total * reps / el / 1e9, 3), "unit": "GB/s",
                "ms_per_pass": round(el / reps * 1e3, 4), "passes": reps,
                "matches_per_pass": int(tot[-1]), "hwlm_records": int(hwlm_records),
                "what": "hs_scan of each block with every match delivered to a host callback "
                        "through the report program (pure-literal hs database of the same "
                        "literals; pipelined passes, replay threads per block)",
                "_digests": [int(x) for x in dg], "_counts": [int(x) for x in cnt]}
    finally:
        corpus.close()
        scratch.close()
        db.close()


def cfg5_proxy(torch, dev, reps, no_parity=False, cpu_threads=0):
    """hsbench block mode at cfg 5's shape (BASELINE configs[4]), the part of
    it this image can build: cfg 5 is a 10k mixed-REGEX database, whose
    compile needs the reference's full compiler (Ragel / Boost, absent), so
    the database here is its pure-literal proxy -- make_mixed_set(10000):
    10k printable literals of length 4-16 (the ones past 8 bytes confirmed on
    the host), 70 % plain / 10 % CASELESS / 10 % SINGLEMATCH / 10 %
    SOM_LEFTMOST, unique ids as hsbench expression files have -- over 1 GiB
    in HBM cut into hsbench's 16 KiB chunks (65,536 hs_scan blocks), a
    literal planted per 64 KiB.  `reps` pipelined passes
    (vsa_hs_corpus_scan_repeats: pass k + 1 scans on the GPU while the host
    replays pass k through the report program, the host-side confirm of the
    north star), after an untimed settle; every pass delivers every match to
    a host callback.  Parity: every chunk's delivered (id, from, to) sequence
    digest and count of the last pass vs oracle/hs_lit.py over the oracle's
    own HWLM records of that chunk (oracle.records_blocks), all 65,536
    chunks."""
    import vectorscan_amd as vsa
    from vectorscan_amd import hs
    exprs, flags, ids = make_mixed_set(10000, shared_ids=False)
    lits = [vsa.HwlmLiteral(e, False, i) for i, e in enumerate(exprs)]
    n, chunk = 1 << 30, 16 << 10
    data = make_corpus_device(torch, 0, n, n, lits, 9, 64 << 10, dev)
    host = data.cpu().numpy()
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    scratch = hs.Scratch(db)
    offs = np.arange(0, n, chunk, dtype=np.uint64)
    lens = np.full(len(offs), chunk, np.uint64)
    corpus = hs.Corpus(db, scratch, data.data_ptr(), offs, lens, h_data=host)
    threads = 16
    try:
        for _ in range(2):  # settle (compiling idled the GPU), as end_to_end
            rc, _, _, _ = corpus.scan_repeats(30, threads=threads)
            if rc:
                return {"error": rc}
        t0 = time.perf_counter()
        rc, tot, cnt, dg = corpus.scan_repeats(reps, counts=True, threads=threads, digests=True)
        el = time.perf_counter() - t0
        if rc:
            return {"error": rc}
        out = {"value": round(n * reps / el / 1e9, 3), "unit": "GB/s",
               "ms_per_gib": round(el / reps * 1e3 * (1 << 30) / n, 4), "passes": reps,
               "matches_per_pass": int(tot[-1]), "chunks": len(offs),
               "live_chunks": int(np.count_nonzero(cnt)), "replay_threads": threads,
               "what": "cfg-5-shaped hsbench block mode: pure-literal proxy of the 10k mixed-regex "
                       "database (make_mixed_set(10000), mixed CASELESS / SINGLEMATCH / "
                       "SOM_LEFTMOST, literals 4-16 B), 1 GiB as 16 KiB hs_scan chunks, pipelined "
                       "passes, every match delivered to a host callback through the report "
                       "program"}
        if not no_parity:
            import oracle
            import oracle.hs_lit as ohl
            odb = ohl.compile_lit_multi(exprs, flags, ids)
            oblob = vsa.hwlm_build([vsa.HwlmLiteral(t, nc, f, noruns=nr)
                                    for t, nc, f, nr in odb.hwlm_literals()])
            e, i, b = oracle.records_blocks(vsa.engine_blob(oblob), host, chunk,
                                            cpu_threads or min(16, os.cpu_count() or 1))
            want_n = np.zeros(len(offs), np.uint64)
            want_d = np.zeros(len(offs), np.uint64)
            cuts = np.flatnonzero(np.diff(b.astype(np.int64))) + 1
            for lo, hi in zip(np.r_[0, cuts], np.r_[cuts, len(b)]):
                if hi <= lo:
                    continue
                k = int(b[lo])
                seq = ohl.scan_records(odb, host[k * chunk:(k + 1) * chunk],
                                       zip(e[lo:hi].tolist(), i[lo:hi].tolist()))
                want_n[k] = len(seq)
                want_d[k] = hs.seq_digest(seq)
            bad = np.flatnonzero((want_n != cnt) | (want_d != dg))
            out["parity"] = len(bad) == 0 and all(int(t) == int(want_n.sum()) for t in tot)
            out["parity_kind"] = ("order-exact per chunk: digest of the delivered (id, from, to) "
                                  "callback sequence and its count vs oracle/hs_lit.py over all "
                                  "%d chunks; every pass's total equal" % len(offs))
            if len(bad):
                print("bench: CFG5 PROXY PARITY FAILURE in chunks %s" % bad[:8].tolist(),
                      file=sys.stderr, flush=True)
        return out
    finally:
        corpus.close()
        scratch.close()
        db.close()
        del data


def blob_domain(blob):
    """FDR.domain of the blob's engine (fdr_internal.h:69-85, byte 25)"""
    import ctypes
    return ctypes.string_at(blob.ptr + 192 + 25, 1)[0]


def host_cpu_share():
    """The host CPUs this process may use (the CPU baseline runs
    one pinned thread per physical core): the affinity set, one CPU per
    physical core (/sys topology: lowest-numbered sibling), and the cgroup
    CPU quota (cpu.max), which caps how many of them can run at once.
    Returns (pin list, quota CPUs or None, visible CPUs, physical cores)."""
    allowed = sorted(os.sched_getaffinity(0))
    cores = {}
    for c in allowed:
        try:
            base = "/sys/devices/system/cpu/cpu%d/topology/" % c
            key = (open(base + "physical_package_id").read().strip(),
                   open(base + "core_id").read().strip())
        except OSError:
            key = ("?", str(c))
        cores.setdefault(key, c)
    pins = sorted(cores.values())
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(period)
    except (OSError, ValueError):
        pass
    return pins, quota, os.cpu_count() or len(allowed), len(pins)


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return "%s, %d cpus visible" % (line.split(":", 1)[1].strip(), os.cpu_count())
    except OSError:
        pass
    return "unknown"


if __name__ == "__main__":
    main()
