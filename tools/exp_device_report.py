#!/usr/bin/env python3
"""Per-pass wall time of the device-side report program
(hs.Corpus(device_report=True).scan_device: scan, report program and matches
all in HBM) against the host path on the same corpus (Corpus.scan_repeats with
a host copy of the corpus and 16 replay threads), cfg-5-shaped database
(bench.make_mixed_set(10000), planted once per 4 KiB).

    python tools/exp_device_report.py                 # every shape
    python tools/exp_device_report.py --shape 4x256m  # one shape

Shapes, smallest first: 64 MiB and 1 GiB of 16 KiB chunks, 4 x 256 MiB blocks
(a 4 x 1 GiB step is left out: its host leg ended with a segmentation fault
whose cause is not found).  Every shape is its own step
under its own `timeout -k 10` and the steps are chained with `&&`, so a fault
ends the run.  Within a shape
the two legs alternate, one process each, followed by one device process with
VSA_HOST_TIMING=1 for the per-stage times (that one synchronises between the
stages, so its total is not a wall time).  One JSON line per leg goes to
profiles/device_report.jsonl.  Nothing here is a pass/fail number, but a leg
whose match total differs from the other's ends the run.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIB = 1 << 20
# name: (bytes, block bytes, per-leg time limit in seconds)
SHAPES = {
    "64m_16k": (64 * MIB, 16 << 10, 120),
    "1g_16k": (1024 * MIB, 16 << 10, 180),
    "4x256m": (1024 * MIB, 256 * MIB, 180),
}
OUT = os.path.join(ROOT, "profiles", "device_report.jsonl")


def make_data(nbytes, lits):
    """printable background (64 MiB of it, tiled) with the set planted once
    per 4 KiB over the whole length"""
    import numpy as np
    import bench
    base = bench.make_corpus(min(nbytes, 64 * MIB), lits, seed=9, plant_every=1 << 40)
    data = np.tile(base, nbytes // len(base))
    idx, val = bench.plant_plan(nbytes, lits, 9, 4 << 10)
    data[idx] = val
    return data


def leg(shape, kind, passes):
    """one leg in this process; prints its JSON line"""
    import numpy as np
    import bench
    import vectorscan_amd as vsa
    from vectorscan_amd import hs
    nbytes, bl, _ = SHAPES[shape]
    exprs, flags, ids = bench.make_mixed_set(10000)
    lits = [vsa.HwlmLiteral(e, False, i) for i, e in enumerate(exprs)]
    data = make_data(nbytes, lits)
    offs = np.arange(0, nbytes, bl, dtype=np.uint64)
    lens = np.full(len(offs), bl, np.uint64)
    db = hs.compile_lit_multi(exprs, flags, ids, hs.MODE_BLOCK)
    scratch = hs.Scratch(db)
    ctx = vsa.Context(0)
    d = ctx.malloc(nbytes)
    ctx.h2d(d, data)
    device = kind != "host"
    if device:
        del data
        corpus = hs.Corpus(db, scratch, d, offs, lens, device_report=True)
        one = lambda: corpus.scan_device()[:2]
    else:
        corpus = hs.Corpus(db, scratch, d, offs, lens, h_data=data)
        one = lambda: corpus.scan(False, 16)[:2]
    for _ in range(3):  # first-launch costs, the output growing, the clock ramp
        rc, total = one()
        if rc != hs.SUCCESS:
            raise SystemExit("%s leg: rc %d" % (kind, rc))
    t0 = time.perf_counter()
    if device:
        totals = [one()[1] for _ in range(passes)]
    else:
        rc, tot, _, _ = corpus.scan_repeats(passes, False, 16)
        if rc != hs.SUCCESS:
            raise SystemExit("host leg: rc %d" % rc)
        totals = [int(t) for t in tot]
    ms = (time.perf_counter() - t0) * 1e3 / passes
    if len(set(totals)) != 1 or totals[0] != total:
        raise SystemExit("%s leg: totals differ between passes: %r" % (kind, totals))
    corpus.close()
    ctx.free(d)
    print(json.dumps({"shape": shape, "leg": kind, "bytes": nbytes, "blocks": len(offs),
                      "passes": passes, "matches": int(total), "ms_per_pass": round(ms, 4),
                      "ms_per_gib": round(ms * (1 << 30) / nbytes, 4)}))


STAGE_RE = re.compile(r"device_report: (\d+) records, (\d+) candidates, (\d+) matches: lead "
                      r"([\d.]+) ms, exhaustion ([\d.]+) ms, count ([\d.]+) ms, emit ([\d.]+) ms")
SCAN_RE = re.compile(r"vsa_hs_corpus_scan_device: scan ([\d.]+) ms")


def run_leg(shape, kind, passes, limit):
    """a leg in a process of its own under `timeout -k 10`; its JSON line"""
    env = dict(os.environ)
    if kind == "stages":
        env["VSA_HOST_TIMING"] = "1"
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
                        "--shape", shape, "--leg", kind, "--passes", str(passes)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("shape %s, %s leg: exit status %d" % (shape, kind, p.returncode))
    line = json.loads(p.stdout.strip().splitlines()[-1])
    if kind == "stages":
        st = [tuple(map(float, m.groups()[3:])) for m in STAGE_RE.finditer(p.stderr)][-passes:]
        sc = [float(m.group(1)) for m in SCAN_RE.finditer(p.stderr)][-passes:]
        m = STAGE_RE.findall(p.stderr)[-1]
        gib = line["bytes"] / float(1 << 30)
        line.update({"records": int(m[0]), "candidates": int(m[1]),
                     "scan_ms_per_gib": round(min(sc) / gib, 4),
                     "lead_ms_per_gib": round(min(s[0] for s in st) / gib, 4),
                     "exhaustion_ms_per_gib": round(min(s[1] for s in st) / gib, 4),
                     "count_ms_per_gib": round(min(s[2] for s in st) / gib, 4),
                     "emit_ms_per_gib": round(min(s[3] for s in st) / gib, 4)})
        del line["ms_per_pass"], line["ms_per_gib"]
    return line


def shape_step(shape, passes, rounds):
    """the legs of one shape, alternating, then the per-stage leg"""
    limit = SHAPES[shape][2]
    lines = []
    for r in range(rounds):
        for kind in ("device", "host"):
            line = run_leg(shape, kind, passes, limit)
            line["round"] = r
            lines.append(line)
    if len(set(ln["matches"] for ln in lines)) != 1:
        raise SystemExit("shape %s: the legs' match totals differ: %r"
                         % (shape, [(ln["leg"], ln["matches"]) for ln in lines]))
    lines.append(run_leg(shape, "stages", min(passes, 5), limit))
    best = {k: min(ln["ms_per_gib"] for ln in lines if ln["leg"] == k) for k in ("device", "host")}
    lines.append({"shape": shape, "leg": "summary", "device_ms_per_gib": best["device"],
                  "host_ms_per_gib": best["host"],
                  "device_over_host": round(best["device"] / best["host"], 4)})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", choices=list(SHAPES))
    ap.add_argument("--leg", choices=["device", "host", "stages"])
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    if a.leg:
        return leg(a.shape, a.leg, a.passes)
    if a.shape:
        return shape_step(a.shape, a.passes, a.rounds)
    # every shape: a step each under its own time limit, chained with &&
    steps = []
    for name, (_, _, limit) in SHAPES.items():
        steps.append("timeout -k 10 %d %s %s --shape %s --passes %d --rounds %d"
                     % (limit * (2 * a.rounds + 1) + 30, sys.executable,
                        os.path.abspath(__file__), name, a.passes, a.rounds))
    return subprocess.call(" && ".join(steps), shell=True)


if __name__ == "__main__":
    sys.exit(main())
