"""Cost of plonk_msm_points_dev (plonk_amd/csrc/msm_points.hip) on one MI355X: the bucket path against the per-term kernel
it replaces above the crossover, one JSON line per size.

  random   m = 2^6, 2^8, ..., 2^20 and m = 106512 (the term count of the K = 8192 verification batch):
           points [g tau^i] G made on the device, seeded full-width scalars, everything resident.  Both paths of the SAME call
           (min_bucket_terms = 1 and = 2^30) alternate in one process on the same input; every shape is warmed; best / median /
           max of --reps calls by a host clock around a device synchronise.  The two results must be byte-identical.  For the
           bucket path also each stage's share, from the context's profile slots in a run of its own (15 load + recode,
           22 scan + scatter, 23 accumulation, 30 slice sums to bucket sums, 31 window sums; the rest of the wall time is the
           two synchronisations and the host's Horner over the windows).
  skewed   all scalars equal at m = 2^17: every term in one bucket per window.  Reported beside the random line of the same
           size; it has no bar, but a figure many times the random one means the slice sums are walked serially.
  final    the crossover: the smallest measured size from which the bucket path's median stays below the per-term path's at
           every larger measured size, moved one size up where the two medians are closer than the spread (max - best) of
           the repetitions.  This is the value for MP_MIN_BUCKET_TERMS (msm_points_core.hpp).

The per-term path is skipped above --per-term-max terms (default 2^20: it is linear, ~0.12 us per term).  The cases run in
a child process under a time limit (--limit seconds); a child that fails, dies or runs over ends the tool with its status
(124 for the limit) and nothing more is started on the GPU.  On a shared machine wrap the whole tool as well:

    timeout -k 10 600 python tools/msm_points_bench.py [--reps 7] [--max-log 20] [--limit 500]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import plonk_amd   # noqa: E402

Q = plonk_amd.Q
TAU = 0x5EED0000 * 0x9E3779B97F4A7C15 % Q
G_SCALAR = 0xA5A5A5A5DEADBEEF
PER_TERM = 1 << 30
SLOTS = {15: "load_recode_ms", 22: "scan_scatter_ms", 23: "accumulate_ms", 30: "bucket_sums_ms", 31: "window_sums_ms"}


def timed(fn, sync):
    sync()
    t = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t) * 1e3


def summary(xs):
    return {"best_ms": round(min(xs), 3), "median_ms": round(statistics.median(xs), 3), "max_ms": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-log", type=int, default=20)
    ap.add_argument("--per-term-max", type=int, default=1 << 20)
    ap.add_argument("--limit", type=int, default=500, help="seconds the child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--max-log", str(args.max_log),
               "--per-term-max", str(args.per_term_max)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        sys.exit(rc if rc >= 0 else 128 - rc)
    sizes = sorted({1 << k for k in range(6, args.max_log + 1, 2)} | ({106512} if args.max_log >= 17 else set()))
    mmax = max(sizes + [1 << 17 if args.max_log >= 17 else 0])
    ctx = plonk_amd.Context(0)
    pts = ctx.alloc(96 * mmax)
    ctx.srs_generate_dev(TAU, G_SCALAR, mmax, pts.ptr)
    rnd = random.Random(13)
    raw = bytearray(rnd.randbytes(32 * mmax))
    for i in range(31, 32 * mmax, 32):
        raw[i] &= 0x3F          # Montgomery limbs below 2^254 < q: uniform full-width scalars
    sc = ctx.alloc(32 * mmax)
    sc.upload(bytes(raw))
    out = ctx.alloc(128)
    ctx.sync()
    head = {"reps": args.reps, "library": plonk_amd.LIB_PATH}

    def run(m, min_terms, scalars=sc):
        ctx.msm_points_dev(pts.ptr, scalars.ptr, m, out.ptr, min_bucket_terms=min_terms)

    def measure(m, case, scalars=sc):
        per_term = m <= args.per_term_max
        run(m, 1, scalars)                                   # warm-up of this shape: workspace growth, code objects
        plan = ctx.last_msm_points()
        want = out.download(97)
        if per_term:
            run(m, PER_TERM, scalars)
            assert out.download(97) == want, "the two paths disagree"
        b, p = [], []
        for _ in range(args.reps):                           # alternating: the same state of the machine for both
            b.append(timed(lambda: run(m, 1, scalars), ctx.sync))
            if per_term:
                p.append(timed(lambda: run(m, PER_TERM, scalars), ctx.sync))
        ctx.profile(True)
        run(m, 1, scalars)
        ctx.profile_reset()
        for _ in range(args.reps):
            run(m, 1, scalars)
        stages = {name: round(ctx.profile_read(s)[0] / args.reps, 3) for s, name in SLOTS.items()}
        ctx.profile(False)
        line = dict(head, case=case, m=m, plan=plan, buckets=summary(b), per_term=summary(p) if p else None, stages=stages)
        print(json.dumps(line), flush=True)
        return line

    lines = [measure(m, "random") for m in sizes]
    if args.max_log >= 17:
        m = 1 << 17
        eq = ctx.alloc(32 * m)
        eq.upload(bytes(raw[:32]) * m)
        measure(m, "skewed", eq)
    # the crossover
    both = [ln for ln in lines if ln["per_term"]]
    cross = None
    for i in range(len(both) - 1, -1, -1):
        ln = both[i]
        if ln["buckets"]["median_ms"] < ln["per_term"]["median_ms"]:
            cross = i
        else:
            break
    if cross is not None:
        ln = both[cross]
        spread = max(ln["buckets"]["max_ms"] - ln["buckets"]["best_ms"], ln["per_term"]["max_ms"] - ln["per_term"]["best_ms"])
        if ln["per_term"]["median_ms"] - ln["buckets"]["median_ms"] < spread and cross + 1 < len(both):
            cross += 1
    print(json.dumps(dict(head, case="final", min_bucket_terms=both[cross]["m"] if cross is not None else None,
                          measured_sizes=[ln["m"] for ln in both])), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
