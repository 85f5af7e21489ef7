"""KZG10 cell proofs (plonk_kzg_open_cells, plonk_amd/csrc/kzg_cells.hip) beside plonk_kzg_open_domain on the same polynomials,
one MI355X, one process.  Per (n, count): a warm-up of every route, then --reps runs per route ALTERNATING between the routes,
wall time of the call (it returns after its last device synchronisation), reported as median [min, max].  One JSON line per
(n, l, count): open_cells, open_domain at the same (n, count), the plan (S, chunks, workspace), the multiplication count times
the 48 ns per multiplication DESIGN.md section 14 measured (the model), and whether the median of open_cells stays under the
median of open_domain.  One JSON line per (n, l) before them: the time of the first call with that cell size, which builds
the A^(u) tables, minus the warm median, and the tables' bytes.

    python tools/kzg_cells_bench.py [--shapes 12:6,13:6,16:6,20:6,20:10] [--counts 1,16] [--reps 5]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS_PER_MUL = 48.0      # a full-width scalar multiplication in a saturated stage


def rand_poly_bytes(rnd, n):
    raw = bytearray(rnd.randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        raw[i] &= 0x3F
    return bytes(raw)


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def stats(ts):
    return {"median_ms": round(1e3 * statistics.median(ts), 3), "min_ms": round(1e3 * min(ts), 3), "max_ms": round(1e3 * max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="12:6,13:6,16:6,20:6,20:10", help="log_n:log_cell, ...")
    ap.add_argument("--counts", default="1,16")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",")]
    counts = [int(x) for x in args.counts.split(",")]
    import plonk_amd
    from oracle import bls12_381 as E
    tau, g = 0x5EED0000 * 0x9E3779B97F4A7C15 % E.Q, 0xA5A5A5A5DEADBEEF   # circuits.synthetic_srs's defaults
    ctx = plonk_amd.Context(0)
    npts = 1 << max(s[0] for s in shapes)
    buf = ctx.alloc(96 * npts)
    ctx.srs_generate_dev(tau, g, npts, buf.ptr)
    ctx.srs_load_dev(buf.ptr, npts)
    ctx.sync()
    buf.free()
    rnd = random.Random(1)
    for log_n in sorted({s[0] for s in shapes}):
        n = 1 << log_n
        cell_logs = [s[1] for s in shapes if s[0] == log_n]
        dom = plonk_amd.KzgDomain(ctx, log_n)
        polys = [rand_poly_bytes(rnd, n) for _ in range(max(counts))]
        dom.open_bytes(polys[:1])
        for c in cell_logs:                                    # the first call with a cell size builds its tables
            first = timed(lambda: dom.open_cells_bytes(polys[:1], c))
            assert dom.cells_last()["built_table"] == 1
            warm = statistics.median(timed(lambda: dom.open_cells_bytes(polys[:1], c)) for _ in range(3))
            print(json.dumps({"log_n": log_n, "log_cell": c, "table_build_ms": round(1e3 * (first - warm), 3),
                              "table_bytes": 2 * n * 256}), flush=True)
        for count in counts:
            routes = {("cells", c): (lambda c=c: dom.open_cells_bytes(polys[:count], c)) for c in cell_logs}
            routes[("domain", 0)] = lambda: dom.open_bytes(polys[:count])
            times = {k: [] for k in routes}
            info = {}
            for k, fn in routes.items():                       # warm-up: buffers grown, NTT tables made
                fn()
                info[k] = dom.cells_last() if k[0] == "cells" else dom.last()
            for _ in range(args.reps):
                for k, fn in routes.items():
                    times[k].append(timed(fn))
            d = stats(times[("domain", 0)])
            for c in cell_logs:
                s, last = stats(times[("cells", c)]), info[("cells", c)]
                print(json.dumps({"log_n": log_n, "log_cell": c, "count": count, "open_cells": s, "open_domain": d,
                                  "ratio": round(d["median_ms"] / s["median_ms"], 2), "cells_not_slower": s["median_ms"] <= d["median_ms"],
                                  "slices": last["slices"], "chunks": last["chunks"], "workspace_bytes": last["workspace_bytes"],
                                  "scalar_muls": last["scalar_muls"], "stage_launches": last["stage_launches"],
                                  "model_ms": round(last["scalar_muls"] * NS_PER_MUL * 1e-6, 3),
                                  "domain_scalar_muls": info[("domain", 0)]["scalar_muls"],
                                  "domain_model_ms": round(info[("domain", 0)]["scalar_muls"] * NS_PER_MUL * 1e-6, 3)}), flush=True)
        dom.close()
    ctx.close()


if __name__ == "__main__":
    main()
