"""Commitments of many short vectors against the fastest route there was before: `count` vectors of n
values resident in HBM.

    new   KzgDomain.commit_many_dev on a handle with window tables (build_many_tables)
    old   KzgDomain.commit_evals_dev on a second handle of the context with Lagrange-basis tables (build_tables, section 20)

Both end in a device synchronisation and are timed with the host clock; the two alternate in one process, `--runs` times each
after a warm-up call in which their bytes are checked equal.  One JSON line per (log_n, count): median, min and max of each,
the time per vector and the bound n x W x 0.146 ns it is held against.  At n = 2^8 also: the widths c = 4 .. 8 side by side
(build time, table bytes, 4096 vectors), and update_many of 4096 single-index updates against committing the 4096 vectors again.

--slices also times 1, 4, 16, 64, 256 and 1024 vectors of 2^8 values with every slice count forced through the test door
(tests/_build/libdev_kzg_many.so): the measurement the rule of kzm_slices rests on.

    python tools/kzg_many_bench.py [--sizes 8:16,8:256,8:4096,8:65536,5:4096,12:4096] [--runs 5] [--widths 4,5,6,7,8] [--slices]
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

TAU, G = 0x5EED0000 * 0x9E3779B97F4A7C15, 0xA5A5A5A5DEADBEEF   # the synthetic key of the test suite
ADD_NS = 0.146                                                  # one mixed addition chip-wide in prove()'s accumulation


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def random_values(ctx, seed, n, count):
    """count x n canonical values resident in HBM, every one of them its own 254 random bits, uploaded 32 MiB at a time"""
    import numpy as np
    gen = np.random.default_rng(seed)
    buf = ctx.alloc(32 * n * count)
    step = max((32 << 20) // (32 * n), 1)
    for first in range(0, count, step):
        k = min(step, count - first)
        raw = gen.integers(0, 256, size=(k * n, 32), dtype=np.uint8)
        raw[:, 31] &= 0x3F                                              # below 2^254 < q
        buf.upload(raw.tobytes(), 32 * n * first)
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8:16,8:256,8:4096,8:65536,5:4096,12:4096")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--widths", default="4,5,6,7,8")
    ap.add_argument("--slices", action="store_true", help="time forced slice counts at 2^8 values (needs the test door)")
    args = ap.parse_args()
    import plonk_amd as P
    Q = P.Q
    sizes = [tuple(int(x) for x in s.split(":")) for s in args.sizes.split(",")]
    for log_n in sorted({s[0] for s in sizes}):
        n = 1 << log_n
        ctx = P.Context(0)
        key = ctx.alloc(96 * n)
        ctx.srs_generate_dev(TAU % Q, G, n, key.ptr)
        ctx.srs_load_dev(key.ptr, n)
        ctx.sync()
        key.free()
        new, old = P.KzgDomain(ctx, log_n), P.KzgDomain(ctx, log_n)
        build_ms = timed(new.build_many_tables)
        old.build_tables()
        rnd = random.Random(log_n)
        for count in [s[1] for s in sizes if s[0] == log_n]:
            vals = random_values(ctx, 1000 * log_n + count, n, count)
            out = ctx.alloc(48 * count)
            ptrs = [vals.ptr + 32 * n * j for j in range(count)]

            def run_new():
                new.commit_many_dev(vals.ptr, count, out.ptr)

            def run_old():
                return old.commit_evals_dev(ptrs)

            run_new()
            assert out.download() == b"".join(run_old()), "the two routes disagree"       # (also the warm-up)
            t_new, t_old = [], []
            for _ in range(args.runs):
                t_new.append(timed(run_new))
                t_old.append(timed(run_old))
            last = new.many_last()
            per_vector_us = statistics.median(t_new) * 1e3 / count
            line = {"log_n": log_n, "count": count, "runs": args.runs, "commit_many_dev": stats(t_new),
                    "commit_evals_dev_with_tables": stats(t_old), "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2),
                    "per_vector_us": round(per_vector_us, 3), "bound_per_vector_us": round(n * last["windows"] * ADD_NS * 1e-3, 3),
                    "tables_build_ms": round(build_ms, 3), "many_last": last}
            print(json.dumps(line), flush=True)
            if log_n == 8 and count == 4096 and args.slices:
                forced_slices(ctx, args, new)
            if log_n == 8 and count == 4096:
                widths(ctx, args, vals, out, count)
                updates(ctx, args, new, vals, out, count, rnd)
            vals.free()
            out.free()
        new.close()
        old.close()
        ctx.close()


def widths(ctx, args, vals, out, count):
    """c = 4 .. 8 side by side on handles of their own: the build and `count` resident vectors"""
    import plonk_amd as P
    doms, build = {}, {}
    for c in [int(x) for x in args.widths.split(",")]:
        doms[c] = P.KzgDomain(ctx, 8)
        build[c] = timed(lambda: doms[c].build_many_tables(c))
    want = None
    for c, d in doms.items():
        d.commit_many_dev(vals.ptr, count, out.ptr)
        got = out.download()
        assert want in (None, got), "the widths disagree"
        want = got
    times = {c: [] for c in doms}
    for _ in range(args.runs):
        for c, d in doms.items():
            times[c].append(timed(lambda: d.commit_many_dev(vals.ptr, count, out.ptr)))
    for c, d in doms.items():
        last = d.many_last()
        print(json.dumps({"log_n": 8, "count": count, "window_bits": c, "windows": last["windows"], "table_bytes": last["table_bytes"],
                          "tables_build_ms": round(build[c], 3), "commit_many_dev": stats(times[c])}), flush=True)
        d.close()


def forced_slices(ctx, args, dom):
    """few vectors of 2^8 values under every forced slice count: one JSON line per count, the rule's own choice beside it"""
    import ctypes
    door = ctypes.CDLL(os.path.join(ROOT, "tests", "_build", "libdev_kzg_many.so"))
    door.dkm_set_slices.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    for count in (1, 4, 16, 64, 256, 1024):
        vals, out = random_values(ctx, 77 + count, 256, count), ctx.alloc(48 * count)
        forced = (1, 2, 4, 8, 16, 32, 64, 128)
        times = {s: [] for s in forced}
        for s in forced:                                                # warm-up
            door.dkm_set_slices(dom.handle, s)
            dom.commit_many_dev(vals.ptr, count, out.ptr)
        for _ in range(args.runs):
            for s in forced:
                door.dkm_set_slices(dom.handle, s)
                times[s].append(timed(lambda: dom.commit_many_dev(vals.ptr, count, out.ptr)))
        door.dkm_set_slices(dom.handle, 0)
        dom.commit_many_dev(vals.ptr, count, out.ptr)
        print(json.dumps({"log_n": 8, "count": count, "ms_by_forced_slices": {s: round(statistics.median(t), 3) for s, t in times.items()},
                          "rule_slices": dom.many_last()["slices"]}), flush=True)
        vals.free()
        out.free()


def updates(ctx, args, dom, vals, out, count, rnd):
    """`count` single-index updates (host arrays, bases in, commitments out) against committing the `count` vectors again"""
    import plonk_amd as P
    dom.commit_many_dev(vals.ptr, count, out.ptr)
    base = out.download()
    import ctypes
    ups = [[(rnd.randrange(256), rnd.randrange(P.Q))] for _ in range(count)]
    bases = [base[48 * j:48 * j + 48] for j in range(count)]
    assert dom.update_many(ups[:4], base=bases[:4]) != bases[:4]
    # the C call on arrays made once: the binding's list handling is not what is measured
    offs = (ctypes.c_uint64 * (count + 1))(*range(count + 1))
    idx = (ctypes.c_uint32 * count)(*[u[0][0] for u in ups])
    deltas = P.fr_to_bytes_mont([u[0][1] for u in ups])
    cm = ctypes.create_string_buffer(48 * count)
    fn, h = ctx.lib.plonk_kzg_update_many, dom.handle

    def call(b):
        ctx._check(fn(h, b, offs, idx, deltas, count, cm))
    t_upd, t_again, t_sparse = [], [], []
    for _ in range(args.runs):
        t_upd.append(timed(lambda: call(base)))
        t_sparse.append(timed(lambda: call(None)))
        t_again.append(timed(lambda: dom.commit_many_dev(vals.ptr, count, out.ptr)))
    print(json.dumps({"log_n": 8, "count": count, "update_many_single_index_with_bases": stats(t_upd),
                      "update_many_single_index_no_bases": stats(t_sparse), "commit_many_dev_again": stats(t_again),
                      "many_last": dom.many_last()}), flush=True)


if __name__ == "__main__":
    main()
