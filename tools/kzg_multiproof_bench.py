"""KZG10 multiproofs against the route a caller had before them: M vectors of n values resident in HBM with
their commitments known, K claims (vector, domain index) at random places.

    new   KzgDomain.open_multi_dev (commitments given: two MSMs of n terms per call) and KzgKey.check_multi
    old   K calls of KzgDomain.open_evals_dev on one vector at w^m (witness only), then KzgKey.check_each on the K openings.  Above
          --old-cap claims only the first --old-cap are opened and that time is scaled by K / cap ("extrapolated_from" says so);
          check_each is measured on K openings all the same, the --old-cap proofs repeated

All end in a device synchronisation and are timed with the host clock, the binding's argument packing included; the routes
alternate in one process, `--runs` times each after a warm-up call.  One JSON line per (log_n, K): median, min and max of each
and, from one extra profiled open_multi_dev, the device time of the aggregation pass (profile slot 12) as ns per product K n.

    python tools/kzg_multiproof_bench.py [--logs 8,12,16,20] [--items 1,64,1024,16384] [--vectors 16] [--runs 5] [--old-cap 64] [--tables]

--tables adds the two opening routes on a second handle of the context that holds Lagrange-basis tables
(KzgDomain.build_tables) to the same alternation, and the one-time cost of building them.
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
AGGREGATION_SLOT = 12


def stats(xs, scale=1.0):
    return {"median_ms": round(statistics.median(xs) * scale, 3), "min_ms": round(min(xs) * scale, 3), "max_ms": round(max(xs) * scale, 3)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def opening_key(P):
    """g || h || [tau] h for the synthetic key, by the test suite's plain-Python curve arithmetic"""
    from tests import kzg_ref
    assert (kzg_ref.TAU, kzg_ref.G_SCALAR) == (TAU % P.Q, G)
    return kzg_ref.opening_key()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="8,12,16,20")
    ap.add_argument("--items", default="1,64,1024,16384")
    ap.add_argument("--vectors", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--old-cap", type=int, default=64)
    ap.add_argument("--tables", action="store_true", help="time both opening routes on a handle with Lagrange-basis tables as well")
    args = ap.parse_args()
    import plonk_amd as P
    Q = P.Q
    M = args.vectors
    key_bytes = opening_key(P)
    for log_n in [int(x) for x in args.logs.split(",")]:
        n = 1 << log_n
        ctx = P.Context(0)
        buf = ctx.alloc(96 * n)
        ctx.srs_generate_dev(TAU % Q, G, n, buf.ptr)
        ctx.srs_load_dev(buf.ptr, n)
        ctx.sync()
        buf.free()
        dom = P.KzgDomain(ctx, log_n)
        tab, build_ms = None, 0.0
        if args.tables:   # a second handle on the same context that holds Lagrange-basis tables
            tab = P.KzgDomain(ctx, log_n)
            build_ms = timed(tab.build_tables)
        key = P.KzgKey(ctx, key_bytes)
        rnd = random.Random(log_n)
        vecs = []
        for _ in range(M):
            raw = bytearray(rnd.randbytes(32 * n))
            for i in range(31, 32 * n, 32):
                raw[i] &= 0x3F
            b = ctx.alloc(32 * n)
            b.upload(bytes(raw))
            vecs.append(b)
        ptrs = [b.ptr for b in vecs]
        cm = dom.commit_evals_dev(ptrs)
        w = dom.points()
        for K in [int(x) for x in args.items.split(",")]:
            items = [(rnd.randrange(M), rnd.randrange(n)) for _ in range(K)]
            label = b"bench"
            cap = min(K, args.old_cap)
            out = {}

            def new_open():
                out["new"] = dom.open_multi_dev(ptrs, items, label, commitments=cm)

            def new_check():
                assert key.check_multi(log_n, cm, items, out["new"][0], out["new"][2], label)

            def old_open():
                out["old"] = [dom.open_evals_dev([ptrs[j]], w[m], None, commitments=False) for j, m in items[:cap]]

            def old_check():
                proofs = [P.KzgProof.make(cm[j], ev[0], wit) for (j, m), (ev, _, wit) in zip(items[:cap], out["old"])]
                points = [w[m] for _, m in items[:cap]]
                reps = (K + cap - 1) // cap
                assert key.check_each((points * reps)[:K], (proofs * reps)[:K]) == [0] * K

            def tab_new_open():
                out["tab_new"] = tab.open_multi_dev(ptrs, items, label, commitments=cm)

            def tab_old_open():
                out["tab_old"] = [tab.open_evals_dev([ptrs[j]], w[m], None, commitments=False) for j, m in items[:cap]]

            new_open(), new_check(), old_open(), old_check()                       # the warm-up; every proof verifies
            assert [ev[0] for ev, _, _ in out["old"]] == out["new"][0][:cap], "the two routes disagree on the values"
            if tab is not None:
                tab_new_open(), tab_old_open()
                assert out["tab_new"] == out["new"] and out["tab_old"] == out["old"], "a handle with tables gives other bytes"
            t = {name: [] for name in ("new_open", "new_check", "old_open", "old_check", "tab_new_open", "tab_old_open")}
            for _ in range(args.runs):
                t["new_open"].append(timed(new_open))
                t["old_open"].append(timed(old_open))
                if tab is not None:
                    t["tab_new_open"].append(timed(tab_new_open))
                    t["tab_old_open"].append(timed(tab_old_open))
                t["new_check"].append(timed(new_check))
                t["old_check"].append(timed(old_check))
            ctx.profile(True)
            ctx.profile_reset()
            wall = timed(new_open)
            agg_ms = ctx.profile_read(AGGREGATION_SLOT)[0]
            ctx.profile(False)
            scale = K / cap
            line = {"log_n": log_n, "vectors": M, "items": K, "runs": args.runs,
                    "open_multi_dev": stats(t["new_open"]), "check_multi": stats(t["new_check"]),
                    "open_evals_dev_x_items": stats(t["old_open"], scale), "check_each": stats(t["old_check"]),
                    "extrapolated_from": cap if cap < K else None, "proof_bytes": {"new": 96, "old": 48 * K},
                    "profiled_open_multi_dev_ms": round(wall, 3), "aggregation_ms": round(agg_ms, 3),
                    "aggregation_ns_per_product": round(agg_ms * 1e6 / (K * n), 4),
                    "multi_last": dom.multi_last()}
            if tab is not None:
                line["tables"] = {"open_multi_dev": stats(t["tab_new_open"]), "open_evals_dev_x_items": stats(t["tab_old_open"], scale),
                                  "build_ms": round(build_ms, 3), "tables_last": tab.tables_last()}
            print(json.dumps(line), flush=True)
        for b in vecs:
            b.free()
        if tab is not None:
            tab.close()
        key.close()
        dom.close()
        ctx.close()


if __name__ == "__main__":
    main()
