"""KZG10 in evaluation form against what a caller did before it: `count` vectors of n values resident in
HBM, opened at a random point with their commitments.

    new   KzgDomain.open_evals_dev (commitments + witness), and KzgDomain.commit_evals_dev on its own
    old   Context.ntt_dev(inverse) per vector into a second set of buffers, then Context.kzg_open_dev on the coefficient forms

Both end in a device synchronisation and are timed with the host clock; the two alternate in one process, `--runs` times each
after a warm-up call.  One JSON line per (log_n, count): median, min and max of each, and from one extra profiled call of the
new route the device time of msm_points_run's phases (profile slots 15, 22, 23, 30, 31) — its share of the call.

    python tools/kzg_evals_bench.py [--logs 12,16,20] [--counts 1,16] [--runs 5] [--tables]

--tables adds a third route in the same alternation: the same calls on a second handle of the context
that holds Lagrange-basis tables (KzgDomain.build_tables), the one-time cost of building them, commit_evals_dev of the call's
vectors as ONE call (finished on the device beyond one group) against one call per four vectors (each finished on the host),
and from one extra profiled call the device time of the table MSMs (profile slots 1 and 2).
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
MSM_POINTS_SLOTS = (15, 22, 23, 30, 31)


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="12,16,20")
    ap.add_argument("--counts", default="1,16")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tables", action="store_true", help="time a handle with Lagrange-basis tables (build_tables) as a third route")
    args = ap.parse_args()
    import plonk_amd as P
    Q = P.Q
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
        if args.tables:   # a second handle on the same context that holds Lagrange-basis tables: the third route
            tab = P.KzgDomain(ctx, log_n)
            build_ms = timed(tab.build_tables)   # (with the Lagrange-point build of that handle)
        rnd = random.Random(log_n)
        raw = bytearray(rnd.randbytes(32 * n))
        for i in range(31, 32 * n, 32):
            raw[i] &= 0x3F
        raw = bytes(raw)
        z, v = rnd.randrange(Q), rnd.randrange(Q)
        for count in [int(x) for x in args.counts.split(",")]:
            vals, coefs = [ctx.alloc(32 * n) for _ in range(count)], [ctx.alloc(32 * n) for _ in range(count)]
            tmp = ctx.alloc(32 * n)
            for b in vals:
                b.upload(raw)
            vp, cp = [b.ptr for b in vals], [b.ptr for b in coefs]
            vv = v if count > 1 else None

            def new_open():
                return dom.open_evals_dev(vp, z, vv)

            def new_commit():
                return dom.commit_evals_dev(vp)

            def old_open():
                for s, d in zip(vp, cp):
                    ctx.ntt_dev(s, d, tmp.ptr, log_n, inverse=True)
                return ctx.kzg_open_dev(cp, [n] * count, z, vv)

            assert new_open() == old_open(), "the two routes disagree"       # (also the warm-up, and the Lagrange-point build)
            assert new_commit() == new_open()[1]
            def tab_open():
                return tab.open_evals_dev(vp, z, vv)

            def tab_commit():
                return tab.commit_evals_dev(vp)

            def tab_commit_by_fours():   # the same commitments as groups the host finishes: one call per four vectors
                return [c for k in range(0, count, 4) for c in tab.commit_evals_dev(vp[k:k + 4])]

            if tab is not None:
                assert tab_open() == new_open() and tab_commit() == tab_commit_by_fours() == new_commit()
            t_new, t_commit, t_old, t_tab, t_tab_commit, t_fours = [], [], [], [], [], []
            for _ in range(args.runs):
                t_new.append(timed(new_open))
                if tab is not None:
                    t_tab.append(timed(tab_open))
                t_old.append(timed(old_open))
                t_commit.append(timed(new_commit))
                if tab is not None:
                    t_tab_commit.append(timed(tab_commit))
                    t_fours.append(timed(tab_commit_by_fours))
            ctx.profile(True)
            ctx.profile_reset()
            wall = timed(new_open)
            msm_ms = sum(ctx.profile_read(s)[0] for s in MSM_POINTS_SLOTS)
            ctx.profile(False)
            line = {"log_n": log_n, "count": count, "runs": args.runs, "open_evals_dev": stats(t_new),
                    "ntt_dev_inverse+kzg_open_dev": stats(t_old), "commit_evals_dev": stats(t_commit),
                    "profiled_open_evals_dev_ms": round(wall, 3), "msm_points_device_ms": round(msm_ms, 3),
                    "evals_last": dom.evals_last()}
            if tab is not None:
                ctx.profile(True)
                ctx.profile_reset()
                wall = timed(tab_open)
                sort_tail_ms, accumulate_ms = ctx.profile_read(2)[0], ctx.profile_read(1)[0]
                ctx.profile(False)
                line.update({"tables": {"open_evals_dev": stats(t_tab), "commit_evals_dev": stats(t_tab_commit),
                                        "commit_evals_dev_by_fours": stats(t_fours), "profiled_open_evals_dev_ms": round(wall, 3),
                                        "msm_sort_and_tail_device_ms": round(sort_tail_ms, 3), "msm_accumulate_device_ms": round(accumulate_ms, 3),
                                        "build_ms": round(build_ms, 3), "tables_last": tab.tables_last()}})
            print(json.dumps(line), flush=True)
            for b in vals + coefs + [tmp]:
                b.free()
        if tab is not None:
            tab.close()
        dom.close()
        ctx.close()


if __name__ == "__main__":
    main()
