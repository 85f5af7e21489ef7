"""Cost of witness diagnosis (plonk_prover_diagnose_dev, plonk_amd/csrc/diagnose.hip) beside the proof it explains, on the
`widgets` workload of bench.py (every selector family, public inputs), columns resident in HBM.  One JSON line per size:

  diagnose leg   the FIRST call on the prover (it builds the selector-value and position caches), then — alternating in
                 this process, after a warm-up — the steady-state call on the satisfied witness, on a witness with three
                 forged cells, and prove_dev on the same prover; best and median of --reps each, the cache bytes
  prove leg      prove_dev alone, unprofiled and with the profile slots read through plonk_profile_read: wall time minus
                 slots 1 and 2 (the MSM kernels) is the non-MSM time of a proof, the bar for the steady-state call

The prove leg needs nothing new from the library: --tree DIR takes the Python package and the library of ANOTHER build of
this repository (e.g. the parent commit's) from DIR, so both builds can be measured in one job on one box.

    python tools/diagnose_bench.py [--log-gates 12,16,20] [--reps 7] [--legs diagnose,prove] [--tree DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, sync):
    sync()
    t = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t) * 1e3


def summary(xs):
    return {"best_ms": round(min(xs), 3), "median_ms": round(statistics.median(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-gates", default="12,16,20")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--legs", default="diagnose,prove")
    ap.add_argument("--tree", default=ROOT, help="checkout whose plonk_amd package and library are measured")
    args = ap.parse_args()
    legs = args.legs.split(",")
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import plonk_amd   # noqa: F401  (before bench: bench.py then finds THIS package in sys.modules)
    sys.path.insert(0, ROOT)
    import bench
    import bench_circuits as BC
    assert os.path.dirname(os.path.abspath(plonk_amd.__file__)) == os.path.join(tree, "plonk_amd")
    Q = plonk_amd.Q
    for log_n in [int(x) for x in args.log_gates.split(",")]:
        n = 1 << log_n
        ctx = plonk_amd.Context(0)
        prover, wbuf, _ = bench.build_prover(ctx, log_n, 0, 1, None, profile="widgets")
        pi = prover.public_inputs
        bl = plonk_amd.fr_to_bytes_mont([(0xB11D0000 + i) * 0x9E3779B97F4A7C15 % Q for i in range(14)])
        out = {"log_gates": log_n, "profile": "widgets", "library": plonk_amd.LIB_PATH, "reps": args.reps}
        proof = prover.prove_dev(wbuf.ptr, pi, bl)
        prover.prove_dev(wbuf.ptr, pi, bl)                       # warm-up
        prove = lambda: prover.prove_dev(wbuf.ptr, pi, bl)       # noqa: E731
        if "diagnose" in legs:
            wires, cols, _ = BC.widget_circuit(log_n)
            nsel = sum(1 for k in cols if k.startswith("q_"))
            out["cache_bytes"] = {"selector_values": 32 * n * nsel, "positions": 16 * n, "selectors": nsel}
            bad = ctx.alloc(4 * 32 * n)
            for k in range(4):
                bad.upload(wires[k], 32 * n * k)
            five = plonk_amd.fr_to_bytes_mont([5])
            for col, row in ((0, 0), (2, n // 2 + 1), (3, n - 1)):   # three forged cells: first, middle and last row
                bad.upload(five, 32 * (n * col + row))
            first = prover.diagnose_dev(wbuf.ptr, pi)
            assert first.ok, first
            out["first_call_ms"] = round(first.ms, 3)
            few = prover.diagnose_dev(bad.ptr, pi)
            assert not few.ok and 3 <= few.rows_failing <= 12, few
            out["failing_rows_of_the_forged_witness"] = few.rows_failing
            sat, unsat, pr = [], [], []
            for _ in range(args.reps):                           # the three alternate: same state of the machine for each
                sat.append(timed(lambda: prover.diagnose_dev(wbuf.ptr, pi), ctx.sync))
                unsat.append(timed(lambda: prover.diagnose_dev(bad.ptr, pi), ctx.sync))
                pr.append(timed(prove, ctx.sync))
            out["diagnose_satisfied"] = summary(sat)
            out["diagnose_few_failing"] = summary(unsat)
            out["prove_dev_alternating"] = summary(pr)
            assert prove() == proof                              # the diagnose calls left the prover as they found it
            bad.free()
        if "prove" in legs:
            plain = [timed(prove, ctx.sync) for _ in range(args.reps)]
            ctx.profile(True)
            prove()
            ctx.profile_reset()
            prof = [timed(prove, ctx.sync) for _ in range(args.reps)]
            slots = {s: ctx.profile_read(s)[0] / args.reps for s in (0, 1, 2, 3, 4)}
            ctx.profile(False)
            out["prove_dev"] = summary(plain)
            out["prove_dev_profiled"] = summary(prof)
            out["profile_slots_ms_per_proof"] = {str(s): round(v, 3) for s, v in slots.items()}
            out["non_msm_ms"] = round(statistics.median(prof) - slots[1] - slots[2], 3)   # the bar for diagnose_satisfied
        print(json.dumps(out), flush=True)
        prover.close()
        wbuf.free()
        ctx.close()


if __name__ == "__main__":
    main()
