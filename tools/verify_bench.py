"""Batch proof verification throughput (plonk_verify, plonk_amd/csrc/verify.hip): proofs of one 2^12-gate circuit with
four public inputs, made once on the GPU with different blinders, verified in batches of K.  One JSON line per K: wall time of
the call (it returns after its last device synchronisation), proofs per second, the plonk_verifier_last phase times,
msm_terms and pairing_checks; then one run with one bad proof per 1024.

With --circuits C, C circuits of different sizes (2^log_n, 2^(log_n - 1), ...) and public-input counts (4, 1, 6, 0, ...) are
compiled from one SRS and their proofs interleaved (proof k of circuit k mod C); each K prints a plonk_verify_mixed line
and, for C = 1, a plonk_verify line on the same batch, the two alternating in this process (best of --reps each).

With --each, plonk_verify_each (one pairing check per proof on the device) alternates with the other
calls on every batch, every line carries best / median / max of the repetitions (at least 5, after a warm-up), and four more
legs run: K = 1024 all valid against all bad (plonk_verify_each; the bisection's all-bad case at K = 256), plonk_kzg_check_each
against sampled count == 1 plonk_kzg_batch_check calls, and the pairing kernel alone (plonk_kzg_pairing_check_each).

    python tools/verify_bench.py [--log-n 12] [--ks 1,64,1024,8192] [--reps 3] [--circuits 1] [--each]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def circuit(ngates, npi, seed=4242):
    """random arithmetic gates with `npi` public inputs (append_public, composer.rs:377-389), ngates rows in all"""
    import random
    from oracle import plonk as O
    from oracle.bls12_381 import Q
    r = random.Random(seed)
    c = O.Composer()
    ws = [c.append_witness(r.randrange(Q)) for _ in range(4)]
    for _ in range(npi):
        v = r.randrange(Q)
        c.append_gate(O.Gate(a=c.append_witness(v), q_l=Q - 1, pi=v))
    while len(c.constraints) < ngates:
        ws.append(c.gate_mul(r.choice(ws), r.choice(ws), r.choice(ws), q_m=r.randrange(1, Q), q_f=1, q_c=r.randrange(Q)))
        ws = ws[-16:]
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=12)
    ap.add_argument("--ks", default="1,64,1024,8192")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--circuits", type=int, default=1)
    ap.add_argument("--each", action="store_true")
    args = ap.parse_args()
    if args.each:
        args.reps = max(args.reps, 5)
    ks = [int(k) for k in args.ks.split(",")]
    import plonk_amd
    from oracle import bls12_381 as E
    from tests import circuits as C
    import g2_ref as G2
    tau, g = 0x5EED0000 * 0x9E3779B97F4A7C15 % E.Q, 0xA5A5A5A5DEADBEEF   # circuits.synthetic_srs's defaults
    ctx = plonk_amd.Context(0)
    npis = [4, 1, 6, 0]
    shapes = [(max(args.log_n - c, 4), npis[c % 4]) for c in range(args.circuits)]
    srs = C.synthetic_srs((1 << args.log_n) + 7)   # one SRS for every circuit, loaded before any is compiled
    ctx.srs_load_bytes(srs, len(srs) // 96)
    opening_key = E.g1_compress(E.g1_mul(E.G1_GEN, g)) + G2.g2_compress(G2.G2_GEN) + G2.g2_compress(G2.g2_mul(G2.G2_GEN, tau))
    kmax = max(ks)
    circs = []
    t0 = time.perf_counter()
    for c, (log_n, npi) in enumerate(shapes):
        label = b"verify-bench" if args.circuits == 1 else b"verify-bench-%d" % c
        comp = circuit(1 << log_n, npi, seed=4242 + c)
        case = C.compile_fast(comp, label)
        cols = C.circuit_columns(comp)
        prover = plonk_amd.Prover.compile(ctx, label, cols["selectors"], cols["wires"], cols["witnesses"])
        verifier = plonk_amd.Verifier(ctx, prover.verifier_to_bytes(opening_key, case["pi_idx"]))
        pis = [case["pi"][i] for i in case["pi_idx"]]
        n = len(range(c, kmax, args.circuits))
        proofs = [prover.prove_witnesses(cols["values"], case["pi"], C.blinders(k)) for k in range(n)]
        circs.append((prover, verifier, pis, proofs))
    items = [(circs[k % args.circuits][1], circs[k % args.circuits][3][k // args.circuits], circs[k % args.circuits][2])
             for k in range(kmax)]
    print(json.dumps({"setup": "proofs", "log_n": args.log_n, "circuits": [{"log_n": ln, "public_inputs": p} for ln, p in shapes],
                      "count": kmax, "seconds": round(time.perf_counter() - t0, 2)}), flush=True)

    def one(batch, call):
        t = time.perf_counter()
        if call == "plonk_verify":
            v = batch[0][0]
            verdicts = v.verify_batch([p for _, p, _ in batch], [x for _, _, x in batch])
            info = v.last()
        elif call == "plonk_verify_each":
            verdicts, info = plonk_amd.verify_each_info(batch)
        else:
            verdicts, info = plonk_amd.verify_mixed(batch)
        return (time.perf_counter() - t) * 1e3, info, verdicts

    def spread(times):
        times = sorted(times)
        return {"wall_ms": round(times[0], 3), "median_ms": round(times[len(times) // 2], 3), "max_ms": round(times[-1], 3),
                "reps": len(times)}

    def run(batch, label, calls=None, reps=None):
        if calls is None:
            calls = ["plonk_verify_mixed"] + (["plonk_verify"] if args.circuits == 1 else []) + (["plonk_verify_each"] if args.each else [])
        best, times = {}, {c: [] for c in calls}
        if args.each:
            for call in calls:   # warm-up: workspace growth, the lazily made line tables
                one(batch, call)
        for _ in range(reps or args.reps):   # the calls alternate, so all see the same state of the machine
            for call in calls:
                r = one(batch, call)
                times[call].append(r[0])
                if call not in best or r[0] < best[call][0]:
                    best[call] = r
        for call in calls:
            ms, info, verdicts = best[call]
            out = {"run": label, "call": call, "circuits": args.circuits, "K": len(batch), "wall_ms": round(ms, 3),
                   "proofs_per_s": round(len(batch) / ms * 1e3, 1), "rejected": sum(v != 0 for v in verdicts)}
            if args.each:
                out.update(spread(times[call]))
            out.update({k: (round(v, 3) if isinstance(v, float) else v) for k, v in info.items()})
            print(json.dumps(out), flush=True)

    def flip(item):
        v, p, x = item
        b = bytearray(p)
        b[528:560] = ((int.from_bytes(b[528:560], "little") + 1) % E.Q).to_bytes(32, "little")
        return v, bytes(b), x

    def each_legs():
        from tests import kzg_ref as K
        # the work of plonk_verify_each does not depend on the verdicts: all valid against all bad
        k = min(1024, kmax)
        run(items[:k], "all valid", ["plonk_verify_each"])
        run([flip(it) for it in items[:k]], "all bad", ["plonk_verify_each"])
        k = min(256, kmax)
        run([flip(it) for it in items[:k]], "all bad (bisection: 2K - 1 checks)", ["plonk_verify_mixed", "plonk_verify_each"], reps=2)
        # KZG openings: 64 distinct honest openings of short polynomials, repeated to the count (the work is per item)
        import random
        rnd = random.Random(77)
        key = plonk_amd.KzgKey(ctx, opening_key)
        points = [rnd.randrange(E.Q) for _ in range(64)]
        proofs = []
        for z in points:
            ev, cm, wit = ctx.kzg_open([[rnd.randrange(E.Q) for _ in range(8)]], z, None)
            proofs.append(plonk_amd.KzgProof.make(cm[0], ev[0], wit))
        single = []
        for z, p in zip(points, proofs):   # 64 count == 1 calls of plonk_kzg_batch_check, scaled to the count below
            t = time.perf_counter()
            assert key.batch_check_code([z], [p])[0] == 0
            single.append((time.perf_counter() - t) * 1e3)
        single_ms = sorted(single)[len(single) // 2]
        for count in (64, 1024, 8192):
            pts, prs = [points[i % 64] for i in range(count)], [proofs[i % 64] for i in range(count)]
            key.check_each_info(pts, prs)
            times, info = [], None
            for _ in range(args.reps):
                t = time.perf_counter()
                verdicts, info = key.check_each_info(pts, prs)
                times.append((time.perf_counter() - t) * 1e3)
                assert verdicts == [0] * count
            out = {"run": "kzg", "call": "plonk_kzg_check_each", "count": count, "single_call_median_ms": round(single_ms, 3),
                   "count_single_calls_ms": round(single_ms * count, 1)}
            out.update(spread(times))
            out.update({k: (round(v, 3) if isinstance(v, float) else v) for k, v in info.items()})
            print(json.dumps(out), flush=True)
        # the pairing kernel alone: ms_pairing is host wall clock around the kernel and its synchronisation
        host_ms = plonk_amd.verify_mixed(items[:1])[1]["ms_pairing"]
        for count in (64, 8192):
            a = [bytes(proofs[i % 64].witness) for i in range(count)]
            b = [bytes(proofs[i % 64].commitment) for i in range(count)]
            key.pairing_check_each_info(a, b)
            times, wall = [], []
            for _ in range(args.reps):
                t = time.perf_counter()
                _, info = key.pairing_check_each_info(a, b)
                wall.append((time.perf_counter() - t) * 1e3)
                times.append(info["ms_pairing"])
            out = {"run": "pairing kernel", "call": "plonk_kzg_pairing_check_each", "count": count,
                   "host_pairing_ms": round(host_ms, 3), "count_host_pairings_ms": round(host_ms * count, 1),
                   "kernel_ms": spread(times)}
            out.update(spread(wall))
            print(json.dumps(out), flush=True)
        key.close()

    for k in ks:
        run(items[:k], "valid")
    bad = list(items[:kmax])
    for i in range(0, kmax, 1024):
        j = i + 517 % min(1024, kmax - i)
        v, p, x = bad[j]
        b = bytearray(p)
        val = (int.from_bytes(b[528:560], "little") + 1) % E.Q
        b[528:560] = val.to_bytes(32, "little")
        bad[j] = (v, bytes(b), x)
    run(bad, "one bad per 1024")
    if args.each:
        each_legs()
    for prover, verifier, _, _ in circs:
        verifier.close()
        prover.close()
    ctx.close()


if __name__ == "__main__":
    main()
