"""Cost of the KZG10 opening layer (plonk_amd/csrc/kzg.hip) on one MI355X, one JSON line per case:

  open      plonk_kzg_open_dev at --log-n coefficients, count = 1 and 15, commitments off, polynomials resident in HBM: the
            first call (workspace growth) on its own, then best / median wall time of --reps calls, and the split read from
            the profile slots in a run of its own: 12 the non-commitment front (trimmed lengths, powers of v, fold +
            evaluate), 13 Ruffini, 14 the witness commitment
  rule      the non-commitment part of the 15-polynomial open (slots 12 + 13) against ONE commitment of the same length
            (plonk_msm_dev), timed in the same process on the same context, alternating with the open.  The rule is
            non_commitment_ms < the BEST msm_dev time; when it does not hold the tool exits with status 3
  batch     plonk_kzg_batch_check at K = 1, 64, 1024, 8192 (honest openings made in the exponent), with the phase times
            plonk_verify_info reports
  srs       plonk_srs_check of the (2^log_n + 7)-point key

Every group of cases (open + rule, batch, srs) runs in a child process of its own under a time limit (--limit seconds,
default 240); a child that fails, dies or runs over ends the tool with its status (124 for the limit) and nothing more is
started on the GPU.  On a shared machine wrap the whole tool as well:

    timeout -k 10 900 python tools/kzg_bench.py [--log-n 20] [--reps 7] [--cases open,rule,batch,srs] [--limit 240]
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


def timed(fn, sync):
    sync()
    t = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t) * 1e3


def summary(xs):
    return {"best_ms": round(min(xs), 3), "median_ms": round(statistics.median(xs), 3), "max_ms": round(max(xs), 3)}


def g1_of(scalar):
    """48 bytes of [scalar] g through the library's own MSM is not available without a key of one point; use the oracle"""
    from oracle import bls12_381 as E
    s = scalar * G_SCALAR % Q
    return E.g1_compress(E.g1_mul(E.G1_GEN, s)) if s else bytes([0xC0]) + bytes(47)


def opening_key():
    from oracle import bls12_381 as E
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import g2_ref as G2
    return E.g1_compress(E.g1_mul(E.G1_GEN, G_SCALAR)) + G2.g2_compress(G2.G2_GEN) + G2.g2_compress(G2.g2_mul(G2.G2_GEN, TAU))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="open,rule,batch,srs")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process (one group of cases) may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:
        wanted = args.cases.split(",")
        groups = [g for g in (["open", "rule"], ["batch"], ["srs"]) if any(c in wanted for c in g)]
        for g in groups:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--log-n", str(args.log_n), "--reps", str(args.reps),
                   "--cases", ",".join(c for c in g if c in wanted)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc:
                sys.exit(rc if rc > 0 else 128 - rc)
        return
    rule_missed = False
    cases = args.cases.split(",")
    n = 1 << args.log_n
    npoints = n + 7
    ctx = plonk_amd.Context(0)
    key_buf = ctx.alloc(96 * npoints)
    ctx.srs_generate_dev(TAU, G_SCALAR, npoints, key_buf.ptr)
    ctx.srs_load_dev(key_buf.ptr, npoints)
    ctx.sync()
    key_buf.free()
    rnd = random.Random(20)
    polys = []
    for _ in range(15 if ("open" in cases or "rule" in cases) else 0):   # the resident polynomials of the open cases
        raw = bytearray(rnd.randbytes(32 * n))
        for i in range(31, 32 * n, 32):
            raw[i] &= 0x3F
        b = ctx.alloc(32 * n)
        b.upload(bytes(raw))
        polys.append(b)
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    out97 = ctx.alloc(128)
    head = {"log_n": args.log_n, "reps": args.reps, "library": plonk_amd.LIB_PATH}

    def do_open(count):
        return ctx.kzg_open_dev([p.ptr for p in polys[:count]], [n] * count, z, v if count > 1 else None, commitments=False)

    def do_msm():
        ctx.msm_dev(polys[0].ptr, n, out97.ptr)

    if "open" in cases or "rule" in cases:
        first = timed(lambda: do_open(15), ctx.sync)           # grows the workspace (and the MSM scratch)
        do_msm()
        for count in (1, 15):
            do_open(count)                                      # warm-up of this shape
            wall = [timed(lambda: do_open(count), ctx.sync) for _ in range(args.reps)]
            ctx.profile(True)
            do_open(count)
            ctx.profile_reset()
            for _ in range(args.reps):
                do_open(count)
            slots = {s: ctx.profile_read(s)[0] / args.reps for s in (12, 13, 14)}
            ctx.profile(False)
            line = dict(head, case="open_dev", count=count, commitments=False, wall=summary(wall),
                        fold_eval_ms=round(slots[12], 3), ruffini_ms=round(slots[13], 3), witness_commit_ms=round(slots[14], 3))
            if count == 15:
                line["first_call_ms"] = round(first, 3)
            print(json.dumps(line), flush=True)
            if count == 15 and "rule" in cases:
                opens, msms = [], []
                for _ in range(args.reps):                      # alternating: the same state of the machine for both
                    opens.append(timed(lambda: do_open(15), ctx.sync))
                    msms.append(timed(do_msm, ctx.sync))
                non_commit = slots[12] + slots[13]
                print(json.dumps(dict(head, case="rule", non_commitment_ms=round(non_commit, 3), open_dev_15=summary(opens),
                                      msm_dev_one_commitment=summary(msms), holds=non_commit < min(msms))), flush=True)
                rule_missed = not non_commit < min(msms)
    if "batch" in cases or "srs" in cases:
        key = plonk_amd.KzgKey(ctx, opening_key())
        if "batch" in cases:
            kmax = 8192
            # honest openings in the exponent, from 64 distinct (commitment, evaluation, witness) triples reused round-robin
            base = []
            for _ in range(64):
                zz, c, e = rnd.randrange(Q), rnd.randrange(Q), rnd.randrange(Q)
                w = (c - e) * pow((TAU - zz) % Q, -1, Q) % Q
                base.append((zz, plonk_amd.KzgProof.make(g1_of(c), e, g1_of(w))))
            points = [base[k % 64][0] for k in range(kmax)]
            proofs = [base[k % 64][1] for k in range(kmax)]
            for K in (1, 64, 1024, 8192):
                rc, info = key.batch_check_code(points[:K], proofs[:K], label=b"bench")
                assert rc == 0, rc
                wall = [timed(lambda: key.batch_check_code(points[:K], proofs[:K], label=b"bench"), ctx.sync) for _ in range(args.reps)]
                rc, info = key.batch_check_code(points[:K], proofs[:K], label=b"bench")
                print(json.dumps(dict(head, case="batch_check", K=K, wall_with_python_marshalling=summary(wall),
                                      info={k: (round(x, 3) if isinstance(x, float) else x) for k, x in info.items()})), flush=True)
        if "srs" in cases:
            seed = bytes(range(32))
            first = timed(lambda: key.srs_check(seed), ctx.sync)
            assert key.srs_check(seed)
            wall = [timed(lambda: key.srs_check(seed), ctx.sync) for _ in range(args.reps)]
            print(json.dumps(dict(head, case="srs_check", points=npoints, first_call_ms=round(first, 3), wall=summary(wall))), flush=True)
        key.close()
    ctx.close()
    if rule_missed:
        sys.exit(3)


if __name__ == "__main__":
    main()
