"""KZG10 cell verification (plonk_kzg_verify_cells / plonk_kzg_verify_cells_each, plonk_amd/csrc/kzg_cell_verify.hip) on one
MI355X, one process.  Per (n, l, K): the items are sampled from blobs opened with plonk_kzg_open_cells and marshalled once; a
warm-up of both calls, then --reps runs of each ALTERNATING, wall time of the call (it returns after its last device
synchronisation), reported as median [min, max] with the phase times of plonk_verify_info of the median run.  The per-item
call is held against K (l + 1) scalar multiplications at the 49 ns DESIGN.md section 16 measured on a full chip plus the 27 ms
of one pairing-kernel launch.  With --host-items K the route callers had before is timed beside them in the same process, once:
B = C - commit(r_k) + x_k proof_k formed on the host in big integers (an l-term MSM per cell over the key's points), then
plonk_kzg_pairing_check_each.

    python tools/kzg_cell_verify_bench.py [--shapes 12:6,16:6] [--counts 1,128,8192] [--reps 5] [--host-items 128]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS_PER_MUL = 49.0        # a full-width scalar multiplication on a full chip
PAIRING_LAUNCH_MS = 27.0  # one launch of the per-item pairing kernel


def rand_poly_bytes(rnd, n):
    raw = bytearray(rnd.randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        raw[i] &= 0x3F
    return bytes(raw)


def stats(ts):
    return {"median_ms": round(1e3 * statistics.median(ts), 3), "min_ms": round(1e3 * min(ts), 3), "max_ms": round(1e3 * max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="12:6,16:6", help="log_n:log_cell, ...")
    ap.add_argument("--counts", default="1,128,8192")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-items", type=int, default=0, help="time the host-formed route at this K (once)")
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",")]
    counts = [int(x) for x in args.counts.split(",")]
    import plonk_amd
    from oracle import bls12_381 as E
    from tests import g2_ref as G2
    Q = E.Q
    tau, g = 0x5EED0000 * 0x9E3779B97F4A7C15 % Q, 0xA5A5A5A5DEADBEEF   # circuits.synthetic_srs's defaults
    ctx = plonk_amd.Context(0)
    lib = ctx.lib
    npts = 1 << max(s[0] for s in shapes)
    buf = ctx.alloc(96 * npts)
    ctx.srs_generate_dev(tau, g, npts, buf.ptr)
    ctx.srs_load_dev(buf.ptr, npts)
    ctx.sync()
    buf.free()
    rnd = random.Random(1)
    for log_n, log_cell in shapes:
        n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
        dom = plonk_amd.KzgDomain(ctx, log_n)
        key = plonk_amd.KzgKey(ctx, E.g1_compress(E.g1_mul(E.G1_GEN, g)) + G2.g2_compress(G2.G2_GEN)
                               + G2.g2_compress(G2.g2_mul(G2.G2_GEN, pow(tau, l, Q))))
        ver = plonk_amd.KzgCellVerifier(key, log_n, log_cell)
        for K in counts:
            blobs = max(1, min(16, K)) if K <= 16 * r else -(-K // r)
            per = -(-K // blobs)
            cells, proofs, cm = dom.open_cells_bytes([rand_poly_bytes(rnd, n) for _ in range(blobs)], log_cell)
            picks = [(j, k) for j in range(blobs) for k in rnd.sample(range(r), per)][:K]
            cidx = (ctypes.c_uint32 * K)(*[j for j, _ in picks])
            kidx = (ctypes.c_uint32 * K)(*[k for _, k in picks])
            vals = b"".join(cells[32 * l * (j * r + k):32 * l * (j * r + k + 1)] for j, k in picks)
            prf = b"".join(proofs[48 * (j * r + k):48 * (j * r + k + 1)] for j, k in picks)
            verdicts = (ctypes.c_int32 * K)()
            infos = {"folded": [], "each": []}

            def folded():
                info = plonk_amd._VerifyInfo()
                t = time.perf_counter()
                rc = lib.plonk_kzg_verify_cells(ver.handle, cm, blobs, cidx, kidx, vals, prf, K, b"bench", 5, None, ctypes.byref(info))
                dt = time.perf_counter() - t
                assert rc == 0, rc
                infos["folded"].append((dt, info))
                return dt

            def each():
                info = plonk_amd._VerifyInfo()
                t = time.perf_counter()
                rc = lib.plonk_kzg_verify_cells_each(ver.handle, cm, blobs, cidx, kidx, vals, prf, K, verdicts, ctypes.byref(info))
                dt = time.perf_counter() - t
                assert rc == 0 and not any(verdicts), rc
                infos["each"].append((dt, info))
                return dt
            folded()                                               # warm-up: buffers grown, line tables made
            last_f = ver.last()
            each()
            infos = {"folded": [], "each": []}
            times = {"folded": [], "each": []}
            for _ in range(args.reps):
                times["folded"].append(folded())
                times["each"].append(each())
            out = {"log_n": log_n, "log_cell": log_cell, "items": K, "commitments": blobs}
            for name in ("folded", "each"):
                med = sorted(infos[name], key=lambda x: x[0])[len(infos[name]) // 2][1]
                out[name] = dict(stats(times[name]), **{p: round(getattr(med, p), 3) for p in ("ms_decode", "ms_scalars", "ms_msm", "ms_pairing")})
            out["msm_path_left"], out["msm_path_right"] = last_f["msm_path_left"], last_f["msm_path_right"]
            out["each_scalar_muls"] = K * (l + 1)
            out["each_predicted_ms"] = round(K * (l + 1) * NS_PER_MUL * 1e-6 + PAIRING_LAUNCH_MS, 3)
            out["device_bytes"] = ver.last()["device_bytes"]
            if args.host_items == K:
                # the route before this call existed: r_k by the inverse-NTT formula, commit(r_k) as an l-term MSM on the host
                from tests import kzg_cells_model as M
                pts = [E.g1_mul(E.G1_GEN, g * pow(tau, j, Q) % Q) for j in range(l)]
                x = dom.cell_points(log_cell)[0]
                t = time.perf_counter()
                a, b = [], []
                for i, (j, k) in enumerate(picks):
                    v = plonk_amd.fr_from_bytes_mont(vals[32 * l * i:32 * l * (i + 1)])
                    c = M.remainder_from_cell(v, log_n, log_cell, k)
                    commit_r = E.msm_pippenger(pts, c)
                    pk = E.g1_decompress(prf[48 * i:48 * (i + 1)])
                    bb = E.g1_add(E.g1_decompress(cm[48 * j:48 * (j + 1)]), E.g1_mul(commit_r, Q - 1) if commit_r is not None else None)
                    bb = E.g1_add(bb, E.g1_mul(pk, x[k]) if pk is not None else None)
                    a.append(prf[48 * i:48 * (i + 1)])
                    b.append(E.g1_compress(bb))
                t_host = time.perf_counter() - t
                t = time.perf_counter()
                got = key.pairing_check_each(a, b)
                t_pair = time.perf_counter() - t
                assert got == [0] * K
                out["host_route"] = {"form_b_ms": round(1e3 * t_host, 1), "pairing_check_each_ms": round(1e3 * t_pair, 3)}
            print(json.dumps(out), flush=True)
        ver.close()
        key.close()
        dom.close()
    ctx.close()


if __name__ == "__main__":
    main()
