"""KZG10 cell recovery (plonk_kzg_recover_cells_dev, plonk_amd/csrc/kzg_recover.hip) beside the transform work it cannot avoid,
one MI355X, one process.  Per (n, l, count), half of the cells missing (a random half), resident form: a warm-up of every
route, then --reps runs per route ALTERNATING between the routes, wall time of the call (it returns after its last device
synchronisation), reported as median [min, max]:

    recover          coefficients and cell values, no proofs: 4 transforms per polynomial + Z_r + the three passes + the verdict
    yardstick        4 x count plonk_ntt_dev calls of size n (inverse, coset, inverse coset, forward) and one synchronisation
    recover+proofs   the same with proofs and commitments
    open_cells       plonk_kzg_open_cells_dev alone on the recovered coefficients (what the proofs cost anyway)

One JSON line per (n, l, count) with the four, recover / yardstick, and the pieces of the remainder each timed on its own
through the test doors (tests/_build/libdev_kzg_recover.so, libdev_poly.so; wall time of a queued kernel plus its
synchronisation, median of --reps, count polynomials): the vanish kernel (with the r powers of phi it reads), the batch
inverse of r values, scatter, divide, tail, and a 4 x count byte read-back.

    python tools/kzg_recover_bench.py [--shapes 12:6,16:6,20:9] [--counts 1,16] [--reps 5]
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


def load_doors():
    build = os.path.join(ROOT, "tests", "_build")
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    try:
        kr, dp = ctypes.CDLL(os.path.join(build, "libdev_kzg_recover.so")), ctypes.CDLL(os.path.join(build, "libdev_poly.so"))
    except OSError:
        return None, None
    kr.dkr_vanish.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp]
    kr.dkr_scatter.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp]
    kr.dkr_divide.argtypes = [vp, vp, vp, u32, u32, u32]
    kr.dkr_tail.argtypes = [vp, vp, u32, u64, u32, vp]
    dp.dp_batch_inverse.argtypes = [vp, vp, u64, ci, ci]
    return kr, dp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="12:6,16:6,20:9", help="log_n:log_cell, ...")
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
    kr, dp = load_doors()
    rnd = random.Random(1)
    for log_n, log_cell in shapes:
        n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
        dom = plonk_amd.KzgDomain(ctx, log_n)
        ids = rnd.sample(range(r), r // 2)
        a, d, top = len(ids), n // 2, max(counts)
        # the blob: `top` polynomials of n / 2 coefficients, opened once on the device; the given cells packed per polynomial
        polys = [ctx.alloc(32 * d) for _ in range(top)]
        for p in polys:
            p.upload(rand_poly_bytes(rnd, d))
        cells, proofs, cm = ctx.alloc(32 * n * top), ctx.alloc(48 * r * top), ctx.alloc(48 * top)
        dom.open_cells_dev([p.ptr for p in polys], [d] * top, log_cell, cells.ptr, proofs.ptr, cm.ptr)
        ref = (cells.download(), proofs.download(), cm.download())
        given = [ctx.alloc(32 * a * l) for _ in range(top)]
        for j, gbuf in enumerate(given):
            gbuf.upload(b"".join(ref[0][32 * (j * n + k * l):32 * (j * n + (k + 1) * l)] for k in ids))
        coeffs, tmp = ctx.alloc(32 * n * top), ctx.alloc(32 * n)
        for count in counts:
            gp = [b.ptr for b in given[:count]]

            def yardstick():
                for j in range(count):
                    p = coeffs.ptr + 32 * n * j
                    ctx.ntt_dev(p, p, tmp.ptr, log_n, inverse=True)
                    ctx.ntt_dev(p, p, tmp.ptr, log_n, coset=True)
                    ctx.ntt_dev(p, p, tmp.ptr, log_n, inverse=True, coset=True)
                    ctx.ntt_dev(p, p, tmp.ptr, log_n)
                ctx.sync()

            routes = {
                "recover": lambda: dom.recover_cells_dev(ids, gp, log_cell, d, coeffs=coeffs.ptr, cells=cells.ptr),
                "yardstick": yardstick,
                "recover_proofs": lambda: dom.recover_cells_dev(ids, gp, log_cell, d, coeffs.ptr, cells.ptr, proofs.ptr, cm.ptr),
            }
            times = {k: [] for k in routes}
            routes["recover_proofs"]()                         # warm-up, and the bytes are those of open_cells
            assert (cells.download(32 * n * count), proofs.download(48 * r * count), cm.download(48 * count)) == \
                (ref[0][:32 * n * count], ref[1][:48 * r * count], ref[2][:48 * count])
            routes["recover"]()
            info = dom.recover_last()
            # open_cells alone on the recovered coefficients (timed in the same alternation)
            cp = [coeffs.ptr + 32 * n * j for j in range(count)]
            routes["open_cells"] = lambda: dom.open_cells_dev(cp, [d] * count, log_cell, cells.ptr, proofs.ptr, cm.ptr)
            times["open_cells"] = []
            for _ in range(args.reps):
                for k in ("recover", "recover_proofs", "open_cells", "yardstick"):      # open_cells reads the coefficients the
                    times[k].append(timed(routes[k]))                                   # recovery left; the yardstick overwrites them
            line = {"log_n": log_n, "log_cell": log_cell, "count": count, "available": a, "missing": r - a,
                    "recover": stats(times["recover"]), "yardstick_4_ntt": stats(times["yardstick"]),
                    "recover_proofs": stats(times["recover_proofs"]), "open_cells": stats(times["open_cells"]),
                    "chunks": info["chunks"], "transforms": info["transforms"], "vanish_muls": info["vanish_muls"]}
            line["ratio"] = round(line["recover"]["median_ms"] / line["yardstick_4_ntt"]["median_ms"], 2)
            if kr is not None:                                 # the pieces of the remainder, each on its own
                pw, zd, zc, fl = ctx.alloc(32 * r), ctx.alloc(32 * r), ctx.alloc(32 * r), ctx.alloc(4 * count)
                miss = [k for k in range(r) if k not in set(ids)]
                mb, sl, vecs = ctx.alloc(4 * len(miss)), ctx.alloc(4 * r), ctx.alloc(8 * count)
                mb.upload(bytes((ctypes.c_uint32 * len(miss))(*miss)))
                slot = [-1] * r
                for i, k in enumerate(ids):
                    slot[k] = i
                sl.upload(bytes((ctypes.c_int32 * r)(*slot)))
                vecs.upload(bytes((ctypes.c_uint64 * count)(*gp)))
                h = ctx.handle
                pieces = {
                    "vanish": lambda: kr.dkr_vanish(h, pw.ptr, mb.ptr, len(miss), log_n, log_cell, zd.ptr, zc.ptr),
                    "batch_inverse": lambda: dp.dp_batch_inverse(h, zc.ptr, r, 0, -1),
                    "scatter": lambda: kr.dkr_scatter(h, vecs.ptr, sl.ptr, zd.ptr, log_n, log_cell, count, coeffs.ptr),
                    "divide": lambda: kr.dkr_divide(h, coeffs.ptr, zc.ptr, log_n, log_cell, count),
                    "tail": lambda: kr.dkr_tail(h, coeffs.ptr, log_n, d, count, fl.ptr),
                    "read_back": lambda: fl.download(),
                }
                line["pieces_ms"] = {}
                for k, fn in pieces.items():
                    assert fn() in (0, None) or k == "read_back"
                    line["pieces_ms"][k] = round(1e3 * statistics.median(timed(fn) for _ in range(args.reps)), 3)
                for b in (pw, zd, zc, fl, mb, sl, vecs):
                    b.free()
            print(json.dumps(line), flush=True)
        for b in polys + given + [cells, proofs, cm, coeffs, tmp]:
            b.free()
        dom.close()
    ctx.close()


if __name__ == "__main__":
    main()
