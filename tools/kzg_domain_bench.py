"""KZG10 openings over a whole domain (plonk_kzg_domain_create / plonk_kzg_open_domain, plonk_amd/csrc/kzg_domain.hip) against
the only way to get the same outputs without them: one plonk_kzg_open of a length-n polynomial per domain point.  One JSON line
per (n, count): wall time of plonk_kzg_domain_create and of plonk_kzg_open_domain (best of --reps after a warm-up, the call
returns after its last device synchronisation), the time of ONE plonk_kzg_open of a length-n polynomial on the same context
times n (times count), and the ratio.  Then, when the doors of the per-kernel tests are built (tests/_build/
libdev_kzg_domain.so), the group transform alone at --stage-log points: time per stage launch, per scalar multiplication, and
the fraction of the integer-VALU issue bound that is (DESIGN.md section 14 has the instruction count behind the bound).

    python tools/kzg_domain_bench.py [--logs 8,12,16] [--counts 1,16] [--reps 3] [--stage-log 17]
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# the issue bound of one butterfly with a twiddle: 128 doublings + ~96 complete additions of the
# double-and-add, 2 additions around it; instructions per lane
BUTTERFLY_INSTRUCTIONS = 128 * 4500 + 98 * 7300
SIMDS, CLOCK_HZ, ISSUE_CYCLES = 1024, 2.4e9, 4.5      # 256 CUs x 4 SIMDs; one wave-instruction per ~4.5 cycles per SIMD


def best(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return min(out)


def rand_poly_bytes(rnd, n):
    raw = bytearray(rnd.randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        raw[i] &= 0x3F
    return bytes(raw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="8,12,16")
    ap.add_argument("--counts", default="1,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stage-log", type=int, default=17)
    args = ap.parse_args()
    logs = [int(x) for x in args.logs.split(",")]
    counts = [int(x) for x in args.counts.split(",")]
    import plonk_amd
    from oracle import bls12_381 as E
    tau, g = 0x5EED0000 * 0x9E3779B97F4A7C15 % E.Q, 0xA5A5A5A5DEADBEEF   # circuits.synthetic_srs's defaults
    ctx = plonk_amd.Context(0)
    npts = 1 << max(logs)
    buf = ctx.alloc(96 * npts)
    ctx.srs_generate_dev(tau, g, npts, buf.ptr)
    ctx.srs_load_dev(buf.ptr, npts)
    ctx.sync()
    buf.free()
    rnd = random.Random(1)
    for log_n in logs:
        n = 1 << log_n
        made = []

        def create():
            if made:
                made.pop().close()
            made.append(plonk_amd.KzgDomain(ctx, log_n))
        t_create = best(create, args.reps)
        dom = made[0]
        polys = [rand_poly_bytes(rnd, n) for _ in range(max(counts))]
        z = rnd.randrange(E.Q)
        t_single = best(lambda: ctx.kzg_open([polys[0]], z, None), args.reps)
        for count in counts:
            t_open = best(lambda: dom.open_bytes(polys[:count]), args.reps)
            last = dom.last()
            print(json.dumps({"log_n": log_n, "count": count, "domain_create_ms": round(1e3 * t_create, 3),
                              "open_domain_ms": round(1e3 * t_open, 3), "kzg_open_single_ms": round(1e3 * t_single, 3),
                              "n_single_openings_ms": round(1e3 * t_single * n * count, 1),
                              "ratio": round(t_single * n * count / t_open, 2), "chunks": last["chunks"],
                              "stage_launches": last["stage_launches"], "scalar_muls": last["scalar_muls"],
                              "device_bytes": last["device_bytes"]}), flush=True)
        dom.close()
    so = os.path.join(ROOT, "tests", "_build", "libdev_kzg_domain.so")
    if args.stage_log and os.path.exists(so):
        lib = ctypes.CDLL(so)
        vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        lib.dkd_twiddles.argtypes = [vp, u32, ctypes.POINTER(vp)]
        lib.dkd_free.argtypes = [vp, vp]
        lib.dkd_transform.argtypes = [vp, vp, u64, u32, u32, ci, vp, u32, vp]
        lib.dkd_pointwise.argtypes = [vp, vp, vp, u64, vp, u64, u32, u32, vp]
        lib.dkd_load_raw.argtypes = [vp, vp, u64, vp]
        sl = args.stage_log
        size = 1 << sl
        base, slots, sc = ctx.alloc(256 * size), ctx.alloc(256 * size), ctx.alloc(32 * size)
        raw = ctx.alloc(96 * size)
        raw.upload(plonk_amd.g1_to_raw96(E.G1_GEN) * size)
        assert lib.dkd_load_raw(ctx.handle, raw.ptr, size, base.ptr) == 0
        raw.free()
        sc.upload(rand_poly_bytes(rnd, size))
        tw = vp()
        assert lib.dkd_twiddles(ctx.handle, sl, ctypes.byref(tw)) == 0

        def fill():
            assert lib.dkd_pointwise(ctx.handle, base.ptr, sc.ptr, size, slots.ptr, size, sl, 1, plonk_amd.fr_to_bytes_mont([1])) == 0
        t_point = best(fill, args.reps)
        for inverse in (0, 1):
            counts2 = (u64 * 2)()
            times = []
            for _ in range(args.reps + 1):
                fill()
                counts2[0] = counts2[1] = 0
                t = time.perf_counter()
                assert lib.dkd_transform(ctx.handle, slots.ptr, size, sl, 1, inverse, tw, sl, counts2) == 0
                times.append(time.perf_counter() - t)
            t_tr = min(times[1:])
            muls = int(counts2[1])
            bound = muls * BUTTERFLY_INSTRUCTIONS / 64 * ISSUE_CYCLES / (SIMDS * CLOCK_HZ)
            print(json.dumps({"transform": "inverse" if inverse else "forward", "size_log": sl, "stages": int(counts2[0]),
                              "total_ms": round(1e3 * t_tr, 3), "ms_per_stage": round(1e3 * t_tr / sl, 3), "scalar_muls": muls,
                              "ns_per_scalar_mul": round(1e9 * t_tr / muls, 2), "issue_bound_ms": round(1e3 * bound, 3),
                              "fraction_of_issue_bound": round(bound / t_tr, 3)}), flush=True)
        print(json.dumps({"pointwise": size, "ms": round(1e3 * t_point, 3), "ns_per_scalar_mul": round(1e9 * t_point / size, 2)}), flush=True)
        lib.dkd_free(ctx.handle, tw)
        for b in (base, slots, sc):
            b.free()
    ctx.close()


if __name__ == "__main__":
    main()
