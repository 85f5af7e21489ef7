"""Cost of witness generation on the device (plonk_prover_fill_inputs / _prove_inputs, plonk_amd/csrc/composer.hip) on the
reference's bench circuit (benches/plonk.rs:33-82: the loop body repeated until the gate count reaches the size), recorded
through plonk_amd.Composer.  One JSON line per size:

  fill_device     plonk_prover_fill_inputs without copying the table back: upload of the inputs, every level launch, the
                  public-input values and the one synchronisation; best and median of --reps
  fill_host       the one-thread host executor of the SAME gadget statements (composer_core.hpp through the CPU harness
                  tests/csrc/host_composer.cpp) on this box: the yardstick for the fill
  prove_inputs    fill + proof; prove_witnesses is the same proof from a witness table in host memory and prove_dev the
                  same proof from resident wire columns (what the parent commit offers once a table exists)
  program         records, levels, widest level, launches per fill

    python tools/composer_bench.py [--log-gates 12,16,20] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x5EED0000 * 0x9E3779B97F4A7C15
G_SCALAR = 0xA5A5A5A5DEADBEEF


def summary(xs):
    return {"best_ms": round(min(xs), 3), "median_ms": round(statistics.median(xs), 3)}


def bench_circuit(case_mod, composer, gates):
    """the reference's loop: rounds are appended while the gates so far plus one round's worth stay below the size"""
    k = case_mod.Case(composer)
    c = composer
    z = case_mod.jj_mul(case_mod.GEN, 7)
    wa, wb, wx, wy = k.inp(2), k.inp(3), k.inp(6), k.inp(7)
    wz = k.point(z)
    diff, prev = 0, c.info()["constraints"]
    while prev + diff < gates:
        r = c.gate_mul(wa, wb)
        c.append_constant(15)
        c.append_constant_point(z)
        c.assert_equal(wx, r)
        c.assert_equal_point(wz, wz)
        c.gate_add(wa, wb)
        c.component_add_point(wz, wz)
        c.append_logic_and(wa, wb, 127)
        c.append_logic_xor(wa, wb, 127)
        c.component_boolean(c.ONE)
        c.component_decomposition(wa, 254)
        c.component_mul_generator(wy, case_mod.GEN)
        c.component_mul_point(wy, wz)
        c.component_range_bits(wa, 256)
        c.component_select(c.ONE, wa, wb)
        c.component_select_identity(c.ONE, wz)
        c.component_select_one(c.ONE, wa)
        c.component_select_point(c.ONE, wz, wz)
        c.component_select_zero(c.ONE, wa)
        now = c.info()["constraints"]
        diff, prev = now - prev, now
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-gates", default="12,16,20")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import plonk_amd
    from tests import composer_cases as CC
    Q = plonk_amd.Q
    for log_n in [int(x) for x in args.log_gates.split(",")]:
        ctx = plonk_amd.Context(0)
        host = bench_circuit(CC, CC.HostComposer(), 1 << log_n)
        dev = bench_circuit(CC, plonk_amd.Composer(), 1 << log_n)
        info = dev.c.info()
        n = CC.domain_size(info["constraints"])
        pts = ctx.alloc(96 * (n + 7))
        ctx.srs_generate_dev(TAU % Q, G_SCALAR, n + 7, pts.ptr)
        ctx.srs_load_dev(pts.ptr, n + 7)
        pts.free()
        t0 = time.perf_counter()
        prover = plonk_amd.Prover.compile_composer(ctx, b"composer-bench", dev.c)
        out = {"log_gates": log_n, "domain": n, "program": info, "compile_ms": round((time.perf_counter() - t0) * 1e3, 1),
               "reps": args.reps}
        inputs = plonk_amd.fr_to_bytes_mont(dev.inputs)
        bl = plonk_amd.fr_to_bytes_mont([(0xB11D0000 + i) * 0x9E3779B97F4A7C15 % Q for i in range(14)])
        layout_rows = dev.c.layout()["pi_rows"]
        table, pi = prover.fill_inputs(inputs)
        t0 = time.perf_counter()
        htable, hpi, err = host.c.fill(host.inputs)
        first_host = (time.perf_counter() - t0) * 1e3
        assert err is None and htable == table and hpi == pi
        fill, hostfill, pin, pwit = [], [], [], []
        proof, _ = prover.prove_inputs(inputs, bl)
        pimap = dict(zip(layout_rows, pi))
        assert prover.prove_witnesses(table, pimap, bl) == proof
        for _ in range(args.reps):
            ctx.sync()
            t = time.perf_counter()
            prover.fill_inputs(inputs, want_witnesses=False)
            fill.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            prover.prove_inputs(inputs, bl)
            pin.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            prover.prove_witnesses(table, pimap, bl)
            pwit.append((time.perf_counter() - t) * 1e3)
        for _ in range(min(args.reps, 3)):
            t = time.perf_counter()
            host.c.fill(host.inputs)
            hostfill.append((time.perf_counter() - t) * 1e3)
        out["fill_device"] = summary(fill)
        out["fill_host_one_thread"] = summary(hostfill + [first_host])
        out["prove_inputs"] = summary(pin)
        out["prove_witnesses"] = summary(pwit)
        # the same proof from resident wire columns: gather them once from the table through the layout
        wires = dev.c.layout()["wires"]
        buf = ctx.alloc(4 * 32 * n)
        zero = bytes(32)
        for k in range(4):
            col = b"".join(table[32 * w:32 * w + 32] for w in wires[k]) + zero * (n - len(wires[k]))
            buf.upload(col, 32 * n * k)
        assert prover.prove_dev(buf.ptr, pimap, bl) == proof
        pdev = []
        for _ in range(args.reps):
            ctx.sync()
            t = time.perf_counter()
            prover.prove_dev(buf.ptr, pimap, bl)
            pdev.append((time.perf_counter() - t) * 1e3)
        out["prove_dev"] = summary(pdev)
        buf.free()
        print(json.dumps(out), flush=True)
        prover.close()
        ctx.close()


if __name__ == "__main__":
    main()
