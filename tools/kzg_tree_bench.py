"""KZG10 vector-commitment trees against the routes a caller had before them.  Resident random leaves, bytes
checked equal first, `--runs` alternating runs after a warm-up, median [min, max] with the host clock around calls that end in a
device synchronisation.  One JSON line per measurement.

    build    KzgTree.build_dev at (2^8, 2) and (2^8, 3) against
               - the sum of commit_many_dev calls on the same per-level counts (that code is not touched: the parent's figure)
               - the old route end to end: per level commit_many_dev, the 48-byte commitments to the host, h there in C
                 (tests/_build/libhost_kzg_tree.so: kzg_tree_core.hpp under g++), the scalars back up
    update   KzgTree.update of 1, 256 and 4096 random leaves at (2^8, 3), the values alternating between two sets so that no delta
             is zero, against
               - plonk_kzg_update_many with checked bases over the same segments, level by level (the copies and the host's h
                 between the levels are NOT counted: the figure favours the old route)
               - a full rebuild (build_dev)
    prove    KzgTree.prove / KzgKey.check_tree of 1, 64 and 4096 leaves at (2^8, 3) against open_multi_dev / check_multi called
             directly with the same items over copies of the levels: the difference is the cost of assembling the path

    python tools/kzg_tree_bench.py [--runs 5] [--depths 2,3] [--updates 1,256,4096] [--proofs 1,64,4096]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU, G = 0x5EED0000 * 0x9E3779B97F4A7C15, 0xA5A5A5A5DEADBEEF   # the synthetic key of the test suite
LOG_N = 8
N1 = 1 << LOG_N


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def host_lib():
    so = os.path.join(ROOT, "tests", "_build", "libhost_kzg_tree.so")
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "csrc", "host_kzg_tree.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hkt_map_many.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return lib


def random_bytes(seed, values):
    import numpy as np
    raw = np.random.default_rng(seed).integers(0, 256, size=(values, 32), dtype=np.uint8)
    raw[:, 31] &= 0x3F                                                  # below 2^254 < q
    return raw.tobytes()                                                # (read as Montgomery limbs: any canonical residue will do)


def level_sets(depth, idx):
    T = [None] * (depth + 1)
    T[depth] = sorted(idx)
    for l in range(depth - 1, -1, -1):
        T[l] = sorted({j >> LOG_N for j in T[l + 1]})
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--depths", default="2,3")
    ap.add_argument("--updates", default="1,256,4096")
    ap.add_argument("--proofs", default="1,64,4096")
    args = ap.parse_args()
    import plonk_amd as P
    host = host_lib()
    ctx = P.Context(0)
    keybuf = ctx.alloc(96 * N1)
    ctx.srs_generate_dev(TAU % P.Q, G, N1, keybuf.ptr)
    ctx.srs_load_dev(keybuf.ptr, N1)
    ctx.sync()
    keybuf.free()
    from tests import kzg_ref
    key = P.KzgKey(ctx, kzg_ref.opening_key())
    dom = P.KzgDomain(ctx, LOG_N)
    dom.build_many_tables(8)
    for depth in [int(x) for x in args.depths.split(",")]:
        N = 1 << (LOG_N * depth)
        raw = random_bytes(depth, N)
        leaves = ctx.alloc(32 * N)
        leaves.upload(raw)
        tree = P.KzgTree(dom, depth)
        counts = [1 << (LOG_N * l) for l in range(depth - 1, -1, -1)]            # nodes per level, bottom up
        out = ctx.alloc(48 * counts[0])
        scal = ctx.alloc(32 * counts[0])
        levels = {}                                                            # level -> host bytes of vals[level] (the old route's)

        def run_tree():
            tree.build_dev(leaves.ptr)

        def run_commits():
            for c in counts:
                dom.commit_many_dev(leaves.ptr, c, out.ptr)

        def run_old():
            src = leaves.ptr
            for l, c in zip(range(depth - 1, -1, -1), counts):
                dom.commit_many_dev(src, c, out.ptr)
                cm = out.download(48 * c)
                if l:
                    vals = ctypes.create_string_buffer(32 * c)
                    assert host.hkt_map_many(cm, c, vals) == 1
                    scal.upload(vals.raw)
                    levels[l - 1] = vals.raw
                    src = scal.ptr
            return cm[:48]

        run_tree()
        run_commits()
        assert run_old() == tree.root(), "the two routes disagree"
        levels[depth - 1] = raw
        t_tree, t_commits, t_old = [], [], []
        for _ in range(args.runs):
            t_tree.append(timed(run_tree))
            t_commits.append(timed(run_commits))
            t_old.append(timed(run_old))
        print(json.dumps({"what": "build", "log_n": LOG_N, "depth": depth, "nodes": sum(counts), "runs": args.runs, "tree_build_dev": stats(t_tree),
                          "sum_of_commit_many_dev": stats(t_commits), "old_route_end_to_end": stats(t_old),
                          "ratio_to_commits": round(statistics.median(t_tree) / statistics.median(t_commits), 3),
                          "last": tree.last()}), flush=True)
        if depth == 3:
            updates(ctx, args, dom, tree, leaves, depth, N)
            proofs(ctx, args, dom, key, tree, levels, depth, N)
        tree.close()
        for b in (leaves, out, scal):
            b.free()
    dom.close()
    key.close()
    ctx.close()


def updates(ctx, args, dom, tree, leaves, depth, N):
    import plonk_amd as P
    rebuild = P.KzgTree(dom, depth)
    rnd = random.Random(23)
    for count in [int(x) for x in args.updates.split(",")]:
        idx = rnd.sample(range(N), count)
        T = level_sets(depth, idx)
        iarr = (ctypes.c_uint64 * count)(*idx)
        sets = [random_bytes(100 + count, count), random_bytes(200 + count, count)]
        fn, h = ctx.lib.plonk_kzg_tree_update, tree.handle
        flip = [0]

        def run_tree():
            flip[0] ^= 1
            ctx._check(fn(h, iarr, sets[flip[0]], count))

        # the old route's calls: per level the touched nodes as segments with their current commitments as checked bases
        calls = []
        for l in range(depth - 1, -1, -1):
            nodes, terms = T[l], T[l + 1]
            offs, k = [0], 0
            for node in nodes:
                while k < len(terms) and terms[k] >> LOG_N == node:
                    k += 1
                offs.append(k)
            level_nodes = tree.nodes(l)
            calls.append((b"".join(level_nodes[node] for node in nodes), (ctypes.c_uint64 * len(offs))(*offs),
                          (ctypes.c_uint32 * len(terms))(*[j & (N1 - 1) for j in terms]), random_bytes(300 + l, len(terms)), len(nodes),
                          ctypes.create_string_buffer(48 * len(nodes))))

        def run_old():
            for base, offs, ix, deltas, cnt, cm in calls:
                ctx._check(ctx.lib.plonk_kzg_update_many(dom.handle, base, offs, ix, deltas, cnt, cm))

        def run_rebuild():
            rebuild.build_dev(leaves.ptr)

        def sync_leaves():
            """the caller's copy of the leaves follows the tree's"""
            for k, j in enumerate(idx):
                leaves.upload(sets[flip[0]][32 * k:32 * k + 32], 32 * j)

        run_tree()
        run_old()
        sync_leaves()
        run_rebuild()
        assert rebuild.root() == tree.root(), "an updated tree and a tree built from the new leaves disagree"
        t_tree, t_old, t_rebuild = [], [], []
        for _ in range(args.runs):
            t_tree.append(timed(run_tree))
            t_old.append(timed(run_old))
            t_rebuild.append(timed(run_rebuild))
        sync_leaves()
        print(json.dumps({"what": "update", "log_n": LOG_N, "depth": depth, "leaves": count, "runs": args.runs, "tree_update": stats(t_tree),
                          "update_many_checked_bases_per_level": stats(t_old), "full_rebuild": stats(t_rebuild), "last": tree.last()}), flush=True)
    rebuild.close()


def proofs(ctx, args, dom, key, tree, levels, depth, N):
    rnd = random.Random(29)
    # copies of the levels for the direct calls (the tree was updated since: build it again from the leaves the levels belong to)
    bufs = {}
    for l, raw in levels.items():
        bufs[l] = ctx.alloc(len(raw))
        bufs[l].upload(raw)
    tree.build_dev(bufs[depth - 1].ptr)
    for count in [int(x) for x in args.proofs.split(",")]:
        idx = rnd.sample(range(N), count)
        T = level_sets(depth, idx)
        vectors = [(l, k) for l in range(depth) for k in T[l]]
        where = {v: i for i, v in enumerate(vectors)}
        items = [(where[(l, j >> LOG_N)], j & (N1 - 1)) for l in range(depth) for j in T[l + 1]]
        ptrs = [bufs[l].ptr + 32 * N1 * k for l, k in vectors]
        label = b"bench"
        values, path, proof = tree.prove(idx, label)
        root = tree.root()
        cms = [root] + path
        dvalues, _, dproof = dom.open_multi_dev(ptrs, items, label, commitments=cms)
        assert dproof == proof, "the tree's proof is not the multiproof of the same items"
        assert key.check_tree(LOG_N, depth, root, idx, values, path, proof, label) and key.check_multi(LOG_N, cms, items, dvalues, proof, label)
        t_prove, t_direct, t_check, t_check_direct = [], [], [], []
        for _ in range(args.runs):
            t_prove.append(timed(lambda: tree.prove(idx, label)))
            t_direct.append(timed(lambda: dom.open_multi_dev(ptrs, items, label, commitments=cms)))
            t_check.append(timed(lambda: key.check_tree(LOG_N, depth, root, idx, values, path, proof, label)))
            t_check_direct.append(timed(lambda: key.check_multi(LOG_N, cms, items, dvalues, proof, label)))
        print(json.dumps({"what": "prove", "log_n": LOG_N, "depth": depth, "leaves": count, "items": len(items), "vectors": len(vectors),
                          "runs": args.runs, "tree_prove": stats(t_prove), "open_multi_dev_same_items": stats(t_direct),
                          "check_tree": stats(t_check), "check_multi_same_items": stats(t_check_direct)}), flush=True)
    for b in bufs.values():
        b.free()


if __name__ == "__main__":
    main()
