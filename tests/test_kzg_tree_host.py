"""CPU: what the host decides of a KZG10 vector-commitment tree.

plonk_amd/csrc/kzg_tree_core.hpp — the level sets T_l of a set of leaves, the duplicate check, the segments and child indices of
an update, the canonical order of a proof and its node count, the chunk plans, and the map h from a node's 48 bytes to the
scalar its parent commits to — is compiled with g++ (tests/csrc/host_kzg_tree.cpp) and checked against the big-int model
tests/kzg_tree_model.py; h against oracle/merlin.py.  The same cases are run through a stand-alone program built with
-fsanitize=address,undefined (tests/csrc/san_kzg_tree.cpp): the index logic takes untrusted indices."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as E
from tests import kzg_many_model as MM
from tests import kzg_ref as K
from tests import kzg_tree_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_kzg_tree.so")
SAN = os.path.join(HERE, "_build", "san_kzg_tree")
Q = E.Q
OK, ERR_ARG = 0, -1
R_MONT = (1 << 256) % Q


def _deps(src):
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    return [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(f) > os.path.getmtime(target) for f in deps)


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_kzg_tree.cpp")
    if _stale(SO, _deps(src)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    u64, u32, vp, ci = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int
    lib.hkt_check_shape.argtypes = [u32, u32]
    lib.hkt_data_bytes.argtypes = [u32, u32]
    lib.hkt_data_bytes.restype = u64
    lib.hkt_nodes.argtypes = [u32, u32]
    lib.hkt_nodes.restype = u64
    lib.hkt_const.argtypes = [ci]
    lib.hkt_const.restype = u64
    lib.hkt_sets.argtypes = [u32, u32, vp, u64, u64, vp, vp, vp]
    lib.hkt_proof_nodes.argtypes = [u32, u32, vp, u64, vp]
    lib.hkt_proof_plan.argtypes = [u32, u32, vp, u64, vp, vp, vp, vp]
    lib.hkt_update_plan.argtypes = [u32, u32, vp, u64, u64, vp, vp, vp, vp, vp, vp]
    lib.hkt_build_plan.argtypes = [u32, u32, u32, u64, vp]
    lib.hkt_build_plan.restype = None
    lib.hkt_map.argtypes = [vp, vp]
    lib.hkt_map_transcript.argtypes = [vp, vp]
    lib.hkt_map_transcript.restype = None
    return lib


def u64s(values):
    values = list(values)
    return (ctypes.c_uint64 * max(len(values), 1))(*values)


def c_sets(lib, log_n, depth, idx, max_count=M.MAX_CLAIMS):
    idx = list(idx)
    count = len(idx)
    sizes = (ctypes.c_uint64 * (depth + 1))()
    flat = (ctypes.c_uint64 * max((depth + 1) * count, 1))()
    order = (ctypes.c_uint64 * max(count, 1))()
    rc = lib.hkt_sets(log_n, depth, u64s(idx) if count else None, count, max_count, sizes, flat, order)
    if rc:
        return rc, None, None
    T, at = [], 0
    for l in range(depth + 1):
        T.append(list(flat[at:at + sizes[l]]))
        at += sizes[l]
    return rc, T, list(order[:count])


def c_proof_plan(lib, log_n, depth, idx):
    idx = list(idx)
    count = len(idx)
    counts = (ctypes.c_uint64 * 3)()
    lv = (ctypes.c_uint64 * (depth + 1))()
    vi = (ctypes.c_uint32 * max(depth * count, 1))()
    pi = (ctypes.c_uint32 * max(depth * count, 1))()
    rc = lib.hkt_proof_plan(log_n, depth, u64s(idx) if count else None, count, counts, lv, vi, pi)
    if rc:
        return rc, None
    return rc, {"vectors": counts[0], "items": list(zip(vi[:counts[1]], pi[:counts[1]])), "path_nodes": counts[2], "level_vector": list(lv)}


def c_update_plan(lib, log_n, depth, idx, ws_cap=MM.WS_CAP_DEFAULT):
    idx = list(idx)
    count = len(idx)
    levels = (ctypes.c_uint64 * (5 * depth))()
    node = (ctypes.c_uint64 * max(depth * count, 1))()
    offsets = (ctypes.c_uint64 * (depth * (count + 1)))()
    flat = (ctypes.c_uint64 * max(depth * count, 1))()
    child = (ctypes.c_uint32 * max(depth * count, 1))()
    totals = (ctypes.c_uint64 * 5)()
    rc = lib.hkt_update_plan(log_n, depth, u64s(idx) if count else None, count, ws_cap, levels, node, offsets, flat, child, totals)
    if rc:
        return rc, None, None
    out = []
    for step in range(depth):
        nodes, terms, node_at, offs_at, term_at = levels[5 * step:5 * step + 5]
        offs = list(offsets[offs_at:offs_at + nodes + 1])
        assert offs[0] == 0 and offs[-1] == terms
        segs = [[(child[term_at + k], flat[term_at + k]) for k in range(offs[j], offs[j + 1])] for j in range(nodes)]
        out.append({"level": depth - 1 - step, "nodes": list(node[node_at:node_at + nodes]), "segments": segs})
    return rc, out, dict(zip(("touched_nodes", "sparse_terms", "most_nodes", "most_terms", "chunks"), totals))


# ---- the cases the issue names, shared with the sanitizer program ------------------------------------------------------------------
def cases():
    out = {}
    for (log_n, depth) in ((2, 3), (1, 3), (8, 2), (3, 1), (12, 2), (1, 26)):
        n, N = 1 << log_n, 1 << (log_n * depth)
        out["single leaf, the first (%d, %d)" % (log_n, depth)] = (log_n, depth, [0])
        out["single leaf, the last (%d, %d)" % (log_n, depth)] = (log_n, depth, [N - 1])
        out["single leaf inside (%d, %d)" % (log_n, depth)] = (log_n, depth, [N // 3])
        out["two leaves in one bottom node (%d, %d)" % (log_n, depth)] = (log_n, depth, [N - n + 1, N - n])
        if depth >= 2:
            out["two bottom nodes under one parent (%d, %d)" % (log_n, depth)] = (log_n, depth, [n, 0])
            out["leaves under different children of the root (%d, %d)" % (log_n, depth)] = (log_n, depth, [N - 1, 0, N // n])
        rnd = random.Random(100 * log_n + depth)
        out["random, caller's order (%d, %d)" % (log_n, depth)] = (log_n, depth, rnd.sample(range(N), min(N, 37)))
    out["all N leaves at (2, 3)"] = (1, 3, list(range(8)))
    out["all N leaves at (4, 3), reversed"] = (2, 3, list(range(63, -1, -1)))
    out["a whole bottom node at (2^8, 2)"] = (8, 2, list(range(512, 768)))
    out["D = 1, all leaves"] = (3, 1, list(range(8)))
    return out


def refused():
    return {"empty": (2, 3, []), "repeated": (2, 3, [5, 9, 5]), "repeated, adjacent": (2, 3, [7, 7]), "out of range by one": (2, 3, [64]),
            "out of range, far": (2, 3, [1 << 63]), "in range and out": (2, 3, [0, 63, 1 << 40]), "depth 0": (2, 0, [0]),
            "log_n 0": (0, 3, [0]), "log_n 13": (13, 2, [0]), "27 bits": (9, 3, [0]), "more indices than leaves": (1, 1, [0, 1, 0]),
            "a depth whose product wraps": (8, 1 << 29, [0])}


def test_constants_and_shapes(lib):
    assert [lib.hkt_const(k) for k in range(5)] == [M.LOG_N_MAX, M.MAX_BITS, M.MAX_UPDATE, M.MAX_PROOF_NODES, M.MAX_CLAIMS]
    for log_n in range(0, 15):
        for depth in range(0, 29):
            assert (lib.hkt_check_shape(log_n, depth) == OK) == M.shape_ok(log_n, depth), (log_n, depth)
    assert lib.hkt_check_shape(8, 1 << 29) == ERR_ARG and lib.hkt_check_shape(1 << 31, 2) == ERR_ARG
    for log_n, depth in ((1, 1), (2, 3), (8, 2), (8, 3), (12, 2), (1, 26)):
        assert lib.hkt_data_bytes(log_n, depth) == M.data_bytes(log_n, depth)
        assert lib.hkt_nodes(log_n, depth) == sum(1 << (log_n * l) for l in range(depth))


@pytest.mark.parametrize("name", list(cases()))
def test_sets_proof_order_and_update_plan_against_the_model(lib, name):
    log_n, depth, idx = cases()[name]
    rc, T, order = c_sets(lib, log_n, depth, idx)
    want = M.sets(log_n, depth, idx)
    assert rc == OK and T == want and T[0] == [0]
    assert [idx[k] for k in order] == T[depth], "order[k] names the caller's position of sorted leaf k"
    rc, plan = c_proof_plan(lib, log_n, depth, idx)
    model = M.proof_plan(log_n, depth, idx)
    assert rc == OK and plan["vectors"] == len(model["vectors"]) and plan["items"] == model["items"]
    assert plan["path_nodes"] == len(model["path"]) == M.proof_nodes(log_n, depth, idx)
    assert plan["level_vector"] == [sum(len(T[k]) for k in range(l)) for l in range(depth + 1)]
    nodes = ctypes.c_uint64(1 << 60)
    assert lib.hkt_proof_nodes(log_n, depth, u64s(idx), len(idx), ctypes.byref(nodes)) == OK and nodes.value == len(model["path"])
    # the items of level l < D-1 are one to one with the path commitments of level l + 1
    inner = [model["vectors"][v] for v, _ in model["items"][:len(model["path"])]]
    assert len(inner) == len(model["path"]) and all(lv + 1 == pl for (lv, _), (pl, _) in zip(inner, model["path"]))
    assert [(l - 1, k >> log_n) for l, k in model["path"]] == inner
    if depth == 1:
        assert model["path"] == [] and plan["vectors"] == 1 and plan["items"] == [(0, j) for j in sorted(idx)]
    rc, levels, totals = c_update_plan(lib, log_n, depth, idx)
    assert rc == OK and levels == M.update_plan(log_n, depth, idx)
    counts = M.update_counts(log_n, depth, idx)
    assert (totals["touched_nodes"], totals["sparse_terms"]) == (counts["touched_nodes"], counts["sparse_terms"])
    assert totals["chunks"] == M.update_chunks(log_n, depth, idx) == depth, "one chunk per level under the default cap"
    assert totals["most_terms"] == len(idx) and totals["most_nodes"] == len(T[depth - 1])


def test_named_cases_have_the_shapes_they_claim(lib):
    c = cases()
    assert M.sets(*c["two leaves in one bottom node (2, 3)"]) == [[0], [3], [15], [60, 61]]
    assert M.sets(*c["two bottom nodes under one parent (2, 3)"]) == [[0], [0], [0, 1], [0, 4]]
    assert M.sets(*c["leaves under different children of the root (2, 3)"]) == [[0], [0, 1, 3], [0, 4, 15], [0, 16, 63]]
    assert M.sets(*c["all N leaves at (2, 3)"]) == [[0], [0, 1], [0, 1, 2, 3], list(range(8))]
    assert M.proof_nodes(*c["all N leaves at (2, 3)"]) == 6 and M.proof_nodes(*c["D = 1, all leaves"]) == 0


@pytest.mark.parametrize("name", list(refused()))
def test_refused_inputs(lib, name):
    log_n, depth, idx = refused()[name]
    assert M.sets(log_n, depth, idx) is None
    spare = (ctypes.c_uint64 * 64)()      # nothing is written: every refusal comes before the first output
    spare32 = (ctypes.c_uint32 * 64)()
    count = len(idx)
    nodes = ctypes.c_uint64(77)
    assert lib.hkt_proof_nodes(log_n, depth, u64s(idx) if count else None, count, ctypes.byref(nodes)) == ERR_ARG and nodes.value == 77
    counts = (ctypes.c_uint64 * 3)()
    assert lib.hkt_sets(log_n, depth, u64s(idx) if count else None, count, M.MAX_CLAIMS, spare, spare, spare) == ERR_ARG
    assert lib.hkt_proof_plan(log_n, depth, u64s(idx) if count else None, count, counts, spare, spare32, spare32) == ERR_ARG
    assert lib.hkt_update_plan(log_n, depth, u64s(idx) if count else None, count, 1 << 30, spare, spare, spare, spare, spare32, spare) == ERR_ARG


def test_caps_of_update_and_proof(lib):
    """2^20 leaves per update; 65536 distinct nodes and 2^20 items per proof"""
    log_n, depth = 10, 2
    idx = list(range(1 << 20))
    assert c_sets(lib, log_n, depth, idx, M.MAX_UPDATE)[0] == OK
    assert c_sets(lib, 12, 2, list(range((1 << 20) + 1)), M.MAX_UPDATE)[0] == ERR_ARG
    # one leaf in each of 65535 bottom nodes + the root: 65536 vectors pass, one more is refused
    log_n, depth = 8, 3
    at_cap = [k << 8 for k in range(65535 - 256)]          # 65279 bottom nodes, their 255 parents, the root: 65535 vectors
    T = M.sets(log_n, depth, at_cap)
    assert sum(len(T[l]) for l in range(depth)) == 65279 + 255 + 1
    nodes = ctypes.c_uint64()
    assert lib.hkt_proof_nodes(log_n, depth, u64s(at_cap), len(at_cap), ctypes.byref(nodes)) == OK and nodes.value == 65534
    one_more = at_cap + [65279 << 8]                        # a 65280th bottom node: parent 255 exists already -> 65536 vectors
    assert lib.hkt_proof_nodes(log_n, depth, u64s(one_more), len(one_more), ctypes.byref(nodes)) == OK and nodes.value == 65535
    over = one_more + [65280 << 8]                          # a new parent too: 65538 vectors
    assert M.proof_plan(log_n, depth, over) is None
    assert lib.hkt_proof_nodes(log_n, depth, u64s(over), len(over), ctypes.byref(nodes)) == ERR_ARG


def test_chunk_plans_against_the_model(lib):
    for log_n, depth in ((1, 1), (2, 3), (8, 2), (8, 3), (12, 2)):
        for c in (4, 8):
            for cap in (1, 304, 5 * 304, 1 << 20, MM.WS_CAP_DEFAULT):
                out = (ctypes.c_uint64 * 3)()
                lib.hkt_build_plan(log_n, depth, c, cap, out)
                want = M.build_counts(log_n, depth, c, cap)
                assert list(out) == [want["touched_nodes"], want["chunks"], want["most_partials"]], (log_n, depth, c, cap)
    out = (ctypes.c_uint64 * 3)()
    lib.hkt_build_plan(2, 3, 8, 5 * 304, out)               # 21 nodes, 5 per chunk: 1 + 1 + 4 chunks
    assert list(out) == [21, 6, 5]
    idx = list(range(64))
    for cap in (1, 304 + 4 * 36, 3 * (304 + 4 * 36) + 1, MM.WS_CAP_DEFAULT):
        _, _, totals = c_update_plan(lib, 2, 3, idx, cap)
        assert totals["chunks"] == M.update_chunks(2, 3, idx, cap)
    assert c_update_plan(lib, 2, 3, idx, 1)[2]["chunks"] == 16 + 4 + 1


# ---- h ----------------------------------------------------------------------------------------------------------------------------------
def c_map(lib, c48, transcript=False):
    out = (ctypes.c_uint32 * 8)()
    if transcript:
        lib.hkt_map_transcript(bytes(c48), out)
    else:
        assert lib.hkt_map(bytes(c48), out) == 1, "the transcript does not meet the node's bytes at KZT_MSG_POS"
    mont = sum(int(w) << (32 * k) for k, w in enumerate(out))
    assert mont < Q
    return mont * pow(R_MONT, -1, Q) % Q


def test_h_against_the_oracle_transcript(lib):
    assert lib.hkt_const(5) == 53
    rnd = random.Random(2310)
    inputs = [K.IDENTITY48, K.scalar_commit(1), K.scalar_commit(Q - 1), bytes(48), bytes([0xFF] * 48), bytes(range(48))]
    inputs += [K.scalar_commit(rnd.randrange(1, Q)) for _ in range(24)]
    flags = set()
    for c48 in inputs:
        want = M.h(c48)
        assert c_map(lib, c48) == want == c_map(lib, c48, transcript=True), c48.hex()
        flags.add(c48[0] & 0xE0)
    assert {0x80, 0xA0, 0xC0} <= flags
    assert len({M.h(c) for c in inputs}) == len(inputs)
    # one flipped bit anywhere in the 48 bytes changes the scalar: every byte of the message reaches the state
    base = K.scalar_commit(5)
    for byte in range(48):
        flipped = bytearray(base)
        flipped[byte] ^= 1 << (byte % 8)
        assert c_map(lib, flipped) == M.h(bytes(flipped)) != M.h(base), byte


def test_model_tree_is_consistent():
    """the model against itself: a node's bytes are the commitment of its scalar, an inner value is h of the child's bytes"""
    rnd = random.Random(9)
    leaves = [rnd.randrange(Q) for _ in range(8)]
    t = M.Tree(1, 3, leaves)
    assert [len(c) for c in t.comp] == [1, 2, 4] and [len(v) for v in t.vals] == [2, 4, 8]
    assert t.comp[2][3] == K.scalar_commit(M.node_scalar(leaves[6:8], 1) * pow(K.G_SCALAR, -1, Q) % Q)
    assert t.vals[1][3] == M.h(t.comp[2][3]) and t.vals[0] == [M.h(t.comp[1][0]), M.h(t.comp[1][1])]
    assert M.Tree(1, 1, [0, 0]).root == K.IDENTITY48


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------------------
def test_index_logic_under_address_and_undefined_behaviour_sanitizers():
    """the same cases, accepted and refused, through tests/csrc/san_kzg_tree.cpp built with -fsanitize=address,undefined: a
    stand-alone program on the CPU; any report fails the run (-fno-sanitize-recover, a non-zero exit)"""
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    src = os.path.join(HERE, "csrc", "san_kzg_tree.cpp")
    if _stale(SAN, _deps(src)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", src, "-o", SAN])
    rows = [(name, v, MM.WS_CAP_DEFAULT) for name, v in cases().items()] + [(name, v, 1 << 20) for name, v in refused().items()]
    rows += [("all leaves, a cap of one segment", (2, 3, list(range(64))), 1)]
    lines = ["%d %d %d %d %s" % (log_n, depth, cap, len(idx), " ".join(str(j) for j in idx)) for _, (log_n, depth, idx), cap in rows]
    run = subprocess.run([SAN], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    got = [[int(x) for x in line.split()] for line in run.stdout.splitlines()]
    assert len(got) == len(rows)
    for (name, (log_n, depth, idx), cap), g in zip(rows, got):
        T = M.sets(log_n, depth, idx)
        if T is None:
            assert g[0] == ERR_ARG, name
            continue
        plan, counts = M.proof_plan(log_n, depth, idx), M.update_counts(log_n, depth, idx)
        assert g[:8] == [OK, OK, len(plan["vectors"]), len(plan["items"]), len(plan["path"]), counts["touched_nodes"], counts["sparse_terms"],
                         M.update_chunks(log_n, depth, idx, cap)], name
        order = sorted(range(len(idx)), key=lambda k: idx[k])
        up = M.update_plan(log_n, depth, idx)
        offs = []
        for lv in up:
            o = [0]
            for seg in lv["segments"]:
                o.append(o[-1] + len(seg))
            offs += o
        level_vector = [sum(len(T[k]) for k in range(l)) for l in range(depth + 1)]
        want = (sum(sum(level) for level in T) + 3 * sum(order) + sum(5 * v + 7 * p for v, p in plan["items"]) + 11 * sum(level_vector)
                + 13 * sum(sum(lv["nodes"]) for lv in up) + 17 * sum(offs) + 19 * sum(j for lv in up for seg in lv["segments"] for _, j in seg)
                + 23 * sum(c for lv in up for seg in lv["segments"] for c, _ in seg))
        assert g[8] == want % (1 << 64), name
