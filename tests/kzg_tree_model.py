"""Big-int model of the KZG10 vector-commitment trees (plonk_amd/csrc/kzg_tree_core.hpp, kzg_tree.hip): a node as the scalar
sum v_i L_i(tau) g (the tests know tau) and its 48 bytes, the map h through oracle/merlin.py, the whole tree, the level sets
T_l of a set of leaves, the canonical order of a proof and the plan of an update.  Nothing here is derived from the code under
test: the sets are built with Python sets and sorted(), the segments by grouping on j // n."""
from oracle import bls12_381 as E
from oracle import merlin
from tests import kzg_evals_model as EM
from tests import kzg_many_model as MM
from tests import kzg_ref as K

Q = E.Q
LOG_N_MAX = 12
MAX_BITS = 26
MAX_UPDATE = 1 << 20
MAX_PROOF_NODES = 65536
MAX_CLAIMS = 1 << 20
ERR_ARG = -1
NONE, BUILD, UPDATE, PROVE = 0, 1, 2, 3
ID48 = K.IDENTITY48


def shape_ok(log_n: int, depth: int) -> bool:
    return 1 <= log_n <= LOG_N_MAX and depth >= 1 and depth * log_n <= MAX_BITS


def h(c48: bytes) -> int:
    """the scalar a parent commits to for the child with these 48 bytes"""
    t = merlin.Transcript(b"kzg10-tree-v1")
    t.append_message(b"node", bytes(c48))
    return t.challenge_scalar(b"node-scalar")


def node_scalar(values, log_n: int, tau=K.TAU) -> int:
    """the discrete log (to the base G) of the node's commitment: sum v_i L_i(tau) g"""
    L = EM.lagrange_at(tau, log_n)
    return sum(a * b for a, b in zip(values, L)) % Q * K.G_SCALAR % Q


def node_bytes(values, log_n: int, tau=K.TAU) -> bytes:
    return MM.commitment(values, log_n, tau)


class Tree:
    """vals[l]: the n^(l+1) values of level l; comp[l]: the n^l commitments"""

    def __init__(self, log_n: int, depth: int, leaves, tau=K.TAU):
        assert shape_ok(log_n, depth) and len(leaves) == 1 << (log_n * depth)
        self.log_n, self.depth, self.n, self.tau = log_n, depth, 1 << log_n, tau
        self.vals = [None] * depth
        self.comp = [None] * depth
        self.vals[depth - 1] = [x % Q for x in leaves]
        for l in range(depth - 1, -1, -1):
            n = self.n
            self.comp[l] = [node_bytes(self.vals[l][k * n:(k + 1) * n], log_n, tau) for k in range(n ** l)]
            if l:
                self.vals[l - 1] = [h(c) for c in self.comp[l]]

    def update(self, leaf_index, values):
        """the touched nodes computed again from their values, bottom up (no deltas: not the way the device goes)"""
        n, touched = self.n, set()
        for j, v in zip(leaf_index, values):
            self.vals[self.depth - 1][j] = v % Q
            touched.add(j >> self.log_n)
        for l in range(self.depth - 1, -1, -1):
            for k in sorted(touched):
                self.comp[l][k] = node_bytes(self.vals[l][k * n:(k + 1) * n], self.log_n, self.tau)
                if l:
                    self.vals[l - 1][k] = h(self.comp[l][k])
            touched = {k >> self.log_n for k in touched}

    @property
    def root(self) -> bytes:
        return self.comp[0][0]

    def all_nodes(self):
        return [list(level) for level in self.comp]


def sets(log_n: int, depth: int, leaf_index):
    """T[l], l = 0 .. depth, or None where the library refuses: no index, an index out of range, a repeated index"""
    idx = list(leaf_index)
    if not shape_ok(log_n, depth) or not idx or len(set(idx)) != len(idx) or any(not 0 <= j < 1 << (log_n * depth) for j in idx):
        return None
    T = [None] * (depth + 1)
    T[depth] = sorted(idx)
    for l in range(depth - 1, -1, -1):
        T[l] = sorted({j >> log_n for j in T[l + 1]})
    return T


def proof_plan(log_n: int, depth: int, leaf_index):
    """{"vectors": [(level, node)], "items": [(vector, point)], "path": [(level, node)]} in the canonical order, or None"""
    T = sets(log_n, depth, leaf_index)
    if T is None:
        return None
    vectors = [(l, k) for l in range(depth) for k in T[l]]
    where = {v: i for i, v in enumerate(vectors)}
    items = [(where[(l, j >> log_n)], j & ((1 << log_n) - 1)) for l in range(depth) for j in T[l + 1]]
    if len(vectors) > MAX_PROOF_NODES or len(items) > MAX_CLAIMS:
        return None
    return {"vectors": vectors, "items": items, "path": vectors[1:]}


def proof_nodes(log_n: int, depth: int, leaf_index):
    p = proof_plan(log_n, depth, leaf_index)
    return None if p is None else len(p["path"])


def update_plan(log_n: int, depth: int, leaf_index):
    """per level l = depth-1 .. 0: {"level", "nodes": T_l, "segments": [[(child index, flat index of vals[l])]] per node}"""
    T = sets(log_n, depth, leaf_index)
    if T is None or len(T[depth]) > MAX_UPDATE:
        return None
    out = []
    for l in range(depth - 1, -1, -1):
        by_node = {}
        for j in T[l + 1]:
            by_node.setdefault(j >> log_n, []).append((j & ((1 << log_n) - 1), j))
        assert sorted(by_node) == T[l]
        out.append({"level": l, "nodes": T[l], "segments": [by_node[k] for k in T[l]]})
    return out


def update_counts(log_n: int, depth: int, leaf_index):
    T = sets(log_n, depth, leaf_index)
    return {"touched_nodes": sum(len(T[l]) for l in range(depth)), "sparse_terms": sum(len(T[l]) for l in range(1, depth + 1))}


def update_chunks(log_n: int, depth: int, leaf_index, ws_cap: int = MM.WS_CAP_DEFAULT) -> int:
    chunks = 0
    for lv in update_plan(log_n, depth, leaf_index):
        offs = [0]
        for seg in lv["segments"]:
            offs.append(offs[-1] + len(seg))
        chunks += MM.sparse_plan(log_n, 8, offs, ws_cap)["chunks"]
    return chunks


def build_counts(log_n: int, depth: int, c: int, ws_cap: int = MM.WS_CAP_DEFAULT):
    plans = [MM.plan(log_n, c, 1 << (log_n * l), ws_cap, False) for l in range(depth)]
    return {"touched_nodes": sum(p["count"] for p in plans), "chunks": sum(p["chunks"] for p in plans),
            "most_partials": max(p["chunk_vectors"] * p["slices"] for p in plans)}


def data_bytes(log_n: int, depth: int) -> int:
    return sum(32 * (1 << (log_n * (l + 1))) + (48 + 96 + 4) * (1 << (log_n * l)) for l in range(depth))
