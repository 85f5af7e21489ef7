"""The schedule of one proof as a function of (size, prover state, configuration): which of the launch orders of
plonk_amd/csrc/prover.hip a proof runs.  Written from the rules, field by field; plonk_amd/csrc/prove_schedule_core.hpp is
compared against this over the whole grid (tests/test_prove_schedule_host.py).

Inputs: logn; lag_on (the wire commitments read the Lagrange-basis key), lag_z (the key has z's third blinding point);
wires_pending (the wire columns are still arriving from the host); world, sharded; n = 2^logn; rank_pts (coefficients a rank
of a sharded prover owns); the six switches as the configuration holds them: wire_by_column (-1 never, 0 by size, 1 / 2 at
every size in 3 / 4 launches), wire_polys_side (-1 by size, 0, 1), side_defer (-1 by size, 0, 1, 2 = round 1 only),
z_commit_coeff (-1 evaluations at every size, 0 by size, 1 coefficients), shard_side (-1 off), shard_z (-1 off, 0 by size, 1 on).
"""
FIELDS = ("by_column", "wire_parts", "polys_on_side", "side_defer_r1", "side_defer_r2", "z_from_evals", "shard_z")


def prove_schedule(logn, lag_on, lag_z, wires_pending, world, sharded, n, rank_pts,
                   wire_by_column, wire_polys_side, side_defer, z_commit_coeff, shard_side, shard_z):
    L = logn
    if not sharded:
        by_column = bool(lag_on and wires_pending and world == 1 and wire_by_column >= 0 and (L > 18 or wire_by_column > 0))
        wire_parts = (4 if wire_by_column == 2 else 3) if by_column else 1
        polys_on_side = bool(lag_on and not by_column and (wire_polys_side == 1 if wire_polys_side >= 0 else L <= 19))
        defer_size = L <= 18 or (L == 19 and not by_column)
        return {
            "by_column": by_column,
            "wire_parts": wire_parts,
            "polys_on_side": polys_on_side,
            "side_defer_r1": side_defer >= 1 if side_defer >= 0 else defer_size,
            "side_defer_r2": side_defer == 1 if side_defer >= 0 else defer_size,
            "z_from_evals": bool(lag_on and lag_z and (L <= 17 or z_commit_coeff < 0)),
            "shard_z": False,
        }
    on = shard_side >= 0
    small = rank_pts <= (1 << 18) + 64
    wanted = True if shard_z > 0 else False if shard_z < 0 else (L >= 19 and world >= 4)
    return {
        "by_column": False,
        "wire_parts": 0,                     # the sharded path does not report a wire schedule
        "polys_on_side": bool(lag_on and on and small),
        "side_defer_r1": on and small,
        "side_defer_r2": on and small,
        "z_from_evals": False,
        "shard_z": wanted and n % world == 0 and n // world >= 2,
    }
