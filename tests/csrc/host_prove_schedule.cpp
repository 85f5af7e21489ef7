// CPU harness for plonk_amd/csrc/prove_schedule_core.hpp (the schedule of one proof: which launch order prover.hip runs for
// a size, a prover state and a configuration), compiled with g++ by tests/test_prove_schedule_host.py and checked against
// the model tests/prove_schedule_model.py.
#include "../../plonk_amd/csrc/prove_schedule_core.hpp"

using namespace plonk;

extern "C" {

// in: `count` rows of 14 values in the order of ProveScheduleIn; out: `count` rows of 7 values in the order of ProveSchedule
void hps_schedule(const int64_t* in, uint64_t count, uint32_t* out) {
  for (uint64_t i = 0; i < count; ++i, in += 14, out += 7) {
    ProveScheduleIn s;
    s.logn = (uint32_t)in[0];
    s.lag_on = in[1] != 0;
    s.lag_z = in[2] != 0;
    s.wires_pending = in[3] != 0;
    s.world = (uint32_t)in[4];
    s.sharded = in[5] != 0;
    s.n = (uint64_t)in[6];
    s.rank_pts = (uint64_t)in[7];
    s.wire_by_column = (int)in[8];
    s.wire_polys_side = (int)in[9];
    s.side_defer = (int)in[10];
    s.z_commit_coeff = (int)in[11];
    s.shard_side = (int)in[12];
    s.shard_z = (int)in[13];
    const ProveSchedule r = prove_schedule(s);
    out[0] = r.by_column;
    out[1] = r.wire_parts;
    out[2] = r.polys_on_side;
    out[3] = r.side_defer_r1;
    out[4] = r.side_defer_r2;
    out[5] = r.z_from_evals;
    out[6] = r.shard_z;
  }
}

}  // extern "C"
