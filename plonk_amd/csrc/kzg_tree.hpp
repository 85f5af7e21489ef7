// Launchers of kzg_tree.hip: the three kernels that connect a level of a vector-commitment tree to the next without leaving
// the device.  Shared with the door of the per-kernel tests (tests/csrc/dev_kzg_tree.hip).  Every pointer is device memory
// unless said otherwise, everything is queued on the context's stream, nothing synchronises.
#pragma once
#include "plonk_internal.hpp"
#include "curve28.cuh"
#include "kzg_tree_core.hpp"

namespace plonk {

struct G1RSlot;   // devmem.cuh

// out[j] = h(the 48 bytes at comp48 + 48 (list ? list[j] : j)), j < count; comp48 4-byte aligned
int kzt_map_run(Ctx* c, const KztSeed& seed, const uint8_t* comp48, const uint64_t* list, uint64_t count, Fr* out);
// Node j < count: the sum of partial[j * slices .. + slices) and, with_base, of the point stored for it, written as the affine
// point pts[node] (96 zero bytes for the identity), kind[node] (VDEC_OK or VDEC_IDENTITY) and the 48 bytes at comp48 + 48 node;
// node = list ? list[j] : first + j.  The base may be the identity, the sum may be, the partial may equal the base or be its
// negative.
int kzt_finish_run(Ctx* c, const G1RSlot* partial, uint32_t slices, const uint64_t* list, uint64_t first, uint64_t count, bool with_base,
                   G1Affine* pts, int32_t* kind, uint8_t* comp48);
// deltas[k] = fresh[k] - vals[flat[k]], then vals[flat[k]] = fresh[k], k < count (flat without repeats)
int kzt_delta_run(Ctx* c, const Fr* fresh, const uint64_t* flat, uint64_t count, Fr* vals, Fr* deltas);
// out48[48 j ..] = comp48[48 list[j] ..], j < count
int kzt_gather_run(Ctx* c, const uint8_t* comp48, const uint64_t* list, uint64_t count, uint8_t* out48);

}  // namespace plonk
