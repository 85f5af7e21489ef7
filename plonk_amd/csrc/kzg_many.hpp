// Launchers of kzg_many.hip: the window tables over a handle's Lagrange points and the many-vector commitments over them.
// Shared with the door of the per-kernel tests (tests/csrc/dev_kzg_many.hip).  Every pointer is device memory unless said
// otherwise, everything is queued on the context's stream, nothing synchronises (kzm_tables_fill does: it frees its scratch).
#pragma once
#include "plonk_internal.hpp"
#include "curve28.cuh"
#include "kzg_many_core.hpp"

namespace plonk {

struct G1RSlot;   // devmem.cuh

struct KzmTables {
  const G1AffineR* entries;   // kzm_table_entries(log_n, window_bits) of them, indexed by kzm_entry
  uint32_t log_n, window_bits, windows;
};

// table[kzm_entry(c, W, i, w, d)] = [d 2^(c w)] lag[i] as affine x || y < 2p (128 zero bytes where lag[i] is the identity:
// 96 zero bytes).  Returns with the stream synchronised.
int kzm_tables_fill(Ctx* c, const G1Affine* lag, uint32_t log_n, uint32_t window_bits, G1AffineR* table);
// *bad |= 1 when one of the `total` values is >= q
int kzm_scan(Ctx* c, const Fr* values, uint64_t total, unsigned long long* bad);
// partial[j * slices + s] = sum over the values [s n / slices, (s + 1) n / slices) of vector j (values + j n), j < count
int kzm_accumulate(Ctx* c, const KzmTables& t, const Fr* values, uint64_t count, uint32_t slices, G1RSlot* partial);
// the sparse form: partial[j] = sum_(k in [offsets[j], offsets[j+1])) deltas[k] L_(index[k]), j < count (offsets: count + 1)
int kzm_accumulate_sparse(Ctx* c, const KzmTables& t, const uint64_t* offsets, const uint32_t* index, const Fr* deltas, uint64_t count,
                          G1RSlot* partial);
// out48[48 j] = the compressed sum of partial[j * slices .. + slices) and, with base != NULL, of base[j] (kind[j]: VDEC_OK or
// VDEC_IDENTITY, decode_points); out48 is 4-byte aligned
int kzm_compress(Ctx* c, const G1RSlot* partial, uint32_t slices, const G1Affine* base, const int32_t* kind, uint64_t count, uint8_t* out48);

struct KzgDomain;
// the window tables the handle holds (false: it holds none) — kzg_tree.hip runs the launchers above over them; the caller holds
// the context's mutex
bool kzm_handle_tables(const KzgDomain* d, KzmTables* out);
// TEST HOOK (tests/csrc/dev_kzg_many.hip): the slices of the dense calls on the handle from now on (0: the plan's own rule)
void kzm_test_force_slices(KzgDomain* d, uint32_t slices);

}  // namespace plonk
