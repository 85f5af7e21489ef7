// The plonk_kzg_domain handle (kzg_domain.hip creates and destroys it) and the way in of every call on it: shared by the
// files whose calls hang off the handle (kzg_domain.hip, kzg_evals.hip, kzg_cells.hip, kzg_recover.hip, kzg_multiproof.hip,
// kzg_many.hip).
// DESIGN.md section 21 has the layout.
#pragma once
#include <mutex>

#include "kzg_domain.hpp"

namespace plonk { struct KzgDomain; }
struct plonk_kzg_domain {
  plonk::KzgDomain* d;
  plonk_ctx* ctx;
};

namespace plonk {

struct G1RSlot;      // devmem.cuh

// The state of a feature: defined in the feature's own file, made by its first call (kzd_state), freed by its release.
struct KzgEvals;     // kzg_evals.hip: the Lagrange points, the opt-in tables and the workspace of the evaluation-form calls
struct KzgCells;     // kzg_cells.hip: the A^(u) tables and the workspace of the cell proofs
struct KzgRecover;   // kzg_recover.hip: the workspace of the cell recovery
struct KzgMulti;     // kzg_multiproof.hip: the invd table and the workspace of plonk_kzg_multiproof_open
struct KzgMany;      // kzg_many.hip: the opt-in window tables and the workspace of the many-vector commitments
void kze_release(KzgEvals* evals);
void kzc_release(KzgCells* cells);
void kzr_release(KzgRecover* recover);
void kmp_release(KzgMulti* multi);
void kzm_release(KzgMany* many);

struct KzdBufs {
  enum { WS, F, G, EVALS, TMP, OUT48, DESC, META, NBUF };   // grow-only buffers of the open calls
};
struct KzgDomain : KzdBufs, DevBufs<KzdBufs::NBUF> {
  Ctx* c = nullptr;
  uint32_t log_n = 0;
  uint64_t srs_gen = 0;          // of the commit key the handle was built on
  G1RSlot* A = nullptr;          // DFT_N(a), bit-reversed: N slots
  GlvScalar* tw = nullptr;       // w_N^e, e < n
  uint64_t fixed_bytes = 0;      // A + tw
  uint64_t ws_cap = KZD_WS_CAP_DEFAULT;   // the cap on the point workspace of a call
  plonk_kzg_domain_info last = {};
  KzgEvals* evals = nullptr;     // the feature states: not in device_bytes()
  KzgCells* cells = nullptr;
  KzgRecover* recover = nullptr;
  KzgMulti* multi = nullptr;
  KzgMany* many = nullptr;
  ~KzgDomain() {   // in this order: the many-vector state (it reads the Lagrange points of the evaluation-form state), the multiproof state, the recovery state, the cell state, the evaluation-form state, the fixed buffers; the base frees the grow-only ones last
    kzm_release(many);
    kmp_release(multi);
    kzr_release(recover);
    kzc_release(cells);
    kze_release(evals);
    (void)hipFree(A);
    (void)hipFree(tw);
  }
  uint64_t device_bytes() const { return fixed_bytes + bytes(); }
};

// the state in `slot`, made on first use; S is complete only in the file that defines it, so a slot of another feature does
// not compile
template <class S>
S* kzd_state(S*& slot) {
  if (!slot) slot = new S();
  return slot;
}

// The way in of a call on a handle: the context's mutex and the refusal of a poisoned context (CTX_ENTER), then the checks
// the call names, in this order.  The key comparison is made under the mutex: plonk_srs_load on another thread replaces the
// key under it.
enum : uint32_t {
  KZD_SET_DEVICE = 1,   // hipSetDevice: the call queues work or frees device memory
  KZD_KEY = 2,          // PLONK_ERR_STATE when the context's commit key is no longer the one the handle was built on
  KZD_WHOLE_KEY = 4,    // PLONK_ERR_STATE on a context with a communicator: it holds only a range of the key
  KZD_WORK = KZD_SET_DEVICE | KZD_KEY | KZD_WHOLE_KEY,
};
int kzd_enter_checks(const char* api_fn, const KzgDomain* d, uint32_t checks);   // kzg_domain.hip; the caller holds the mutex
#define KZD_ENTER(D, FN, CHECKS) \
  CTX_ENTER(*(D)->c, FN);        \
  PTRY(plonk::kzd_enter_checks(FN, D, CHECKS))

// DESC / META of the state `s` reserved (resident form) and kzd_lengths over them
template <class S>
int kzd_lengths_on(const char* api_fn, Ctx* c, S* s, uint32_t log_n, const void* const* polys, const uint64_t* lens, uint64_t count,
                   bool resident, uint64_t* trimmed) {
  if (resident) {
    PTRY(s->need(S::DESC, sizeof(KzdDesc) * count));
    PTRY(s->need(S::META, 16 * count));
  }
  return kzd_lengths(api_fn, c, log_n, polys, lens, count, resident, s->template at<KzdDesc>(S::DESC),
                     s->template at<unsigned long long>(S::META), trimmed);
}

}  // namespace plonk
