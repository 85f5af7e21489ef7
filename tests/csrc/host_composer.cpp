// CPU test harness of the gadget composer: the recorder and the one-thread host executor of composer_host.hpp /
// composer_core.hpp compiled with g++ and driven from tests/test_composer_host.py through ctypes.  The recording calls are
// the ones the C ABI wraps (composer_api_*), with the ABI's signatures; hc_program exposes the scheduled records, hc_fill the host executor.
#include <cstdint>
#include <cstring>

#include "../../plonk_amd/csrc/composer_host.hpp"

using namespace plonk;

extern "C" {

void* hc_create() { return new Composer(); }
void hc_destroy(void* c) { delete static_cast<Composer*>(c); }
int hc_witness(void* c, uint32_t* out) { *out = static_cast<Composer*>(c)->input(); return PLONK_OK; }
int hc_gate(void* c, const uint64_t* selectors, const uint32_t* wires, uint32_t flags, uint32_t* out) {
  const char* why = "";
  return composer_api_gate(*static_cast<Composer*>(c), selectors, wires, flags, out, &why);
}
int hc_gadget(void* c, int kind, uint32_t width, const uint32_t* in, uint32_t nin, const uint64_t* consts, uint32_t nconsts,
              uint32_t* out, uint32_t out_cap, uint32_t* nout) {
  const char* why = "";
  return composer_api_gadget(*static_cast<Composer*>(c), kind, width, in, nin, consts, nconsts, out, out_cap, nout, &why);
}
int hc_info(void* c, plonk_composer_summary* out) { composer_api_info(*static_cast<Composer*>(c), out); return PLONK_OK; }
int hc_layout(void* c, uint64_t* const* selectors, uint32_t* const* wires, uint32_t* input_slots, uint64_t* pi_rows) {
  composer_api_layout(*static_cast<Composer*>(c), selectors, wires, input_slots, pi_rows);
  return PLONK_OK;
}
// records: 11 words each (kind width in0..3 out0 nout cst level id) in scheduled order; level_off: levels + 1 entries
void hc_program(void* c, uint32_t* records, uint32_t* level_off) {
  const ComposerSchedule& s = static_cast<Composer*>(c)->schedule();
  static_assert(sizeof(ComposerOp) == 44, "record layout");
  if (!s.ops.empty()) memcpy(records, s.ops.data(), s.ops.size() * sizeof(ComposerOp));
  memcpy(level_off, s.level_off.data(), s.level_off.size() * sizeof(uint32_t));
}
// *misses: table accesses out of range or writes outside the running record's outputs (must be 0)
uint32_t hc_fill(void* c, const uint64_t* inputs, uint64_t* table, uint64_t* pi_out, uint64_t* misses) {
  return composer_fill_host(*static_cast<Composer*>(c), reinterpret_cast<const Fr*>(inputs), reinterpret_cast<Fr*>(table),
                            reinterpret_cast<Fr*>(pi_out), misses);
}

}  // extern "C"
