// What composer.hip offers prover.hip: the handle behind plonk_composer, and a prover's device-resident witness program.
#pragma once
#include "plonk_internal.hpp"
#include "composer_host.hpp"

struct plonk_composer {
  plonk::Composer c;
  std::mutex mu;
};

namespace plonk {

// one launch of a fill: either ONE level wider than COMPOSER_NARROW (a lane per record, 64-lane workgroups), or a run of
// consecutive levels none of which is — walked by a single workgroup with a barrier between levels
struct ComposerLaunch {
  uint32_t l0, l1;      // levels [l0, l1)
  bool walk;
};
// A level is "narrow" when one workgroup of the walker holds all its records at once.  Below that width a launch per level
// would leave almost every CU idle anyway and pay a launch (~5 us) per level: a 3000-gate dependent chain is ONE launch here.
static constexpr uint32_t COMPOSER_NARROW = 256;
static constexpr uint32_t COMPOSER_WIDE_T = 64;   // lanes per workgroup of a wide level: a wave runs one kind (the lanes are sorted by kind)

struct ComposerProgram {
  ComposerOp* ops = nullptr;            // scheduled order
  uint32_t* level_off = nullptr;
  Fr* pool = nullptr;
  uint32_t* input_slots = nullptr;
  ComposerPiRow* pi = nullptr;
  Fr* inputs = nullptr;                 // [ninputs] the inputs of one fill
  Fr* pi_vals = nullptr;                // [npi] + the error word behind them
  uint32_t* err = nullptr;
  uint8_t* back_host = nullptr;         // pinned: npi values + the error word (valid until the next fill of this program)
  Fr* inputs_pinned = nullptr;          // pinned: the inputs on their way up
  uint64_t nops = 0, ninputs = 0, npi = 0, witnesses = 0, levels = 0;
  std::vector<ComposerLaunch> launches;
  std::vector<uint32_t> level_begin;    // host copy of level_off
  std::vector<uint64_t> pi_rows;
};

int composer_program_upload(Ctx* c, const Composer& comp, ComposerProgram** out);
void composer_program_free(ComposerProgram* pg);
void composer_program_abandon(ComposerProgram* pg);   // host object only: a poisoned context whose streams are busy (hipFree would hang)
// queues one fill on c->stream: the inputs' upload, the scatter, the level launches, the public-input values, the copy
// back of those and of the error word.  No allocation, no synchronisation.
int composer_fill_queue(Ctx* c, ComposerProgram* pg, const Fr* inputs_host, Fr* table_dev);
// after the stream was synchronised: PLONK_ERR_DATA (with its text) when a record reported a malformed JubJub scalar
int composer_fill_result(ComposerProgram* pg, const Fr** pi_vals_host);

}  // namespace plonk
