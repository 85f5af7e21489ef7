// The gadget composer: the recording entry points (plonk_composer_*, host only — the recorder is composer_host.hpp) and the
// device executor of the witness program, which fills a prover's resident witness table from the inputs of one proof.
//
//   composer_scatter_kernel   one lane per input: table[input_slot[i]] = inputs[i]
//   composer_levels_kernel    launched two ways.  ONE wide level: a lane per record, 64-lane workgroups; the records of a level
//                             are sorted by kind, so all but the boundary waves run a single kind.  A run of narrow levels (each
//                             at most COMPOSER_NARROW records): ONE workgroup walks them, a lane per record, __syncthreads()
//                             between levels — a deep chain of small dependent ops is one launch.  No grid-wide barrier, no
//                             spinning between workgroups.
//   composer_pi_kernel        one lane per public-input row: the value that satisfies the row
// Every lane runs composer_exec (composer_core.hpp), the statement of the gadgets the recorder and the host executor share.
// The scalar multiplications and the torsion check run as whole gadgets on one lane, in projective coordinates, with ONE
// inversion per gadget; their intermediates are parked in the gadget's own output slots (no per-lane arrays, no scratch).
// The only atomic is a vector atomicMin on the error word (lowest record id that met a malformed JubJub scalar).
#include "composer.hpp"
#include "devmem.cuh"

namespace plonk {

namespace {

struct DevExec {   // executor backend of composer_core.hpp over the witness table in HBM
  static constexpr bool EXEC = true;
  Fr* tab;
  uint32_t next;
  __device__ __forceinline__ Fr get(uint32_t i) const { return ld_fr(tab + i); }
  __device__ __forceinline__ void put(uint32_t i, const Fr& v) { st_fr(tab + i, v); }
  __device__ __forceinline__ uint32_t alloc(const Fr& v) { st_fr(tab + next, v); return next++; }
  __device__ __forceinline__ uint32_t mark() const { return next; }
  __device__ __forceinline__ void skip(uint32_t n) { next += n; }
  __device__ __forceinline__ void emit(const ComposerRow&) {}
};
struct DevPool {
  const Fr* pool;
  __device__ __forceinline__ Fr operator()(uint32_t i) const { return ld_fr(pool + i); }
};

__device__ __forceinline__ void run_record(const ComposerOp* ops, uint32_t i, Fr* tab, const Fr* pool, uint32_t* err) {
  const ComposerOp op = ops[i];
  DevExec b{tab, op.out0};
  if (!composer_exec(b, op, DevPool{pool})) atomicMin(err, op.id);
}

// levels [l0, l1): lane (workgroup, thread) takes record level_off[l] + its global index of every level l, with a barrier
// between levels.  A wide level is launched alone (l1 = l0 + 1) over as many 64-lane workgroups as it has records; a run of
// narrow levels is launched as ONE workgroup of COMPOSER_NARROW lanes, which holds every level of the run whole, so the
// workgroup barrier is all the ordering the run needs.
__global__ void __launch_bounds__(COMPOSER_NARROW) composer_levels_kernel(const ComposerOp* ops, const uint32_t* level_off, uint32_t l0,
                                                                         uint32_t l1, Fr* tab, const Fr* pool, uint32_t* err) {
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t l = l0; l < l1; ++l) {
    const uint32_t i = level_off[l] + lane;
    if (i < level_off[l + 1]) run_record(ops, i, tab, pool, err);
    __syncthreads();   // the next level reads what this one wrote (workgroup scope: one workgroup walks a run)
  }
}

__global__ void __launch_bounds__(256) composer_scatter_kernel(const Fr* inputs, const uint32_t* slots, uint64_t n, Fr* tab) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) st_fr(tab + slots[i], ld_fr(inputs + i));
}

__global__ void __launch_bounds__(256) composer_pi_kernel(const ComposerPiRow* rows, uint64_t n, const Fr* tab, const Fr* pool, Fr* out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const DevExec b{const_cast<Fr*>(tab), 0};
  st_fr(out + i, composer_pi_value(b, rows[i], DevPool{pool}));
}

template <class T> int upload(Ctx* c, T** dst, const T* src, size_t count) {
  HIP_TRY(hipMalloc((void**)dst, sizeof(T) * (count ? count : 1)));
  if (count) HIP_TRY(hipMemcpyAsync(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice, c->stream));
  return PLONK_OK;
}

}  // namespace

void composer_program_abandon(ComposerProgram* pg) { delete pg; }

void composer_program_free(ComposerProgram* pg) {
  if (!pg) return;
  for (void* b : {(void*)pg->ops, (void*)pg->level_off, (void*)pg->pool, (void*)pg->input_slots, (void*)pg->pi, (void*)pg->inputs,
                  (void*)pg->pi_vals})
    if (b) (void)hipFree(b);
  if (pg->back_host) (void)hipHostFree(pg->back_host);
  if (pg->inputs_pinned) (void)hipHostFree(pg->inputs_pinned);
  delete pg;
}

int composer_program_upload(Ctx* c, const Composer& comp, ComposerProgram** out) {
  const ComposerSchedule& s = comp.schedule();
  ComposerProgram* pg = new ComposerProgram();
  struct Guard { ComposerProgram* p; ~Guard() { if (p) composer_program_free(p); } } g{pg};
  pg->nops = s.ops.size();
  pg->ninputs = comp.inputs.size();
  pg->npi = comp.pi_rows.size();
  pg->witnesses = comp.witnesses();
  pg->levels = s.level_off.size() - 1;
  int rc;
  if ((rc = upload(c, &pg->ops, s.ops.data(), s.ops.size()))) return rc;
  if ((rc = upload(c, &pg->level_off, s.level_off.data(), s.level_off.size()))) return rc;
  if ((rc = upload(c, &pg->pool, comp.pool.data(), comp.pool.size()))) return rc;
  if ((rc = upload(c, &pg->input_slots, comp.inputs.data(), comp.inputs.size()))) return rc;
  if ((rc = upload(c, &pg->pi, comp.pi_rows.data(), comp.pi_rows.size()))) return rc;
  HIP_TRY(hipMalloc((void**)&pg->inputs, sizeof(Fr) * (pg->ninputs ? pg->ninputs : 1)));
  HIP_TRY(hipMalloc((void**)&pg->pi_vals, sizeof(Fr) * (pg->npi + 1)));
  pg->err = reinterpret_cast<uint32_t*>(pg->pi_vals + pg->npi);
  HIP_TRY(hipHostMalloc((void**)&pg->back_host, sizeof(Fr) * (pg->npi + 1)));
  HIP_TRY(hipHostMalloc((void**)&pg->inputs_pinned, sizeof(Fr) * (pg->ninputs ? pg->ninputs : 1)));
  HIP_TRY(hipStreamSynchronize(c->stream));   // the uploads read the composer's vectors
  pg->level_begin = s.level_off;
  for (const ComposerPiRow& r : comp.pi_rows) pg->pi_rows.push_back(r.row);
  // the launch list: a wide level is a launch of its own, a run of narrow levels is one walk
  for (uint32_t l = 0; l < pg->levels;) {
    const auto width = [&](uint32_t k) { return s.level_off[k + 1] - s.level_off[k]; };
    if (width(l) > COMPOSER_NARROW) {
      pg->launches.push_back(ComposerLaunch{l, l + 1, false});
      ++l;
      continue;
    }
    uint32_t e = l + 1;
    while (e < pg->levels && width(e) <= COMPOSER_NARROW) ++e;
    pg->launches.push_back(ComposerLaunch{l, e, true});
    l = e;
  }
  g.p = nullptr;
  *out = pg;
  return PLONK_OK;
}

int composer_fill_queue(Ctx* c, ComposerProgram* pg, const Fr* inputs_host, Fr* table_dev) {
  if (pg->ninputs) {
    // through the program's pinned block: the caller's memory may be pageable, and a pageable source makes the "async" copy a
    // staged, synchronising one.  The block is free: every fill ends with a synchronisation before it returns.
    memcpy(pg->inputs_pinned, inputs_host, sizeof(Fr) * pg->ninputs);
    HIP_TRY(hipMemcpyAsync(pg->inputs, pg->inputs_pinned, sizeof(Fr) * pg->ninputs, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(composer_scatter_kernel, dim3((unsigned)((pg->ninputs + 255) / 256)), dim3(256), 0, c->stream, pg->inputs,
                       pg->input_slots, pg->ninputs, table_dev);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemsetAsync(pg->err, 0xFF, sizeof(uint32_t), c->stream));
  for (const ComposerLaunch& L : pg->launches) {
    const uint32_t width = pg->level_begin[L.l0 + 1] - pg->level_begin[L.l0];
    const dim3 grid(L.walk ? 1u : (width + COMPOSER_WIDE_T - 1) / COMPOSER_WIDE_T), block(L.walk ? COMPOSER_NARROW : COMPOSER_WIDE_T);
    hipLaunchKernelGGL(composer_levels_kernel, grid, block, 0, c->stream, pg->ops, pg->level_off, L.l0, L.l1, table_dev, pg->pool, pg->err);
    HIP_TRY(hipGetLastError());
  }
  if (pg->npi) {
    hipLaunchKernelGGL(composer_pi_kernel, dim3((unsigned)((pg->npi + 255) / 256)), dim3(256), 0, c->stream, pg->pi, pg->npi, table_dev,
                       pg->pool, pg->pi_vals);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(pg->back_host, pg->pi_vals, sizeof(Fr) * pg->npi + sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  return PLONK_OK;
}

int composer_fill_result(ComposerProgram* pg, const Fr** pi_vals_host) {
  uint32_t err;
  memcpy(&err, pg->back_host + sizeof(Fr) * pg->npi, sizeof err);
  if (err != COMPOSER_NO_ERROR) {
    static thread_local char text[160];
    // component_mul_generator is the only gadget that reports (composer_core.hpp: cg_mul_generator)
    snprintf(text, sizeof text, "component_mul_generator (record %u): the scalar is not below the order of the JubJub subgroup (Error::JubJubScalarMalformed)", err);
    set_last_error("witness program", text, __FILE__, __LINE__);
    return PLONK_ERR_DATA;
  }
  if (pi_vals_host) *pi_vals_host = reinterpret_cast<const Fr*>(pg->back_host);
  return PLONK_OK;
}

}  // namespace plonk

using namespace plonk;

extern "C" {

int plonk_composer_create(plonk_composer** out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!out) return (plonk::set_last_error("invalid argument", api_fn, __FILE__, __LINE__), PLONK_ERR_ARG);
  *out = new plonk_composer();
  return PLONK_OK;
  });
}

void plonk_composer_destroy(plonk_composer* c) { delete c; }

int plonk_composer_witness(plonk_composer* c, uint32_t* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!c || !out) return (plonk::set_last_error("invalid argument", api_fn, __FILE__, __LINE__), PLONK_ERR_ARG);
  std::lock_guard<std::mutex> lk(c->mu);
  *out = c->c.input();
  return PLONK_OK;
  });
}

int plonk_composer_gate(plonk_composer* c, const uint64_t* selectors, const uint32_t wires[4], uint32_t flags, uint32_t* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!c || !selectors || !wires || ((flags & 2u) && !out)) return (plonk::set_last_error("invalid argument", api_fn, __FILE__, __LINE__), PLONK_ERR_ARG);
  std::lock_guard<std::mutex> lk(c->mu);
  const char* why = "";
  const int rc = composer_api_gate(c->c, selectors, wires, flags, out, &why);
  if (rc) plonk::set_last_error(api_fn, why, __FILE__, __LINE__);
  return rc;
  });
}

int plonk_composer_gadget(plonk_composer* c, int kind, uint32_t width, const uint32_t* in, uint32_t nin, const uint64_t* consts,
                          uint32_t nconsts, uint32_t* out, uint32_t out_cap, uint32_t* nout) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!c) return (plonk::set_last_error("invalid argument", api_fn, __FILE__, __LINE__), PLONK_ERR_ARG);
  std::lock_guard<std::mutex> lk(c->mu);
  const char* why = "";
  const int rc = composer_api_gadget(c->c, kind, width, in, nin, consts, nconsts, out, out_cap, nout, &why);
  if (rc) plonk::set_last_error(api_fn, why, __FILE__, __LINE__);
  return rc;
  });
}

int plonk_composer_info(plonk_composer* c, plonk_composer_summary* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!c || !out) return (plonk::set_last_error("invalid argument", api_fn, __FILE__, __LINE__), PLONK_ERR_ARG);
  std::lock_guard<std::mutex> lk(c->mu);
  composer_api_info(c->c, out);
  return PLONK_OK;
  });
}

int plonk_composer_layout(plonk_composer* c, uint64_t* const selectors[11], uint32_t* const wires[4], uint32_t* input_slots,
                          uint64_t* pi_rows) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!c) return (plonk::set_last_error("invalid argument", api_fn, __FILE__, __LINE__), PLONK_ERR_ARG);
  std::lock_guard<std::mutex> lk(c->mu);
  composer_api_layout(c->c, selectors, wires, input_slots, pi_rows);
  return PLONK_OK;
  });
}

}  // extern "C"
