/* libplonk_hip.so — C-ABI of the MI355X (gfx950) backend for dusk-plonk's prover hot path.
 *
 * The reference has no FFI seam; the path sits behind two crate-private leaf
 * call families.  Each entry point below names the reference
 * interface it replaces (paths relative to the dusk-network/plonk tree):
 *
 *   plonk_ntt / plonk_ntt_batch   bodies of EvaluationDomain::{fft,ifft,coset_fft,
 *                                 coset_ifft}_in_place, src/fft/domain.rs:173-232
 *                                 (i.e. best_fft :383-422 + n^-1 scale :195 +
 *                                 distribute_powers :198-204)
 *   plonk_srs_load                CommitKey { powers_of_g } upload,
 *                                 src/commitment_scheme/kzg10/key.rs:37-41
 *   plonk_msm / plonk_msm_batch   the msm_variable_base call inside
 *                                 CommitKey::commit, key.rs:376-388, and the 4-way
 *                                 rayon::join fan-out of Prover::commit_polynomials,
 *                                 src/compiler/prover.rs:187-210
 *   plonk_kzg_open / _flatten /   CommitKey::compute_aggregate_witness + commit, AggregateProof::flatten and
 *   _batch_check                  OpeningKey::batch_check, key.rs:394-417, 661-707, proof.rs:69-109
 *
 * Data conventions (bit-identical to the reference's in-memory types):
 *   Fr  = BlsScalar.0 : 4 x uint64 little-endian limbs, Montgomery form, R = 2^256.
 *   G1 base           : 96 bytes = x || y, each 6 x uint64 LE limbs, Montgomery,
 *                       R = 2^384 (first 96 bytes of G1Affine::to_raw_bytes,
 *                       key.rs:215-229).  An SRS never contains the identity.
 *   MSM result        : 97 bytes = x || y (as above) || infinity flag (0/1); the Rust
 *                       shim rebuilds G1Affine / Commitment from it.
 *
 * Ownership: the caller owns every host buffer; nothing is retained after return
 * except the SRS copy made by plonk_srs_load.  The context owns all device memory.
 * Errors: 0 = ok, < 0 = error code below; nothing throws or aborts across the ABI (every
 * entry point catches C++ exceptions: PLONK_ERR_NOMEM for std::bad_alloc, else PLONK_ERR_STATE).
 * The shim maps a non-zero NTT code to a panic (the reference asserts,
 * domain.rs:394,449) and PLONK_ERR_DEGREE to Error::PolynomialDegreeTooLarge
 * (key.rs:362-370).  Threading: every entry point takes a per-context mutex, so
 * rayon workers may call concurrently (prover.rs:174-177,194-197).
 */
#ifndef PLONK_HIP_H
#define PLONK_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plonk_ctx plonk_ctx;

enum {
  PLONK_OK = 0,
  PLONK_ERR_ARG = -1,     /* null pointer, log_n out of range, length mismatch          */
  PLONK_ERR_HIP = -2,     /* a HIP runtime call failed; see plonk_last_error()          */
  PLONK_ERR_DEGREE = -3,  /* more scalars than SRS points (PolynomialDegreeTooLarge)    */
  PLONK_ERR_NO_SRS = -4,  /* plonk_msm before plonk_srs_load                            */
  PLONK_ERR_NO_GPU = -5,  /* no gfx950 device visible                                   */
  PLONK_ERR_UNSAT = -6,   /* prover: quotient degree check failed (CircuitUnsatisfied)  */
  PLONK_ERR_STATE = -7,   /* prover: called out of order / missing key                  */
  PLONK_ERR_BYTES = -8,   /* serialized input too short (Error::NotEnoughBytes)         */
  PLONK_ERR_DATA = -9,    /* serialized input malformed (dusk_bytes::Error::InvalidData) */
  PLONK_ERR_POINT = -10,  /* commit-key point off curve / not in the subgroup (Error::PointMalformed) */
  PLONK_ERR_NOMEM = -11,  /* a host allocation failed inside the library (std::bad_alloc caught at the ABI)  */
  PLONK_ERR_VERIFY = -12  /* a proof does not verify (Error::ProofVerificationError)    */
};

/* `devices`: HIP device ordinals; ndev must be 1 (one process per GPU — multi-GPU runs
 * use one context per rank).  devices == NULL -> device 0. */
int plonk_ctx_create(plonk_ctx** out, const int* devices, int ndev);
/* Frees every device buffer, stream and event the context owns.  Provers built on the context hold a pointer to it:
 * destroy them FIRST (plonk_prover_destroy locks and synchronises the context it was created on). */
void plonk_ctx_destroy(plonk_ctx* ctx);
const char* plonk_last_error(void);

/* ---- configuration ("a small plonk_gpu_config struct passed at context creation") ----------------
 * Everything that changes what a context BUILDS or RUNS is a field here; a zeroed struct with struct_size set means "all
 * defaults", and plonk_ctx_create(out, devices, ndev) == plonk_ctx_create_ex(out, device, NULL).  The environment names of
 * earlier rounds (PLONK_MSM_TABLE, PLONK_MSM_BUCKETS, PLONK_QUOTIENT_DOMAIN, PLONK_WIRE_COMMIT, PLONK_SHARD_QUOTIENT /
 * _Z / _SIDE, PLONK_NTT_ELOG, PLONK_COMM_TIMEOUT_MS, PLONK_TABLE_BUDGET_MB, PLONK_SIDE_CUS and the kernel-tuning names
 * listed in DESIGN.md section 2) remain as OVERRIDES FOR A/B RUNS ONLY: they are read once, when a context is created or
 * reconfigured, on top of the struct — never latched inside the library at first use.
 *
 * table_budget_bytes: HBM that ALL precomputed point tables of this context may take together (its commit key and the
 *   Lagrange-basis keys of the provers built on it).  0 = 80 % of the device's TOTAL memory.  The layout of a key is the
 *   densest that fits: the commit key takes a row per bit position (32 KiB per point) when that is at most 60 % of the
 *   budget, a row per second bit position (16 KiB) when at most 30 %, else the 16 window rows (2 KiB); a prover's
 *   Lagrange-basis key, built last, takes the densest layout that fits in what is left.  The rule reads the budget and what
 *   THIS context already holds — not the memory that happens to be free — so two contexts given the same budget choose the
 *   same layouts whatever their neighbours do (until round 4: "half of what hipMemGetInfo reports free right now").
 *   Keys of at most 2^18 + 64 points always take window rows (measured faster), table_mode forces a layout.
 *   The four layouts, bytes per point and point additions per scalar (uniform scalars, 2^19 buckets where the layout
 *   allows them): PLONK_TABLE_BITPOS 256 rows, 32 KiB, 12.1; PLONK_TABLE_HALFPOS 128 rows, 16 KiB, 12.8;
 *   PLONK_TABLE_QUARTERPOS 64 rows (a row per fourth bit position), 8 KiB, 13.0 (16.0 over the 2^15 buckets of MSMs of at
 *   most 2^18 + 64 terms); PLONK_TABLE_WINDOW 16 rows, 2 KiB, 16.  The automatic rule never takes the 64-row layout: it is
 *   for a caller who forces it (several provers, or a second large one, on one device).
 * plonk_ctx_get_config returns the EFFECTIVE values (defaults and overrides resolved); plonk_ctx_set_config replaces
 *   them for the key loads, provers and MSMs that follow (e.g. a key that is loaded only to derive another one from it:
 *   table_mode = PLONK_TABLE_WINDOW for that load).  Existing tables and provers keep what they were built with. */
enum { PLONK_TABLE_AUTO = 0, PLONK_TABLE_WINDOW = 16, PLONK_TABLE_QUARTERPOS = 64, PLONK_TABLE_HALFPOS = 128, PLONK_TABLE_BITPOS = 256 };
typedef struct plonk_gpu_config {
  uint32_t struct_size;          /* sizeof(plonk_gpu_config) of the caller (shorter = older header: missing fields default) */
  uint32_t reserved;             /* 0 */
  uint64_t table_budget_bytes;   /* 0 = 80 % of the device's total memory */
  int32_t table_mode;            /* PLONK_TABLE_AUTO | _WINDOW | _QUARTERPOS | _HALFPOS | _BITPOS; a forced layout holds at any key size */
  int32_t msm_bucket_bits;       /* 0 = by the number of terms (2^19 buckets above 2^18 terms over bit-position rows), 15, 19 */
  int32_t quotient_domain;       /* 0 = 4: quotient on the 4n coset + de-aliasing; 8: the reference's 8n evaluation */
  int32_t wire_commit;           /* 0 = from the wire VALUES over the Lagrange-basis key; 1 = coefficient form like the reference */
  int32_t shard_quotient;        /* multi-GPU: 0 = default (by residue class for world 2 / 4 / 8), 1 = on, -1 = off (MSMs only) */
  int32_t shard_grand_product;   /* multi-GPU: 0 = default (from 2^19 gates and 4 ranks), 1 = on, -1 = off (replicated) */
  int32_t shard_side_stream;     /* multi-GPU: 0 / 1 = replicated transforms on the side stream under the commitments, -1 = off */
  int32_t ntt_elements_log2;     /* 0 = default (2: four elements per lane; side-stream transforms under a busy MSM: 3), 2, 3 */
  int32_t comm_timeout_ms;       /* 0 = 120000: how long a wait behind a collective polls before the communicator is aborted */
  int32_t side_stream_cus;       /* 0 = none; k > 0: the side stream (challenge-independent transforms under the commitments) is confined
                                    to k compute units by a CU mask and uses the four-wave NTT kernels there; the main stream keeps all.
                                    The masked stream (hipExtStreamCreateWithCUMask) has DEFAULT priority and blocking semantics
                                    against the NULL stream — not the low priority / non-blocking flags of the stream it replaces */
} plonk_gpu_config;
int plonk_ctx_create_ex(plonk_ctx** out, int device, const plonk_gpu_config* config /* NULL = defaults */);
int plonk_ctx_get_config(plonk_ctx* ctx, plonk_gpu_config* out /* struct_size set by the caller */);
int plonk_ctx_set_config(plonk_ctx* ctx, const plonk_gpu_config* config);

/* What an MSM of `count` scalar sets of at most m terms WOULD run as on this context right now — over the commit key
 * (table_rows = 0) or over a key of table_rows rows / table_points points (a prover's Lagrange-basis key); bit_sum_tail = 1:
 * as plonk_msm, plonk_msm_batch and every commitment group of prove() run (the host finishes the bit sums: the only tail the
 * 2^19-bucket kernels have), 0: as plonk_msm_dev (final sum on the device, 2^15 buckets) — and what the LAST one did run as
 * (plonk_ctx_last_msm).  The variant tests assert these, so a switch that is silently
 * ignored fails a test. */
enum { PLONK_PLAN_TAIL_SERIAL = 1, PLONK_PLAN_BUCKET_SUM_LANE = 2, PLONK_PLAN_ACCUMULATE_LDS = 4, PLONK_PLAN_SORT13 = 8 };
typedef struct plonk_msm_plan {
  uint32_t table_rows;           /* 16 window rows / 64 / 128 / 256 bit-position rows of the key */
  uint32_t bucket_bits;          /* 15 or 19 (17: opt-in A/B build) */
  uint32_t digit_width;          /* bits of a signed digit: 16 (windows), or bucket_bits + 2 (NAF over bit positions; + 1 for half and quarter density: 16 / 20) */
  uint32_t slice_entries;        /* entries a lane accumulates serially */
  uint32_t ordered_lanes;        /* 1: msm_accumulate_ordered_kernel (lanes in order of slice length) */
  uint32_t wide_words;           /* 1: 64-bit sort words (rows x points above 2^27) */
  uint32_t flags;                /* PLONK_PLAN_*: which opt-in kernel variants of the A/B switches are in effect */
  uint32_t reserved;
  uint64_t terms;                /* m the plan was made for */
  char accumulate_kernel[64];    /* e.g. "nbl::msm_accumulate_ordered_kernel" */
} plonk_msm_plan;
int plonk_ctx_describe_msm(plonk_ctx* ctx, uint64_t m, int count, int bit_sum_tail, uint32_t table_rows, uint64_t table_points,
                           plonk_msm_plan* out);
int plonk_ctx_last_msm(plonk_ctx* ctx, plonk_msm_plan* out);
/* bytes of precomputed tables the context holds right now (commit key + Lagrange-basis keys) and its budget */
int plonk_ctx_table_bytes(plonk_ctx* ctx, uint64_t* in_use, uint64_t* budget);

/* In-place transform of a[0 .. 1<<log_n) (host memory).
 *   inverse = 0: forward with w;  1: inverse with w^-1 and the n^-1 scale.
 *   coset   = 1: forward pre-scales coefficient i by 7^i for i < in_len;
 *                inverse post-scales output i by 7^-i.
 *   in_len  : number of valid leading coefficients; the rest are treated as zero
 *             (the zero-padding of Vec::resize, domain.rs:174).  Use 1<<log_n for
 *             inverse transforms. */
int plonk_ntt(plonk_ctx* ctx, uint64_t* a, uint32_t log_n, int inverse, int coset, uint64_t in_len);
int plonk_ntt_batch(plonk_ctx* ctx, uint64_t* const* a, int count, uint32_t log_n, int inverse,
                    int coset, const uint64_t* in_len);

/* Load the commit key (npoints x 96 B, npoints <= 2^23) and build the per-window tables 2^(16 w) * P_i in HBM
 * (16 x 128 B per point).  The key is STREAMED from host memory in 2^18-point chunks through two device
 * staging buffers, the upload of chunk k + 1 overlapping the table build of chunk k; pass memory from
 * plonk_host_alloc (pinned) for asynchronous uploads.  A multi-GPU rank passes only its point range. */
int plonk_srs_load(plonk_ctx* ctx, const uint8_t* xy96, uint64_t npoints);
int plonk_host_alloc(uint64_t bytes, void** out);   /* pinned host memory (hipHostMalloc) */
int plonk_host_free(void* p);

/* sum_i scalars[i] * P_i for i < m.  m == 0 -> identity. */
int plonk_msm(plonk_ctx* ctx, const uint64_t* scalars, uint64_t m, uint8_t out_xy_inf[97]);
int plonk_msm_batch(plonk_ctx* ctx, const uint64_t* const* scalars, const uint64_t* m, int count,
                    uint8_t* out /* count x 97 */);

/* ---- device-resident variants (buffers stay in HBM between calls) -------------
 * Pointers are device pointers on the context's GPU (e.g. torch.Tensor.data_ptr()).
 * dst may equal src.  tmp must hold 1<<log_n elements when log_n > 10. */
int plonk_ntt_dev(plonk_ctx* ctx, const void* src, void* dst, void* tmp, uint32_t log_n,
                  int inverse, int coset, uint64_t in_len);
int plonk_msm_dev(plonk_ctx* ctx, const void* scalars, uint64_t m, void* out97_dev);
int plonk_srs_load_dev(plonk_ctx* ctx, const void* xy96_dev, uint64_t npoints);
/* Synthetic "random SRS" [tau^i] G for i < npoints generated on the GPU
 * (PublicParameters::setup semantics, src/commitment_scheme/kzg10/srs.rs:61-100);
 * tau and g_scalar are Fr (Montgomery).  Writes npoints x 96 B to out_dev. */
int plonk_srs_generate_dev(plonk_ctx* ctx, const uint64_t tau[4], const uint64_t g_scalar[4],
                           uint64_t npoints, void* out_dev);
/* The Lagrange-basis form of the context's commit key for the domain of size n = 1 << log_n (the key must hold n + 2
 * points): out[i] = [L_i(tau)] G for i < n, then [tau^n] G - G and [tau^(n+1)] G - [tau] G — (n + 2) x 96 bytes, host
 * memory.  An inverse FFT over the group on the GPU.  A single-GPU prover computes this itself; a multi-GPU run calls
 * it once where the whole key is available and hands every rank its slice (plonk_prover_desc.lagrange_xy96). */
int plonk_lagrange_key(plonk_ctx* ctx, uint32_t log_n, uint8_t* out_xy96);

/* plain device memory helpers so callers need no HIP bindings of their own */
int plonk_dev_alloc(plonk_ctx* ctx, uint64_t bytes, void** out);
int plonk_dev_free(plonk_ctx* ctx, void* p);
int plonk_dev_h2d(plonk_ctx* ctx, void* dst_dev, const void* src_host, uint64_t bytes);
int plonk_dev_d2h(plonk_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes);
int plonk_dev_sync(plonk_ctx* ctx);
void* plonk_ctx_stream(plonk_ctx* ctx); /* the hipStream_t of the context's main stream (prove() also uses a private side stream) */
/* Rows of the commit-key tables the context holds: 256 = one row per bit position (2^r * P_i: NAF digits over 2^19 buckets,
 * ~12.1 additions per scalar), 128 = a row for every second position (12.8), 64 = a row for every fourth position (13.0; only
 * when table_mode forces it), 16 = window rows (2^(16 w) * P_i, 16 additions
 * per scalar), 0 = no key loaded.  Chosen from the context's table budget (plonk_gpu_config above) for keys of more than
 * 2^18 + 64 points; same results whichever; plonk_gpu_config.table_mode / .msm_bucket_bits force a layout / bucket count. */
int plonk_ctx_table_rows(plonk_ctx* ctx);

/* ---- device-resident Prover::prove (V3) -------------------------------------------
 * Replaces prove_inner (src/compiler/prover.rs:415-761) minus witness generation and the
 * RNG, which stay with the caller (Composer::prove, src/composer.rs:442; BlsScalar::random).
 * The context must hold the commit key (plonk_srs_load: >= size + 7 points).  A prover is bound to
 * the key its context held at plonk_prover_create: after a later plonk_srs_load /
 * plonk_prover_from_bytes on the same context, plonk_prover_prove on the older prover returns
 * PLONK_ERR_STATE (its degree bounds and shard ranges describe a key that is gone) — rebuild it.
 *
 * desc.polys: the 15 ProverKey polynomials in coefficient form (Fr Montgomery limbs), order
 *   q_m q_l q_r q_o q_f q_c q_arith q_range q_logic q_fixed_group_add q_variable_group_add
 *   s_sigma_1 s_sigma_2 s_sigma_3 s_sigma_4   (src/proof_system/widget.rs:284-313)
 * desc.vk_commitments: the 15 VerifierKey commitments (48-byte compressed, same order) that
 *   seed the transcript (widget.rs:218-258); NULL = commit to the polynomials on the GPU as
 *   Compiler::preprocess does (src/compiler.rs:213-232).
 * The 8n coset evaluations, sigma evaluations and vanishing inverses (compiler.rs:310-425,
 * prover.rs:78-100) are rebuilt on the device.  On one GPU the prover also derives the Lagrange-basis form of the
 * commit key ([L_i(tau)] G, an inverse FFT over the group — needs size + 2 key points) and takes the four wire
 * commitments from the wire VALUES: the same group elements as CommitKey::commit of the blinded coefficient forms
 * (prover.rs:139-152,187-210), cheaper the smaller the witness values are.  PLONK_WIRE_COMMIT=coeff disables it. */
typedef struct plonk_prover plonk_prover;
/* Multi-GPU (one process per GPU): rank r loads only SRS points [r*S, (r+1)*S), S = ceil(srs_total / world),
 * into its context (srs_total >= size + 7) and owns the same range of polynomial COEFFICIENTS:
 *   - every MSM runs on the rank's point range; the per-rank partial sums (192-byte XYZZ points) are
 *     all-gathered and added locally (EC addition is not an RCCL reduce op);
 *   - world in {2, 4, 8}: the quotient is computed per residue class of the quotient coset (rank r owns
 *     the size-n cosets g w^j H_n with j = r mod world), one all-to-all turns the per-class remainders into
 *     the coefficient range of t the rank commits to, and evaluations / linearisation / opening quotients
 *     work on that range with two more small all-gathers;
 *   - other world sizes (or PLONK_SHARD_QUOTIENT=0): only the MSMs are sharded.
 * Transport: RCCL on the library's stream when the context has a communicator (plonk_comm_init below);
 * otherwise this host callback — an all-gather, `recv` laid out rank-major — which is how the tests run
 * several ranks on one device.  Return 0 on success. */
typedef int (*plonk_allgather_fn)(void* user, const void* send, void* recv, uint64_t bytes_per_rank);
typedef struct {
  uint64_t constraints;          /* gate count; domain size = next power of two        */
  const uint8_t* label;          /* transcript label (Compiler::compile `label`)        */
  uint64_t label_len;
  const uint64_t* polys[15];
  uint64_t poly_len[15];         /* coefficients per polynomial, <= size                */
  const uint8_t* vk_commitments; /* 15 x 48 bytes or NULL                               */
  int shard_rank;                /* 0 when shard_world <= 1                             */
  int shard_world;               /* <= 1: single GPU, the context holds the whole SRS   */
  uint64_t srs_total;            /* global SRS length (only read when shard_world > 1)  */
  plonk_allgather_fn allgather;
  void* allgather_user;
  /* The Lagrange-basis key of plonk_lagrange_key, or this rank's part of it.
   * shard_world <= 1: all size + 2 points (lagrange_count == size + 2) of a key computed earlier for the same
   *   commit key and size — the prover then skips the group FFT (the bulk of its build time); NULL = derive it.
   * shard_world > 1: the slice [shard_rank * S, shard_rank * S + lagrange_count) of those points, S as above;
   *   NULL / 0 = commit to the wire polynomials in coefficient form.
   * A supplied key is validated: every point on the curve and in the prime-order subgroup (PLONK_ERR_POINT) and, on one
   * GPU, the whole key against the context's commit key by a random linear combination — one inverse transform and two
   * MSMs (PLONK_ERR_DATA for the key of another setup, a permuted or otherwise wrong key).  Sharded provers (round 6): every
   * rank must pass the SAME kind — NULL, its slice (a non-NULL pointer even when the slice is empty) or the whole key; one
   * mode byte per rank is all-gathered at creation and a disagreement is PLONK_ERR_ARG on every rank (mixed modes would add
   * whole-column commitments to point-range partial sums: silently wrong wire commitments).  The same random-combination
   * identity then runs over the ranks — slices summed like any sharded commitment, whole keys compared per rank with the
   * verdict shared — so a wrong key on any rank is PLONK_ERR_DATA on all of them. */
  const uint8_t* lagrange_xy96;
  uint64_t lagrange_count;
} plonk_prover_desc;
int plonk_prover_create(plonk_ctx* ctx, const plonk_prover_desc* desc, plonk_prover** out);
void plonk_prover_destroy(plonk_prover* p);
/* Prover::prove_with_version (prover.rs:365-413): version 3 = PlonkVersion::V3, the default of every prover (Transcript::base_v3,
 * transcript.rs:131-145); version 2 = the legacy seeding the reference keeps behind its `legacy-proving` feature
 * (Transcript::base + VerifierKey::seed_transcript_legacy, transcript.rs:110-129, widget.rs:224-228,260-265: the label s_sigma_4
 * carries the commitment of s_sigma_1).  Nothing else of a proof depends on the version.  Other values: PLONK_ERR_ARG (V1 is
 * Error::UnsupportedProvingVersion in the reference).  Applies to the proofs made after the call. */
int plonk_prover_set_version(plonk_prover* p, int version);
int plonk_prover_vk(plonk_prover* p, uint8_t out[15 * 48]);
/* What the prover was BUILT as — the configuration of its context at plonk_prover_create / plonk_compile, resolved: tests assert
 * it so that a configuration switch the library ignores cannot pass for the variant it names. */
typedef struct plonk_prover_info {
  uint64_t size;                 /* domain size n */
  uint32_t quotient_domain;      /* 4: quotient interpolated on the 4n coset and de-aliased; 8: the reference's 8n evaluation */
  uint32_t wire_commit_values;   /* 1: wire commitments from the wire VALUES over a Lagrange-basis key; 0: coefficient form */
  uint32_t lagrange_table_rows;  /* rows of that key's tables (16 / 64 / 128 / 256), 0 without one */
  uint32_t shard_world, shard_rank;
  uint32_t sharded_quotient;     /* 1: quotient by residue class, rounds 4-5 by coefficient range; 0: only the MSMs are sharded */
  uint32_t quotient_classes;     /* Q: 4, or 8 for eight ranks (0 when the quotient is not sharded) */
  uint32_t wire_group_launches;  /* of the LAST proof's wire commitments: 1 = one grouped launch (resident columns); 3 = columns a, b, then c + d
                                    as they arrive from the host (plonk_prover_prove from 2^19 gates on); 4 = one launch per column; 0 before the first proof */
  uint64_t lagrange_points;      /* points of the Lagrange-basis key (or of this rank's slice) */
} plonk_prover_info;
int plonk_prover_describe(plonk_prover* p, plonk_prover_info* out);
uint64_t plonk_prover_size(plonk_prover* p);
/* diagnostic: read `count` Fr at `offset` of internal array `which` (0 wire polys, 1 z poly,
 * 2 pi poly, 3 coset evals z|a|b|c|d|pi, 4 quotient, 5 t_low|t_mid|t_high, 6 lin. comb., 7 opening
 * witness, 8 key coset evals, 9 sigma evals, 10 scratch, 11 evaluations, 12 key polynomials) */
int plonk_prover_peek(plonk_prover* p, int which, uint64_t offset, uint64_t count, uint64_t* out);
/* wires: a, b, c, d columns padded to `size` (prover.rs:446-460), Fr Montgomery.
 * pi_idx/pi_val: sparse public inputs (gate row, value), rows ascending (composer.rs:465-485).
 * blinders: 14 Fr in the reference's RNG draw order: a0 a1 b0 b1 c0 c1 d0 d1 (prover.rs:154-161),
 *           z0 z1 z2 (:133-135,503), b12 b13 b14 (:553-555).
 * proof: 1008 bytes = Proof::to_bytes (src/proof_system/proof.rs:137-162).
 * PLONK_ERR_UNSAT mirrors Error::CircuitUnsatisfied (quotient_poly.rs:132).  By default the quotient is
 * interpolated on the 4n coset and de-aliased — the same t(X), hence the same proof
 * bytes — and an unsatisfied witness is recognised by the quotient identity failing at the evaluation
 * challenge (probability of missing it <= 5n/q); PLONK_QUOTIENT_DOMAIN=8 in the environment selects the
 * reference's 8n evaluation with its exact degree test.
 * One deviation: when the evaluation challenge z or z * omega is ZERO (probability 2^-254) the opening quotients are
 * computed with 1 / z, and the call returns PLONK_ERR_STATE where the reference would go on to emit a proof.
 * Cost of the host columns: they cross PCIe inside the call, one after the other on a copy stream; from 2^19 gates on the
 * library commits to column a, then b, then c + d as each lands (plonk_prover_info.wire_group_launches = 3), so only the
 * FIRST column's copy is exposed — a proof from PINNED columns (plonk_host_alloc) is 0.8-1.15 ms slower than
 * plonk_prover_prove_dev at 2^20 gates (bench.py: prove_ms_host_wires_pinned, host_wires.pcie_floor_ms).  Pageable memory
 * works but the copies then stage synchronously and overlap nothing. */
int plonk_prover_prove(plonk_prover* p, const uint64_t* const wires[4], const uint64_t* pi_idx,
                       const uint64_t* pi_val, uint64_t pi_count, const uint64_t* blinders,
                       uint8_t proof[1008]);
/* same with the 4 x size wire columns already resident in HBM (contiguous a|b|c|d) */
int plonk_prover_prove_dev(plonk_prover* p, const void* wires_dev, const uint64_t* pi_idx,
                           const uint64_t* pi_val, uint64_t pi_count, const uint64_t* blinders,
                           uint8_t proof[1008]);

/* ---- Compiler::preprocess on the device -------------------------------------------------
 * plonk_compile replaces Compiler::preprocess (src/compiler.rs:132-461) for a circuit the caller has
 * already laid out as gates: what Composer holds after Circuit::circuit ran (src/composer.rs:119-167 —
 * per gate the 11 selector values and the witness index on each of its four wires).  On the device:
 * the 11 selector interpolations (compiler.rs:177-187), the four sigma polynomials
 * (Permutation::compute_sigma_polynomials, src/composer/permutation.rs:106-211), the 15 VerifierKey
 * commitments (compiler.rs:213-232) and the evaluation arrays of the ProverKey (compiler.rs:310-425; on the
 * quotient domain this library uses, see plonk_prover_create).  The result is a prover like the one
 * plonk_prover_create builds from coefficient forms; plonk_prover_vk returns the commitments.
 *
 * selectors[k]: `constraints` Fr values (Montgomery limbs) of selector k in plonk_prover_desc.polys order
 *   (q_m q_l q_r q_o q_f q_c q_arith q_range q_logic q_fixed_group_add q_variable_group_add); NULL = zero.
 * wires[w]: `constraints` witness indices (Witness::index) on wires a, b, c, d; every index < witnesses.
 * The shard_* / allgather / lagrange_* fields mean what they mean in plonk_prover_desc.
 * Errors: PLONK_ERR_ARG (NULL wires, index out of range, fewer than 2 gates), PLONK_ERR_DEGREE (commit key
 * shorter than the domain), PLONK_ERR_NO_SRS. */
typedef struct {
  uint64_t constraints;
  const uint8_t* label;
  uint64_t label_len;
  const uint64_t* selectors[11];
  const uint32_t* wires[4];
  uint64_t witnesses;            /* number of witnesses the composer allocated                */
  int shard_rank;
  int shard_world;
  uint64_t srs_total;
  plonk_allgather_fn allgather;
  void* allgather_user;
  const uint8_t* lagrange_xy96;
  uint64_t lagrange_count;
} plonk_circuit_desc;
int plonk_compile(plonk_ctx* ctx, const plonk_circuit_desc* circuit, plonk_prover** out);
/* Prove from the witness VALUES (count x Fr, count == circuit.witnesses) on a prover built by plonk_compile:
 * the four wire columns of prove_inner (prover.rs:446-460) are gathered in HBM from the witness table, so
 * only the distinct values cross PCIe.  Everything else as plonk_prover_prove.  PLONK_ERR_STATE on a prover
 * that was not compiled from a circuit. */
int plonk_prover_prove_witnesses(plonk_prover* p, const uint64_t* witnesses, uint64_t count, const uint64_t* pi_idx,
                                 const uint64_t* pi_val, uint64_t pi_count, const uint64_t* blinders,
                                 uint8_t proof[1008]);

/* ---- witness diagnosis: which gates and copy constraints fail --------------------------------
 * The proving entry points answer an unsatisfied witness with the bare PLONK_ERR_UNSAT, found at the very end of a proof
 * (the quotient identity at the evaluation challenge), when the rows have long been folded into one polynomial.  These
 * three calls give the row-level answer the reference's debugger gives its users (src/debugger.rs:95-236) — and the
 * copy-constraint violations it cannot see — from what the prover already holds in HBM, without a proof: no group
 * operation, no challenge, nothing probabilistic.  Use them as a pre-check before a proof or as a post-mortem after one.
 *
 * The arguments mean what they mean for plonk_prover_prove / _prove_dev / _prove_witnesses (wire columns over the whole
 * domain, Fr Montgomery; sparse public inputs); there are no blinders.  Rows are taken over the whole domain of size n;
 * the rotated values a_w, b_w, d_w of row i are those of row i + 1 mod n — the last row reads row 0, a live row when the
 * gate count is a power of two (debugger.rs:74-93).  For every row the 17 gate identities are evaluated and each is tested
 * for zero on its own; bit f of `families` is set when identity f is non-zero there:
 *    0       arithmetic   (q_m a b + q_l a + q_r b + q_o c + q_f d + q_c) q_arith + PI
 *    1 - 4   range        the quad deltas of c/d, b/c, a/b, next-row d / a, each times q_range
 *    5 - 9   logic        the quad deltas of a, b, d, the product term, the xor/and relation, each times q_logic
 *   10 - 13  fixed base   bit consistency, xy consistency, x accumulator, y accumulator, each times q_fixed_group_add
 *   14 - 16  variable-base addition   xy consistency, x3, y3, each times q_variable_group_add
 * Bit k of `copy_wires` (0..3 = a, b, c, d) is set when the value on wire k of the row differs from the value at the
 * position sigma maps (k, row) to; the position is decoded from the prover's own sigma evaluations, and a value that
 * decodes to no position counts as failing.  All copy masks are empty iff the columns are constant on every cycle of the
 * permutation.  A row fails when either mask is non-zero; `out` receives the failing rows in ascending order, the first
 * min(cap, rows_failing) of them, while the totals of `info` count all.  out == NULL with cap == 0 asks for the summary
 * only; info may be NULL.
 * Returns PLONK_OK when no row fails, PLONK_ERR_UNSAT when at least one does (info and the records are filled), and the
 * usual PLONK_ERR_ARG / _STATE / _HIP otherwise: the witness form needs a prover from plonk_compile (PLONK_ERR_STATE), a
 * sharded prover holds only its slices and answers PLONK_ERR_STATE.  Every single-GPU prover works (plonk_prover_create,
 * plonk_compile, plonk_prover_from_bytes).
 * Cost: the first call on a prover builds two proof-independent caches that live until plonk_prover_destroy — the values
 * of the non-zero selector polynomials over the domain (32 n bytes each) and the decoded positions (16 n bytes); a prover
 * that is never diagnosed allocates neither.  A call works in the prover's per-proof scratch and leaves the prover as it
 * found it: the next proof is bit-identical to one made without the call.  DESIGN.md, "Witness diagnosis". */
typedef struct plonk_unsat_row {
  uint64_t row;
  uint32_t families;          /* bit f: identity f (0..16) is non-zero on this row */
  uint32_t copy_wires;        /* bit k: wire k (a, b, c, d) of this row breaks its copy constraint */
} plonk_unsat_row;
typedef struct plonk_unsat_info {
  uint64_t rows_checked;      /* n */
  uint64_t rows_failing;      /* all of them, also beyond cap */
  uint64_t family_rows[18];   /* rows failing family f (0..16); [17] = rows with a copy-constraint failure */
  uint64_t first_row;         /* lowest failing row, UINT64_MAX when none */
  uint32_t first_family;      /* lowest set bit of that row's families, 17 when only a copy constraint fails there */
  uint32_t reserved;
  double ms;                  /* host wall clock of the call */
} plonk_unsat_info;
int plonk_prover_diagnose(plonk_prover* p, const uint64_t* const wires[4], const uint64_t* pi_idx,
                          const uint64_t* pi_val, uint64_t pi_count, plonk_unsat_row* out, uint64_t cap,
                          plonk_unsat_info* info);
int plonk_prover_diagnose_dev(plonk_prover* p, const void* wires_dev, const uint64_t* pi_idx,
                              const uint64_t* pi_val, uint64_t pi_count, plonk_unsat_row* out, uint64_t cap,
                              plonk_unsat_info* info);
int plonk_prover_diagnose_witnesses(plonk_prover* p, const uint64_t* witnesses, uint64_t count, const uint64_t* pi_idx,
                                    const uint64_t* pi_val, uint64_t pi_count, plonk_unsat_row* out, uint64_t cap,
                                    plonk_unsat_info* info);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ---------------------------------------
 * Rank 0 calls plonk_comm_unique_id and hands the 128 bytes (an ncclUniqueId) to the other ranks by
 * whatever out-of-band channel the host program has; every rank then calls plonk_comm_init on its
 * context (collective: it returns when all `world` ranks have joined).  A context with a communicator
 * runs every exchange of a sharded prover (plonk_prover_desc.shard_world > 1) as ncclAllGather /
 * ncclAllToAll on its own stream — no host callback is involved and desc.allgather may be NULL.
 * RCCL is loaded with dlopen at the first of these calls, so the library itself does not depend on it.
 * plonk_comm_selftest runs both collectives once with a rank-dependent pattern and checks the result.
 * What is exchanged and why EC partial sums are all-gathered rather than all-reduced: DESIGN.md §5.
 * plonk_comm_info reports the rank / size the communicator itself holds (ncclCommUserRank / ncclCommCount).
 *
 * Environment: this platform's driver only supports dmabuf IPC, so RCCL between processes needs
 * HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment before the HSA runtime starts (the first HIP call of the process).
 * The HOST PROGRAM exports it before its first HIP call (bench.py and the Python binding do); the library does not touch the
 * process environment.  plonk_comm_init names the variable in its error text when the communicator cannot be created
 * without it.
 *
 * Failure of a peer: a sharded proof is a sequence of collectives, and a rank that fails (or never arrives) would
 * leave the others waiting inside one.  Every wait that follows a collective polls the stream instead of blocking; after
 * PLONK_COMM_TIMEOUT_MS (default 120000) the communicator is aborted (ncclCommAbort) and the call returns
 * PLONK_ERR_STATE on every surviving rank — the context then has no communicator and must be given a new one
 * (plonk_comm_init) before the next sharded proof.  The host program should still tear the job down when one rank
 * reports an error (bench.py does: the launcher kills the remaining ranks).
 *
 * Measurement aid, never for production: after plonk_comm_measure_loopback(ctx, 1) every collective of a sharded prover on
 * THIS context returns data of the rank's own in its peers' places (local copies, no transport: the all-to-all the blocks the
 * rank addressed to each peer, the device all-gather rotated copies of its slice — W different blocks, so that what follows
 * them works on scalars as dense as a real run's), so that one rank of a W-rank job can be timed alone on one GPU
 * (tools/rank_alone.py).  Proofs made that way are wrong by construction:
 * plonk_prover_prove* returns PLONK_ERR_UNSAT from its final identity check.  Nothing in the environment switches it on.
 *
 * Transport library: RCCL is looked up as librccl.so(.1) on the loader path, then under /opt/rocm/lib.
 * plonk_comm_set_library(path) names another shared object exporting the nccl* entry points BEFORE the first
 * communicator call of the process (PLONK_ERR_STATE once a library is loaded): a deployment whose RCCL lives elsewhere, or
 * the test suite's stand-in (tests/fake_rccl: device-pointer collectives over hipIpc between ranks that SHARE one GPU —
 * RCCL refuses two ranks per device — so that the W > 1 branch of every exchange runs on a 1-GPU box).
 * plonk_comm_library writes the path of what was actually loaded (NUL-terminated, truncated to cap); a host program that
 * reports which collective a measurement used must take it from here (bench.py prints "rccl" only for a librccl file).
 * After a time-out whose abort did not drain the stream (or a transport without ncclCommAbort) the context is UNUSABLE:
 * every entry point that queues work on the context or waits for it (transforms, commitments, key loads, copies, provers,
 * plonk_comm_init) returns PLONK_ERR_STATE at once instead of queueing behind the dead collective; destroy it.  The destroy
 * calls (plonk_prover_destroy, plonk_comm_destroy, plonk_ctx_destroy) poll the streams for at most 2 s and, if they are still
 * busy, ABANDON the context's device memory, streams and pinned buffers instead of freeing them — hipFree and
 * hipStreamSynchronize would wait for the dead kernel for ever; plonk_comm_destroy then returns PLONK_ERR_STATE.  A host that
 * wants the memory back resets the device (hipDeviceReset) or exits.
 * plonk_comm_warning: the note plonk_comm_init left on this context when it SUCCEEDED with something to say (today: the
 * dmabuf IPC variable missing from the environment), "" otherwise — a successful call never writes plonk_last_error(). */
int plonk_comm_set_library(const char* path);
int plonk_comm_library(char* out, uint64_t cap);
int plonk_comm_measure_loopback(plonk_ctx* ctx, int on);
int plonk_comm_unique_id(uint8_t out[128]);
int plonk_comm_init(plonk_ctx* ctx, const uint8_t unique_id[128], int rank, int world);
int plonk_comm_info(plonk_ctx* ctx, int* rank, int* world);
int plonk_comm_warning(plonk_ctx* ctx, char* out, uint64_t cap);
int plonk_comm_selftest(plonk_ctx* ctx);
int plonk_comm_destroy(plonk_ctx* ctx);

/* ---- serialized Prover ---------------------------------------------------------------
 * plonk_prover_from_bytes replaces Prover::try_from_bytes (src/compiler/prover.rs:266-345): `blob`
 * is exactly what the reference's Prover::to_bytes() writes (prover.rs:238-263 — six big-endian u64
 * lengths, label, ProverKey::to_var_bytes widget.rs:347-447, CommitKey::to_raw_var_bytes
 * key.rs:215-229, VerifierKey::to_bytes widget.rs:84-111).  It validates the blob as the
 * reference does (errors: PLONK_ERR_BYTES / PLONK_ERR_DATA / PLONK_ERR_POINT), loads the commit
 * key into `ctx` (replacing any SRS it held) and builds the device prover.  The 8n evaluation
 * arrays in the blob are validated structurally and then rebuilt on the device from the
 * coefficient forms.
 * plonk_prover_blob_check is the host-only decoder/validator (no GPU, no context): offsets of the
 * pieces inside `blob`; polynomials in the plonk_prover_desc order.  It checks the curve
 * equation of the commit-key points; the subgroup check needs the GPU (plonk_srs_validate).
 * plonk_srs_validate: CommitKey::from_raw_var_bytes' per-point is_on_curve & is_torsion_free
 * (key.rs:283-294) for x||y points as taken by plonk_srs_load. */
/* The other direction.  plonk_prover_to_bytes writes what the reference's Prover::to_bytes() writes
 * (prover.rs:238-263) for this prover and the commit key its context holds — the key polynomials, their 8n coset
 * evaluations (computed on the device and streamed out: 17 x 8 x size scalars, 4.6 GB at 2^20 gates), the raw commit
 * key and the VerifierKey — so a circuit compiled by plonk_compile can be loaded by the unmodified reference
 * (Prover::try_from_bytes) or by plonk_prover_from_bytes later.  plonk_verifier_to_bytes writes Verifier::to_bytes()
 * (src/compiler/verifier.rs:88-117) from the prover's label / sizes / VerifierKey, the caller's OpeningKey::to_bytes()
 * (copied as given; plonk_verifier_from_bytes below decodes it) and the public-input indexes.
 * Both: out == NULL reports the length in *len; otherwise cap >= *len bytes are written.  Single-GPU provers only.
 * Known differences from the reference's bytes (format parity is pinned only to the restated layout):
 * plonk_prover_from_bytes keeps the size + 8 commit-key points prove() can touch, so from_bytes -> to_bytes writes a
 * SHORTER commit key than a blob whose key was trimmed to (constraints + 6).next_power_of_two() + 7 points (the proofs
 * are identical; the blob is not byte-identical, and generic plonk_msm calls on that context cannot use the dropped
 * degrees).  No new format entry points are planned until a reference-produced blob pins these (tools/dump_kat_blob.rs). */
int plonk_prover_to_bytes(plonk_prover* p, uint8_t* out, uint64_t cap, uint64_t* len);
int plonk_verifier_to_bytes(plonk_prover* p, const uint8_t* opening_key, uint64_t opening_key_len,
                            const uint64_t* pi_idx, uint64_t pi_count, uint8_t* out, uint64_t cap, uint64_t* len);
/* Proof verification (Verifier::try_from_bytes / Verifier::verify, src/compiler/verifier.rs:121-253, src/proof_system/
 * proof.rs:218-513), for a batch of proofs of one circuit.
 * plonk_verifier_from_bytes takes the blob plonk_verifier_to_bytes (or the reference's Verifier::to_bytes) writes and
 * validates it like the reference: the six big-endian lengths (PLONK_ERR_BYTES when the blob is shorter than they say or
 * they overflow), the 15 VerifierKey commitments (PLONK_ERR_DATA), the OpeningKey's g, h and x_h (on their curves, in the
 * subgroup, not the identity: PLONK_ERR_DATA), a power-of-two domain size, vk.n == constraints and public-input indexes
 * inside the domain (PLONK_ERR_DATA).  The VK points and g are decoded on the device once; h and x_h are prepared for
 * the Miller loop on the host.  A verifier holds device memory of its context and never touches the context's commit
 * key, tables or provers; destroy it before its context.
 * plonk_verifier_set_version: 3 (default) = PlonkVersion::V3 transcript, 2 = the legacy seeding (the rule of
 * plonk_prover_set_version); anything else PLONK_ERR_ARG.
 * plonk_verify checks `count` proofs (count x 1008 bytes, Proof::to_bytes).  pi: count x pi_count Fr (Montgomery limbs,
 * like pi_val of plonk_prover_prove), dense, in the verifier's public-input index order.  verdicts (count entries; may be
 * NULL when count == 1): PLONK_OK, PLONK_ERR_VERIFY, PLONK_ERR_DATA (non-canonical evaluation), PLONK_ERR_POINT (a
 * commitment is not a valid compressed point of G1).  Returns PLONK_OK iff every proof is valid, PLONK_ERR_VERIFY when
 * at least one is not, PLONK_ERR_ARG for pi_count != the verifier's count (Error::InconsistentPublicInputsLen), count == 0
 * or count > 2^24.
 * The K checks e(-L_k, x_h) e(R_k, h) == 1 are folded with the powers 1, rho, rho^2, ... of a challenge rho drawn from
 * a transcript over the whole (sub-)batch ("plonk-batch-verify-v1": its length, every proof's bytes and public inputs):
 * one MSM of 13 K + 16 terms for L and R on the device and ONE pairing check on the host, whatever K is.  With K = 1 the
 * weight is 1 and the check is exactly the reference's.  A failing batch is bisected, a fresh rho per sub-batch, until
 * every failing proof is found: b bad proofs cost O(b log K) further checks; the verdicts equal those of count == 1
 * calls (up to the aggregation's soundness error, <= K / q per check; DESIGN.md, "Proof verification").  The call holds
 * the context for its whole duration, bisection included: a batch of K proofs that are ALL bad costs 2K - 1 checks (each one
 * MSM launch and one pairing, ~10 ms at small sizes), so a caller verifying untrusted batches on a context it also proves
 * on should bound K.  For untrusted batches plonk_verify_each (below) gives the same verdicts with one pairing per proof
 * on the device, at a cost that does not depend on how many proofs are bad.
 * plonk_verifier_last reports the last plonk_verify: msm_terms counts the terms of both sums of its FIRST check,
 * pairing_checks all checks (1 for a valid batch), the phase times are host wall-clock milliseconds. */
typedef struct plonk_verifier plonk_verifier;
typedef struct {
  uint64_t proofs, msm_terms;
  uint32_t pairing_checks, rejected;
  double ms_decode, ms_scalars, ms_msm, ms_pairing;
} plonk_verify_info;
int plonk_verifier_from_bytes(plonk_ctx* ctx, const uint8_t* blob, uint64_t len, plonk_verifier** out);
void plonk_verifier_destroy(plonk_verifier* v);
int plonk_verifier_set_version(plonk_verifier* v, int version);
int plonk_verify(plonk_verifier* v, const uint8_t* proofs, const uint64_t* pi, uint64_t pi_count, uint64_t count,
                 int32_t* verdicts);
int plonk_verifier_last(plonk_verifier* v, plonk_verify_info* out);
/* plonk_verify_mixed checks `count` proofs of several circuits that share one opening key (circuits compiled from one
 * PublicParameters) in one aggregated check.  Proof k (1008 bytes, Proof::to_bytes) belongs to verifiers[circuit[k]];
 * each verifier's current version applies to its proofs, and one handle may appear in `verifiers` more than once (each
 * position is a slot of its own).  pi: the proofs' public inputs concatenated, proof by proof, each in its verifier's count
 * and index order (Montgomery limbs, like plonk_verify); pi_total: the number of Fr values in pi.  verdicts (count entries;
 * may be NULL when count == 1) and the return value as plonk_verify: each verdict equals what a count == 1 plonk_verify
 * of that proof with its own verifier returns, up to the aggregation's soundness error.  PLONK_ERR_ARG, with a text that
 * names the check, for a NULL argument, nverifiers == 0, count == 0 or count > 2^24, circuit[k] >= nverifiers, pi_total
 * not the sum of the proofs' public-input counts, verifiers on different contexts, or verifiers whose 240-byte opening
 * keys (g, h, x_h) differ (mixing setups is not supported).
 * Every check e(-L_k, x_h) e(R_k, h) == 1 shares (g, h, x_h), so the checks fold with the powers 1, rho, rho^2, ... of
 * one challenge: one MSM over the 15 VK points of every circuit the batch uses (each with its circuit's summed scalars),
 * g and 11 commitments per proof (13 K + 15 C + 1 terms, C the circuits used), and ONE pairing check; the probability
 * that a batch with a bad proof passes is at most K / q per check, as for plonk_verify.  The transcripts replay on the
 * device (one lane per proof, from its circuit's transcript seeded once by the host); each proof's replay draws
 * challenge_bytes("batch digest", 32) after u, a digest of everything that proof's check depends on.  rho is
 * challenge_scalar("rho") of a Merlin transcript "plonk-batch-verify-mixed-v1" that absorbs append_u64("batch length", m);
 * for every slot the (sub-)batch uses, ascending, append_u64("slot", s) and append_message("circuit", verifier digest);
 * for every proof in order append_u64("circuit", slot) and append_message("proof", proof digest).  The verifier digest
 * is challenge_bytes("circuit digest", 32) of a transcript "plonk-verifier-digest-v1" over append_message("label"),
 * append_u64("version"), append_u64("size"), append_u64("constraints"), 15 x append_message("vk", commitment)
 * (VerifierKey::to_bytes order), append_message("opening key", 240 bytes), append_u64("public inputs", count) and
 * append_u64("public input index", i) per index.  With m = 1 the weight is 1.  A failing batch is bisected like
 * plonk_verify's, a fresh rho per sub-batch: b bad proofs cost O(b log K) further checks, an all-bad batch 2K - 1.  The
 * call holds the context for its whole duration, writes nothing into any verifier's plonk_verifier_last and fills `info`
 * (may be NULL) the same way instead; ms_scalars covers the replay kernel, the rho derivation and the weighting. */
int plonk_verify_mixed(plonk_verifier* const* verifiers, uint32_t nverifiers, const uint32_t* circuit, const uint8_t* proofs,
                       const uint64_t* pi, uint64_t pi_total, uint64_t count, int32_t* verdicts, plonk_verify_info* info);
/* plonk_verify_each: the arguments of plonk_verify_mixed (circuit == NULL: every proof belongs to verifiers[0]), but every
 * proof is checked ON ITS OWN: decode, device replay and statuses as plonk_verify_mixed, then per proof its own 2 + 27 terms
 * (L: W_z with 1 and W_zw with u; R: the 15 VK points of its circuit, g and its 11 commitments, unweighted), one wave per
 * proof for the two sums and ONE PAIRING CHECK PER PROOF in one lane of a device kernel.  No rho, no
 * batch transcript, no bisection, no K / q soundness term: verdict k equals exactly what a count == 1 plonk_verify of proof k
 * with its own verifier and version returns, and the cost does not depend on how many proofs are bad.  verdicts is
 * required (count entries; there is no NULL form); a malformed proof (PLONK_ERR_POINT, PLONK_ERR_DATA) never stops the
 * others from being decided.  Returns PLONK_OK iff every verdict is, PLONK_ERR_VERIFY otherwise, PLONK_ERR_ARG for
 * everything plonk_verify_mixed refuses.  info (may be NULL): proofs = count, pairing_checks = the proofs that reached the
 * pairing kernel (never more than count), msm_terms = 29 per such proof, rejected = verdicts other than PLONK_OK, the phase
 * times host wall clock around the phases (ms_scalars: replay and packing, ms_msm: the per-proof sums, ms_pairing: the
 * pairing kernel).  Writes nothing into any verifier's plonk_verifier_last; the line tables of (x_h, h) for the pairing
 * kernel (about 47 KB of device memory) are made by the first call that uses a verifier's opening key and freed with that
 * verifier.  When to use it (measured on an MI355X at 2^12 gates): a device pairing check is about
 * 28 ms of latency whatever the count (8192 checks: 29 ms), so a VALID batch costs 1.8x (K = 1024) to 3.4x (K = 1) what
 * plonk_verify_mixed costs (K = 8192: 79 ms against 39 ms) — keep that call for input expected to be valid.  A bad proof
 * costs the bisection about 2 log2 K further checks of 6 to 10 ms (K = 8192 with 8 bad proofs: 1875 ms against 80 ms here;
 * K = 256 all bad: 3.0 s against 39 ms), so from K = 64 on, one expected bad proof per batch already makes this the cheaper
 * call, and it is the one whose cost an adversary cannot raise.  Below about 4 proofs, count == 1 calls of plonk_verify
 * are cheaper. */
int plonk_verify_each(plonk_verifier* const* verifiers, uint32_t nverifiers, const uint32_t* circuit, const uint8_t* proofs,
                      const uint64_t* pi, uint64_t pi_total, uint64_t count, int32_t* verdicts, plonk_verify_info* info);
typedef struct {
  uint64_t size, constraints;
  uint64_t label_off, label_len;
  uint64_t poly_off[15], poly_len[15]; /* canonical 32-byte little-endian scalars */
  uint64_t srs_off, srs_points;        /* 97-byte raw points (x || y || infinity) */
  uint64_t vk_off;                     /* 15 x 48 bytes, VerifierKey::to_bytes order */
} plonk_prover_blob_info;
int plonk_prover_blob_check(const uint8_t* blob, uint64_t len, plonk_prover_blob_info* info);
int plonk_prover_from_bytes(plonk_ctx* ctx, const uint8_t* blob, uint64_t len, plonk_prover** out);
int plonk_srs_validate(plonk_ctx* ctx, const uint8_t* xy96, uint64_t npoints);

/* ---- PublicParameters on disk -> commit key on the device ------------------------------------
 * The files a dusk-plonk user keeps (src/commitment_scheme/kzg10/srs.rs:103-178).  Both start with
 * OpeningKey::to_bytes() (240 B: g 48 B, h 96 B, x_h 96 B, compressed; key.rs:436-452); then
 *   RAW        PublicParameters::to_raw_var_bytes(): CommitKey::to_raw_var_bytes() = u64 LE count, count x 97 B raw points
 *              x || y || infinity flag (key.rs:215-229);
 *   COMPRESSED PublicParameters::to_var_bytes(): CommitKey::to_var_bytes() = 48-byte compressed points, no count (key.rs:303-308).
 * mode:
 *   PLONK_PP_RAW_UNCHECKED  PublicParameters::from_slice_unchecked (srs.rs:131-146): the commit-key points are trusted; like
 *                           CommitKey::from_slice_unchecked (key.rs:243-258) it takes min(count, whole 97-byte chunks present) points;
 *   PLONK_PP_RAW            CommitKey::from_raw_var_bytes (key.rs:263-300): count != 0 (PLONK_ERR_DATA), exact length
 *                           (PLONK_ERR_BYTES), EVERY point of the file is_on_curve & is_torsion_free (PLONK_ERR_POINT; on the
 *                           GPU) — also the ones a trim drops afterwards, as in the reference;
 *   PLONK_PP_COMPRESSED     PublicParameters::from_slice (srs.rs:164-178) = one G1Affine::from_slice per 48-byte chunk
 *                           (key.rs:319-326): compression flag, x < p, x^3 + 4 a square, torsion-free — any failure, a short
 *                           last chunk included, is a dusk_bytes error (PLONK_ERR_DATA), wherever in the file.  Decompression
 *                           (one square root per point, g1codec.cuh) and the subgroup test run on the GPU.
 *   All modes: OpeningKey::from_bytes + try_new (key.rs:596-648) — g a valid compressed G1 point, h and x_h valid compressed G2
 *   points (flags, canonical coordinates, on the twist curve, of order q; hostg2.hpp, on the host) and NONE of the three the
 *   identity (try_new refuses a degenerate key: the pairing check would be trivially satisfiable) — PLONK_ERR_DATA otherwise.
 *   The prover never uses them; they are handed back as the 240 bytes they came as.
 *   truncated_degree > 0: PublicParameters::trim (srs.rs:188-196) = CommitKey::truncate(truncated_degree + 6)
 *   (key.rs:336-355): PLONK_ERR_DEGREE when the key is shorter (Error::TruncatedDegreeTooLarge); 0 keeps every point.  The
 *   unchecked mode never reads beyond the trim.  At most 240 bytes: PLONK_ERR_BYTES (Error::NotEnoughBytes, srs.rs:165-167).
 *   ONE deliberate divergence: an identity point in the commit key (flag byte 1 / the 0xC0 encoding) is refused with
 *   PLONK_ERR_POINT in every mode, although G1Affine::from_bytes and is_on_curve & is_torsion_free accept it: no SRS
 *   [tau^i] G holds one and the precomputed table rows cannot represent it (tests/test_public_parameters.py names this case).
 * plonk_public_parameters_check is the host-side part (no GPU): structure, opening key, trim, flags and coordinate ranges.
 * plonk_srs_load_public_parameters = check + the per-point work on the GPU + window tables of the kept points. */
enum { PLONK_PP_RAW_UNCHECKED = 0, PLONK_PP_RAW = 1, PLONK_PP_COMPRESSED = 2 };
typedef struct plonk_public_parameters_info {
  uint64_t opening_key_off;   /* 240 bytes */
  uint64_t points_off;        /* first point */
  uint64_t point_stride;      /* 97 (raw) or 48 (compressed) */
  uint64_t points_total;      /* points the file holds */
  uint64_t points_kept;       /* after the trim */
} plonk_public_parameters_info;
int plonk_public_parameters_check(const uint8_t* bytes, uint64_t len, uint64_t truncated_degree, int mode,
                                  plonk_public_parameters_info* info);
int plonk_srs_load_public_parameters(plonk_ctx* ctx, const uint8_t* bytes, uint64_t len, uint64_t truncated_degree,
                                     int mode, uint8_t opening_key_out[240] /* may be NULL */,
                                     uint64_t* points_loaded /* may be NULL */);

/* ---- KZG10 openings -----------------------------------------------------------------------------
 * The part of the reference's commitment scheme that PROVES something about a commitment: CommitKey::compute_aggregate_witness,
 * open_single / open_multiple, AggregateProof::flatten and OpeningKey::batch_check (src/commitment_scheme/kzg10/key.rs:394-417,
 * 571-591, 661-707, 724-809; proof.rs:15-111).  Scalars are Fr in Montgomery limbs, commitments 48-byte compressed G1
 * (Commitment::to_bytes), errors the codes above.
 *
 * plonk_kzg_open: `count` polynomials in coefficient form (host pointers; lengths may differ, zero lengths are allowed,
 *   count <= 65536), opened at `point`:
 *     evaluations[i] = p_i(point);  commitments[i] = commit(p_i) (NULL skips them: 48 bytes each otherwise);
 *     witness48 = commit of (sum_i v^i p_i) / (X - point) with the remainder dropped — compute_aggregate_witness followed by
 *     commit.  count == 1 is open_single (v_challenge may be NULL then: the weight is 1); count == 0 gives the identity witness
 *     (Polynomial::zero()).  point == 0 works (the quotient is a shift).
 *   Degrees are checked on the length WITHOUT trailing zeros (Polynomial::from_coefficients_vec, then commit):
 *   PLONK_ERR_DEGREE when that exceeds the commit key, PLONK_ERR_NO_SRS for any call with count > 0 before a key is loaded
 *   (also when every polynomial is empty; count == 0 needs no key).  A context with a communicator holds only a range of
 *   the key: PLONK_ERR_STATE.  An error leaves nothing of the call queued on the context's streams.  Every coefficient crosses HBM once per call (fold contribution and
 *   evaluation partial in one pass); the host form stages the polynomials through two context-owned buffers of
 *   max(longest polynomial, 2^16) coefficients, group after group, the upload of one group under the kernel of the one before,
 *   so count x length is never resident.  The workspace grows on demand and is released with the context.  The call leaves
 *   the context as it found it: the next proof of a prover on the same context is bit-identical.
 * plonk_kzg_open_dev: the same with an array (host memory) of `count` DEVICE pointers on the context's GPU.
 * plonk_kzg_flatten: AggregateProof::flatten (proof.rs:87-110): out.commitment = sum_i v^i C_i (on the device), out.evaluation =
 *   sum_i v^i e_i, out.witness = witness48 unchanged.  PLONK_ERR_ARG for count == 0 (the reference underflows there),
 *   PLONK_ERR_POINT for a commitment that is not a valid compressed G1 point, PLONK_ERR_DATA for a non-canonical scalar.
 * plonk_kzg_key_create: OpeningKey::from_bytes + try_new on the 240 bytes g || h || x_h (key.rs:609-648), validated as
 *   plonk_verifier_from_bytes validates its opening key (PLONK_ERR_DATA); g is decoded on the device, h and x_h are prepared
 *   for the Miller loop once.  Destroy the key before its context.
 * plonk_kzg_batch_check: OpeningKey::batch_check (key.rs:661-707) of `count` openings, proofs[k] at points[k]:
 *     total_w = sum_k u^k W_k,  total_c = sum_k u^k C_k + sum_k (u^k z_k) W_k - (sum_k u^k v_k) g    (3 count + 1 terms, ONE
 *     launch of the verifier's two-sum MSM), then e(-total_w, x_h) e(total_c, h) == 1 on the host.  count == 1 is the
 *     reference's single `check`.  With u_override == NULL, u is the reference's batch_challenge on a fresh
 *     Transcript::new(label): append_message("dom-sep", "kzg10-batch-check-v1"), append_u64("batch-len", count), per item
 *     append_scalar("batch-point"), append_commitment("batch-polynomial-commitment"), append_scalar("batch-evaluation"),
 *     append_commitment("batch-witness-commitment"), then challenge_scalar("batch-challenge").  A caller whose surrounding
 *     transcript already has state derives u from ITS transcript the same way and passes it as u_override — a u the prover
 *     of the openings could predict (a constant, a counter, anything fixed before the batch is) VOIDS the check.
 *   PLONK_OK; PLONK_ERR_VERIFY for a failing batch and for count == 0 (key.rs:667); PLONK_ERR_POINT for a commitment that is
 *   not a valid compressed G1 point (the identity is legal); PLONK_ERR_DATA for a non-canonical scalar.  No bisection: a
 *   caller who wants per-item answers calls plonk_kzg_check_each (or this with count == 1).  info (may be NULL) is filled as plonk_verify_mixed fills it.
 * plonk_srs_check: is the commit key the key's context holds (N points P_i) [tau^i] g for the tau of THIS opening key?
 *     P_0 == g  and  e(sum_{i < N-1} r^i P_(i+1), h) == e(sum_{i < N-1} r^i P_i, x_h),
 *   r = challenge_scalar("r") of a Merlin transcript "plonk-srs-check-v1" over append_message("seed", seed32),
 *   append_u64("points", N), append_message("opening key", 240 bytes).  seed32 is the CALLER's fresh randomness, chosen after
 *   the file under test is fixed: whoever wrote the file must not be able to predict it.  A wrong key passes with probability
 *   at most N / q.  A file whose points are all on the curve and in the subgroup passes every other
 *   check of this library although no proof made from it verifies; this call closes that hole.  PLONK_OK, PLONK_ERR_VERIFY on a
 *   mismatch, PLONK_ERR_NO_SRS, PLONK_ERR_STATE on a context with a communicator, PLONK_ERR_ARG for a NULL argument (a key is
 *   bound to the context it was created on, so "the key of another context" cannot be expressed). */
typedef struct plonk_kzg_proof {   /* kzg10::Proof, proof.rs:15-23 */
  uint8_t  commitment[48];         /* commitment_to_polynomial */
  uint64_t evaluation[4];          /* evaluated_point */
  uint8_t  witness[48];            /* commitment_to_witness */
} plonk_kzg_proof;                 /* 128 bytes */
typedef struct plonk_kzg_key plonk_kzg_key;   /* an OpeningKey bound to a context */
int plonk_kzg_open(plonk_ctx* ctx, const uint64_t* const* polys, const uint64_t* lens, uint64_t count, const uint64_t point[4],
                   const uint64_t* v_challenge /* 4 limbs; may be NULL when count <= 1 */, uint64_t* evaluations /* count x 4 */,
                   uint8_t* commitments /* count x 48, or NULL */, uint8_t witness48[48]);
int plonk_kzg_open_dev(plonk_ctx* ctx, const void* const* polys_dev, const uint64_t* lens, uint64_t count, const uint64_t point[4],
                       const uint64_t* v_challenge, uint64_t* evaluations, uint8_t* commitments, uint8_t witness48[48]);
int plonk_kzg_flatten(plonk_ctx* ctx, const uint8_t* commitments /* count x 48 */, const uint64_t* evaluations /* count x 4 */,
                      uint64_t count, const uint64_t v[4], const uint8_t witness48[48], plonk_kzg_proof* out);
int plonk_kzg_key_create(plonk_ctx* ctx, const uint8_t opening_key240[240], plonk_kzg_key** out);
void plonk_kzg_key_destroy(plonk_kzg_key* key);
int plonk_kzg_batch_check(plonk_kzg_key* key, const uint64_t* points /* count x 4 */, const plonk_kzg_proof* proofs, uint64_t count,
                          const uint8_t* label, uint64_t label_len, const uint64_t* u_override /* 4 limbs or NULL */,
                          plonk_verify_info* info);
int plonk_srs_check(plonk_kzg_key* key, const uint8_t seed32[32]);
/* Per-item verdicts in one pass: one pairing check per item on the device, where
 * plonk_kzg_batch_check answers for the whole batch.  Exact: no challenge u, so nothing can cancel between items.
 * plonk_kzg_pairing_check_each: verdicts[k] = PLONK_OK iff e(A_k, x_h) == e(B_k, h), computed as e(-A_k, x_h) e(B_k, h) == 1
 *   for the key's (h, x_h); a48 / b48: count x 48 bytes, compressed G1.  (O, O) passes, a pair with exactly one identity
 *   fails.  With consecutive points of a powers-of-tau file (A_i = P_i, B_i = P_(i+1)) the failing pairs name the wrong
 *   point, which plonk_srs_check cannot.
 * plonk_kzg_check_each: OpeningKey::check of every opening proofs[k] at points[k] on its own: L_k = W_k, R_k = C_k + z_k W_k -
 *   v_k g (terms packed and summed on the device, one wave per opening).  Each verdict equals what plonk_kzg_batch_check
 *   with count == 1 returns for that item.
 * Both: verdicts (count entries, required) are PLONK_OK, PLONK_ERR_VERIFY, PLONK_ERR_POINT (a point that does not decode or
 * is outside the subgroup; the compressed identity is legal) or PLONK_ERR_DATA (a non-canonical scalar; looked at before the
 * points, as plonk_kzg_batch_check does); a malformed item never stops the others from being decided.  Return PLONK_OK iff
 * every verdict is, PLONK_ERR_VERIFY otherwise, PLONK_ERR_ARG for a NULL argument, count == 0 or count > 2^24.  info (may be
 * NULL): proofs = count, pairing_checks = items that reached the pairing kernel, msm_terms = 4 per such opening (0 for the
 * bare pairing call), rejected = verdicts other than PLONK_OK, phase times as plonk_verify_each.  The workspace is owned by
 * the context and grows on demand; the key's line tables (about 47 KB of device memory) are made by the first call and freed
 * with the key.  The calls leave the context, its commit key, tables and provers as they found them. */
int plonk_kzg_pairing_check_each(plonk_kzg_key* key, const uint8_t* a48, const uint8_t* b48, uint64_t count, int32_t* verdicts,
                                 plonk_verify_info* info /* may be NULL */);
int plonk_kzg_check_each(plonk_kzg_key* key, const uint64_t* points /* count x 4 */, const plonk_kzg_proof* proofs, uint64_t count,
                         int32_t* verdicts, plonk_verify_info* info);

/* ---- KZG10 openings over a whole domain ---------------------------------------------------------------
 * One polynomial opened at EVERY point of its evaluation domain: the n = 2^log_n witnesses pi_i = commit((f - f(w^i)) / (X - w^i))
 * by group FFTs (Feist-Khovratovich) — O(n log n) scalar multiplications where n calls of plonk_kzg_open cost n MSMs of n terms.
 * w is the generator plonk_ntt uses for size n.  With s_l = [tau^l] g the commit key and N = 2n:
 *     A = DFT_N(s_0 .. s_(n-2), O ...) (per handle);  G = NTT_N(f_(n-1), f_(n-2) .. f_1, 0 ...);  P_i = [G_i] A_i;
 *     c = DFT_N^-1(P);  h_k = c_(n-2-k) (k <= n-2), h_(n-1) = O;  pi = DFT_n(h)                       
 * plonk_kzg_domain_create: A and the split twiddles for (the context's commit key, log_n): 2n x 256 + n x 32 bytes of device
 *   memory.  log_n in [1, 20], else PLONK_ERR_ARG; PLONK_ERR_STATE on a context with a communicator (it holds only a range of
 *   the key, as for plonk_kzg_open); PLONK_ERR_NO_SRS before a key is loaded; PLONK_ERR_DEGREE for a key of fewer than n points.
 *   The handle remembers the key it was built on: once the context's key is reloaded every call on the handle except
 *   plonk_kzg_domain_destroy returns PLONK_ERR_STATE.  Destroy the handle before its context.
 * plonk_kzg_domain_points: out[i] = w^i, i < n (n x 4 limbs, Montgomery): the point witness i and evaluation i belong to.
 * plonk_kzg_open_domain: `count` polynomials in coefficient form (host pointers; lengths may differ; count <= 65536, else
 *   PLONK_ERR_ARG; count == 0 is PLONK_OK and writes nothing):
 *     evaluations[j][i] = p_j(w^i) (count x n x 4 limbs, Montgomery);  witnesses48[j][i] = pi_i of p_j (count x n x 48 bytes,
 *     compressed G1, encoded on the device: 48 bytes per witness cross PCIe);  commitments48[j] = commit(p_j) (count x 48, NULL
 *     skips them) through the ordinary commitment path.
 *   A caller builds plonk_kzg_proof items from the three arrays and hands them to plonk_kzg_check_each / plonk_kzg_batch_check
 *   with the points of plonk_kzg_domain_points.  Lengths are judged WITHOUT trailing zeros, as plonk_kzg_open judges them: more
 *   than n is PLONK_ERR_DEGREE; a coefficient that is not a canonical residue is PLONK_ERR_DATA.  A zero or constant polynomial
 *   has n compressed identities (0xC0 00 ..) as witnesses.  Every check is made before anything is queued or written: an
 *   error leaves nothing queued and no output touched.  The polynomials are processed in chunks so that the point workspace
 *   (2n slots of 256 bytes per polynomial of a chunk, owned by the handle, grown on demand) stays under
 *   workspace_cap_bytes (2 GiB; a chunk of one polynomial is always allowed, and a chunk never exceeds 4096 polynomials).
 *   The calls leave the context, its tables and its provers as they found them.
 * plonk_kzg_open_domain_dev: polys_dev is a HOST array of `count` device pointers; the three outputs are device pointers on
 *   the context's GPU.
 * plonk_kzg_domain_last: what the last open call on the handle ran as (count == 0 before the first): the tests assert it
 *   against the plan computed on the host (plonk_amd/csrc/kzg_domain_core.hpp). */
typedef struct plonk_kzg_domain plonk_kzg_domain;   /* A and the split twiddles for one (commit key, log_n), bound to a context */
typedef struct plonk_kzg_domain_info {
  uint32_t log_n;
  uint32_t chunks;                 /* chunks the polynomials of the last call were processed in */
  uint64_t count;                  /* polynomials of the last call */
  uint64_t device_bytes;           /* device memory the handle holds: A, twiddles and its workspace */
  uint64_t workspace_cap_bytes;    /* the cap on the point workspace */
  uint64_t chunk_polys;            /* polynomials per chunk (the last chunk may be shorter) */
  uint64_t stage_launches;         /* group-FFT stage launches: (2 log_n + 1) per chunk */
  uint64_t scalar_muls;            /* full-width scalar multiplications issued: 2n pointwise + the butterflies whose twiddle is not 1 */
} plonk_kzg_domain_info;
int plonk_kzg_domain_create(plonk_ctx* ctx, uint32_t log_n, plonk_kzg_domain** out);
void plonk_kzg_domain_destroy(plonk_kzg_domain* domain);
int plonk_kzg_domain_points(plonk_kzg_domain* domain, uint64_t* out /* n x 4, Montgomery: w^i */);
int plonk_kzg_open_domain(plonk_kzg_domain* domain, const uint64_t* const* polys, const uint64_t* lens, uint64_t count,
                          uint64_t* evaluations /* count x n x 4 */, uint8_t* witnesses48 /* count x n x 48 */,
                          uint8_t* commitments48 /* count x 48, or NULL */);
int plonk_kzg_open_domain_dev(plonk_kzg_domain* domain, const void* const* polys_dev, const uint64_t* lens, uint64_t count,
                              void* evaluations_dev, void* witnesses48_dev, void* commitments48_dev /* or NULL */);
int plonk_kzg_domain_last(plonk_kzg_domain* domain, plonk_kzg_domain_info* out);

/* ---- KZG10 in evaluation form ---------------------------------------------------------------------------
 * Commitments and openings of polynomials given by their VALUES on the handle's domain — witness columns, a table, a blob,
 * the `evaluations` of plonk_kzg_open_domain — without the inverse transform and the second copy in coefficient form that
 * plonk_kzg_open needs.  n = 2^log_n, w the generator plonk_ntt uses for size n, e_j[i] = p_j(w^i), every vector exactly n
 * Montgomery Fr:
 *     commit_j = sum_i e_j[i] [L_i(tau)] G                          the 48 bytes of plonk_msm of plonk_ntt(inverse) of e_j
 *     y_j = (z^n - 1) / n * sum_i e_j[i] w^i / (z - w^i)            z outside the domain;   y_j = e_j[m]  for z = w^m
 *     F[i] = sum_j v^j e_j[i],  Y = sum_j v^j y_j                   (weight 1 for a single vector)
 *     q[i] = (F[i] - Y) / (w^i - z)  (w^i != z),   q[m] = -w^(-m) sum_(i != m) q[i] w^i    (the derivative, for z = w^m)
 *     witness = sum_i q[i] [L_i(tau)] G                             the 48 bytes plonk_kzg_open returns for the same z and v
 *   The point may be ANY canonical field element, a point of the domain included.  The denominators are shared by the vectors
 *   of a call and inverted once; every value crosses HBM once per call (fold contribution and evaluation partial in one
 *   pass).  Commitments and the witness are bucket MSMs over the n Lagrange points [L_i(tau)] G (96 bytes each), which the
 *   first call that commits builds from the commit key by one group transform and the handle keeps until it is destroyed: no
 *   tables, nothing of the context's table budget (plonk_ctx_table_bytes is unchanged), and neither plonk_kzg_domain_info
 *   nor plonk_kzg_domain_last counts them — plonk_kzg_evals_last does.  A key of exactly n points is enough.
 * plonk_kzg_commit_evals: commitments48[j] = commit_j, j < count (count x 48 bytes).  count == 0 is PLONK_OK and writes nothing.
 * plonk_kzg_open_evals: evaluations[j] = y_j (count x 4 limbs, Montgomery); commitments48[j] = commit_j (NULL skips them);
 *   witness48 as above.  witness48 == NULL evaluates only: no quotient and no MSM run (with commitments48 == NULL the
 *   Lagrange points are not even built).  count == 0 writes the compressed identity as the witness, as plonk_kzg_open does.
 *   The host form stages the vectors through the two upload buffers of plonk_kzg_open (max(n, 2^16) values each), group
 *   after group, so count x n is never resident.
 * The _dev forms: evals_dev is a HOST array of `count` device pointers on the context's GPU; the outputs stay host memory, as
 *   for plonk_kzg_open_dev.
 * PLONK_ERR_ARG for a NULL argument (domain, the array, one of its entries, point, evaluations; commitments48 of
 *   plonk_kzg_commit_evals), count > 65536, or v_challenge == NULL with count > 1; PLONK_ERR_DATA for a point, a challenge or
 *   a value that is not a canonical residue; PLONK_ERR_STATE once the context's key was reloaded, and on a context with a
 *   communicator.  Every check is made before anything is queued or written: an error leaves nothing queued and no output
 *   touched.  The calls leave the context, its tables and its provers as they found them; plonk_ctx_last_msm_points keeps
 *   describing the caller's own last call.
 * plonk_kzg_evals_last: what the last evaluation-form call on the handle ran as (count == 0 before the first): the tests
 *   assert it against the plan computed on the host (plonk_amd/csrc/kzg_evals_core.hpp). */
typedef struct plonk_kzg_evals_info {
  uint32_t log_n;
  uint32_t built_points;           /* 1: this call built the Lagrange points */
  uint64_t count;                  /* vectors of the last call */
  uint64_t in_domain_index;        /* m with point == w^m, all ones when the point is outside the domain (or the call had no point) */
  uint64_t msm_launches;           /* bucket MSMs the call ran: one per commitment, one for the witness */
  uint64_t msm_terms;              /* terms of each: n */
  uint64_t lagrange_bytes;         /* bytes of the Lagrange points the handle holds: 96 n once built */
} plonk_kzg_evals_info;
int plonk_kzg_commit_evals(plonk_kzg_domain* domain, const uint64_t* const* evals, uint64_t count, uint8_t* commitments48 /* count x 48 */);
int plonk_kzg_commit_evals_dev(plonk_kzg_domain* domain, const void* const* evals_dev, uint64_t count, uint8_t* commitments48);
int plonk_kzg_open_evals(plonk_kzg_domain* domain, const uint64_t* const* evals, uint64_t count, const uint64_t point[4],
                         const uint64_t* v_challenge /* 4 limbs; may be NULL when count <= 1 */, uint64_t* evaluations /* count x 4 */,
                         uint8_t* commitments48 /* count x 48, or NULL */, uint8_t* witness48 /* 48, or NULL */);
int plonk_kzg_open_evals_dev(plonk_kzg_domain* domain, const void* const* evals_dev, uint64_t count, const uint64_t point[4],
                             const uint64_t* v_challenge, uint64_t* evaluations, uint8_t* commitments48, uint8_t* witness48);
int plonk_kzg_evals_last(plonk_kzg_domain* domain, plonk_kzg_evals_info* out);

/* ---- Lagrange-basis tables on a domain handle (opt-in) -----------------------------------------------------
 * By default the commitments and witnesses of the evaluation-form calls and of plonk_kzg_multiproof_open are table-free
 * bucket MSMs over the handle's Lagrange points.  plonk_kzg_evals_tables_build gives the handle the table rows a prover's
 * Lagrange-basis key has (the layout the context's rule gives a key that is built last; a forced table_mode forces it here
 * too): from then on those calls run the prover's grouped table MSM, four commitments per launch, and return the same bytes.
 * A call whose MSMs fit one group is finished on the host; a call with more queues all its groups and finishes and
 * compresses their commitments on the device, up to 4096 per kernel launch.
 * plonk_kzg_evals_tables_build: builds the Lagrange points if no call has yet, then the tables.  rows x n x 128 bytes count
 *   against the context's table budget and show in plonk_ctx_table_bytes while the handle holds them: the documented
 *   exception to "leaves the context as found".  A second call is PLONK_OK with built == 0.  PLONK_ERR_ARG for NULL or when
 *   rows x n exceeds 2^31; PLONK_ERR_STATE once the context's key was reloaded, and on a context with a communicator.  A
 *   failed build leaves the handle without tables and the budget as it was.
 * plonk_kzg_evals_tables_drop: frees them (PLONK_OK when the handle holds none; works after a key reload);
 *   plonk_kzg_domain_destroy drops them too.
 * plonk_kzg_evals_tables_last: the tables the handle holds and how the last call that used them ran: the tests assert it
 *   against the plan computed on the host (kze_tables_plan, plonk_amd/csrc/kzg_evals_core.hpp).  plonk_kzg_evals_last and
 *   plonk_kzg_multiproof_last keep every field and meaning with tables present. */
typedef struct plonk_kzg_evals_tables_info {
  uint32_t log_n;
  uint32_t table_rows;        /* 0: the handle holds no tables; else 16 / 64 / 128 / 256 */
  uint64_t table_bytes;       /* rows x n x 128, counted in plonk_ctx_table_bytes while held */
  uint32_t built;             /* 1: the last plonk_kzg_evals_tables_build call built them (0: they were there) */
  uint32_t bucket_bits;       /* of the last table MSM on the handle (0 before the first) */
  uint64_t msms;              /* last call that used the tables: commitments + witness / D / pi computed */
  uint64_t group_launches;    /* grouped table MSM launches it made */
  uint32_t device_finished;   /* 1: its commitments were finished and compressed on the device */
  uint32_t reserved;
} plonk_kzg_evals_tables_info;
int plonk_kzg_evals_tables_build(plonk_kzg_domain* domain);
int plonk_kzg_evals_tables_drop(plonk_kzg_domain* domain);
int plonk_kzg_evals_tables_last(plonk_kzg_domain* domain, plonk_kzg_evals_tables_info* out);

/* ---- commitments of MANY SHORT vectors on a domain handle (opt-in window tables) ----------------------------
 * Building or updating a vector-commitment tree means committing to very many short vectors (2^8 values: a tree node).  The
 * MSM routes above pay a bucket sort and a reduction tail per commitment; for a short FIXED base neither is needed.  The
 * handle is given window tables over its Lagrange points L_i = [L_i(tau)] G, n = 2^log_n <= 2^12: for a digit width c
 * (window_bits) every value s < q is written in W(c) signed digits, s = sum_w d_w 2^(c w), d_w in [-2^(c-1), 2^(c-1)]
 * (W = 128, 86, 64, 52, 43, 37, 32 for c = 2 .. 8: the smallest count for which no scalar below q carries out), and the
 * tables hold every affine point [d 2^(c w)] L_i, d = 1 .. 2^(c-1): n x W x 2^(c-1) entries of 128 bytes (128 MiB for n = 2^8,
 * c = 8).  One wave then owns a vector and adds its n x W table entries: mixed additions only, no doublings, no buckets.
 *     commitments48[j] = sum_i values[j][i] L_i            the same 48 bytes plonk_kzg_commit_evals gives for that vector
 *     update:   out_j = base_j + sum_(k in [offsets[j], offsets[j+1])) deltas[k] L_(index[k])
 * plonk_kzg_many_tables_build: builds the Lagrange points if no call has yet, then the tables for window_bits = 2 .. 8; 0
 *   picks the widest width whose tables fit what is left of the context's table budget.  The bytes count against that budget
 *   and show in plonk_ctx_table_bytes while held, as for plonk_kzg_evals_tables_build; they are returned by
 *   plonk_kzg_many_tables_drop and plonk_kzg_domain_destroy.  A second build with the width the handle holds is PLONK_OK with
 *   built == 0; another width replaces the tables: the new ones are built beside the old, which a failed build keeps, so both
 *   must fit the budget for that moment (PLONK_ERR_ARG otherwise: drop the old ones first).  A Lagrange point that is the identity (tau in the domain) gets entries of
 *   128 zero bytes, which the accumulation skips.  PLONK_ERR_ARG for NULL, log_n > 12, window_bits outside {0, 2 .. 8}, and
 *   for tables that do not fit what is left of the budget (window_bits == 0: no width fits); PLONK_ERR_STATE once the
 *   context's key was reloaded, and on a context with a communicator.  A refused or failed build leaves the handle and the
 *   budget as they were.
 * plonk_kzg_many_tables_drop: frees them (PLONK_OK when the handle holds none; works after a key reload).
 * plonk_kzg_commit_many: `values` holds count x n Montgomery Fr, vector after vector; count <= 2^24; count == 0 is PLONK_OK
 *   and writes nothing.  The vectors are staged chunk by chunk through the two upload buffers of plonk_kzg_open, so count x n
 *   is never resident.
 * plonk_kzg_commit_many_dev: values_dev (16-byte aligned) and commitments48_dev (4-byte aligned) are DEVICE pointers on the
 *   context's GPU, as for plonk_kzg_open_domain_dev: the values are read in place, the count x 48 bytes written there.
 * plonk_kzg_update_many: the sparse form, count segments; index[k] < n; a repeated index inside a segment simply adds; an
 *   empty segment returns its base re-encoded; base48 == NULL means the identity for every segment (a sparse commit).  The
 *   identity (0xC0 00 ..) is a legal base.  count <= 2^24, offsets[count] <= 2^28, and one segment at most 2^16 terms (a
 *   segment is one wave's work; longer sums are split by the caller and chained through base48).  All arrays are host memory.
 * Errors of the three: PLONK_ERR_ARG for a NULL argument, a count, total or segment above its cap, offsets that do not start at 0 or
 *   decrease, an index >= n, a misaligned device pointer; PLONK_ERR_DATA for a value or delta that is not a canonical residue;
 *   PLONK_ERR_POINT for a base that does not decode or is not in the subgroup; PLONK_ERR_STATE when the handle holds no
 *   many-vector tables (there is no fallback: use plonk_kzg_commit_evals), once the context's key was reloaded, and on a
 *   context with a communicator.  Every check is made before anything of the call's result is queued or written: an error
 *   leaves the outputs untouched.  The calls leave the context, its other tables, its provers, plonk_ctx_last_msm and
 *   plonk_ctx_last_msm_points as they found them.
 * plonk_kzg_many_last: the tables the handle holds and how the last of these calls ran: the tests assert it against the plan
 *   computed on the host (plonk_amd/csrc/kzg_many_core.hpp). */
typedef struct plonk_kzg_many_info {
  uint32_t log_n;
  uint32_t window_bits;       /* 0: the handle holds no many-vector tables */
  uint32_t windows;           /* W(window_bits) */
  uint32_t built;             /* 1: the last plonk_kzg_many_tables_build call built them (0: they were there) */
  uint64_t table_bytes;       /* n x W x 2^(c-1) x 128, counted in plonk_ctx_table_bytes while held */
  uint64_t count;             /* last call: vectors (segments) */
  uint64_t terms;             /* values it added up: count x n, or offsets[count] */
  uint64_t chunks;            /* chunks it ran in, under the handle's workspace cap */
  uint64_t chunk_vectors;     /* vectors of a full chunk (sparse form: of the largest chunk) */
  uint32_t slices;            /* partial sums per vector: > 1 when the call had too few vectors to fill the device */
  uint32_t reserved;
  uint64_t additions;         /* the bound terms x W on its mixed additions (zero digits are not counted on the device) */
} plonk_kzg_many_info;
int plonk_kzg_many_tables_build(plonk_kzg_domain* domain, uint32_t window_bits /* 2..8, 0 = automatic */);
int plonk_kzg_many_tables_drop(plonk_kzg_domain* domain);
int plonk_kzg_commit_many(plonk_kzg_domain* domain, const uint64_t* values /* count x n x 4, contiguous */, uint64_t count,
                          uint8_t* commitments48 /* count x 48 */);
int plonk_kzg_commit_many_dev(plonk_kzg_domain* domain, const void* values_dev, uint64_t count, void* commitments48_dev);
int plonk_kzg_update_many(plonk_kzg_domain* domain, const uint8_t* base48 /* count x 48, or NULL */, const uint64_t* offsets /* count + 1 */,
                          const uint32_t* index, const uint64_t* deltas /* offsets[count] x 4 */, uint64_t count, uint8_t* commitments48);
int plonk_kzg_many_last(plonk_kzg_domain* domain, plonk_kzg_many_info* out);

/* ---- KZG10 vector-commitment trees: build, update, prove on the device --------------------------------------
 * A dense n-ary tree of KZG commitments over a domain handle that holds many-vector tables, n = 2^log_n <= 2^12, depth D >= 1,
 * D x log_n <= 26.  Level l (0 = the root) has n^l nodes; the tree keeps ALL levels resident:
 *     vals[l]    one flat array of n^(l+1) Montgomery Fr; vals[D-1] holds the N = n^D leaves
 *     C[l][k]  = sum_i vals[l][k n + i] L_i              the 48 bytes plonk_kzg_commit_evals gives for that vector
 *     vals[l][j] = h(C[l+1][j])   for l < D-1            the flat index of a child is its slot in the parent level
 *     h(c48)   = Transcript::new("kzg10-tree-v1"); append_message("node", c48); challenge_scalar("node-scalar")
 *   (Merlin, a 64-byte wide reduction; the identity 0xC0 00 .. is hashed like any other 48 bytes).  Per node the tree also keeps
 *   the 48 bytes and the decoded affine point with its identity flag, so an update never decodes or subgroup-checks a node.
 *   These bytes are data, not tables: they are not counted against the table budget; plonk_kzg_tree_last reports them.
 * plonk_kzg_tree_create: PLONK_ERR_ARG for NULL, depth == 0, log_n > 12 or depth x log_n > 26; PLONK_ERR_STATE on a context
 *   with a communicator or once its key was reloaded, as for every call below that takes the tree.  The tree is EMPTY.  A tree
 *   is destroyed before its domain.
 * plonk_kzg_tree_build (leaves: N x 4 limbs, host) / _build_dev (leaves_dev: 16-byte aligned device pointer): the host form
 *   stages the leaves through the two upload buffers of plonk_kzg_open into vals[D-1], the _dev form copies them there.  Then
 *   per level, bottom up, on the stream with no host round trip: the accumulation of plonk_kzg_commit_many (chunked under the
 *   handle's workspace cap), a finish kernel (point, flag, 48 bytes) and the map h into the level above.  PLONK_ERR_ARG for a
 *   NULL or misaligned pointer, PLONK_ERR_DATA for a leaf >= q, PLONK_ERR_STATE when the domain holds no many-vector tables
 *   (their window width may differ from the last build's).  A failed or refused build leaves the tree EMPTY: every call but
 *   build, destroy and plonk_kzg_tree_last (built == 0) then returns PLONK_ERR_STATE.
 * plonk_kzg_tree_root / _nodes: 48 bytes per node; PLONK_ERR_ARG for a level >= D or first + count beyond the level.
 * plonk_kzg_tree_update: leaf leaf_index[k] becomes values[k], k < count.  Every check comes before anything is changed, in
 *   this order: PLONK_ERR_ARG (NULL, count == 0 or > 2^20, an index >= N, a REPEATED index), PLONK_ERR_DATA (a value >= q),
 *   PLONK_ERR_STATE (an empty tree, no many-vector tables).  The touched nodes of all levels, their segments and child indices
 *   are computed once on the host and uploaded once; then per level, bottom up: delta = new - old with the store of the new
 *   value, the sparse accumulation of plonk_kzg_update_many over (child index, delta), the finish kernel with the stored point
 *   as base, the map, and the delta of the parent's value.  Afterwards every stored byte equals a build from the new leaves.
 * plonk_kzg_tree_proof_nodes: host only: the number of path commitments a proof of these leaves carries.
 * plonk_kzg_tree_prove: with T_D the sorted distinct leaf indices and T_l = { j / n : j in T_(l+1) }, the multiproof's vectors
 *   are the nodes of T_0 (the root), T_1, .., T_(D-1), each ascending; its items are, per level l in that order, the flat
 *   indices of T_(l+1) as (node j / n, point j mod n); path48 holds the commitments of T_1 .. T_(D-1) in that order — the
 *   items of level l < D-1 are one to one with the path commitments of level l + 1 and their values are h of those.
 *   values[k] is the leaf leaf_index[k] (the caller's order).  The vectors are read where the tree holds them; the transcript
 *   of plonk_kzg_multiproof_open is used unchanged under the caller's label, and so are its Lagrange-basis tables.
 *   PLONK_ERR_ARG for NULL, count == 0, a repeated or out-of-range index, more than 65536 distinct nodes or 2^20 items;
 *   PLONK_ERR_DATA / PLONK_ERR_STATE as plonk_kzg_multiproof_open_dev.  An error leaves the outputs untouched.
 * plonk_kzg_tree_check: needs no tree and no domain.  Rebuilds the items from the indices, computes the inner values with h
 *   on the host and calls plonk_kzg_multiproof_check on root48 || path48: PLONK_ERR_ARG also for `nodes` other than what the
 *   indices imply; otherwise PLONK_ERR_ARG, _DATA, _POINT, PLONK_OK or PLONK_ERR_VERIFY as that call.
 * plonk_kzg_tree_last: the tree and how its last build / update / prove ran; the tests assert it against the plan computed
 *   on the host (plonk_amd/csrc/kzg_tree_core.hpp).
 * The tree calls leave the context, its tables and budget, plonk_ctx_last_msm and plonk_kzg_many_last as they found them;
 * plonk_kzg_tree_prove runs the MSMs plonk_kzg_multiproof_open documents. */
typedef struct plonk_kzg_tree plonk_kzg_tree;
typedef struct plonk_kzg_tree_info {
  uint32_t log_n, depth;
  uint32_t built;             /* 0: the tree is EMPTY */
  uint32_t kind;              /* the last call that ran: 0 none, 1 build, 2 update, 3 prove */
  uint64_t leaves;            /* N = n^depth */
  uint64_t device_bytes;      /* the values, bytes, points and flags of all levels, and the tree's workspace */
  uint64_t touched_nodes;     /* nodes it committed (build: all; update: |T_0| + .. + |T_(D-1)|) or opened (prove) */
  uint64_t sparse_terms;      /* update: |T_1| + .. + |T_D| */
  uint64_t chunks;            /* accumulation launches of a build or an update */
  uint64_t items, vectors;    /* prove: K and M of the multiproof */
} plonk_kzg_tree_info;
int plonk_kzg_tree_create(plonk_kzg_domain* domain, uint32_t depth, plonk_kzg_tree** out);
void plonk_kzg_tree_destroy(plonk_kzg_tree* tree);
int plonk_kzg_tree_build(plonk_kzg_tree* tree, const uint64_t* leaves /* N x 4 */);
int plonk_kzg_tree_build_dev(plonk_kzg_tree* tree, const void* leaves_dev);
int plonk_kzg_tree_root(plonk_kzg_tree* tree, uint8_t out48[48]);
int plonk_kzg_tree_nodes(plonk_kzg_tree* tree, uint32_t level, uint64_t first, uint64_t count, uint8_t* out48 /* count x 48 */);
int plonk_kzg_tree_update(plonk_kzg_tree* tree, const uint64_t* leaf_index, const uint64_t* values /* count x 4 */, uint64_t count);
int plonk_kzg_tree_proof_nodes(uint32_t log_n, uint32_t depth, const uint64_t* leaf_index, uint64_t count, uint64_t* nodes);
int plonk_kzg_tree_prove(plonk_kzg_tree* tree, const uint64_t* leaf_index, uint64_t count, const uint8_t* label, uint64_t label_len,
                         const uint64_t* challenges_override /* 8 limbs or NULL */, uint64_t* values /* count x 4 out */,
                         uint8_t* path48 /* nodes x 48 out */, uint8_t proof96[96]);
int plonk_kzg_tree_check(plonk_kzg_key* key, uint32_t log_n, uint32_t depth, const uint8_t root48[48], const uint64_t* leaf_index,
                         const uint64_t* values /* count x 4 */, uint64_t count, const uint8_t* path48, uint64_t nodes,
                         const uint8_t proof96[96], const uint8_t* label, uint64_t label_len, const uint64_t* challenges_override,
                         plonk_verify_info* info /* may be NULL */);
int plonk_kzg_tree_last(plonk_kzg_tree* tree, plonk_kzg_tree_info* out);

/* ---- KZG10 cell proofs: a polynomial opened on every coset of its domain --------------------------------
 * The n = 2^log_n evaluations of a polynomial cut into r = n / l cells of l = 2^log_cell values, each cell with ONE 48-byte
 * proof that opens all l of its values at once (Feist-Khovratovich section 3; data-availability sampling).  w is the generator
 * plonk_ntt uses for size n, phi = w^l, s_i = [tau^i] g the commit key, f_0 .. f_(n-1) the zero-padded coefficients:
 *     cell k (k < r) = the coset { w^(k + r j) : j < l }, with vanishing polynomial X^l - x_k,  x_k = phi^k = w^(l k)
 *     cells[k l + j] = f(w^(k + r j))        cell-major: the forward NTT of f read as an l x r matrix and transposed
 *     proofs[k] = commit(q_k),  f = q_k (X^l - x_k) + r_k,  deg r_k < l
 *     r_k has the coefficients c_j = sum_t f_(j + t l) x_k^t = w^(-k j) * (the size-l inverse NTT of cell k's values)_j
 *   computed as proofs = DFT_r(H), H_m = sum_j f_(j + (m+1) l) s_j, the sum over u < l of the Toeplitz products of
 *   plonk_kzg_open_domain at size r:  A^(u) = DFT_2r(s_u, s_(u+l) .. s_(u+l(r-2)), O ...) (per handle and cell size);
 *   G^(u) = NTT_2r(f_(u+l(r-1)) .. f_(u+l), 0 ...);  P_i = sum_u [G^(u)_i / 2r] A^(u)_i;  c = DFT_2r^-1(P);
 *   H_m = c_(r-2-m) (m <= r-2), H_(r-1) = O                                                          
 *   A VERIFIER checks cell k with  e(proofs[k], [tau^l] h) == e(C - commit(r_k) + x_k proofs[k], h):  with an opening key whose
 *   third element is [tau^l] h instead of [tau] h that is plonk_kzg_pairing_check_each(key_l, A = proofs[k],
 *   B = C - commit(r_k) + x_k proofs[k]), C the commitment and r_k from the cell's values by the formula above.
 *   plonk_kzg_verify_cells / plonk_kzg_verify_cells_each (below) do all of this on the device.
 * plonk_kzg_open_cells: `count` polynomials in coefficient form (host pointers; lengths may differ).  cells: count x n x 4
 *   limbs, Montgomery, cell-major; proofs48: count x r x 48 bytes, compressed G1, encoded on the device; commitments48:
 *   count x 48 through the ordinary commitment path, NULL skips them.  A polynomial of fewer than l + 1 coefficients has r
 *   compressed identities as proofs (and c_j = f_j).  Checks, in this order: PLONK_ERR_ARG for a NULL domain, log_cell
 *   outside [1, log_n - 1] (so a handle of log_n = 1 has no cell size), count > 65536, a NULL polys / lens / cells / proofs48
 *   with count > 0, polys[i] NULL with lens[i] > 0; PLONK_ERR_STATE once the context's key was reloaded, and on a context
 *   with a communicator; count == 0 is PLONK_OK and writes nothing; lengths are judged WITHOUT trailing zeros: a coefficient
 *   that is not a canonical residue is PLONK_ERR_DATA, then more than n coefficients is PLONK_ERR_DEGREE.  Every check is
 *   made before anything is queued or written: an error leaves nothing queued and none of the three outputs touched.
 *   The first call with a cell size builds its A^(u) (2n slots of 256 bytes) and the handle keeps them until it is destroyed;
 *   the point workspace (S x 2r slots per polynomial of a chunk, S the slice count of the accumulate) stays under the
 *   handle's workspace cap, chunked as plonk_kzg_open_domain chunks.  Neither plonk_kzg_domain_info nor
 *   plonk_kzg_domain_last counts any of this memory; plonk_kzg_cells_last does.  The calls leave the context, its tables,
 *   its provers and the handle's other entry points as they found them.
 * plonk_kzg_open_cells_dev: polys_dev is a HOST array of `count` device pointers; the three outputs are device pointers on
 *   the context's GPU.
 * plonk_kzg_cell_points: x[k] = x_k = w^(l k) and shift[k] = w^k (NULL skips it), k < r, Montgomery: cell k is shift[k] times
 *   the size-l subgroup.  PLONK_ERR_ARG / PLONK_ERR_STATE as above.
 * plonk_kzg_cells_last: what the last plonk_kzg_open_cells call on the handle ran as (count == 0 before the first): the
 *   tests assert it against the plan computed on the host (plonk_amd/csrc/kzg_cells_core.hpp). */
typedef struct plonk_kzg_cells_info {
  uint32_t log_n;
  uint32_t log_cell;               /* cell size of the last call */
  uint32_t chunks;                 /* chunks the polynomials of the last call were processed in */
  uint32_t built_table;            /* 1: this call built the A^(u) of its cell size */
  uint64_t count;                  /* polynomials of the last call */
  uint64_t slices;                 /* S: lanes per position of the accumulate, each with l / S terms */
  uint64_t chunk_polys;            /* polynomials per chunk (the last chunk may be shorter) */
  uint64_t workspace_bytes;        /* point workspace of the call: S x 2r slots per polynomial of a chunk */
  uint64_t table_bytes;            /* bytes of all A^(u) tables the handle holds: 2n x 256 per cell size used */
  uint64_t stage_launches;         /* group-FFT stage launches: (2 log r + 1) per chunk */
  uint64_t scalar_muls;            /* full-width scalar multiplications issued: 2n in the accumulate + the butterflies whose twiddle is not 1 */
} plonk_kzg_cells_info;
int plonk_kzg_open_cells(plonk_kzg_domain* domain, uint32_t log_cell, const uint64_t* const* polys, const uint64_t* lens, uint64_t count,
                         uint64_t* cells /* count x n x 4, cell-major, Montgomery */, uint8_t* proofs48 /* count x r x 48 */,
                         uint8_t* commitments48 /* count x 48, or NULL */);
int plonk_kzg_open_cells_dev(plonk_kzg_domain* domain, uint32_t log_cell, const void* const* polys_dev, const uint64_t* lens, uint64_t count,
                             void* cells_dev, void* proofs48_dev, void* commitments48_dev /* or NULL */);
int plonk_kzg_cell_points(plonk_kzg_domain* domain, uint32_t log_cell, uint64_t* x /* r x 4: w^(l k) */, uint64_t* shift /* r x 4: w^k, or NULL */);
int plonk_kzg_cells_last(plonk_kzg_domain* domain, plonk_kzg_cells_info* out);

/* ---- KZG10 cell verification: a folded batch check and per-cell verdicts --------------------------------
 * The checking side of plonk_kzg_open_cells.  Items i < count each name a commitment c_i < ncommitments and a cell k_i < r and
 * bring the cell's l values v_i and its proof pi_i.  With c_ij = w^(-k_i j) * (the size-l inverse NTT of v_i)_j, the
 * coefficients of the remainder r_i, and weights rho^i (item 0 has weight 1):
 *     L   = sum_i rho^i pi_i
 *     Rhs = sum_c (sum_(i : c_i = c) rho^i) C_c + sum_i (rho^i x_(k_i)) pi_i - sum_(j < l) (sum_i rho^i c_ij) s_j
 *     accept iff e(L, [tau^l] h) == e(Rhs, h)
 *   and per item, weight 1:  e(pi_i, [tau^l] h) == e(C_(c_i) + x_(k_i) pi_i - sum_j c_ij s_j, h)   (DESIGN.md section 17).
 * plonk_kzg_cell_verifier_create: key_l is a plonk_kzg_key whose third element is [tau^l] h (NOT the ordinary opening key's
 *   [tau] h); log_n in [2, 20]; log_cell in [1, min(log_n - 1, 11)]: a cell is transformed by ONE workgroup in LDS, larger
 *   cells are out of scope.  The handle COPIES the first l points of the context's commit key into device memory of its own
 *   and builds x_k and w^(-k) (k < r) and the l / 2 inverse twiddles there: l points and 2r + l / 2 scalars, none of the
 *   tables of a plonk_kzg_domain.  Reloading the context's commit key afterwards does not affect the verifier.  Errors, in
 *   this order: PLONK_ERR_ARG (a NULL pointer, a size outside the ranges above); PLONK_ERR_STATE for a context with a
 *   communicator; PLONK_ERR_NO_SRS; PLONK_ERR_DEGREE for a commit key of fewer than l points; PLONK_ERR_VERIFY when s_0 is not
 *   the key's g; PLONK_ERR_VERIFY when e(s_l, h) != e(s_0, x_h) — one host pairing, made only when the commit key has more
 *   than l points (it catches an ordinary opening key passed by mistake); with exactly l points the check cannot be made and
 *   plonk_kzg_cell_verifier_last reports key_checked = 0.  Destroy the verifier before its key, the key before its context.
 * plonk_kzg_verify_cells: the folded check: one call, two MSM launches (plonk_msm_points' kernels, per-term or buckets by its
 *   own rule), ONE pairing on the host whatever count is; no bisection, as plonk_kzg_batch_check.  PLONK_OK when the batch
 *   verifies; PLONK_ERR_VERIFY for a failing batch and for count == 0.  Checks, in this order: PLONK_ERR_ARG (a NULL
 *   argument, an index >= ncommitments or >= r, count > 2^20, count * l > 2^25, ncommitments > 65536); PLONK_ERR_DATA (a
 *   value or rho_override that is not a canonical residue); PLONK_ERR_POINT (a commitment or proof that does not decode or is
 *   outside the subgroup; the compressed identity is legal); then the pairing.  An error leaves nothing queued.
 *   rho: with rho_override == NULL it is drawn from a fresh Merlin transcript Transcript::new(label): "dom-sep" =
 *   "kzg10-cell-batch-check-v1"; u64 "log-n", "log-cell", "commitments", "items"; "opening-key" = the key's 240 bytes;
 *   "commitment" per commitment; per item u64 "commitment-index", u64 "cell-index", "cell" = its l x 32 canonical
 *   little-endian bytes, "cell-proof"; challenge_scalar("cell-batch-challenge").  The transcript runs on the host over
 *   count x l x 32 bytes (info->ms_scalars shows its cost).  rho_override replaces it — for a caller whose own transcript
 *   already binds all of the above.  A rho the prover could predict VOIDS the check (errors of two items can be made to
 *   cancel); with an unpredictable rho a batch with a false item passes with probability at most count / q.
 * plonk_kzg_verify_cells_each: exact per-item verdicts, one device pairing per item (the kernels of
 *   plonk_kzg_pairing_check_each): verdicts[i] = PLONK_OK, PLONK_ERR_VERIFY, PLONK_ERR_DATA (one of its values is not
 *   canonical) or PLONK_ERR_POINT (its proof or the commitment it names); a malformed item never stops the others, and
 *   verdicts[i] is what the folded call returns for that item alone.  Returns PLONK_OK when every verdict is, PLONK_ERR_VERIFY
 *   when at least one is not (as plonk_kzg_check_each), PLONK_ERR_ARG as above (and for count == 0) with verdicts untouched.
 * plonk_verify_info (may be NULL) is filled as plonk_kzg_batch_check / plonk_kzg_check_each fill it: proofs = count;
 *   msm_terms = 2 count + ncommitments + l (folded) or l + 2 per checked item (each).
 * plonk_kzg_cell_verifier_last: what the last call on the handle ran as; the tests assert it against the plan computed on the
 *   host (plonk_amd/csrc/kzg_cell_verify_core.hpp).  The calls leave the context, its commit key, tables, provers and
 *   plonk_ctx_last_msm_points as they found them; the workspaces belong to the handle, only grow, and go with it. */
typedef struct plonk_kzg_cell_verifier plonk_kzg_cell_verifier;
typedef struct plonk_kzg_cell_verify_info {
  uint32_t log_n;
  uint32_t log_cell;
  uint32_t key_checked;            /* 1: e(s_l, h) == e(s_0, x_h) was checked at creation */
  uint32_t path_each;              /* 1: the last call was plonk_kzg_verify_cells_each */
  uint64_t items;                  /* of the last call (0 before the first) */
  uint64_t commitments;
  uint64_t transforms;             /* size-l inverse transforms: one per item */
  uint64_t msm_terms_left;         /* folded: count */
  uint64_t msm_terms_right;        /* folded: ncommitments + count + l */
  uint32_t msm_path_left;          /* 0 per-term kernel, 1 buckets */
  uint32_t msm_path_right;
  uint64_t scalar_muls;            /* each: count x (l + 1) full-width scalar multiplications */
  uint64_t device_bytes;           /* everything the handle holds on the device */
} plonk_kzg_cell_verify_info;
int plonk_kzg_cell_verifier_create(plonk_kzg_key* key_l, uint32_t log_n, uint32_t log_cell, plonk_kzg_cell_verifier** out);
void plonk_kzg_cell_verifier_destroy(plonk_kzg_cell_verifier* v);
int plonk_kzg_verify_cells(plonk_kzg_cell_verifier* v, const uint8_t* commitments48 /* M x 48 */, uint64_t ncommitments,
                           const uint32_t* commitment_index /* count */, const uint32_t* cell_index /* count */,
                           const uint64_t* values /* count x l x 4, Montgomery */, const uint8_t* proofs48 /* count x 48 */, uint64_t count,
                           const uint8_t* label, uint64_t label_len, const uint64_t* rho_override /* 4 limbs or NULL */,
                           plonk_verify_info* info /* may be NULL */);
int plonk_kzg_verify_cells_each(plonk_kzg_cell_verifier* v, const uint8_t* commitments48, uint64_t ncommitments,
                                const uint32_t* commitment_index, const uint32_t* cell_index, const uint64_t* values,
                                const uint8_t* proofs48, uint64_t count, int32_t* verdicts /* count */, plonk_verify_info* info);
int plonk_kzg_cell_verifier_last(plonk_kzg_cell_verifier* v, plonk_kzg_cell_verify_info* out);

/* ---- KZG10 cell recovery: a polynomial rebuilt from a subset of its cells --------------------------------
 * The third part of data-availability sampling next to plonk_kzg_open_cells and plonk_kzg_verify_cells: from `available`
 * distinct cells of a polynomial of at most max_len coefficients (max_len <= available x l) the call rebuilds the
 * coefficients, all r cells, their proofs and the commitment.  Notation as above; M = the r - available missing cells:
 *     Z(X) = Z_r(X^l),  Z_r(Y) = prod_(m in M) (Y - phi^m)     Z(w^(k + r j)) = Z_r(phi^k),  Z(7 w^i) = Z_r(7^l phi^(i mod r))
 *     E = the values, 0 in missing cells;  P = f Z = NTT^-1(E Z) exactly (deg < max_len + l |M| <= n)
 *     f = coset-NTT^-1( coset-NTT(P)_i / Z_r(7^l phi^(i mod r)) )       (7 the generator of plonk_ntt's coset; 7^n != 1)
 *   The values are consistent with a polynomial of at most max_len coefficients iff the result is zero from index max_len on;
 *   with max_len < available x l a single changed value is always detected, with max_len == available x l there is no
 *   redundancy and every input is consistent (the call returns the interpolant).                       
 * plonk_kzg_recover_cells: all `count` polynomials share ONE set of cells (rows of a blob matrix that lost the same columns):
 *   cell_ids: `available` distinct indexes < r in any order; values[b]: available x l x 4 limbs, Montgomery, the cells in the
 *   order of cell_ids, each cell as plonk_kzg_open_cells writes it.  Outputs, each may be NULL but not all four: coeffs (count
 *   x n x 4, zero above the polynomial), cells (count x n x 4, cell-major), proofs48 (count x r x 48) and commitments48
 *   (count x 48): byte for byte what plonk_kzg_open_cells returns for the recovered polynomial (proofs and commitments come
 *   through its code).  status (count entries, may be NULL): PLONK_OK or PLONK_ERR_VERIFY per polynomial.
 *   Checks, in this order, every one before anything is queued or written: PLONK_ERR_ARG (a NULL domain; log_cell outside
 *   [1, log_n - 1]; log_n - log_cell > 11, that is r > 2048 — Z_r is evaluated by direct products, 2r |M| multiplications,
 *   and a product tree for larger r is not built; count > 65536; available == 0 or > r; a cell index >= r or repeated; NULL
 *   cell_ids or values, or values[b] NULL, with count > 0; max_len == 0 or > n; all four outputs NULL); PLONK_ERR_STATE
 *   exactly where plonk_kzg_open_cells returns it; count == 0 is PLONK_OK and writes nothing; PLONK_ERR_DEGREE for max_len >
 *   available x l; PLONK_ERR_DATA for a value that is not a canonical residue; PLONK_ERR_VERIFY when any polynomial is
 *   inconsistent: the verdict is read back with one synchronisation before any output is written, status is filled, and the
 *   four outputs stay untouched (all or nothing).  On success status is all PLONK_OK.
 *   The workspace (3 arrays of n values per polynomial of a chunk) stays under the handle's workspace cap, chunked as
 *   plonk_kzg_open_domain chunks; a call of several chunks computes the coefficients twice, before and after the verdict.
 *   With proofs48 == NULL the call leaves plonk_kzg_cells_last as it was; with proofs48 set it runs plonk_kzg_open_cells'
 *   body (and may build its A^(u) tables: built_table).  The context, its tables and the handle's other entry points are
 *   left as found.
 * plonk_kzg_recover_cells_dev: values_dev is a HOST array of `count` device pointers, the four outputs are device pointers
 *   on the context's GPU; cell_ids and status stay host memory.
 * plonk_kzg_recover_last: what the last plonk_kzg_recover_cells call on the handle ran as (count == 0 before the first): the
 *   tests assert it against the plan computed on the host (plonk_amd/csrc/kzg_recover_core.hpp). */
typedef struct plonk_kzg_recover_info {
  uint32_t log_n;
  uint32_t log_cell;               /* cell size of the last call */
  uint32_t chunks;                 /* chunks the polynomials of the last call were processed in */
  uint32_t built_table;            /* 1: this call made plonk_kzg_open_cells' body build the A^(u) of its cell size */
  uint64_t count;                  /* polynomials of the last call */
  uint64_t available;              /* cells given */
  uint64_t missing;                /* r - available */
  uint64_t max_len;
  uint64_t chunk_polys;            /* polynomials per chunk (the last chunk may be shorter) */
  uint64_t transforms;             /* size-n transforms issued: 3 per polynomial (6 in a call of several chunks), + 1 for cell values */
  uint64_t vanish_muls;            /* 2r x missing */
  uint64_t workspace_bytes;        /* 3 x n x 32 per polynomial of a chunk */
  uint64_t inconsistent;           /* polynomials whose values fit no polynomial of max_len coefficients */
} plonk_kzg_recover_info;
int plonk_kzg_recover_cells(plonk_kzg_domain* domain, uint32_t log_cell, const uint32_t* cell_ids, uint64_t available,
                            const uint64_t* const* values, uint64_t count, uint64_t max_len, uint64_t* coeffs /* count x n x 4, or NULL */,
                            uint64_t* cells /* count x n x 4, cell-major, or NULL */, uint8_t* proofs48 /* count x r x 48, or NULL */,
                            uint8_t* commitments48 /* count x 48, or NULL */, int32_t* status /* count, or NULL */);
int plonk_kzg_recover_cells_dev(plonk_kzg_domain* domain, uint32_t log_cell, const uint32_t* cell_ids, uint64_t available,
                                const void* const* values_dev, uint64_t count, uint64_t max_len, void* coeffs_dev, void* cells_dev,
                                void* proofs48_dev, void* commitments48_dev, int32_t* status);
int plonk_kzg_recover_last(plonk_kzg_domain* domain, plonk_kzg_recover_info* out);

/* ---- KZG10 multiproofs: many evaluation-form openings, one 96-byte proof -----------------------------------
 * K claims "vector j_k has the value y_k at index m_k" over M committed vectors of n = 2^log_n values (e_j[i] = p_j(w^i), C_j
 * their commitments as plonk_kzg_commit_evals makes them) behind one proof of 96 bytes, whatever K is — the multiproof by
 * random evaluation.  Item k has the weight r^k:
 *     g(X) = sum_k r^k (p_(j_k)(X) - y_k) / (X - w^(m_k))      D = commit(g)                          (degree <= n - 2)
 *     s_j  = sum_(k : j_k = j) r^k / (t - w^(m_k))             h = sum_j s_j e_j                       (t outside the domain)
 *     y    = sum_k r^k y_k / (t - w^(m_k))   = h(t) - g(t)     pi = commit(((h - g)[i] - y) / (w^i - t))
 *     proof96 = D || pi;    accept iff e(pi, [tau] h) == e(sum_j s_j C_j - D - [y] g + t pi, h)        
 *   Everything stays in evaluation form: the quotients are aggregated per distinct point index with the derivative entry of
 *   plonk_kzg_open_evals, K n field products in all; D and pi are two MSMs of n terms over the handle's Lagrange points (built
 *   by whichever evaluation-form call of the handle commits first, shared with plonk_kzg_commit_evals / plonk_kzg_open_evals).
 * Challenges: a fresh Merlin transcript Transcript::new(label), the same on both sides: "dom-sep" = "kzg10-multiproof-v1";
 *   u64 "log-n", "commitments" (M), "items" (K); "commitment" for each of the M commitments; per item, in the caller's order,
 *   u64 "vector-index", u64 "point-index" and "value" (32 canonical little-endian bytes); r = challenge_scalar("multiproof-r");
 *   then "multiproof-d" = D's 48 bytes; t = challenge_scalar("multiproof-t").  challenges_override: 8 limbs, r then t,
 *   Montgomery, replaces BOTH — for a caller whose own transcript binds all of the above.  A predictable r lets false claims
 *   cancel each other and a predictable t lets a prover fit g to it: either voids the check.
 * plonk_kzg_multiproof_open: evals[j]: n x 4 limbs, Montgomery; items k < count name vector_index[k] < nvectors and
 *   point_index[k] < n.  The prover reads y_k from the vectors itself (values: count x 4 limbs out), so a false claim cannot be
 *   made.  commitments_in (nvectors x 48): hashed as given, not decoded — a wrong commitment gives a proof that fails; NULL:
 *   computed as plonk_kzg_commit_evals computes them (nvectors more MSMs) and those are hashed.  commitments_out, if not NULL,
 *   receives whichever set was used.  Duplicate items, and vectors that no item names, are legal.  The host form uploads ALL
 *   nvectors vectors into a grow-only workspace of the handle (nvectors x n x 32 bytes, hence its cap); the _dev form reads
 *   them where they are and has no such cap.
 *   Checks, in this order, every one before anything is queued or written; an error leaves nothing queued and no output
 *   touched: PLONK_ERR_ARG (a NULL required pointer — domain, evals, evals[j], both index arrays, values, proof96, label with
 *   label_len > 0; count == 0 or > 2^20; nvectors == 0 or > 65536; an index >= nvectors or >= n; host form only: nvectors x n
 *   > 2^28); PLONK_ERR_DATA (an override that is not canonical or whose t has t^n == 1; a value of a vector that is not a
 *   canonical residue — the _dev form finds that by a scan on the device, after the state checks, still before any output is
 *   written); PLONK_ERR_STATE (the domain's commit key was replaced on its context; the context has a communicator; a
 *   transcript-drawn t that lies in the domain: probability n / q, below 2^-234 — open again under another label; t exists
 *   only once D does, so this one check comes after the aggregation, still with no output written and nothing left queued).
 *   The call leaves the context, its tables, its provers, plonk_ctx_last_msm_points, plonk_kzg_domain_last and
 *   plonk_kzg_evals_last as it found them, except that plonk_kzg_evals_last.lagrange_bytes reports the shared Lagrange points
 *   once this call has built them.
 * plonk_kzg_multiproof_open_dev: evals_dev is a HOST array of nvectors device pointers; every other argument stays host memory.
 * plonk_kzg_multiproof_last: what the last plonk_kzg_multiproof_open call on the handle ran as (items == 0 before the first);
 *   the tests assert it against the plan computed on the host (plonk_amd/csrc/kzg_multiproof_core.hpp).
 * plonk_kzg_multiproof_check: key is the ordinary opening key (third element [tau] h).  One weights kernel, ONE launch of
 *   plonk_msm_points' kernels over [C_0 .. C_(M-1) | D | pi | g] with the scalars [s_j | -1 | t | -y] (per-term or buckets by
 *   its own rule) and ONE host pairing: PLONK_OK or PLONK_ERR_VERIFY — a multiproof has one verdict.  Checks, in this order:
 *   PLONK_ERR_ARG (as above, the pointers being key, commitments48, both index arrays, values, proof96; and log_n outside
 *   [1, 20]); PLONK_ERR_DATA (a value or an override that is not canonical, an override t in the domain); PLONK_ERR_POINT (a
 *   commitment, D or pi that does not decode or lies outside the subgroup; the compressed identity is legal); then the
 *   pairing.  A transcript-drawn t inside the domain is PLONK_ERR_VERIFY: no prover returns such a proof.  info (may be NULL):
 *   proofs = count, msm_terms = ncommitments + 3, pairing_checks = 1 and the phase times. */
typedef struct plonk_kzg_multiproof_info {
  uint32_t log_n;
  uint32_t built_points;           /* 1: this call built the Lagrange points */
  uint64_t items;                  /* K */
  uint64_t vectors;                /* M */
  uint64_t point_groups;           /* distinct point indexes among the items */
  uint64_t commitments_computed;   /* M when commitments_in was NULL, else 0 */
  uint64_t msm_launches;           /* commitments_computed + 2 */
  uint64_t msm_terms;              /* terms of each: n */
  uint64_t products;               /* field products of the aggregation pass: (K + 2 point_groups) x n */
  uint64_t device_bytes;           /* what the multiproof state of the handle holds: invd, workspaces, staged vectors */
} plonk_kzg_multiproof_info;
int plonk_kzg_multiproof_open(plonk_kzg_domain* domain, const uint64_t* const* evals, uint64_t nvectors,
                              const uint8_t* commitments_in /* nvectors x 48, or NULL: computed */, const uint32_t* vector_index,
                              const uint32_t* point_index, uint64_t count, const uint8_t* label, uint64_t label_len,
                              const uint64_t* challenges_override /* 8 limbs or NULL */, uint64_t* values /* count x 4 out: y_k */,
                              uint8_t* commitments_out /* nvectors x 48 or NULL */, uint8_t proof96[96]);
int plonk_kzg_multiproof_open_dev(plonk_kzg_domain* domain, const void* const* evals_dev, uint64_t nvectors, const uint8_t* commitments_in,
                                  const uint32_t* vector_index, const uint32_t* point_index, uint64_t count, const uint8_t* label,
                                  uint64_t label_len, const uint64_t* challenges_override, uint64_t* values, uint8_t* commitments_out,
                                  uint8_t proof96[96]);
int plonk_kzg_multiproof_last(plonk_kzg_domain* domain, plonk_kzg_multiproof_info* out);
int plonk_kzg_multiproof_check(plonk_kzg_key* key, uint32_t log_n, const uint8_t* commitments48, uint64_t ncommitments,
                               const uint32_t* vector_index, const uint32_t* point_index, const uint64_t* values, uint64_t count,
                               const uint8_t proof96[96], const uint8_t* label, uint64_t label_len, const uint64_t* challenges_override,
                               plonk_verify_info* info /* may be NULL */);

/* ---- variable-base MSM over caller-supplied points ------------------------------------------------
 * sum_i scalars[i] * P_i for points the CALLER brings — the reference's msm_variable_base (the primitive under Proof::verify
 * and OpeningKey::batch_check) — where plonk_msm / _batch / _dev run over the loaded commit key and its precomputed tables.
 * No key is needed and none is touched.  A bucket method (Pippenger) on the device: every scalar is split through the
 * curve's endomorphism into two 128-bit halves, each half into signed digits of c bits, the (point, digit) entries are
 * grouped by (window, bucket) with a counting sort, accumulated by slices, summed per bucket, per window and over the
 * windows.
 *   points   m x 96 bytes x || y (the layout plonk_srs_load takes); 96 zero bytes are the identity ((0, 0) is not on the
 *            curve).  PLONK_POINTS_COMPRESSED: m x 48 bytes, G1Affine::to_bytes, decoded on the device; the compressed
 *            identity is legal, a point that does not decode is PLONK_ERR_POINT.  PLONK_POINTS_CHECK: every finite point is
 *            tested for the curve equation and the prime-order subgroup, a failure is PLONK_ERR_POINT and nothing is written
 *            to the output.  Without it raw points are trusted, as plonk_srs_load trusts its input.
 *   scalars  m x 4 limbs, Montgomery, as plonk_msm.
 *   out      97 bytes, as plonk_msm.  m == 0 gives the identity; m > 2^24 is PLONK_ERR_ARG.
 *   opts     NULL or a zeroed struct with struct_size set = automatic.  PLONK_ERR_ARG for a struct_size below
 *            sizeof(plonk_msm_points_opts), an unknown flag, window_bits outside 2..16 or slice_entries above 2^20.
 * plonk_msm_points_dev: points, scalars and the 97 output bytes are device pointers on the context's GPU (4-byte aligned).
 * Both forms return with the context's main stream synchronised; a context with a communicator runs the call locally.  The
 * workspace is owned by the context, grows on demand and is freed by plonk_ctx_destroy.
 * plonk_ctx_last_msm_points: what the last call on the context ran as (PLONK_ERR_STATE before the first): the tests assert it
 * against the plan computed on the host (plonk_amd/csrc/msm_points_core.hpp), so a switch that is ignored fails a test. */
enum { PLONK_POINTS_COMPRESSED = 1, PLONK_POINTS_CHECK = 2 };
typedef struct plonk_msm_points_opts {   /* all 0 = automatic */
  uint32_t struct_size, flags;
  uint32_t window_bits;        /* force the digit width c (test hook; 2..16) */
  uint32_t slice_entries;      /* force the longest run one lane accumulates serially */
  uint32_t min_bucket_terms;   /* below this many terms use the per-term kernel; 1 forces buckets */
  uint32_t reserved;
} plonk_msm_points_opts;
typedef struct plonk_msm_points_info {   /* what the last call ran as */
  uint32_t path;               /* 0 per-term, 1 buckets */
  uint32_t window_bits, windows, slice_entries;
  uint64_t terms, nonzero_digits, slices, longest_bucket;
} plonk_msm_points_info;
int plonk_msm_points(plonk_ctx* ctx, const uint8_t* points, const uint64_t* scalars, uint64_t m,
                     const plonk_msm_points_opts* opts /* NULL */, uint8_t out_xy_inf[97]);
int plonk_msm_points_dev(plonk_ctx* ctx, const void* points_dev, const void* scalars_dev, uint64_t m,
                         const plonk_msm_points_opts* opts, void* out97_dev);
int plonk_ctx_last_msm_points(plonk_ctx* ctx, plonk_msm_points_info* out);

/* ---- gadget composer: circuits from gadgets, witness generation on the device -------------------
 * What the reference's Composer does for a Circuit (src/composer.rs and src/composer/{bits,range,logic,select,truncate,
 * point,fixed_base}.rs): a plonk_composer RECORDS gadget calls and yields (a) the gate layout plonk_compile takes and
 * (b) a witness program that computes every witness of one proof from the circuit's INPUT values — on the device, into the
 * prover's resident witness table, where the reference re-runs the circuit on one host thread (Composer::prove,
 * composer.rs:442).  A composer starts as Composer::initialized: witnesses 0 and 1 are the constants zero and one, four
 * gates are there.  Witness indices are Witness::index; a point is a pair (x, y) of indices.
 *
 * plonk_composer_witness: append_witness — allocates an INPUT and returns its index; the inputs of a proof are given in
 *   allocation order (PLONK_G_PUBLIC, _POINT and _PUBLIC_POINT allocate inputs too: one, two, two).
 * plonk_composer_gate: one arithmetic gate.  selectors: q_m q_l q_r q_o q_f q_c (6 x 4 Montgomery limbs), wires a b c d.
 *   flags bit 0: the row is a public-input row.  flags bit 1: append_evaluated_output (composer.rs:307-359) — solve the row
 *   for c, allocate it, wire it (wires[2] is ignored) and return its index in *out; gate_add / gate_mul are this with
 *   q_o = -1.  With q_o = 0 nothing is allocated, *out = 0xFFFFFFFF and the gate is appended with wires[2] as given (the
 *   reference's None, composer.rs:352-356).
 *   DEVIATION from the reference: its evaluated c includes the row's PI term (composer.rs:326), because its public value
 *   is known while the circuit runs.  Here a public value is never given when recording, so with BOTH flags set c is
 *   solved with PI = 0 and the fill then reports PI = 0 for the row.  A caller that needs a non-zero public term on an
 *   evaluated row feeds it through a PLONK_G_PUBLIC witness on wire d instead.
 * plonk_composer_gadget: one gadget call.  in: its input witnesses; width: its const parameter; consts: Montgomery limbs of a
 *   constant, or x || y of a constant point / generator; out: the witnesses it returns (*nout of them; PLONK_ERR_ARG when
 *   out_cap is smaller).  Per kind (inputs; constants; outputs):
 *     PLONK_G_CONSTANT (-; value; w)        PLONK_G_PUBLIC (-; -; w)            PLONK_G_ASSERT_EQUAL (a b; -; -)
 *     PLONK_G_ASSERT_EQUAL_CONSTANT (a; value; -), width bit 0 makes the row public as well
 *     PLONK_G_BOOLEAN (a; -; -)             PLONK_G_SELECT (bit a b; -; w)      PLONK_G_SELECT_ONE / _ZERO (bit value; -; w)
 *     PLONK_G_DECOMPOSITION<width 1..256> (a; -; width bits, little-endian)
 *     PLONK_G_RANGE_BITS<width 0..256> (a; -; -), odd widths included     PLONK_G_RANGE<width = bit pairs> (a; -; -)
 *     PLONK_G_TRUNCATE<width 0..254> (a; -; low)
 *     PLONK_G_BIND_TRUNCATION_SPLIT<width> (input low; -; -)      PLONK_G_CANONICAL_TRUNCATION<width> (high low; -; -)
 *     PLONK_G_LOGIC_AND / _XOR<width = bit pairs 0..127> (a b; -; w), the inputs bound as logic.rs:181-212 binds them
 *     PLONK_G_POINT (-; -; x y)             PLONK_G_CONSTANT_POINT (-; x y; x y)      PLONK_G_PUBLIC_POINT (-; -; x y)
 *     PLONK_G_ASSERT_EQUAL_POINT (ax ay bx by; -; -)              PLONK_G_ASSERT_EQUAL_PUBLIC_POINT (x y; -; -)
 *     PLONK_G_NEG_POINT (x y; -; x y)       PLONK_G_SUB_POINT / _ADD_POINT (ax ay bx by; -; x y)
 *     PLONK_G_SELECT_IDENTITY (bit x y; -; x y)                   PLONK_G_SELECT_POINT (bit ax ay bx by; -; x y)
 *     PLONK_G_TORSION_FREE (x y; -; -)      PLONK_G_CANONICAL_JUBJUB_SCALAR (s; -; -)
 *     PLONK_G_MUL_GENERATOR (s; generator x y; x y)               PLONK_G_MUL_POINT (s x y; -; x y)
 *   A constant point is validated on the host as the reference validates it — on the curve and torsion-free, of exact prime
 *   order for a generator: PLONK_ERR_POINT otherwise.  DEVIATION in form, not in result: a public row's value is not given
 *   when recording; a fill computes it as whatever satisfies the row under the filled witnesses, which is the value the
 *   honest reference passes, since its PI and its witness come from the same circuit field.
 * plonk_composer_info / _layout: the counts, and what plonk_compile would be given (selectors[k] / wires[w]: `constraints`
 *   entries each, any pointer may be NULL) plus the witness slot of every input and the rows of the public inputs,
 *   ascending — for tests, and for callers who want plonk_compile with sharding.
 * plonk_compile_composer: single GPU; the same prover plonk_compile builds from the exported layout, with the witness
 *   program uploaded and attached.  The composer may be destroyed afterwards.
 *
 * Per proof, on a prover from plonk_compile_composer (PLONK_ERR_STATE on any other; PLONK_ERR_ARG when count differs from the
 * circuit's inputs): inputs = count x 4 Montgomery limbs.
 *   plonk_prover_fill_inputs: runs the witness program; witnesses_out (witnesses x 4 limbs) and pi_out (public_rows x 4
 *     limbs) may be NULL.
 *   plonk_prover_prove_inputs: fill, then the proof of plonk_prover_prove_witnesses over the filled table with the computed
 *     public inputs (returned in pi_out, nullable).
 *   plonk_prover_diagnose_inputs: fill, then the report of plonk_prover_diagnose_witnesses.
 * A scalar that is not below the order of the JubJub subgroup handed to PLONK_G_MUL_GENERATOR is the reference's
 * Error::JubJubScalarMalformed: PLONK_ERR_DATA with a text naming the gadget and the record, and no proof.  Everything else
 * is total: an off-curve point falls back to the identity as point.rs:379-383 does, and the gates reject. */
typedef enum plonk_gadget {
  PLONK_G_CONSTANT = 0, PLONK_G_PUBLIC, PLONK_G_ASSERT_EQUAL, PLONK_G_ASSERT_EQUAL_CONSTANT, PLONK_G_BOOLEAN,
  PLONK_G_SELECT, PLONK_G_SELECT_ONE, PLONK_G_SELECT_ZERO, PLONK_G_DECOMPOSITION, PLONK_G_RANGE_BITS, PLONK_G_RANGE,
  PLONK_G_TRUNCATE, PLONK_G_BIND_TRUNCATION_SPLIT, PLONK_G_CANONICAL_TRUNCATION, PLONK_G_LOGIC_AND, PLONK_G_LOGIC_XOR,
  PLONK_G_POINT, PLONK_G_CONSTANT_POINT, PLONK_G_PUBLIC_POINT, PLONK_G_ASSERT_EQUAL_POINT, PLONK_G_ASSERT_EQUAL_PUBLIC_POINT,
  PLONK_G_NEG_POINT, PLONK_G_SUB_POINT, PLONK_G_ADD_POINT, PLONK_G_SELECT_IDENTITY, PLONK_G_SELECT_POINT,
  PLONK_G_TORSION_FREE, PLONK_G_CANONICAL_JUBJUB_SCALAR, PLONK_G_MUL_GENERATOR, PLONK_G_MUL_POINT
} plonk_gadget;
typedef struct plonk_composer_summary {
  uint64_t constraints, witnesses, inputs, public_rows;
  uint64_t records, levels, widest_level;   /* of the witness program: records, dependency levels, records of the widest level */
} plonk_composer_summary;
typedef struct plonk_composer plonk_composer;
int plonk_composer_create(plonk_composer** out);
void plonk_composer_destroy(plonk_composer* c);
int plonk_composer_witness(plonk_composer* c, uint32_t* out);
int plonk_composer_gate(plonk_composer* c, const uint64_t* selectors /* 6 x 4 */, const uint32_t wires[4], uint32_t flags, uint32_t* out);
int plonk_composer_gadget(plonk_composer* c, int kind, uint32_t width, const uint32_t* in, uint32_t nin, const uint64_t* consts,
                          uint32_t nconsts, uint32_t* out, uint32_t out_cap, uint32_t* nout);
int plonk_composer_info(plonk_composer* c, plonk_composer_summary* out);
int plonk_composer_layout(plonk_composer* c, uint64_t* const selectors[11], uint32_t* const wires[4], uint32_t* input_slots,
                          uint64_t* pi_rows);
int plonk_compile_composer(plonk_ctx* ctx, plonk_composer* c, const uint8_t* label, uint64_t label_len, plonk_prover** out);
int plonk_prover_fill_inputs(plonk_prover* p, const uint64_t* inputs, uint64_t count, uint64_t* witnesses_out, uint64_t* pi_out);
int plonk_prover_prove_inputs(plonk_prover* p, const uint64_t* inputs, uint64_t count, const uint64_t* blinders, uint8_t proof[1008],
                              uint64_t* pi_out);
int plonk_prover_diagnose_inputs(plonk_prover* p, const uint64_t* inputs, uint64_t count, plonk_unsat_row* out, uint64_t cap,
                                 plonk_unsat_info* info);

/* ---- measurement --------------------------------------------------------------
 * When enabled, every launch of the dominant kernels is bracketed by a hipEvent
 * pair ON THE LIBRARY'S STREAM and accumulated per slot.  Slots:
 *   0 ntt pass kernels, 1 msm bucket accumulation, 2 msm (all other kernels),
 *   3 quotient/pointwise kernels, 4 the polynomial work of prove() rounds 1-2 (wire / permutation
 *   polynomials: what stays replicated on every rank of a multi-GPU run).
 *   With PLONK_PROF_FINE=1 in the environment also, per phase of a commitment group (groups of >= 3 commitments: 16 + phase,
 *   smaller groups: 24 + phase): 0 bucket sort, 1 accumulation, 2 bucket sums, 3 heavy buckets, 4 row / column sums, 5 bit sums.
 *   HOST time of plonk_prover_prove* (wall clock, no events; `launches` = occurrences): 8 the arithmetic
 *   that turns the bit sums of a commitment group into compressed commitments, 9 from the return of each of the five
 *   synchronisations of a proof (six or seven for a rank of a sharded proof: the grand product's and the opening
 *   quotients' range totals are exchanged too) to the next launch (slot 8 included: the device's main stream is idle for that long),
 *   10 the time blocked in those synchronisations; 11 (a count, not a time) the helper threads each commitment group had.
 *   plonk_kzg_open / _open_dev (device events): 12 the non-commitment front of an open — the trimmed-length kernel of resident
 *   polynomials with its copies, the powers of v and every fold + evaluate launch (in the host form NOT the uploads the
 *   launches wait for, nor the polynomial commitments between them); 13 Ruffini (or the shift at the point 0); 14 the witness
 *   commitment, bit sums copied back included (its MSM kernels also count in slots 1 and 2).
 *   plonk_kzg_multiproof_open / _open_dev (device events): 12 the aggregation pass, every aggregate and fix-up launch of the
 *   call as one interval.
 *   plonk_msm_points / _dev, bucket path (device events): 15 load + recode (points, scalars, histogram), 22 scan + scatter,
 *   23 slice accumulation, 30 slice sums to bucket sums, 31 window sums.
 *   Slots 0 .. 31 are valid.
 *
 * Host threads.  A context starts up to 3 helper threads (none when the process may run on fewer than 8 CPUs: sched_getaffinity) with its first
 * commitment group of more than one commitment: they take the independent finishing chains of a group (slot 8) beside the
 * calling thread.  They are woken when the caller blocks in the group's synchronisation and SPIN until the bit sums have
 * arrived — up to one device phase per group — and sleep otherwise; plonk_ctx_destroy joins them.  PLONK_HOST_THREADS=k in
 * the environment (read at context creation) sets their number, 0 switches them off. */
int plonk_profile_enable(plonk_ctx* ctx, int on);
int plonk_profile_read(plonk_ctx* ctx, int slot, double* total_ms, uint64_t* launches);
int plonk_profile_reset(plonk_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* PLONK_HIP_H */
