/*
 * sipp_hip.h -- C ABI of the MI355X-native SIPP STARK sub-prover (libsipp_hip.so).
 *
 * This is the drop-in boundary for the hot path of qope/SIPP: the three starky
 * sub-proofs that reference src/verifier_circuit.rs:133-135 delegates to
 * starky-bn254 (g1_exp_circuit / g2_exp_circuit / fq12_exp_circuit).  At proving
 * time each of those runs, inside a plonky2 witness generator,
 *     stark.generate_trace(&ios); stark.generate_public_inputs(&ios);
 *     starky::prover::prove::<F, C, S, D>(stark, &config, trace, public_inputs, &mut timing)
 * (starky-bn254 @ 2d46f9e and starky @ InternetMaximalism/plonky2 541e127,
 * reference Cargo.toml:24,26 -- not vendored under /root/reference).  The three
 * sipp_*_exp_prove entry points below replace exactly that body: native IO
 * records in, flat StarkProofWithPublicInputs buffer out.  Trace fill happens
 * on the device; the caller never materialises the N x W table.
 *
 * Conventions
 *  - plain C, no callbacks, no exceptions; every function returns a sipp_status.
 *  - field elements are canonical little-endian uint64_t (< 2^64 - 2^32 + 1);
 *    extension elements are two consecutive uint64_t (c0, c1).
 *  - BN254 integers are 8 x uint32_t little-endian limbs, exactly the limb
 *    stream of reference src/transcript_native.rs:68-77 and src/statements.rs:90-131.
 *  - `d_` parameters are DEVICE pointers (HBM of the ctx's GPU); everything else
 *    is host memory owned by the caller.
 *  - a sipp_ctx is bound to one GPU and is not thread-safe; distinct contexts on
 *    distinct GPUs may be used concurrently (one process per GPU in bench.py).
 */
#ifndef SIPP_HIP_H
#define SIPP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sipp_ctx sipp_ctx;

typedef enum {
    SIPP_OK = 0,
    SIPP_E_BADARG = -1,      /* null pointer, non power of two, size out of range */
    SIPP_E_HIP = -2,         /* a HIP runtime call failed; see sipp_last_error */
    SIPP_E_NOMEM = -3,       /* workspace arena exhausted */
    SIPP_E_BUFSZ = -4,       /* caller's output buffer too small */
    SIPP_E_SUBGROUP = -5,    /* zeta landed in the trace subgroup (starky prover.rs ensure!) */
    SIPP_E_QUOTIENT = -6,    /* constraints not satisfied: quotient has too high degree */
    SIPP_E_UNSUPPORTED = -7, /* configuration not supported by this build */
    SIPP_E_WITNESS = -8,     /* IO record not provable (point at infinity / not on curve) */
    SIPP_E_VERIFY = -9       /* sipp_stark_verify: the proof is not accepted (the stage is reported through `reason`) */
} sipp_status;

/* starky StarkConfig::standard_fast_config(); supported ranges in brackets */
typedef struct {
    uint32_t rate_bits;       /* 1   [1 .. 3: blowup 2, 4, 8; the quotient stays on the 2N coset]   */
    uint32_t cap_height;      /* 4   [0 .. 8]                                                        */
    uint32_t pow_bits;        /* 16  [0 .. 32]                                                       */
    uint32_t arity_bits;      /* 4   [1 .. 4: FriReductionStrategy::ConstantArityBits, arity 2 .. 16] */
    uint32_t final_poly_bits; /* 5   [0 .. 12]; together with arity_bits it must leave every committed FRI layer at least 16
                                 values for the trace length proved (else SIPP_E_UNSUPPORTED from the prove call)   */
    uint32_t num_queries;     /* 84  [1 .. 1024]                                                     */
    uint32_t num_challenges;  /* 2   [2]                                                             */
    uint32_t pow_rule;        /* SIPP_POW_DUPLEX (0): observe the witness, response = next challenge (plonky2 fri/prover.rs
                                 of 2023); SIPP_POW_HASH (1): response = hash_no_pad(challenger.get_hash() || witness)[0]
                                 (the earlier rule).  Kept as data until upstream's pinned revision can be read. */
    uint32_t fs_rule;         /* where Fiat-Shamir starts.  SIPP_FS_STATEMENT (0, default): this repository's format -- the challenger
                                 observes the statement (kind, shape, config, Merkle root of the public inputs) before the trace cap;
                                 SIPP_FS_UPSTREAM (1): starky's order as recalled: the challenger starts at the
                                 trace cap, the public inputs are NOT in the transcript (upstream's exposure: a verifier must bind them
                                 by other means, as the recursive circuit does by connecting them to its own targets) */
    uint32_t lookup_rule;     /* challenges of a lookup's two permutation factors.  SIPP_LOOKUP_INDEPENDENT (0, default):
                                 Z' (pin + gamma)(ptab + beta) = Z (col + gamma)(tab + beta) -- column and table cannot trade entries;
                                 SIPP_LOOKUP_SHARED (1): both factors use gamma, (beta, gamma) are drawn as before and beta is unused
                                 -- starky's permutation pairs of ONE column each as recalled (reduce_with_powers over a single
                                 column leaves beta^0), which proves only the union multiset.  Header word 15 of a flat proof
                                 records fs_rule | lookup_rule << 1. */
} sipp_stark_config;
#define SIPP_POW_DUPLEX 0
#define SIPP_POW_HASH 1
#define SIPP_FS_STATEMENT 0
#define SIPP_FS_UPSTREAM 1
#define SIPP_LOOKUP_INDEPENDENT 0
#define SIPP_LOOKUP_SHARED 1

void sipp_default_config(sipp_stark_config *cfg);

/* Which STARK (reference src/verifier_circuit.rs:133 / :134 / :135) */
typedef enum { SIPP_G1_EXP = 0, SIPP_G2_EXP = 1, SIPP_FQ12_EXP = 2,
               SIPP_MAP_G2 = 3 /* src/bin/bls_aggregation.rs:65, see sipp_map_to_g2_prove */,
               /* G1 / G2 exponentiation with the HARDENED AIR (same records, same rows, about 14 % more columns): x3 canonical; where
                * an addition is used, an inequality witness for the two x-coordinates -- the chord rule of the plain AIR is satisfied by
                * ANY slope where the accumulator meets the running power; that case (R = P) is proved through the
                * next row's double and R = -P through an identity state bit instead of being refused: every record whose OUTPUT is a
                * finite point has a proof, except one that meets R = P on the LAST add row of its 512 rows (bit 255 of a 256-bit exponent:
                * no row is left to hand the double over) -- SIPP_E_WITNESS, like an output at the identity.  Through sipp_prove / sipp_prove_async and the generic size / shape / trace functions. */
               SIPP_G1_EXP_HARDENED = 4, SIPP_G2_EXP_HARDENED = 5,
               SIPP_PAIRING = 6 /* src/bin/bls_aggregation.rs:76-77, see sipp_pairing_prove */ } sipp_kind;

/* u32 words per IO record, (x, offset, exp_val, output) order:
 * G1 7*8 = 56, G2 13*8 = 104, Fq12 37*8 = 296. */
#define SIPP_G1_IO_WORDS 56
#define SIPP_G2_IO_WORDS 104
#define SIPP_FQ12_IO_WORDS 296
/* MapToG2 records (u, x, y): the message in Fp2 and its point on the twist, 6*8 = 48 */
#define SIPP_MAP_G2_IO_WORDS 48
/* final-pairing records (P, Q, Z): a G1 point (16), a G2 point (32: x.c0, x.c1, y.c0, y.c1), e(P, Q) as 12 MyFq12 coefficients (96) */
#define SIPP_PAIRING_IO_WORDS 144

/* ---- context ---------------------------------------------------------------- */
/* `workspace_bytes` of HBM are reserved once; afterwards the only allocations are the constant tables of a transform SIZE at its
 * first use on the ctx (twiddles / node constants: at most 8 B per LDE row, built on the host once and kept until destroy).
 * Pass 0 to size the arena for n = 128 (about 24 GiB). */
int sipp_ctx_create(sipp_ctx **out, int device, const sipp_stark_config *cfg, size_t workspace_bytes);
/* The version of THIS header (bumped whenever a struct of the ABI changes size or meaning: 2 = sipp_stark_config with ten fields,
 * round 5; 3 = round 6, SIPP_PAIRING).  A binding that cannot be rebuilt with the library (the Rust shim) creates its contexts through
 * sipp_ctx_create_checked, which refuses (SIPP_E_BADARG, *out = NULL, nothing read from cfg) a caller whose header version or
 * sizeof(sipp_stark_config) differs from the library's -- a struct two fields short would otherwise be read past its end and stray
 * bits taken for fs_rule / lookup_rule. */
#define SIPP_ABI_VERSION 3u
uint32_t sipp_abi_version(void);
int sipp_ctx_create_checked(sipp_ctx **out, int device, const sipp_stark_config *cfg, size_t cfg_size, uint32_t abi_version,
                            size_t workspace_bytes);
/* Which of two equivalent kernels serves a step (results are identical; the non-default routes are the fallbacks the tests keep
 * alive -- until round 5 they hid behind environment variables).  routes = OR of:
 *   SIPP_ROUTE_OPENINGS_UNGROUPED  openings at zeta / g zeta by one block per column instead of the grouped kernel (traces >= 1024 rows)
 *   SIPP_ROUTE_LDE_COLUMN_WIDE     columns of 2^13 / 2^14 rows through the whole-column-in-LDS transform instead of the tree sweeps
 *   SIPP_ROUTE_WITNESS_NO_GRAPH    sipp_plonk_generate_witness_levels launches its two kernels per level one by one instead of replaying
 *                                  the captured hipGraph
 *   SIPP_ROUTE_WITNESS_INTERP_ONE_LANE  on thin levels a SIPP_GEN_COSET_INTERPOLATION row runs on lane 0 of its sixteen lanes instead of the
 *                                  sixteen-lane scan (one point per lane).  Bit 8 stays unassigned: the setter refuses it as an unknown
 *                                  bit, which tests/test_gpu_stark.py holds it to
 *   SIPP_ROUTE_WITNESS_REDUCE_ONE_LANE  on thin levels of a circuit with a SIPP_GEN_REDUCING_EXT or SIPP_GEN_QUOTIENT_EXT generator, a
 *                                  SIPP_GEN_REDUCING / _REDUCING_EXT row runs on lane 0 of its sixteen lanes instead of the sixteen-lane scan
 *                                  (a chunk of ceil(K / 16) coefficients per lane).  Circuits without such a generator never take the scan
 * Only while no proof is in flight on the ctx. */
#define SIPP_ROUTE_OPENINGS_UNGROUPED 1u
#define SIPP_ROUTE_LDE_COLUMN_WIDE 2u
#define SIPP_ROUTE_WITNESS_NO_GRAPH 4u
#define SIPP_ROUTE_WITNESS_INTERP_ONE_LANE 16u
#define SIPP_ROUTE_WITNESS_REDUCE_ONE_LANE 32u
int sipp_ctx_set_kernel_routes(sipp_ctx *ctx, uint32_t routes);
void sipp_ctx_destroy(sipp_ctx *ctx);
/* The ctx's HIP stream: level > 0 = a stream of the highest priority the device offers; level <= 0 = a stream with a hardware
 * queue of its own at normal priority (created with an all-ones CU mask: the runtime multiplexes ordinary streams onto a pool of
 * four queues, such a stream is kept out of the pool -- measured 1.5 ms per n = 128 instance, HISTORY.md section 6c; level < 0 used
 * to mean the lowest priority and still does under SIPP_DEDICATED_QUEUES=0).  Such a stream is BLOCKING with respect to the legacy
 * default (NULL) stream -- hipExtStreamCreateWithCUMask takes no flags -- whereas the high-priority stream is hipStreamNonBlocking:
 * an embedder that launches on the NULL stream serialises with the level <= 0 ctxs (not with a level > 0 one); launch on streams
 * of your own (or per-thread default streams), or run with SIPP_DEDICATED_QUEUES=0 (every ctx stream non-blocking, the runtime's
 * queue pool, about 1 ms per n = 128 instance).  With the three proofs of an instance on three ctxs:
 * G1 and G2 <= 0, Fq12 high.  Only while no proof is in flight on the ctx.  sipp_ctx_create makes a level-0 stream. */
int sipp_ctx_set_stream_priority(sipp_ctx *ctx, int level);
/* on != 0: on this ctx the kinds SIPP_G1_EXP / SIPP_G2_EXP mean the HARDENED AIRs (SIPP_G1_EXP_HARDENED / SIPP_G2_EXP_HARDENED below) in
 * every call that takes the ctx -- sipp_g1_exp_prove, sipp_prove_async, sipp_instance_prove, sipp_instances_prove, sipp_proof_size,
 * sipp_stark_shape, sipp_trace_build; the proof's header carries kind 4 / 5.  Size the arena with sipp_workspace_bytes(kind + 4, ..)
 * (that function takes no ctx).  Only while no proof is in flight on the ctx. */
int sipp_ctx_set_hardened(sipp_ctx *ctx, int on);
const char *sipp_last_error(const sipp_ctx *ctx);
int sipp_sync(sipp_ctx *ctx);
/* the hipStream_t every launch of this ctx goes to (as void*) */
void *sipp_stream(sipp_ctx *ctx);

/* ---- the three provers (replace the body of starky-bn254's *ProofGenerator::run_once) */
/* ios: num_io records of SIPP_*_IO_WORDS u32 each, outputs included (they are
 * checked against the device-computed result).  num_io is padded internally to
 * the next power of two by repeating the last record, as upstream does.
 * On success *proof_len u64 words of proof_out are written (layout: INTEGRATION.md). */
int sipp_g1_exp_prove(sipp_ctx *ctx, const uint32_t *ios, size_t num_io, uint64_t *proof_out, size_t proof_cap,
                      size_t *proof_len);
int sipp_g2_exp_prove(sipp_ctx *ctx, const uint32_t *ios, size_t num_io, uint64_t *proof_out, size_t proof_cap,
                      size_t *proof_len);
int sipp_fq12_exp_prove(sipp_ctx *ctx, const uint32_t *ios, size_t num_io, uint64_t *proof_out, size_t proof_cap,
                        size_t *proof_len);
/* The same for any sipp_kind (the only synchronous entry point of the hardened kinds). */
int sipp_prove(sipp_ctx *ctx, int kind, const uint32_t *ios, size_t num_io, uint64_t *proof_out, size_t proof_cap,
               size_t *proof_len);
/* Asynchronous form ("who calls it"): plonky2 runs the three witness generators behind
 * reference src/verifier_circuit.rs:133-135 serially on one thread, so a patched caller starts each proof as soon as
 * its IO values exist and collects the three afterwards.  sipp_prove_async hands the job to the ctx's own worker
 * thread and returns at once; `ios` and `proof_out` must stay valid until sipp_wait returns.  One proof in flight
 * per ctx (a second sipp_prove_async before sipp_wait fails with SIPP_E_BADARG).  sipp_wait blocks until the
 * proof is complete and returns ITS status; *proof_len as for the synchronous calls. */
int sipp_prove_async(sipp_ctx *ctx, int kind, const uint32_t *ios, size_t num_io, uint64_t *proof_out,
                     size_t proof_cap);
int sipp_wait(sipp_ctx *ctx, size_t *proof_len);
/* One SIPP instance = the three sub-proofs, concurrently on three DISTINCT ctxs (one HIP stream each; they may sit
 * on one GPU or on up to three GPUs, SURVEY.md section 8e level L-B).  Arrays are indexed by sipp_kind.  Returns the
 * first failing status; every proof that was started is waited for in any case.  num_io[k] == 0 skips kind k
 * (proof_len[k] = 0).
 * ctxs[0] == ctxs[1] == ctxs[2]: ONE ctx, the three proofs back to back on its stream and arena (workspace = the largest of the
 * three sipp_workspace_bytes) -- for configurations whose three arenas do not fit the card together: n = 4096 needs 159 GB this
 * way instead of 246 GB (179 / 276 GB with the hardened AIRs, which only fit this way) at 5.5 % more time per instance (1234 against
 * 1169 ms; 13 - 15 % at n = 1024, where the proofs' thin phases overlap more).  Two equal handles and a third are SIPP_E_BADARG. */
int sipp_instance_prove(sipp_ctx *const ctxs[3], const uint32_t *const ios[3], const size_t num_io[3],
                        uint64_t *const proof_out[3], const size_t proof_cap[3], size_t proof_len[3]);
/* A queue of `count` independent instances on one GPU (or several): `in_flight` slots of three distinct ctxs each
 * (ctxs[3 * slot + kind]) take the instances from a shared counter, so the latency-bound head and tail of one instance
 * overlap the hashing of the others.  Arrays of instance i: ios[3 i + kind], num_io[3 i + kind], proof_out / proof_cap /
 * proof_len likewise; status[i] (may be NULL) receives sipp_instance_prove's result for instance i.  Returns the first
 * failing status; every instance is attempted.  Every ctx's workspace must hold the largest proof of its kind. */
int sipp_instances_prove(sipp_ctx *const *ctxs, size_t in_flight, size_t count, const uint32_t *const *ios,
                         const size_t *num_io, uint64_t *const *proof_out, const size_t *proof_cap, size_t *proof_len,
                         int *status);
/* From the points to the three proofs: sipp_prove_native_ex(native_ctx, A, B, n) -- native_proof, statement, accepted as there, each
 * may be NULL -- then sipp_instance_prove(ctxs) on the obligation lists it produced (n - 1, n - 1 and 2 log2 n records; n = 1 has none
 * and yields three empty proofs).  native_ctx may be one of the three ctxs (the native stage has ended before the proofs start); its
 * workspace is sipp_prove_native_ex's.  A refusal of the native stage is returned and no proof is attempted (proof_len 0). */
int sipp_flow_prove(sipp_ctx *native_ctx, sipp_ctx *const ctxs[3], const uint32_t *A, const uint32_t *B, size_t n,
                    uint32_t *native_proof, uint32_t *statement, uint64_t *const proof_out[3], const size_t proof_cap[3],
                    size_t proof_len[3], int *accepted);
/* sipp_instances_prove with a producer in front: `count` instances of n pairs each.  One host thread runs sipp_prove_native_ex for
 * instance 0, 1, ... on native_ctx; the `in_flight` slots (ctxs[3 * slot + kind], as in sipp_instances_prove) take instance i as soon as
 * its lists exist, so the latency-bound native stage of the next instance runs beside the hash-bound proofs of the current ones.
 * A[i], B[i]: the points; native_proof[i], statement[i], accepted[i], status[i]: per instance, the ARRAYS native_proof / statement /
 * accepted / status and the entries of the first two may be NULL; proof_out / proof_cap / proof_len [3 i + kind].
 * native_ctx equal to a slot ctx, duplicate slot ctxs, a NULL A[i] / B[i] (or proof_out entry, n > 1): SIPP_E_BADARG before anything
 * starts.  An instance whose native stage is refused gets that code in status[i] and proof_len 0 and no proof is attempted for it;
 * every other instance is still proved.  Returns the first failing status BY INSTANCE INDEX.  count = 0 is SIPP_OK.  The lists of the
 * instances the producer is ahead by are held on the host (160 (n - 1) + 2368 log2 n u32 each). */
int sipp_flows_prove(sipp_ctx *native_ctx, sipp_ctx *const *ctxs, size_t in_flight, size_t count, size_t n,
                     const uint32_t *const *A, const uint32_t *const *B, uint32_t *const *native_proof,
                     uint32_t *const *statement, uint64_t *const *proof_out, const size_t *proof_cap, size_t *proof_len,
                     int *accepted, int *status);
/* IO-sharded sub-proofs (level L-D): the obligation list of one kind is cut into
 * `world` contiguous, balanced ranges and every rank proves ITS range as a STARK of its own -- on the reference side one
 * g1_exp_circuit / g2_exp_circuit / fq12_exp_circuit call per range instead of one per list (src/verifier_circuit.rs:133-135
 * take any slice of obligations).  No data is exchanged between ranks.  Range of `rank`: records [*first, *first + *count);
 * *count may be 0 when num_io < world (sipp_instance_prove skips a kind whose num_io is 0 and reports proof_len 0). */
int sipp_io_shard(size_t num_io, uint32_t world, uint32_t rank, size_t *first, size_t *count);
/* The outputs alone: what the generators behind g1_exp_circuit / g2_exp_circuit / fq12_exp_circuit assign to the
 * returned output targets (reference src/verifier_circuit.rs:133-135 `*_exp_outputs`): out = offset + [exp_val] x
 * (G1, G2) or offset * x^exp_val (Fq12), computed on the device by the trace kernels' accumulator chains.  `ios` are
 * full-size records as for the provers; their (x, offset, exp_val) words are read and their output words are
 * OVERWRITTEN.  Unprovable inputs (a point at infinity on the way) return SIPP_E_WITNESS as in the provers. */
int sipp_exp_outputs(sipp_ctx *ctx, int kind, uint32_t *ios, size_t num_io);
/* upper bound (u64 words) of the flat proof for `num_io` records of `kind` */
size_t sipp_proof_size(const sipp_ctx *ctx, int kind, size_t num_io);
/* HBM workspace (bytes) one proof of `kind` with `num_io` records needs; pass it (or more) to sipp_ctx_create */
size_t sipp_workspace_bytes(int kind, size_t num_io);
/* the same for a non-default configuration (the LDEs grow with the blowup 2^rate_bits); cfg == NULL = default */
size_t sipp_workspace_bytes_cfg(int kind, size_t num_io, const sipp_stark_config *cfg);
/* memory of GPU `device` in bytes (hipMemGetInfo): what is free now and what the card has -- to decide between three concurrent
 * arenas and one (sipp_instance_prove).  Either pointer may be NULL. */
int sipp_device_memory(int device, size_t *free_bytes, size_t *total_bytes);
/* trace shape the prover will use: rows (log2), main columns, permutation-Z columns, quotient chunks */
int sipp_stark_shape(const sipp_ctx *ctx, int kind, size_t num_io, uint32_t *log_rows, uint32_t *main_cols,
                     uint32_t *perm_cols, uint32_t *quotient_cols);

/* ---- next row: messages -> G2 in front of SIPP's BLS example ----------------- */
/* The STARK behind `batch_map_to_g2_circuit(builder, &messages)` (reference src/bin/bls_aggregation.rs:65): for every
 * message u in Fp2 the point (x, y) = map_to_g2_without_cofactor_mul(u) on the twist y^2 = x^3 + 3/(9+u) (:102; the
 * Shallue - van de Woestijne map of RFC 9380 F.1 with Z = 1, sgn0(y) = sgn0(u)).  ios: num_io records (u, x, y) of
 * SIPP_MAP_G2_IO_WORDS u32, the point included (compared with the device-computed one; SIPP_E_WITNESS if it differs or if a
 * word is >= p; the four u with u^2 g(1) = +-1 follow the RFC's inv0(0) = 0).  Eight trace rows per message, at least 1024 rows.  The cofactor
 * multiplication that follows the map in the reference (`mul_by_cofactor`, :103) is a pair of ordinary G2ExpStark
 * obligations: sipp_map_to_g2 below writes them.  Proof layout and the generic entry points (sipp_prove_async,
 * sipp_proof_size, sipp_workspace_bytes, sipp_stark_shape, sipp_trace_build, sipp_exp_outputs) as for the other kinds
 * with kind = SIPP_MAP_G2. */
int sipp_map_to_g2_prove(sipp_ctx *ctx, const uint32_t *ios, size_t num_io, uint64_t *proof_out, size_t proof_cap,
                         size_t *proof_len);
/* The STARK behind the in-circuit FINAL PAIRING of the reference's BLS example (src/bin/bls_aggregation.rs:76-77:
 * `let z = pairing_circuit(builder, final_A, final_B); Fq12Target::connect(builder, &z, &final_Z)`), the way this path does
 * everything else: as a STARK obligation instead of outer-circuit gates.  ios: num_io records (P, Q, Z) of SIPP_PAIRING_IO_WORDS u32;
 * Z = e(P, Q) with the value `plonky2_bn254_pairing::pairing::pairing` returns (src/prover_native.rs:8,20; as recalled it restates
 * arkworks' Bn254::pairing: the reduced optimal ate pairing raised to 2u(6u^2 + 3u + 1), ark-ec's final exponentiation) is compared with the device-computed one (SIPP_E_WITNESS if it
 * differs, if P / Q are off their curves, if a word is >= p, or if a step of the affine Miller loop degenerates -- Q outside the
 * r-torsion).  2^13 trace rows per pairing, one modular identity per row (64 tangent + 38 chord steps, the easy part, ark-ec's hard-part
 * chain: 7185 active rows), at least two blocks.  A VERIFIER of such a proof must check [r] Q = O besides the curve equations (oracle/stark.c does): the chord
 * rows are sound for points of order r only.  Generic entry points (sipp_prove, sipp_prove_async, sipp_proof_size,
 * sipp_workspace_bytes, sipp_stark_shape, sipp_trace_build, sipp_exp_outputs: Z computed and written) with kind = SIPP_PAIRING. */
int sipp_pairing_prove(sipp_ctx *ctx, const uint32_t *ios, size_t num_io, uint64_t *proof_out, size_t proof_cap,
                       size_t *proof_len);
/* ---- verification ----------------------------------------------------------------------------------------------------------
 * The check of a flat proof made by any of the provers above (every kind): what starky's native `verify_stark_proof` does inside the
 * reference's proof generators right after `prove` (starky-bn254 @ 2d46f9e, un-vendored) and what `data.verify`
 * (src/verifier_circuit.rs:254) rests on.  HOST code (about 40 k Poseidon permutations and one evaluation of the AIR at zeta: a few
 * milliseconds to a few tens on up to eight threads; no GPU, no ctx): header and configuration, canonical words, the PUBLIC conditions of the
 * statement (record elements below p; points on their curves; MapToG2: the sign rule; pairing: Q of order r), the Fiat-Shamir replay,
 * the constraints at zeta against the quotient openings, FRI (proof of work, Merkle paths of the three oracles and of every layer, the
 * fold of every query, the final polynomial).  cfg = NULL: the default configuration.
 * Returns SIPP_OK, SIPP_E_BADARG / SIPP_E_UNSUPPORTED, or SIPP_E_VERIFY with the stage in *reason (may be NULL):
 *   100 header  101 kind / size  102 shape or configuration differs  103 FRI rounds  104 / 105 public-input words  106 truncated
 *   107 zeta in the trace domain  108 a record element >= p  109 a record's point off its curve / sign rule / order of Q
 *   110 / 111 the constraints of challenge 0 / 1 do not meet the quotient  120 FRI section  121 proof of work
 *   122 query truncated  123 / 124 / 125 Merkle path of the trace / Z / quotient oracle  130 layer truncated  131 fold mismatch
 *   132 Merkle path of a layer  133 final polynomial  140 trailing words  141 a word that is not a canonical field element
 * (the oracle's verifier, oracle/stark.c, reports the same stages: tests/test_product_verifier.py compares them proof by proof). */
int sipp_stark_verify(const uint64_t *proof, size_t len, const sipp_stark_config *cfg, int *reason);

/* What the reference computes natively per message (src/bin/bls_aggregation.rs:100-104), on the device:
 *   map_ios [n][48]      (u, x, y) records for sipp_map_to_g2_prove;
 *   g2_ios  [2n][104]    (may be NULL) the G2ExpStark obligations of the cofactor clearing, h = 2p - r:
 *                        record i      : x = (x, y)_i, offset = G2 generator, exp_val = h, output = G + [h](x, y)_i
 *                        record n + i  : x = -G,       offset = that output,  exp_val = 1, output = [h](x, y)_i
 *   cleared [n][32]      (may be NULL) the points [h](x, y)_i of G2 (x.c0, x.c1, y.c0, y.c1), i.e. `ms` of :100-104. */
int sipp_map_to_g2(sipp_ctx *ctx, const uint32_t *msgs, size_t n, uint32_t *map_ios, uint32_t *g2_ios, uint32_t *cleared);

/* ---- next row: the native prover's pairing products ------------------------- */
/* inner_product of reference src/prover_native.rs:15-23: prod_i pairing(A_i, B_i) for n pairs, on the device.
 * g1: n x 16 u32 (x, y), g2: n x 32 u32 (x.c0, x.c1, y.c0, y.c1) -- the limb stream of src/transcript_native.rs:42-54;
 * all-zero coordinates stand for the point at infinity.  out: the 12 MyFq12 coefficients, 96 u32 (src/transcript_native.rs:32-40).
 * sipp_inner_products computes `count` independent products (pairs [k n, (k + 1) n) -> out[k]) in one pass, e.g. the Z_L and
 * Z_R of one SIPP round (src/prover_native.rs:51-52).  Uses the ctx's workspace (about 600 bytes per pair; SIPP_E_NOMEM, nothing
 * launched, if it does not fit).  n * count is at most 2^24 (SIPP_E_BADARG beyond, and for n = 0 or count = 0).
 * Input contract: every coordinate is canonical (< p), every point that is not all-zero lies on its curve and B_i in G2; NEITHER is
 * checked here (the result for other inputs is unspecified), and all-zero words in A_i or in B_i or in both mean infinity. */
int sipp_inner_product(sipp_ctx *ctx, const uint32_t *g1, const uint32_t *g2, size_t n, uint32_t *out);
int sipp_inner_products(sipp_ctx *ctx, const uint32_t *g1, const uint32_t *g2, size_t n, size_t count, uint32_t *out);

/* The native chain around those products (host code over the device routines; the transcript stays on the host):
 * sipp_prove_native = reference src/prover_native.rs:26-80: A (n x 16 u32), B (n x 32 u32), n a power of two ->
 *   proof = 2 log2 n + 1 Fq12 messages of 96 u32 each, in the reference's (reversed) order; sipp_native_proof_words(n) u32.
 * sipp_verify_native = reference src/verifier_native.rs:14-85: replays the transcript, folds A, B, Z and returns
 *   statement (16n + 32n + 96 + 16 + 32 + 96 u32: A | B | Z | final_A | final_B | final_Z, src/statements.rs:24-39),
 *   the three obligation lists as complete IO records for sipp_*_exp_prove (src/verifier_circuit.rs:68-131:
 *   (n - 1) x 56, (n - 1) x 104 and 2 log2 n x 296 u32, round-major), and *accepted = (pairing(final_A, final_B) == final_Z).
 *   Any output pointer may be NULL.  The ctx's workspace must hold the widest fold (sipp_workspace_bytes(SIPP_G2_EXP, n / 2)).
 * Where the chain DIVERGES from the reference (and from oracle/py/sipp_native.py): a point at infinity among A or B is the neutral
 *   element there and folds like any other; here both calls refuse it with SIPP_E_WITNESS, as they refuse a point off its curve or a
 *   fold that passes through infinity, because the exponentiation AIRs have no witness for such an obligation (n = 1, which folds
 *   nothing, takes infinity as the products do).  After a refusal the ctx is usable as before: no fold stays in flight and the
 *   workspace is handed back. */
size_t sipp_native_proof_words(size_t n);
int sipp_prove_native(sipp_ctx *ctx, const uint32_t *A, const uint32_t *B, size_t n, uint32_t *proof);
int sipp_verify_native(sipp_ctx *ctx, const uint32_t *A, const uint32_t *B, size_t n, const uint32_t *proof,
                       uint32_t *statement, uint32_t *g1_ios, uint32_t *g2_ios, uint32_t *fq12_ios, int *accepted);
/* Both in ONE pass: the prover's loop, with the verifier's outputs taken on the way instead of folded a second time.
 *   proof                       sipp_prove_native(A, B)'s, word for word;
 *   statement, the three lists  what sipp_verify_native(A, B, that proof) returns, word for word (layouts above), and so is
 *   *accepted                   (pairing(final_A, final_B) == final_Z; that pairing is launched only when the pointer is not NULL).
 * ANY output pointer may be NULL.  The G1 / G2 lists are the records every round's fold leaves complete; the Fq12 list is one pass over
 * the 2 log2 n powers Z_L^x, Z_R^(1/x) after the last challenge, with the running product on the host as in sipp_verify_native.  With
 * statement, fq12_ios and accepted all NULL nothing is launched that sipp_prove_native does not launch (g1_ios / g2_ios cost two host
 * copies per round).  n = 1 has no round: the lists are empty, final_A / final_B are the inputs and final_Z = Z.
 * Workspace: the widest fold, sipp_workspace_bytes(SIPP_G2_EXP, n / 2), as for sipp_prove_native; and, when statement, fq12_ios or
 * accepted is asked for, the Fq12 trace of the powers, sipp_workspace_bytes(SIPP_FQ12_EXP, 2 log2 n) -- one after the other, so the
 * larger of the two.  Refusals are sipp_prove_native's: SIPP_E_BADARG (n no power of two, a NULL ctx / A / B), SIPP_E_WITNESS (infinity,
 * a point off its curve, a fold through infinity), and SIPP_E_NOMEM, also for a workspace that holds the fold but not the Fq12 trace
 * (returned after the folds; the outputs written until then are to be ignored).  After any refusal no fold is in flight, the workspace
 * is handed back and the ctx works as before. */
int sipp_prove_native_ex(sipp_ctx *ctx, const uint32_t *A, const uint32_t *B, size_t n, uint32_t *proof,
                         uint32_t *statement, uint32_t *g1_ios, uint32_t *g2_ios, uint32_t *fq12_ios, int *accepted);

/* ---- next row (SURVEY.md section 8f, rank 2 -- the generic half of the outer plonky2 prover) ---------------------------
 * PolynomialBatch commitments and FRI opening proofs for ARBITRARY FriParams: what reference src/verifier_circuit.rs:225
 * (`builder.build`) fixes and :253 (`data.prove`) runs four times per proof in plonky2 (constants/sigmas, wires,
 * zs/partial products, quotient; blowup 8, arity 16, 28 queries in `standard_recursion_config`, salted wires when zero
 * knowledge is on).  The gate constraints of the outer circuit are NOT part of this (upstream's circuit is not vendored). */
#define SIPP_SALT_SIZE 4
#define SIPP_FRI_MAX_ROUNDS 32
typedef struct {
    uint32_t rate_bits, cap_height, pow_bits, num_queries, pow_rule;
    uint32_t hiding;                           /* FriParams::hiding: salted oracles open their salt words too */
    uint32_t n_rounds;
    uint32_t arity_bits[SIPP_FRI_MAX_ROUNDS];  /* FriParams::reduction_arity_bits, each 1 .. 4 */
} sipp_fri_params;
/* FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits) for polynomials of 2^degree_bits coefficients;
 * rate_bits and cap_height of *p must be set before the call */
void sipp_fri_const_arity(sipp_fri_params *p, uint32_t arity_bits, uint32_t final_poly_bits, uint32_t degree_bits);
/* a committed oracle, all pointers DEVICE memory owned by the caller:
 *   d_coeffs [n_polys][N] natural, d_lde [n_polys + n_salt][N << rate_bits] leaf order, d_tree (2 leaves x 4 u64, levels back to back) */
typedef struct {
    const uint64_t *d_coeffs;
    const uint64_t *d_lde;
    const uint64_t *d_tree;
    uint32_t n_polys, n_salt;
} sipp_oracle;
/* PolynomialBatch::from_values (from_coeffs != 0: from_coeffs) with explicit blowup / cap height and optional blinding:
 * d_salt = n_salt (0 or SIPP_SALT_SIZE) columns of N << rate_bits words in NATURAL LDE order (plonky2 draws them at random;
 * here the caller supplies them so that proofs are reproducible), appended to every leaf.  d_lde must hold ncols + n_salt
 * columns.  cap_out (host): 2^min(cap_height, log leaves) x 4 u64. */
int sipp_commit_batch_ex(sipp_ctx *ctx, const uint64_t *d_in, int from_coeffs, uint64_t *d_coeffs, uint64_t *d_lde,
                         uint64_t *d_tree, size_t ncols, uint32_t log_n, uint32_t rate_bits, uint32_t cap_height,
                         const uint64_t *d_salt, uint32_t n_salt, uint64_t *cap_out);
typedef struct { uint32_t oracle, col_begin, col_end; } sipp_poly_range;
typedef struct {
    uint64_t point[2];              /* extension element (c0, c1), not in the trace subgroup (SIPP_E_SUBGROUP); zero is allowed */
    uint32_t n_ranges;              /* may be 0, and ranges may be empty (col_begin == col_end): a batch without a polynomial opens nothing */
    const sipp_poly_range *ranges;  /* FriBatchInfo::polynomials as ranges of oracle columns, in opening order */
} sipp_fri_batch;
/* plonky2 Challenger state as plain data: the caller's transcript goes in and comes out */
typedef struct {
    uint64_t state[12];
    uint64_t in_buf[8];
    uint64_t n_in;
    uint64_t out_buf[8];
    uint64_t n_out;
} sipp_challenger;
/* PolynomialBatch::prove_openings: the opened values are computed, written and observed batch by batch, then alpha, the
 * final polynomial, the commit phase, the proof of work and the query rounds.  Flat proof (u64 words):
 *   header[8]: "SIPPFRI1", n_rounds, final_len, num_queries, n_oracles, n_batches, total_len, log_n
 *   opened values (ext) per batch | commit caps | final_poly | pow_witness | query rounds
 * Supported range (SIPP_E_UNSUPPORTED outside it): log_n 10 .. 24, rate_bits 1 .. 3, arity_bits 1 .. 4 per round, cap_height
 * <= 8, and every committed layer holds at least 16 values; SIPP_E_BADARG for parameters the protocol itself forbids (a layer
 * with fewer leaves than its cap, arities that exceed the degree). */
size_t sipp_fri_proof_size(const sipp_oracle *oracles, size_t n_oracles, const sipp_fri_batch *batches, size_t n_batches,
                           uint32_t log_n, const sipp_fri_params *p);
int sipp_fri_prove_openings(sipp_ctx *ctx, const sipp_oracle *oracles, size_t n_oracles, const sipp_fri_batch *batches,
                            size_t n_batches, uint32_t log_n, const sipp_fri_params *p, sipp_challenger *ch,
                            uint64_t *proof_out, size_t proof_cap, size_t *proof_len);

/* ---- SURVEY.md section 8f, rank 2, continued: plonky2's WIRE PERMUTATION ARGUMENT -------------------------------------------------
 * The protocol-generic part of `data.prove(pw)` (reference src/verifier_circuit.rs:253) between the wires commitment and the opening
 * proof: plonk/prover.rs wires_permutation_partial_products_and_zs, the Z(1) = 1 and partial-product terms of
 * plonk/vanishing_poly.rs, compute_quotient_polys -- for any number of routed wires, chunk size (= quotient degree factor, a power
 * of two) and number of challenges, on the caller's wires and sigma polynomials.  The GATE constraints of the reference's circuit
 * are not part of this (the circuit is built by un-vendored crates). */
typedef struct {
    uint32_t num_routed_wires;   /* CircuitConfig::num_routed_wires (80 in standard_recursion_config) */
    uint32_t max_degree;         /* quotient_degree_factor = chunk size of the partial products (8); a power of two, 2 .. 64 for
                                  * sipp_plonk_zs_partial_products alone: the quotient and the whole argument need
                                  * 2^rate_bits >= max_degree with rate_bits <= 3, so 2 .. 8 (16 .. 64: SIPP_E_UNSUPPORTED there) */
    uint32_t num_challenges;     /* CircuitConfig::num_challenges (2); 1 .. 8 */
} sipp_plonk_params;
/* CommonCircuitData::num_partial_products = ceil(num_routed_wires / max_degree) - 1 */
uint32_t sipp_plonk_num_partial_products(const sipp_plonk_params *p);
/* d_wires, d_sigmas: [num_routed_wires][N] VALUES in natural row order (sigma[j][i] = k_col' w^row' of the wire that (j, i) maps to,
 * k_j = 7^j); betas, gammas: num_challenges host words.  d_out [num_challenges (1 + num_partial_products)][N] values in the column order
 * of the zs_partial_products commitment: Z_0 .. Z_{C-1}, then the partial products of challenge 0, of challenge 1, ...
 * A chunk whose denominator prod_j (w_j + beta sigma_j + gamma) vanishes is 0 (1 / 0 = 0, chunk by chunk, as plonky2's batch inversion
 * and oracle/plonk.c have it): that chunk alone -- the row's other chunks, and the other challenges, keep their values.
 * betas, gammas (and alphas below) and the cells of d_wires may be any u64 congruent to the value; d_sigmas and every LDE handed to the
 * quotient hold canonical words (< p), as the commitments write them. */
int sipp_plonk_zs_partial_products(sipp_ctx *ctx, const uint64_t *d_wires, const uint64_t *d_sigmas, uint32_t log_n,
                                   const sipp_plonk_params *p, const uint64_t *betas, const uint64_t *gammas, uint64_t *d_out);
/* compute_quotient_polys for the permutation terms, from the three committed oracles' LDEs (leaf order, blowup 2^rate_bits >=
 * max_degree; column strides N << rate_bits): d_chunks [num_challenges max_degree][N] receives the coefficient chunks (chunk d of
 * challenge c at row c max_degree + d) -- the input of sipp_commit_batch_ex(from_coeffs = 1). */
int sipp_plonk_quotient_chunks(sipp_ctx *ctx, const uint64_t *d_wires_lde, const uint64_t *d_sigmas_lde, const uint64_t *d_zs_lde,
                               uint32_t log_n, uint32_t rate_bits, const sipp_plonk_params *p, const uint64_t *betas,
                               const uint64_t *gammas, const uint64_t *alphas, uint64_t *d_chunks);
/* The same with the circuit's GATE-CONSTRAINT terms (round 4): plonk/vanishing_poly.rs builds vanishing_terms = vanishing_z_1_terms ++
 * vanishing_partial_products_terms ++ constraint_terms and runs ONE reduce_with_powers over all of them per challenge.  The gates of the
 * reference's circuit live in un-vendored crates, so their terms are the caller's: d_gate_terms [num_gate_terms][N << rate_bits], one
 * column per constraint, at the rows of the committed LDEs in leaf order (only the first N max_degree rows -- the quotient coset 7 <w_(N D)>
 * -- are read; any u64 congruent to the value).  A patched plonky2 whose gates stay on the CPU (or in its own kernels) evaluates them on
 * the wires LDE it committed through sipp_commit_batch_ex and hands the columns over.  num_gate_terms == 0 / NULL: the call above. */
int sipp_plonk_quotient_chunks_ex(sipp_ctx *ctx, const uint64_t *d_wires_lde, const uint64_t *d_sigmas_lde, const uint64_t *d_zs_lde,
                                  uint32_t log_n, uint32_t rate_bits, const sipp_plonk_params *p, const uint64_t *betas,
                                  const uint64_t *gammas, const uint64_t *alphas, const uint64_t *d_gate_terms, uint32_t num_gate_terms,
                                  uint64_t *d_chunks);
/* The whole argument as one call: commitments of sigmas, wires, zs_partial_products and quotient chunks, the transcript
 * (circuit_digest[4], public_inputs_hash[4], wires cap -> betas, gammas; zs cap -> alphas; quotient cap -> zeta) and one opening proof
 * (zeta: the four oracles; g zeta: the Z columns).  Flat proof (u64 words):
 *   header[8]: "SIPPPLK1", log_n, num_routed_wires, max_degree, num_challenges, total_len, 0, 0
 *   wires cap | zs_partial_products cap | quotient cap | sipp_fri_prove_openings' proof
 * The workspace must hold the four oracles (coefficients, LDE, tree each). */
size_t sipp_plonk_perm_proof_size(uint32_t log_n, const sipp_plonk_params *p, const sipp_fri_params *fp);
int sipp_plonk_perm_prove(sipp_ctx *ctx, const uint64_t *d_wires, const uint64_t *d_sigmas, uint32_t log_n, const sipp_plonk_params *p,
                          const sipp_fri_params *fp, const uint64_t circuit_digest[4], const uint64_t public_inputs_hash[4],
                          uint64_t *proof_out, size_t proof_cap, size_t *proof_len);

/* prove() of plonk/prover.rs except gate evaluation and witness generation: as sipp_plonk_perm_prove, plus
 *   - the gate-constraint terms in the quotient (d_gate_terms as for sipp_plonk_quotient_chunks_ex; may be NULL / 0),
 *   - the PUBLIC INPUTS: public_inputs_hash = hash_n_to_hash_no_pad(public_inputs) is computed here and observed after circuit_digest;
 *     the inputs themselves travel behind the opening proof,
 *   - oracles the caller committed already with sipp_commit_batch_ex at this blowup and cap height (both optional): sigmas_oracle (the
 *     constants_sigmas commitment is made once per circuit), and wires_oracle + wires_cap (the caller needed the wires LDE for its gates:
 *     the same buffers are opened here, nothing is transformed twice).  d_wires / d_sigmas VALUES are always needed (Z and the partial
 *     products are computed from values).
 * Flat proof "SIPPPLK2": header[8] = magic, log_n, num_routed_wires, max_degree, num_challenges, total_len, num_gate_terms,
 * n_public_inputs | wires cap | zs_partial_products cap | quotient cap | opening proof | public_inputs.
 * proof_cap >= sipp_plonk_perm_proof_size(..) + n_public_inputs. */
int sipp_plonk_prove_ex(sipp_ctx *ctx, const uint64_t *d_wires, const uint64_t *d_sigmas, const sipp_oracle *wires_oracle,
                        const uint64_t *wires_cap, const sipp_oracle *sigmas_oracle, uint32_t log_n, const sipp_plonk_params *p,
                        const sipp_fri_params *fp, const uint64_t circuit_digest[4], const uint64_t *public_inputs,
                        uint32_t n_public_inputs, const uint64_t *d_gate_terms, uint32_t num_gate_terms, uint64_t *proof_out,
                        size_t proof_cap, size_t *proof_len);

/* ---- round 5: GATES AS DATA -- evaluate_gate_constraints on the device ---------------------------------------------------------------
 * plonk/vanishing_poly.rs evaluate_gate_constraints / gates/gate.rs eval_filtered / gates/selectors.rs for a gate set the CALLER describes
 * (the reference's circuit, src/verifier_circuit.rs:213-226, is built by un-vendored crates): a gate = its selector (which selector
 * column, which value = the gate's index, the range of gate indices of its selector group) and a PROGRAM -- one polynomial per
 * constraint over the row's wires, the constant columns and the public-inputs hash, as a sum of monomials.  Constraint term j of the
 * circuit = sum over gates of filter_g * constraint_{g,j};  filter_g(s) = prod_{i in group, i != g} (i - s) * (UNUSED - s when the
 * circuit has more than one selector column), UNUSED = 2^32 - 1.  The terms follow the permutation terms in ONE reduce_with_powers.
 * Program words (int64, host memory): per constraint  n_mono, then per monomial  coef, n_factors, (kind, index) x n_factors;
 * kind 0 = wire, 1 = constant column (index into the num_constants columns, selectors included), 2 = public_inputs_hash word. */
typedef struct {
    uint32_t selector_index, row, group_lo, group_hi;
    uint32_t prog_offset, num_constraints;
} sipp_plonk_gate;
typedef struct {
    uint32_t num_wires;       /* all wire columns of the wires oracle (>= num_routed_wires; 135 / 136 in plonky2's standard configs) */
    uint32_t num_constants;   /* columns of the constants_sigmas oracle in front of the sigmas: num_selectors selector columns, then gate constants */
    uint32_t num_selectors;
    uint32_t num_gates;
    const sipp_plonk_gate *gates;
    const int64_t *programs;
    uint32_t program_words;
} sipp_plonk_circuit;
/* prove() of plonk/prover.rs except witness generation: d_wires [num_wires][N] (the first num_routed_wires are routed) and
 * d_constants_sigmas [num_constants + num_routed_wires][N] are VALUES in natural row order; the gate constraints are evaluated on the
 * quotient coset by the interpreter inside the quotient kernel (no column per constraint is materialised).  Optional pre-committed
 * oracles as for sipp_plonk_prove_ex (constants_sigmas once per circuit).  Flat proof "SIPPPLK3": header[16] = magic, log_n,
 * num_routed_wires, max_degree, num_challenges, total_len, num_wires, num_constants, num_selectors, num_gates, num_gate_constraints,
 * n_public_inputs, 0, 0, 0, 0 | wires cap | zs_partial_products cap | quotient cap | opening proof (zeta: every column of the four
 * oracles constants_sigmas, wires, zs_partial_products, quotient chunks; g zeta: the Z columns) | public_inputs.
 * SIPP_E_BADARG for a malformed circuit (an operand out of range, a program that runs past program_words). */
size_t sipp_plonk_gates_proof_size(uint32_t log_n, const sipp_plonk_params *p, const sipp_fri_params *fp, const sipp_plonk_circuit *c,
                                   uint32_t n_public_inputs);
int sipp_plonk_prove_gates(sipp_ctx *ctx, const uint64_t *d_wires, const uint64_t *d_constants_sigmas, const sipp_oracle *wires_oracle,
                           const uint64_t *wires_cap, const sipp_oracle *constants_sigmas_oracle, uint32_t log_n, const sipp_plonk_params *p,
                           const sipp_fri_params *fp, const sipp_plonk_circuit *c, const uint64_t circuit_digest[4],
                           const uint64_t *public_inputs, uint32_t n_public_inputs, uint64_t *proof_out, size_t proof_cap, size_t *proof_len);

/* ---- round 6: the gates' WITNESS GENERATORS on the device ---------------------------------------------------------------------------
 * plonky2's prove() starts with generate_partial_witness (iop/generator.rs; reference src/verifier_circuit.rs:253 `data.prove(pw)`): every
 * gate instance's SimpleGenerator fills the wires its constraints determine from the wires the caller (or a copy constraint) set.  Here the
 * generators of the gate families a recursive verifier is made of run for ALL rows of their gate at once, one lane per row, in place on
 * the wire table the prover reads next: a generator = (family, the selector column and value that mark its rows, layout parameters p[]).
 *   SIPP_GEN_ARITHMETIC     p = n_ops, const col c0, const col c1       w[4k+3] = c0 w[4k] w[4k+1] + c1 w[4k+2]          (ArithmeticBaseGenerator)
 *   SIPP_GEN_BASE_SPLIT     p = n_limbs, bits per limb                  w[1+i] = limb i of the integer w[0]                (BaseSplitGenerator)
 *   SIPP_GEN_CONSTANT       p = n, first const col                      w[i] = const[p1 + i]                               (ConstantGate)
 *   SIPP_GEN_PUBLIC_INPUT   --                                          w[i] = public_inputs_hash[i], i < 4                (PublicInputGate)
 *   SIPP_GEN_U32_MUL_ADD    p = n_ops, stride, limbs per half           per op at b: (lo, hi) of w[b] w[b+1] + w[b+2] into b+3, b+4, then the
 *                                                                       2-bit limbs of lo and of hi                        (U32ArithmeticGenerator)
 *   SIPP_GEN_RANDOM_ACCESS  p = copies, stride, bits                    per copy at b: index, claimed, 2^bits items, bits: claimed = items[index],
 *                                                                       bits of index                                      (RandomAccessGenerator)
 *   SIPP_GEN_REDUCING       p = K, W                                    alpha (2), old acc (2), K coefficients, K accumulators (2 each) over
 *                                                                       F[X]/(X^2 - W): acc_i = acc_(i-1) alpha + c_i      (ReducingGenerator)
 *   SIPP_GEN_POSEIDON       p = in, out, sbox                           Poseidon without swap: the permutation of w[in .. in+12), every S-box
 *                                                                       input of rounds 1 .. 29 (36 + 22 + 48 wires from sbox) and the 12
 *                                                                       outputs
 *   SIPP_GEN_POSEIDON_SWAP  p = in, out, sbox, swap, delta              Poseidon with swap (a Merkle-path step): delta_i = w[swap] (w[in+4+i] -
 *                                                                       w[in+i]) into w[delta+i], i < 4, then the permutation as above of
 *                                                                       (w[in+i] + delta_i, w[in+4+i] - delta_i, w[in+8 .. in+12)); upstream's
 *                                                                       layout is in 0, out 12, swap 24, delta 25, sbox 29 = 135 wires
 *                                                                       (PoseidonGenerator).  The written cells (out, sbox, delta) must not
 *                                                                       meet the read cells (in, swap)
 *   SIPP_GEN_ARITHMETIC_EXT p = n_ops, const col c0, const col c1, W    per op at b = 8k over F[X]/(X^2 - W): (w[b+6], w[b+7]) = c0 (w[b], w[b+1])
 *                                                                       (w[b+2], w[b+3]) + c1 (w[b+4], w[b+5])             (ArithmeticExtensionGenerator)
 *   SIPP_GEN_EXPONENTIATION p = n_bits (1 .. 64)                        base 0, bits 1 .. n_bits (little-endian), output 1 + n_bits, intermediates
 *                                                                       from 2 + n_bits: the bits from the top wire down, prev_0 = 1,
 *                                                                       intermediate_i = prev_i^2 (bit base + 1 - bit), bit = w[n_bits - i] as a
 *                                                                       field value; output = the last intermediate         (ExponentiationGenerator)
 *   SIPP_GEN_COSET_INTERPOLATION p = subgroup_bits s (1 .. 4), degree d (>= 2), W
 *                                                                       n = 2^s: shift 0, n values (2 each) from 1, the evaluation point (2), the
 *                                                                       evaluation value (2), then from 5 + 2n: ni = (n - 2) / (d - 1)
 *                                                                       intermediate evals (2 each), ni intermediate products (2 each), the
 *                                                                       shifted point (2) = point * inv(shift) (0 for shift 0).  Over the domain
 *                                                                       x_i = g^i (g of order n) with the barycentric weights w_i = g^i / n:
 *                                                                       (e, q) starts at (0, 1) and takes point after point
 *                                                                       (e (shifted - x_i) + value_i w_i q, q (shifted - x_i)); the first chunk
 *                                                                       is min(d, n) points, the others d - 1; the state after every chunk but
 *                                                                       the last goes to intermediate c, the last e to the evaluation value
 *                                                                                                                          (InterpolationGenerator)
 *   SIPP_GEN_REDUCING_EXT   p = K (>= 1), W                             SIPP_GEN_REDUCING with extension coefficients: alpha (2) at 0, old acc (2)
 *                                                                       at 2, K coefficients (2 each) from 4, K accumulators (2 each) from
 *                                                                       4 + 2K: acc_i = acc_(i-1) alpha + c_i              (ReducingExtensionGenerator)
 *   SIPP_GEN_QUOTIENT_EXT   p = n_ops, const col c0, const col c1, W    on a row of SIPP_GEN_ARITHMETIC_EXT's shape (out = c0 a m + c1 c per op at
 *                                                                       b = 8k): READS a = (w[b], w[b+1]), c = (w[b+4], w[b+5]) and out =
 *                                                                       (w[b+6], w[b+7]), WRITES the multiplicand (w[b+2], w[b+3]) =
 *                                                                       (out - c1 c) inv(c0 a), inv(x0 + x1 X) = (x0 - x1 X) inv(x0^2 - W x1^2)
 *                                                                       with inv(0) = 0: a = 0, c0 = 0, or an a of zero norm under a residue W
 *                                                                       all write (0, 0).  The constraints, not the generator, refuse such
 *                                                                       rows (they hold only if out = c1 c)               (QuotientGeneratorExtension)
 *   SIPP_GEN_BASE_SUM       p = n_limbs, bits per limb                  SIPP_GEN_BASE_SPLIT's row read the other way (le_sum): w[0] = sum_l w[1+l]
 *                                                                       2^(bits l) in the field.  The limbs are taken as field values, whatever
 *                                                                       they hold (the constraints, not the generator, range-check them); the
 *                                                                       same limits as kind 2: 1 + n_limbs <= num_wires, bits 1 .. 32,
 *                                                                       n_limbs bits <= 64                                  (BaseSumGenerator)
 *   SIPP_GEN_POSEIDON_MDS   p = in, out                                 the permutation's linear layer on twelve EXTENSION elements, element c
 *                                                                       limb l at in + 2c + l and out + 2c + l: out = M in limb by limb (M is
 *                                                                       over the base field: two independent products), M the MDS matrix of
 *                                                                       the Poseidon kinds.  The inputs are field values, whatever word they
 *                                                                       hold; the outputs are canonical.  in + 24 <= num_wires, out + 24 <=
 *                                                                       num_wires, and the two ranges must not meet         (PoseidonMdsGenerator)
 *   SIPP_GEN_LOOKUP         p = look_wire0, n_look, tab_const0, n_tab,  a looking row's y cells from a DENSE table: entry t has x = t and sits
 *                               base_col                                in table row row0 + t / n_tab, slot t % n_tab (the constant columns
 *                                                                       tab_const0 + 2 slot, + 2 slot + 1 of "LOOKUP TABLES" below).  On a
 *                                                                       row it holds, row0 = const[base_col], T = const[base_col + 1] (field
 *                                                                       values).  T = 0: a plain looking row, nothing is written.  Otherwise
 *                                                                       for every slot k < n_look, x = w[look_wire0 + 2k]:
 *                                                                       w[look_wire0 + 2k + 1] = const[tab_const0 + 2 (x % n_tab) + 1] on row
 *                                                                       row0 + x / n_tab (canonical) if x < T and that row is below N, else 0.
 *                                                                       n_look, n_tab >= 1, look_wire0 + 2 n_look <= num_wires, tab_const0 +
 *                                                                       2 n_tab <= num_constants, base_col + 1 < num_constants
 *   SIPP_GEN_U32_ARITHMETIC p = n_ops, stride, limbs per half           per op at b = stride k: a, b, c at b .. b+2 (operands by their low 32 bits), a b + c
 *                                                                       = lo + 2^32 hi: lo at b+3, hi at b+4, the INVERSE CELL inv(2^32 - 1 - hi)
 *                                                                       at b+5 (0 when hi = 2^32 - 1), then the 2-bit limbs of lo and of hi from
 *                                                                       b+6.  a b + c <= p - 1, so (lo, hi) is the split of a canonical value,
 *                                                                       which (inverse (2^32 - 1 - hi) - 1) lo = 0 lets the constraints say.
 *                                                                       Where lo = 0 no constraint binds the inverse cell: a free cell by design.
 *                                                                       limbs <= 16, stride >= 6 + 2 limbs, n_ops stride <= num_wires
 *                                                                                                                          (U32ArithmeticGenerator)
 *   SIPP_GEN_U32_ADD_MANY   p = n_ops, stride, n_addends A, carry limbs C
 *                                                                       per op at b = stride k: A addends at b .., the carry-in at b+A (all by
 *                                                                       their low 32 bits), their sum = lo + 2^32 carry-out: lo at b+A+1, the
 *                                                                       carry-out at b+A+2, the sixteen 2-bit limbs of lo from b+A+3, the C low
 *                                                                       2-bit limbs of the carry-out from b+A+19.  A 1 .. 32, C <= 16, stride >=
 *                                                                       A + 19 + C, n_ops stride <= num_wires.  The widest column of an 8 x 8
 *                                                                       limb product with one more addend is A = 16: carry-out <= 16, C = 3
 *                                                                                                                          (U32AddManyGenerator)
 *   SIPP_GEN_NONNATIVE      p = op, x0, m0, out0                        x = the eight u32 limbs at x0 .., the modulus m = the eight at m0 .. (least
 *                                                                       significant first, by their low 32 bits; m is data, copied from Constant
 *                                                                       rows).  Writes 24 cells from out0: result (8), quotient (8), slack (8) =
 *                                                                       m - 1 - result.  op 0: result = x mod m, quotient = x / m.  op 1: result
 *                                                                       = (x mod m)^-1 mod m, quotient = k with x result = k m + 1.  m = 0, or
 *                                                                       under op 1 an even m, m = 1 or gcd(x, m) != 1: 24 zeros.  op <= 1, the
 *                                                                       three ranges inside the table, the written 24 cells apart from the 16
 *                                                                       read ones.  One lane per row: a 256-bit division bit by bit, a binary
 *                                                                       extended Euclid, a 512 / 256-bit division for k
 * Only the U32 instantiations of the witness kernels carry the last three kinds; a generator list without them launches what it did before.
 * The five families from SIPP_GEN_ARITHMETIC_EXT to SIPP_GEN_QUOTIENT_EXT take ANY field value in every input cell; W != 0.
 * Defined behaviour outside a gate's range (the constraints, not the generators, refuse such rows): BASE_SPLIT drops the bits of w[0] at
 * and above n_limbs * bits; U32_MUL_ADD takes the low 32 bits of an operand that is not a u32, and with a stride wider than 5 + 2 limbs
 * the cells behind an op's limbs stay untouched; RANDOM_ACCESS with an index >= 2^bits selects by the low `bits` bits of the index;
 * LOOKUP writes y = 0 for an x outside the table (x >= T, or an entry's row outside the circuit; the row arithmetic is in 64 bits, so a
 * row0 or T of any field value cannot wrap): the lookup argument refuses such a row, the multiplicities answer SIPP_E_WITNESS.
 * The generators are ROW-LOCAL: values that reach a gate's inputs through copy constraints from another gate's outputs have to be there
 * already (the caller orders its calls by level); d_constants = the circuit's constant columns [num_constants][N] (selectors first: the
 * front of d_constants_sigmas).  SIPP_E_BADARG for a layout that leaves the wire table or an unknown family. */
#define SIPP_GEN_ARITHMETIC 1
#define SIPP_GEN_BASE_SPLIT 2
#define SIPP_GEN_CONSTANT 3
#define SIPP_GEN_PUBLIC_INPUT 4
#define SIPP_GEN_U32_MUL_ADD 5
#define SIPP_GEN_RANDOM_ACCESS 6
#define SIPP_GEN_REDUCING 7
#define SIPP_GEN_POSEIDON 8
#define SIPP_GEN_POSEIDON_SWAP 9
#define SIPP_GEN_ARITHMETIC_EXT 10
#define SIPP_GEN_EXPONENTIATION 11
#define SIPP_GEN_COSET_INTERPOLATION 12
#define SIPP_GEN_REDUCING_EXT 13
#define SIPP_GEN_QUOTIENT_EXT 14
#define SIPP_GEN_BASE_SUM 15
#define SIPP_GEN_POSEIDON_MDS 16
#define SIPP_GEN_LOOKUP 17
/* 18 = SIPP_GEN_RANDOM (ZERO KNOWLEDGE below) */
#define SIPP_GEN_U32_ARITHMETIC 19
#define SIPP_GEN_U32_ADD_MANY 20
#define SIPP_GEN_NONNATIVE 21
typedef struct {
    uint32_t kind, selector_index, row;
    uint32_t p[5];
} sipp_plonk_generator;
int sipp_plonk_generate_witness(sipp_ctx *ctx, uint64_t *d_wires, const uint64_t *d_constants, uint32_t log_n, uint32_t num_wires,
                                uint32_t num_constants, const sipp_plonk_generator *gens, size_t n_gens, const uint64_t public_inputs_hash[4]);
/* The same for a circuit whose COPY CONSTRAINTS carry outputs of one row to inputs of another (hash chains, Merkle paths, accumulators):
 * generate_partial_witness resolves that order with a work list at proving time; here the circuit builder fixes it once as a SCHEDULE --
 * the rows sorted by level and, per level, the cells its outputs feed (cell = wire * N + row).  For l = 0 .. n_levels - 1: the generators
 * on d_rows[level_offsets[l] .. level_offsets[l + 1]) (one lane per row; a row runs the generator whose selector value it holds), then
 * d_wires[d_copy_dst[k]] = d_wires[d_copy_src[k]] for k in [copy_offsets[l], copy_offsets[l + 1]).  Two small launches per level: the
 * sequence is captured once as a hipGraph per ctx and replayed while the arguments stay the same (SIPP_ROUTE_WITNESS_NO_GRAPH, or an
 * enabled profile, launches them one by one).  d_rows / d_copy_* are device arrays, the offsets host arrays of n_levels + 1 entries.
 * SIPP_E_BADARG also for a row or cell outside the table (checked on the device, reported after the last level).
 * n_gens is at most 32 here (the row-local call above has no limit): the generators travel in the level kernels' arguments, a circuit of
 * up to 16 in the 16-entry struct and kernels it always had, one of 17 .. 32 in a 32-entry struct and the wide instantiation of the
 * same kernels.  More than 32: SIPP_E_BADARG, decided on the host before anything is launched or uploaded; the ctx stays usable.
 * sipp_circuit_build refuses such a circuit when it is given a schedule. */
typedef struct {
    uint32_t n_levels;
    const uint32_t *d_rows;
    const uint32_t *level_offsets;
    const uint64_t *d_copy_src;
    const uint64_t *d_copy_dst;
    const uint32_t *copy_offsets;
} sipp_plonk_schedule;
int sipp_plonk_generate_witness_levels(sipp_ctx *ctx, uint64_t *d_wires, const uint64_t *d_constants, uint32_t log_n, uint32_t num_wires,
                                       uint32_t num_constants, const sipp_plonk_generator *gens, size_t n_gens,
                                       const uint64_t public_inputs_hash[4], const sipp_plonk_schedule *sched);

/* ---- round 6: CIRCUIT DATA -- `builder.build()` / `data.prove(pw)` / `data.verify(proof)` with HOST pointers only -----------------------
 * The reference builds its circuit once (src/verifier_circuit.rs:225 `builder.build::<C>()`), then proves and verifies through the
 * CircuitData (:253 `data.prove(pw)`, :254 `data.verify(proof)`).  The entry points above take DEVICE buffers of the caller; a caller
 * without HIP bindings of its own (the Rust shim) uses these instead: everything the circuit fixes -- the gate set, the generators
 * with their level schedule, the constants_sigmas VALUES -- goes in once and stays on the device with its commitment; a proof takes the
 * wire table with the INPUT cells set (plonky2's PartialWitness; every generated cell is overwritten) and the public inputs from host
 * memory and returns the flat "SIPPPLK3" proof to host memory.  One proof at a time per circuit data; it belongs to its ctx (stream,
 * arena >= sipp_circuit_workspace_bytes) and must be destroyed before it.
 * circuit_digest: 4 words, or NULL = hash_no_pad(constants_sigmas cap || log_n, num_wires, num_routed_wires, num_constants,
 * num_selectors, num_gates) (plonky2 hashes the cap and its common data the same way; the exact word list is this library's).
 * sched may be NULL (row-local generators: sipp_plonk_generate_witness); its arrays are HOST arrays (copied). */
typedef struct sipp_circuit_data sipp_circuit_data;
typedef struct {
    uint32_t n_levels;
    const uint32_t *rows;
    const uint32_t *level_offsets;
    const uint64_t *copy_src;
    const uint64_t *copy_dst;
    const uint32_t *copy_offsets;
} sipp_plonk_schedule_host;
size_t sipp_circuit_workspace_bytes(uint32_t log_n, const sipp_plonk_params *p, const sipp_fri_params *fp, const sipp_plonk_circuit *c);
int sipp_circuit_build(sipp_ctx *ctx, uint32_t log_n, const sipp_plonk_params *p, const sipp_fri_params *fp, const sipp_plonk_circuit *c,
                       const uint64_t *constants_sigmas, const sipp_plonk_generator *gens, size_t n_gens,
                       const sipp_plonk_schedule_host *sched, const uint64_t *circuit_digest, sipp_circuit_data **out);
void sipp_circuit_destroy(sipp_circuit_data *cd);
/* the verifier's half (VerifierOnlyCircuitData): cap_out 2^cap_height x 4 words, digest_out 4 words */
int sipp_circuit_verifier_data(const sipp_circuit_data *cd, uint64_t *cap_out, uint64_t *digest_out);
size_t sipp_circuit_proof_size(const sipp_circuit_data *cd, uint32_t n_public_inputs);
/* wires: HOST [num_wires][N]; the proof's public inputs are bound through public_inputs_hash (PublicInput generator / gate) */
int sipp_circuit_prove(sipp_circuit_data *cd, const uint64_t *wires, const uint64_t *public_inputs, uint32_t n_public_inputs,
                       uint64_t *proof_out, size_t proof_cap, size_t *proof_len);
/* the same proof from the input cells as a list (plonky2's PartialWitness is a set of (target, value)): cells[k] = wire * N + row takes
 * values[k], every other cell starts 0; all pointers are HOST memory.  On the ctx stream: the data's wire table is zeroed, the pairs are
 * copied into arena staging and scattered, a second pass compares every pair with what the table holds, then the call goes on as
 * sipp_circuit_prove does after its upload; the proof is word for word that call's for the dense table with those cells set.
 * n_inputs = 0 (cells / values may then be NULL) is allowed.  Values are stored as given (any u64, as in the dense call).  A cell
 * >= num_wires * N: SIPP_E_BADARG, found on the host before anything is launched.  A cell listed twice with one value is accepted; with
 * two different values: SIPP_E_BADARG, found by the second pass through a device flag read back before witness generation starts, no
 * proof written.  After either refusal the circuit data proves as before.  SIPP_E_NOMEM, nothing launched, if the staging (16 bytes a
 * pair) does not fit the arena. */
int sipp_circuit_prove_inputs(sipp_circuit_data *cd, const uint64_t *cells, const uint64_t *values, size_t n_inputs,
                              const uint64_t *public_inputs, uint32_t n_public_inputs,
                              uint64_t *proof_out, size_t proof_cap, size_t *proof_len);
/* the same proof straight from the words the input cells are copies of (a flat proof the circuit verifies, say): which cell takes
 * which word is fixed when the circuit is built, so the map goes to the device once and a proof sends the words alone.
 * sipp_circuit_set_input_map: pair k says cell cells[k] = wire * N + row takes word sources[k] of words || extra, where words are
 * n_words and extra n_extra u64 (what the words do not carry: a transcript, points, caps).  Both arrays are HOST memory and are copied
 * to device memory of the circuit data's own, freed by sipp_circuit_destroy; a second call replaces the map; n = 0 is a map.  A cell
 * >= num_wires * N or a source >= n_words + n_extra: SIPP_E_BADARG, found on the host, and the map set before stays in force.
 * sipp_circuit_prove_words: words / extra are HOST memory (NULL where their count is 0).  SIPP_E_BADARG when no map is set or when
 * n_words / n_extra are not the map's; SIPP_E_NOMEM, nothing launched, if the staging (8 bytes a word) does not fit the arena.  On the
 * ctx stream: words || extra are copied into arena staging, the wire table is zeroed, one kernel stores staged[sources[k]] at cells[k]
 * (one lane per pair), a second pass compares every pair with the table; a cell that received two different values raises a device flag
 * read back before witness generation starts: SIPP_E_BADARG, no proof written (two pairs with equal values are accepted).  Then the call
 * goes on as sipp_circuit_prove_inputs does; the proof is word for word that call's for cells[k], staged[sources[k]].  After any refusal
 * the circuit data proves as before. */
int sipp_circuit_set_input_map(sipp_circuit_data *cd, const uint64_t *cells, const uint64_t *sources, size_t n,
                               size_t n_words, size_t n_extra);
int sipp_circuit_prove_words(sipp_circuit_data *cd, const uint64_t *words, size_t n_words, const uint64_t *extra, size_t n_extra,
                             const uint64_t *public_inputs, uint32_t n_public_inputs,
                             uint64_t *proof_out, size_t proof_cap, size_t *proof_len);
int sipp_circuit_verify(const sipp_circuit_data *cd, const uint64_t *proof, size_t len, int *reason);

/* ---- LOOKUP TABLES by a log-derivative argument: the columns below the quotient ----------------------------
 * The library's own statement of a LogUp lookup (not plonky2's RE / SLDC bookkeeping): the table lives in CONSTANT columns, the
 * multiplicities in WIRES.  A description is eight uint32 words:
 *   q_look, look_wire0, n_look, q_tab, tab_const0, tab_mult0, n_tab, tag_const0.
 *   q_look, q_tab: constant columns (not selector columns) of 0 / 1 that mark looking rows and table rows;
 *   slot k < n_look of a looking row: the pair (x, y) = wires (look_wire0 + 2k, look_wire0 + 2k + 1);
 *   slot k < n_tab of a table row: the pair (tx, ty) = constant columns (tab_const0 + 2k, + 2k + 1), multiplicity m = wire tab_mult0 + k;
 *   unused table slots repeat a real entry, unused looking slots look a real entry up;  n_look = n_tab = 0: no lookups (the calls
 *   below do nothing);
 *   tag_const0 = 0: ONE table; every call, transcript and proof is what it was before this word had a meaning.  Non-zero: SEVERAL
 *   TABLES told apart by a tag, in two consecutive constant columns (not selector columns): column tag_const0 holds the tag of every
 *   looking row, column tag_const0 + 1 the tag of every table row.  A tag is any field value, whatever u64 holds it; all slots of a
 *   row share its tag, and unmarked rows may hold anything there.  An entry is then the triple (tag, x, y): a pair that exists only
 *   under another tag is absent.
 * Refusals: n_look or n_tab above 128 SIPP_E_UNSUPPORTED; a column outside the circuit, q_look or q_tab below num_selectors, one of
 * n_look / n_tab zero and the other not, a non-zero tag_const0 below num_selectors or with tag_const0 + 1 >= num_constants (or in an
 * empty description), a marker cell that is neither 0 nor 1: SIPP_E_BADARG.
 * d_wires [num_wires][N], d_constants [num_constants][N] (the constant columns in front of the constants_sigmas batch): VALUES in
 * natural row order.  A looking or table value is its field value, whatever u64 holds it.
 *
 * sipp_plonk_lookup_multiplicities: zeroes the m cells of the table rows, then adds one for every slot of every looking row to the
 * table slot with the equal pair (with tags: the equal (tag, x, y), the looking row's tag against the table row's).  Among equal
 * table entries the first in (row, slot) order takes every look; the search goes through a sorted index of the table's distinct
 * entries (built here on the host from the constant columns), so the counts do not depend on the order the device reaches the rows
 * in.  A looked-up pair that is in no table slot of its tag: SIPP_E_WITNESS (a device flag read back once; the m cells are then
 * unspecified, the ctx stays usable).
 *
 * sipp_plonk_lookup_sums: the running-sum columns for the caller's eta, theta (num_challenges host words each; any u64 congruent to
 * the value).  With D = max_degree, the looking slots in Jl = ceil(n_look / D) groups of up to D and the table slots in Jt =
 * ceil(n_tab / D) groups, J = Jl + Jt, per challenge and row:
 *   looking group j:  U_j - U_(j-1) = q_look sum_k 1 / d_k,        d_k = theta - (x_k + eta y_k + eta^2 tag_look(row))
 *   table group j:    U_j - U_(j-1) = - q_tab sum_k m_k / e_k,     e_k = theta - (tx_k + eta ty_k + eta^2 tag_tab(row))
 * (the eta^2 terms only with tag_const0 != 0; a constant column has a wire's degree, so no term's degree and no column count changes)
 * U_(-1) = S(x), U_(J-1) = S(g x), S(1) = 0.  d_out [num_challenges J][N], the order of the columns behind the permutation's in the
 * zs_partial_products oracle: S_0 .. S_(C-1), then U_0 .. U_(J-2) of challenge 0, of challenge 1, ...
 * (sipp_plonk_lookup_num_columns = num_challenges J; 0 for an empty description or one outside the supported range).
 * A row whose marker is 0 contributes 0 whatever it holds.  On a marked row a vanishing d_k or e_k (theta hit a combination) is
 * SIPP_E_WITNESS -- not 1 / 0 = 0; d_out is then unspecified. */
uint32_t sipp_plonk_lookup_num_columns(const sipp_plonk_params *p, const uint32_t *lookup);
int sipp_plonk_lookup_multiplicities(sipp_ctx *ctx, uint64_t *d_wires, const uint64_t *d_constants, uint32_t log_n, uint32_t num_wires,
                                     uint32_t num_constants, uint32_t num_selectors, const uint32_t *lookup);
int sipp_plonk_lookup_sums(sipp_ctx *ctx, const uint64_t *d_wires, const uint64_t *d_constants, uint32_t log_n, uint32_t num_wires,
                           uint32_t num_constants, uint32_t num_selectors, const sipp_plonk_params *p, const uint32_t *lookup,
                           const uint64_t *etas, const uint64_t *thetas, uint64_t *d_out);
/* The whole argument: sipp_plonk_prove_gates / sipp_plonk_gates_proof_size / sipp_plonk_verify_gates with a description (`lookup`,
 * eight words, never NULL).  An EMPTY description is those calls, the proof "SIPPPLK3" byte for byte.  With a non-empty one:
 *   - the transcript draws eta_0 .. eta_(C-1), then theta_0 .. theta_(C-1) behind the gammas;
 *   - the S / U columns of sipp_plonk_lookup_sums go behind the Z / partial-product columns of the zs_partial_products oracle;
 *   - the C boundary terms L_0(x) S_c(x), then challenge by challenge the J chain terms
 *       looking group:  (U_j - U_(j-1)) Dl - q_look Nl,   Dl = prod_k d_k,  Nl = sum_k prod_(k' != k) d_k'
 *       table group:    (U_j - U_(j-1)) Dt + q_tab Nt,    Dt = prod_k e_k,  Nt = sum_k m_k prod_(k' != k) e_k'
 *     follow the gate-constraint terms in the one reduce_with_powers list (each of degree <= max_degree + 1, as a partial-product term);
 *   - batch 0 opens every new column at zeta, batch 1 the S columns at g zeta behind the Z columns;
 *   - flat proof "SIPPPLK4": header[24] = the sixteen words of "SIPPPLK3" with the new magic, then the eight description words
 *     | wires cap | zs_partial_products cap | quotient cap | opening proof | public_inputs.
 * The wire table holds the multiplicities already (sipp_plonk_lookup_multiplicities); a table the caller spoiled gives a proof the
 * verifier refuses (stage 210) or SIPP_E_WITNESS (theta on a combination).  The verifier refuses (201) a header whose eight words are
 * not the caller's description, and a description that does not fit the circuit; the lookup terms are part of the stage-210 check.
 * sipp_circuit_set_lookup: the description of a circuit data (refusals as above; the sorted index of the table is built here, once).
 * After it sipp_circuit_prove / _prove_inputs / _prove_words run the multiplicities behind witness generation and prove with the
 * description, sipp_circuit_proof_size and sipp_circuit_verify follow it.  An empty description takes it off again. */
size_t sipp_plonk_gates_lookup_proof_size(uint32_t log_n, const sipp_plonk_params *p, const sipp_fri_params *fp, const sipp_plonk_circuit *c,
                                          uint32_t n_public_inputs, const uint32_t *lookup);
int sipp_plonk_prove_gates_lookup(sipp_ctx *ctx, const uint64_t *d_wires, const uint64_t *d_constants_sigmas, const sipp_oracle *wires_oracle,
                                  const uint64_t *wires_cap, const sipp_oracle *constants_sigmas_oracle, uint32_t log_n,
                                  const sipp_plonk_params *p, const sipp_fri_params *fp, const sipp_plonk_circuit *c,
                                  const uint64_t circuit_digest[4], const uint64_t *public_inputs, uint32_t n_public_inputs,
                                  const uint32_t *lookup, uint64_t *proof_out, size_t proof_cap, size_t *proof_len);
int sipp_plonk_verify_gates_lookup(const uint64_t *proof, size_t len, const uint64_t *constants_sigmas_cap, const sipp_plonk_params *p,
                                   const sipp_fri_params *fp, const sipp_plonk_circuit *c, const uint64_t circuit_digest[4],
                                   const uint32_t *lookup, int *reason);
int sipp_circuit_set_lookup(sipp_circuit_data *cd, const uint32_t *lookup);

/* ---- ZERO KNOWLEDGE: salted oracles and blinding rows, the randomness drawn on the device from a seed ---------
 * What plonky2's `zero_knowledge` switch does, as recalled: the wires, Z / partial-products and quotient oracles carry SIPP_SALT_SIZE
 * salt words per leaf (FriParams::hiding), and the circuit carries blinding rows.  ONE random function serves both:
 *   block(seed[4], counter, stream, index) = the first 8 words of hash_n_to_m_no_pad([seed0..3, counter, stream, index], 8), that is one
 *   Poseidon permutation of [seed0, seed1, seed2, seed3, counter, stream, index, 0, 0, 0, 0, 0]; every output is canonical.
 *   seed: four canonical words, secret and fresh per prover (a word >= p: SIPP_E_BADARG; the same for a counter >= p);
 *   counter: the number of the proof under this seed -- two proofs never share blinding;
 *   stream: 0 = blinding rows, 1 = wires salt, 2 = Z / partial-products salt, 3 = quotient salt.
 *   Salt: leaf j of stream s, in LEAF order (the order of d_lde), takes words 4 (j & 1) .. 4 (j & 1) + 3 of block(seed, counter, s, j >> 1).
 *   Blinding rows: wire w of table row r takes word w & 7 of block(seed, counter, 0, r 2^9 + (w >> 3))  (num_wires <= 4096).
 * sipp_blind_salt: the four salt columns of one oracle, written behind its ncols polynomial columns: d_lde [ncols + 4][2^log_m] in leaf
 * order, 16-byte aligned, stream 1 .. 3.  For callers that commit their wires themselves.
 * SIPP_GEN_RANDOM (p = first wire, number of wires; first + number <= num_wires): on its rows those wires take the blinding-row words.
 * It depends on no other cell: both witness calls fill its rows with a kernel of their own before anything else runs.  The seed reaches
 * it through the _blind siblings of the two witness calls (the plain names pass NULL); a SIPP_GEN_RANDOM generator without a seed is
 * SIPP_E_BADARG, as a PublicInput generator without its hash.
 * sipp_plonk_prove_gates_zk: sipp_plonk_prove_gates_lookup with `blind`.  NULL: that call, byte for byte.  Not NULL: fp->hiding must be 1
 * (and blind must not be NULL under a hiding fp): SIPP_E_BADARG otherwise.  Oracles 1 .. 3 then hold four salt columns behind their
 * polynomials, filled by one launch before the first commitment, and are opened with n_salt = 4; constants_sigmas is never salted.  A
 * pre-committed wires oracle brings its own salt: n_salt must be 4 under blinding and 0 without.
 * Flat proof "SIPPPLK5": the 24 header words of "SIPPPLK4" with the new magic and header[12] = 1; the eight description words are all
 * zero without lookups.  Caps, opening section and public inputs follow as before.
 * Verification: sipp_plonk_verify_gates / _verify_gates_lookup decide by fp->hiding which proof they accept: under hiding = 1 only
 * "SIPPPLK5" with header[12] = 1, opened with n_salt = {0, 4, 4, 4}; under hiding = 0 only "SIPPPLK3" / "SIPPPLK4".  Anything else is
 * stage 201.
 * Circuit data: sipp_circuit_build accepts a hiding fp.  sipp_circuit_set_blinding sets the seed and zeroes the counter; every
 * sipp_circuit_prove / _prove_inputs / _prove_words uses the current counter, then increments it (a refusal increments it too).  A hiding
 * circuit data without a seed proves nothing (SIPP_E_BADARG); a seed on a non-hiding one is SIPP_E_BADARG. */
#define SIPP_GEN_RANDOM 18
/* `blind` below: FIVE u64 words -- seed[0 .. 3], then the counter -- which is the memory of this struct (a caller that holds one passes
 * its address, cast); NULL where the text above allows none */
typedef struct sipp_blinding { uint64_t seed[4]; uint64_t counter; } sipp_blinding;
int sipp_blind_salt(sipp_ctx *ctx, uint64_t *d_lde, uint32_t ncols, uint32_t log_m, const uint64_t *blind, uint32_t stream);
int sipp_plonk_generate_witness_blind(sipp_ctx *ctx, uint64_t *d_wires, const uint64_t *d_constants, uint32_t log_n, uint32_t num_wires,
                                      uint32_t num_constants, const sipp_plonk_generator *gens, size_t n_gens,
                                      const uint64_t public_inputs_hash[4], const uint64_t *blind);
int sipp_plonk_generate_witness_levels_blind(sipp_ctx *ctx, uint64_t *d_wires, const uint64_t *d_constants, uint32_t log_n,
                                             uint32_t num_wires, uint32_t num_constants, const sipp_plonk_generator *gens, size_t n_gens,
                                             const uint64_t public_inputs_hash[4], const sipp_plonk_schedule *sched,
                                             const uint64_t *blind);
size_t sipp_plonk_gates_zk_proof_size(uint32_t log_n, const sipp_plonk_params *p, const sipp_fri_params *fp, const sipp_plonk_circuit *c,
                                      uint32_t n_public_inputs, const uint32_t *lookup);
int sipp_plonk_prove_gates_zk(sipp_ctx *ctx, const uint64_t *d_wires, const uint64_t *d_constants_sigmas, const sipp_oracle *wires_oracle,
                              const uint64_t *wires_cap, const sipp_oracle *constants_sigmas_oracle, uint32_t log_n,
                              const sipp_plonk_params *p, const sipp_fri_params *fp, const sipp_plonk_circuit *c,
                              const uint64_t circuit_digest[4], const uint64_t *public_inputs, uint32_t n_public_inputs,
                              const uint32_t *lookup, const uint64_t *blind, uint64_t *proof_out, size_t proof_cap, size_t *proof_len);
int sipp_circuit_set_blinding(sipp_circuit_data *cd, const uint64_t seed[4]);

/* ---- verification of the generic proofs (host code like sipp_stark_verify; stages in *reason, may be NULL) -------------------------
 * sipp_fri_verify_openings: PolynomialBatch::verify_openings over a proof of sipp_fri_prove_openings -- caps[o] = the cap of oracle o
 * (2^cap_height x 4 words), ncols / n_salt (may be NULL = 0) per oracle, the batches as proved; the caller's transcript goes in and
 * comes out (the opened values are observed as they are read).  Stages: 100 header, 106 truncated openings, 120 .. 133 as in
 * sipp_stark_verify, 140 trailing words, 141 a non-canonical word.
 * sipp_plonk_verify_gates: plonk/verifier.rs for a proof of sipp_plonk_prove_gates ("SIPPPLK3") -- what `data.verify(proof)` (reference
 * src/verifier_circuit.rs:254) does with the outer proof: the gate constraints at zeta from the OPENED constants and wires through the
 * same gate programs, Z(1) = 1, the partial products, one reduce_with_powers per challenge against the quotient chunks, the opening
 * proof.  constants_sigmas_cap and circuit_digest are the circuit's (verifier data).  Stages: 201 header / circuit / parameters,
 * 202 size, 203 truncated, 210 the vanishing polynomial does not meet the quotient, then the FRI stages above. */
int sipp_fri_verify_openings(const uint64_t *proof, size_t len, const uint64_t *const *caps, const uint32_t *ncols, const uint32_t *n_salt,
                             size_t n_oracles, const sipp_fri_batch *batches, size_t n_batches, uint32_t log_n, const sipp_fri_params *p,
                             sipp_challenger *ch, int *reason);
int sipp_plonk_verify_gates(const uint64_t *proof, size_t len, const uint64_t *constants_sigmas_cap, const sipp_plonk_params *p,
                            const sipp_fri_params *fp, const sipp_plonk_circuit *c, const uint64_t circuit_digest[4], int *reason);

/* ---- KECCAK-256 MERKLE TREES: plonky2's KeccakGoldilocksConfig for the generic commitments and the outer prover ----
 * The tree hasher is an explicit argument of the _h entries: SIPP_HASH_POSEIDON (0) is the entry without the suffix, byte for byte;
 * SIPP_HASH_KECCAK25 (1) hashes leaves, nodes and caps with Keccak-256 truncated to 25 bytes (KeccakHash<25>); anything else is
 * SIPP_E_BADARG.  The challenger, the proof of work and the public-input hash stay Poseidon under either.  The hash, as recalled from
 * plonky2 hash/keccak.rs:
 *   keccak256 is original Keccak (rate 136 bytes, padding 0x01 .. 0x80, not SHA-3's 0x06);
 *   hash_no_pad(elements): every element as its CANONICAL u64, 8 bytes little endian, concatenated; keccak256; the first 25 bytes;
 *   hash_or_noop(elements): at most 3 elements (24 bytes): the bytes in a zeroed 25-byte array, nothing hashed; else hash_no_pad;
 *   two_to_one(l, r): keccak256 of the 50 bytes l || r, the first 25 bytes;
 *   a digest is FOUR u64 words -- bytes 0..6, 7..13, 14..20, 21..24, little endian (BytesHash::to_vec) -- so words 0 - 2 are below 2^56
 *   and word 3 below 2^32: canonical field elements, observed by the Poseidon challenger like any cap.  Tree layout, cap sizes, proof
 *   sizes and proof layouts are those of the Poseidon trees (the size functions serve both).  Salt words are leaf elements like any other.
 * sipp_merkle_leaves_h: hash_or_noop of every leaf, d_lde [ncols][2^log_leaves] leaf order -> d_digests [2^log_leaves][4]; the words
 *   of d_lde may be any u64 congruent to the element (they are reduced before they are hashed).  log_leaves <= 31 here and below
 *   (one lane per leaf in one launch): SIPP_E_BADARG beyond.
 * sipp_merkle_levels_h: the levels above the leaf digests up to the cap (min(cap_height, log_leaves)), cap_out as sipp_merkle_cap.
 * sipp_fri_leaves_h: the leaves of a FRI layer tree: d_vals [2][len] (c0 row, c1 row; leaf order), leaf k = the 2^arity_bits values
 *   from k 2^arity_bits, flattened (c0, c1) -> d_digests [len >> arity_bits][4].  Arity 2 (four words) is hashed under Keccak.
 * sipp_host_keccak256: keccak256 of len bytes on the host, out32 = 32 bytes.  sipp_host_merkle_hash: the host verifier's node functions
 *   under either hasher (host_tree_hash.hpp, the text verify.cpp climbs paths with; test surface): right == NULL: out4 = hash_or_noop(elements[0 .. n)); else n = 4 and out4 = two_to_one(elements, right).
 * sipp_commit_batch_h / sipp_fri_prove_openings_h / sipp_fri_verify_openings_h: sipp_commit_batch_ex / sipp_fri_prove_openings /
 *   sipp_fri_verify_openings with the hasher.  All oracles and all layer trees of one opening proof use one hasher (a tree committed with
 *   the other fails verification at its Merkle stage).  Under Keccak the verifier refuses (141) a cap or sibling word outside its range
 *   -- words 0 - 2 at or above 2^56, word 3 at or above 2^32 -- whose high bits the repacking would otherwise drop.
 * sipp_plonk_prove_gates_h: sipp_plonk_prove_gates_zk (lookup description and blinding words, either may be NULL = none) with the
 *   hasher; sipp_plonk_verify_gates_h: sipp_plonk_verify_gates_lookup (lookup may be NULL) with the hasher.  The flat "SIPPPLK3/4/5" proof
 *   records the hasher in header[13] (zero before, zero under Poseidon); the verifier refuses (201) a header[13] that is not its argument.
 *   Pre-committed oracles must have been committed with the same hasher.
 * sipp_circuit_build_h: sipp_circuit_build with the hasher; the circuit data remembers it: its constants_sigmas commitment, the three
 *   prove calls and sipp_circuit_verify follow it.  The derived circuit digest (circuit_digest == NULL) stays the Poseidon hash of the cap
 *   and the common data (plonky2 would hash it with the tree hasher). */
#define SIPP_HASH_POSEIDON 0u
#define SIPP_HASH_KECCAK25 1u
int sipp_merkle_leaves_h(sipp_ctx *ctx, const uint64_t *d_lde, size_t ncols, uint32_t log_leaves, uint32_t hasher, uint64_t *d_digests);
int sipp_merkle_levels_h(sipp_ctx *ctx, uint64_t *d_tree, uint32_t log_leaves, uint32_t cap_height, uint32_t hasher, uint64_t *cap_out);
int sipp_fri_leaves_h(sipp_ctx *ctx, const uint64_t *d_vals, size_t len, uint32_t arity_bits, uint32_t hasher, uint64_t *d_digests);
int sipp_host_keccak256(const void *bytes, size_t len, void *out32);
int sipp_host_merkle_hash(uint32_t hasher, const uint64_t *elements, size_t n, const uint64_t *right, uint64_t *out4);
int sipp_commit_batch_h(sipp_ctx *ctx, const uint64_t *d_in, int from_coeffs, uint64_t *d_coeffs, uint64_t *d_lde,
                        uint64_t *d_tree, size_t ncols, uint32_t log_n, uint32_t rate_bits, uint32_t cap_height,
                        const uint64_t *d_salt, uint32_t n_salt, uint32_t hasher, uint64_t *cap_out);
int sipp_fri_prove_openings_h(sipp_ctx *ctx, const sipp_oracle *oracles, size_t n_oracles, const sipp_fri_batch *batches,
                              size_t n_batches, uint32_t log_n, const sipp_fri_params *p, uint32_t hasher, sipp_challenger *ch,
                              uint64_t *proof_out, size_t proof_cap, size_t *proof_len);
int sipp_fri_verify_openings_h(const uint64_t *proof, size_t len, const uint64_t *const *caps, const uint32_t *ncols, const uint32_t *n_salt,
                               size_t n_oracles, const sipp_fri_batch *batches, size_t n_batches, uint32_t log_n, const sipp_fri_params *p,
                               uint32_t hasher, sipp_challenger *ch, int *reason);
int sipp_plonk_prove_gates_h(sipp_ctx *ctx, const uint64_t *d_wires, const uint64_t *d_constants_sigmas, const sipp_oracle *wires_oracle,
                             const uint64_t *wires_cap, const sipp_oracle *constants_sigmas_oracle, uint32_t log_n,
                             const sipp_plonk_params *p, const sipp_fri_params *fp, const sipp_plonk_circuit *c,
                             const uint64_t circuit_digest[4], const uint64_t *public_inputs, uint32_t n_public_inputs,
                             const uint32_t *lookup, const uint64_t *blind, uint32_t hasher, uint64_t *proof_out, size_t proof_cap,
                             size_t *proof_len);
int sipp_plonk_verify_gates_h(const uint64_t *proof, size_t len, const uint64_t *constants_sigmas_cap, const sipp_plonk_params *p,
                              const sipp_fri_params *fp, const sipp_plonk_circuit *c, const uint64_t circuit_digest[4],
                              const uint32_t *lookup, uint32_t hasher, int *reason);
int sipp_circuit_build_h(sipp_ctx *ctx, uint32_t log_n, const sipp_plonk_params *p, const sipp_fri_params *fp, const sipp_plonk_circuit *c,
                         const uint64_t *constants_sigmas, const sipp_plonk_generator *gens, size_t n_gens,
                         const sipp_plonk_schedule_host *sched, const uint64_t *circuit_digest, uint32_t hasher, sipp_circuit_data **out);

/* ---- building blocks (device buffers; used by the parity tests and bench.py) -- */
/* plonky2 fft()/ifft(): natural order in, natural order out, in place.
 * d_cols is [ncols][col_stride] u64 with the first 2^log_n entries of each column used. */
int sipp_ntt_batch(sipp_ctx *ctx, uint64_t *d_cols, size_t col_stride, size_t ncols, uint32_t log_n, int inverse);
/* PolynomialBatch::from_values, column-major and transpose-free:
 *   d_values [ncols][N] natural order  ->  d_coeffs [ncols][N] (natural, may alias d_values)
 *   d_lde [ncols][N << rate_bits] in LEAF order (position j = natural LDE row bitrev(j)).
 * ALIGNMENT (this call, sipp_commit_batch, sipp_commit_batch_ex and the oracles handed to the plonk entry points): for columns of
 * 2^13 rows and more every device pointer must be 16-byte aligned (the transforms move 16 bytes per lane); an 8-byte-aligned
 * view is SIPP_E_BADARG.  hipMalloc / torch allocations are; slices at odd u64 offsets are not. */
int sipp_lde_batch(sipp_ctx *ctx, const uint64_t *d_values, uint64_t *d_coeffs, uint64_t *d_lde, size_t ncols,
                   uint32_t log_n);
/* hash_or_noop of every leaf: d_lde [ncols][n_leaves] leaf order -> d_digests [n_leaves][4] */
int sipp_poseidon_leaves(sipp_ctx *ctx, const uint64_t *d_lde, size_t ncols, uint32_t log_leaves,
                         uint64_t *d_digests);
/* Merkle levels above the leaf digests; d_tree holds every level back to back
 * (level l at digest offset sum_{i<l} n_leaves >> i), level 0 = leaf digests (input).
 * cap_out (host, 2^cap_height * 4 u64) receives the cap. */
int sipp_merkle_cap(sipp_ctx *ctx, uint64_t *d_tree, uint32_t log_leaves, uint64_t *cap_out);
/* values -> (coeffs, lde, tree, cap) in one call; d_tree sized 2 * n_leaves * 4 u64 */
int sipp_commit_batch(sipp_ctx *ctx, const uint64_t *d_values, uint64_t *d_coeffs, uint64_t *d_lde,
                      uint64_t *d_tree, size_t ncols, uint32_t log_n, uint64_t *cap_out);
/* Trace generation only (test surface for the trace-fill kernels): ios as for sipp_*_exp_prove;
 * d_trace receives the column-major trace [width][2^log_rows] in natural row order, where
 * width = main_cols of sipp_stark_shape.  d_trace must hold width * 2^log_rows u64. */
int sipp_trace_build(sipp_ctx *ctx, int kind, const uint32_t *ios, size_t num_io, uint64_t *d_trace);
/* batched Poseidon permutation of n states, d_states [n][12] in place (KAT surface) */
int sipp_poseidon_permute(sipp_ctx *ctx, uint64_t *d_states, size_t n);
/* the HOST permutation of the Fiat-Shamir challenger (no GPU involved): n states [n][12] in host memory, in place.
 * impl: -1 = the implementation the provers use on this CPU, 0 = portable scalar, 1 = scalar with look-ahead partial
 * rounds, 2 / 3 = AVX-512 (SIPP_E_UNSUPPORTED when the CPU lacks it).  All are bit-identical. */
int sipp_host_poseidon_permute(uint64_t *states, size_t n, int impl);

/* ---- measurement ------------------------------------------------------------- */
/* Per-kernel HIP-event timing on the ctx stream (the stream the kernels run on).
 * enable != 0 starts bracketing every launch with an event pair. */
int sipp_profile_enable(sipp_ctx *ctx, int enable);
int sipp_profile_reset(sipp_ctx *ctx);
/* writes a JSON object {"kernel": {"calls": n, "ms": total}, ...} into buf */
int sipp_profile_report(sipp_ctx *ctx, char *buf, size_t cap);
/* wall-clock bracket on the ctx stream */
int sipp_timer_start(sipp_ctx *ctx);
int sipp_timer_stop(sipp_ctx *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif
