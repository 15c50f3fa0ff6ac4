/*
 * ddl_amd.h — C-ABI of the MI355X gradient-bucket allreduce engine.
 *
 * This is the drop-in boundary for the reference's allreduce hot path
 * (LYL232/Experiment-Distributed-Deep-Learning, paths relative to its src/):
 *
 *   reference                                             replaced by
 *   ---------------------------------------------------   -----------------------------
 *   cpp/c_api.h:15-17   communicator_rank/size            communicator_rank/size
 *   cpp/c_api.h:19      world_communicator                world_communicator
 *   cpp/c_api.h:33-35   split/detach_communicator         split_communicator/detach_communicator
 *   cpp/c_api.h:37-41   py_info/py_debug/py_error         py_info/py_debug/py_error
 *   cpp/global/initialize.cc:57-65 + MPIBackend.cc:77-97  ddl_get_unique_id + ddl_init
 *     (MPI_Init_thread at dlopen)                          (explicit RCCL bootstrap)
 *   cpp/communicate/backend/Communicator.h:45-48 /        ddl_allreduce (device buffers; at
 *     mpi/MPICommunicator.cc:14-28  (MPI_Allreduce SUM)     P > 2 by default the direct schedule:
 *                                                          reduce-scatter of slices to every peer
 *                                                          over RCCL send/recv, a HIP fold of the P
 *                                                          inputs in MPICH's order, allgather; a
 *                                                          ring at P = 2; autotuned per size class)
 *   cpp/op/tensorflow/AllreduceOp.cc:32-66 →              ddl_allreduce_submit
 *     TensorsCollectiveCommunicateController::handleRequest (keyed async request, done callback)
 *     (.../controller/TensorsCollectiveCommunicateController.h:14-34)
 *
 * Conventions (mirroring the reference):
 *   - communicator ids are 64-bit integers (Communicator::ID = long long, Communicator.h:20);
 *   - dtypes use tensorflow::DataType numbers, as the reference does (def.h:10 uses
 *     tensorflow::DataType; ascending enum order is the fusion group order,
 *     MPIRingTokenCommunication.cc:735-749);
 *   - every call returns an int status (StatusCode, def.h:70-74, extended); no C++
 *     exception crosses this boundary; ddl_last_error() describes the last failure
 *     on the calling thread;
 *   - buffers are device (HBM) pointers; hip_stream is a hipStream_t (NULL = legacy
 *     default stream); calls are stream-ordered and never synchronise the host unless
 *     documented.
 */
#ifndef DDL_AMD_H
#define DDL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* tensorflow::DataType numeric values (reference def.h:10-53 comment block). */
enum ddl_dtype {
    DDL_FLOAT = 1,
    DDL_DOUBLE = 2,
    DDL_INT32 = 3,
    DDL_INT64 = 9,
    DDL_BFLOAT16 = 14, /* extension: the reference rejects it (AllreduceOp.cc:18) */
    DDL_HALF = 19,     /* extension: the reference rejects it (MPIBackend.cc:48-66) */
    DDL_UINT64 = 23
};

/* StatusCode (reference def.h:70-74) + extensions. */
enum ddl_status {
    DDL_STATUS_OK = 0,
    DDL_STATUS_COMM_ERROR = 1, /* was STATUS_MPI_ERROR: RCCL / control-channel failure */
    DDL_STATUS_ERROR_UNKNOWN = 2,
    DDL_STATUS_INVALID_ARGUMENT = 3,
    DDL_STATUS_UNSUPPORTED_DTYPE = 4,
    DDL_STATUS_HIP_ERROR = 5,
    DDL_STATUS_NOT_INITIALIZED = 6,
    DDL_STATUS_DUPLICATE_KEY = 7, /* TensorCommunicateRequest.h:21: one pending request per key */
    DDL_STATUS_CONFIG_MISMATCH = 8 /* the ranks' shared tunables differ (see ddl_set_config): the
                                      collective or keyed round fails on every rank, nothing runs */
};

/* Where a keyed request's buffers live: SURVEY §8(b)'s device_ptr_flag. The reference's op is
 * CPU-only (AllreduceOp.cc:68): its tensors are host memory, copied into the MPI buffer
 * (MPIRingTokenCommunication.cc:548-733). Host requests are staged through pinned chunks to the
 * device and back; device requests stay in HBM. */
enum ddl_memory { DDL_MEMORY_DEVICE = 0, DDL_MEMORY_HOST = 1 };

/* Communicator::AllreduceOperation (reference Communicator.h:22-24 has SUM only). AVG (MI355X
 * extension) is the SUM result divided by the communicator's size, the quotient taken on the GPU
 * by the kernel that writes the result (see the data-plane section). MIN / MAX (MI355X extension,
 * Horovod's numbers; 2 is not an op) are the element-wise minimum / maximum over the ranks. */
enum ddl_allreduce_op { DDL_ALLREDUCE_OP_SUM = 0, DDL_ALLREDUCE_OP_AVG = 1, DDL_ALLREDUCE_OP_MIN = 3,
                        DDL_ALLREDUCE_OP_MAX = 4 };
/* Wire format of a keyed device allreduce of DDL_FLOAT tensors (MI355X extension, Horovod's
 * Compression.fp16): at most one flag, OR-ed into `op`. The gradients travel and are summed as
 * 16-bit values and come back as fp32 (see the data-plane section). */
enum ddl_allreduce_wire { DDL_ALLREDUCE_WIRE_FP16 = 0x100, DDL_ALLREDUCE_WIRE_BF16 = 0x200,
                          /* error feedback: only OR-ed with exactly one of the two above */
                          DDL_ALLREDUCE_WIRE_FEEDBACK = 0x1000 };
/* Stochastic rounding onto the bf16 wire (MI355X extension; the data-plane section): one more bit of the
 * same `op`, valid only OR-ed with DDL_ALLREDUCE_WIRE_BF16 and never with DDL_ALLREDUCE_WIRE_FEEDBACK. */
enum ddl_allreduce_wire_rounding { DDL_ALLREDUCE_WIRE_STOCHASTIC = 0x8000 };
/* The block-scaled 8-bit wire (MI355X extension; "The e4m3 wire" in the data-plane section): OCP e4m3fn codes
 * with one power-of-two fp32 scale per 252 elements. OR-ed into the `op` (SUM or AVG) of the keyed entry points
 * for DDL_FLOAT device requests, optionally with DDL_ALLREDUCE_SUMSQ and DDL_ALLREDUCE_SCALE; never with a
 * ddl_allreduce_wire flag, DDL_ALLREDUCE_WIRE_FEEDBACK or DDL_ALLREDUCE_WIRE_STOCHASTIC. */
enum ddl_allreduce_wire8 { DDL_ALLREDUCE_WIRE_E4M3 = 0x20000 };
/* Error feedback of the e4m3 wire ("Error feedback of the e4m3 wire" in the data-plane section): one more bit of
 * the same `op`, valid only OR-ed with DDL_ALLREDUCE_WIRE_E4M3. A bit of its own, not DDL_ALLREDUCE_WIRE_FEEDBACK
 * (which stays refused with WIRE_E4M3): another rule — per granule, no overflow case, another byte cost. */
enum ddl_allreduce_wire8_feedback { DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK = 0x40000 };
/* Sum of squares of a keyed device allreduce of DDL_FLOAT or DDL_BFLOAT16 tensors (MI355X extension; the data-plane
 * section): OR-ed into the `op` of ddl_allreduce_submit / _submit_batch (and _submit_mem /
 * _submit_batch_mem with DDL_MEMORY_DEVICE), SUM or AVG, with or without a wire flag. With the bit
 * `user` (every users[i] of a batch) points to a ddl_sumsq_arg, read during the call only: `done`
 * receives arg->user, and *arg->sumsq (host memory, valid until `done`; NULL = this request does not
 * want it) holds the value when `done` fires with DDL_STATUS_OK. */
enum ddl_allreduce_stat { DDL_ALLREDUCE_SUMSQ = 0x2000 };
struct ddl_sumsq_arg {
    void *user;    /* what `done` receives */
    double *sumsq; /* where the sum of squares goes, or NULL */
};

/* Scale factors of a keyed device allreduce of DDL_FLOAT or DDL_BFLOAT16 tensors (MI355X extension, Horovod's
 * prescale_factor / postscale_factor; the data-plane section): OR-ed into the `op` of the same entry
 * points as DDL_ALLREDUCE_SUMSQ, SUM or AVG, with or without a wire flag, the feedback bit and
 * DDL_ALLREDUCE_SUMSQ. With the bit `user` (every users[i] of a batch) points to a ddl_scale_arg, read
 * during the call only; `done` receives arg->user. Its first two members are ddl_sumsq_arg's, so with
 * DDL_ALLREDUCE_SCALE | DDL_ALLREDUCE_SUMSQ `sumsq` is read from the same struct; without the SUMSQ bit
 * `sumsq` is ignored. */
enum ddl_allreduce_scale { DDL_ALLREDUCE_SCALE = 0x4000 };
struct ddl_scale_arg {
    void *user;      /* what `done` receives */
    double *sumsq;   /* with DDL_ALLREDUCE_SUMSQ: where the sum of squares goes, or NULL */
    float prescale;  /* finite, > 0; 1.0f = absent */
    float postscale; /* finite, > 0; 1.0f = absent */
};

typedef long long ddl_communicator_id;

/* Completion callback of a keyed request: TensorCommunicateRequest::done(StatusCode)
 * (reference TensorCommunicateRequest.h:41). Runs on the communicator's engine thread. */
typedef void (*ddl_done_fn)(int status, void *user);

/* Output allocation of a keyed allgather, called on the engine thread once the gathered first
 * dimension is known (the reference allocates through OpContext::allocateOutput,
 * MPIRingTokenCommunication.cc:299-306): returns a device buffer of `bytes` for an output of
 * `first_dim` rows, or NULL on failure (the request then completes with an error). */
typedef void *(*ddl_alloc_fn)(size_t first_dim, size_t bytes, void *user);

/* ---- library / lifecycle ------------------------------------------------------- */
int ddl_version(void);
/* "src=<sha1 of the engine sources, 16 hex> arch=gfx950": which sources this library was built
 * from (tests rebuild a stale library rather than test it). */
const char *ddl_build_info(void);
const char *ddl_last_error(void);
const char *ddl_dtype_name(int dtype);
size_t ddl_dtype_size(int dtype); /* 0 for unsupported */

/* RCCL bootstrap id (128 bytes). Rank 0 creates it and the launcher distributes it. */
int ddl_get_unique_id(void *out, size_t len);
/* Creates the world communicator for this process (one process per GPU). */
int ddl_init(int rank, int size, int device, const void *unique_id, size_t len);

/* Same, for a single-process world (size 1); no RCCL involved. */
int ddl_init_single(int device);
/* Optional control channel for keyed requests at size > 1: TCP links in a star around rank 0
 * (3 hops per negotiation round at any size), replacing the MPI p2p token ring
 * (MPIRingTokenCommunication.cc:29-102) with the same token header. ddl_control_listen opens a
 * listener and returns "ip:port"; ddl_control_connect takes every rank's endpoint, separated by
 * ';', in rank order. */
int ddl_control_listen(char *endpoint_out, size_t len);
int ddl_control_connect(const char *endpoints);
/* Negotiation rounds so far by token form: ids as strings, or as indices into the table of ids
 * agreed in earlier rounds (a repeated key set, e.g. every training step's gradients). */
int ddl_control_stats(long long *string_rounds, long long *cached_rounds);
int ddl_finalize(void);
int ddl_is_initialized(void);

/* Tunables: "algo" (0 multi-ring, 1 direct all-to-all, 2 one-shot, 3 gather-fold: one
 * ncclAllGather then the rank-order fold, 4 direct-gather: the direct reduce-scatter then one
 * in-place ncclAllGather of the reduced chunks when they are equal), "slice_bytes", "rings", "max_slices",
 * "fusion_threshold_bytes", "log_level", "cycle_time_us", "host_chunk_bytes" (host-staged
 * transfers move in chunks of this size, default 32 MiB), "tune",
 * "host_copy_threads" (memcpy workers of the keyed host staging), "host_zero_copy" (1, default:
 * a keyed host allreduce plan whose outputs are all pinned and mapped on the device — torch
 * pin_memory, hipHostMalloc, hipHostRegister — is unpacked by the fusion kernel straight into
 * them over PCIe, no D2H copy or host memcpy; 0: always stage through the pinned slots; the
 * read-only "host_zero_copy_plans" counts the plans that took that path),
 * "host_numa_bind" (1, default: the handler's engine thread and copy threads bind to the CPUs of
 * the GPU's NUMA node, where pinned host memory lives; 0: placement left to the OS),
 * "host_register_cache_bytes" (0, default = off; > 0: pageable host tensors of keyed requests
 * are hipHostRegister'ed once and the registrations kept, least recently used out past this many
 * bytes, so repeated allreduce(cpu_tensor) calls take the pinned paths — a cached range must be
 * released with ddl_host_unregister before its memory is freed (the torch mirror does this for
 * the tensors it submits); setting it to 0 unregisters every cached range at once, after
 * ddl_wait_all; read-only statistics "host_registered_bytes", "host_register_hits",
 * "host_register_failures", "host_unregistered_ranges"), the read-only timeline of keyed host plans "host_pack_us" / "host_wait_us" /
 * "host_unpack_us" (microseconds the engine thread spent packing chunks, waiting for a pinned
 * slot's DMA / device work, waiting for the unpack lane — staged results are unpacked by their own
 * copy threads while the next chunks are packed), "capture_mode" (0, default: inside a
 * hipGraph capture the program is posted serially on the captured stream — one chain; 2: as a
 * single-stream DAG, every op on the captured stream with its dependencies set explicitly, which
 * keeps the recv / reduce / send overlap in the graph; r03's 1, the forked comm / compute
 * streams, crashed HIP 7.0's hipStreamEndCapture and is refused since r04 — DESIGN §9; so is its
 * older key "capture_forked"), "compute_cu_mask" (0,
 * default: all CUs; 8 / 4 / 2: the compute streams of multi-rank executors and handlers — the
 * reduce / fold / pack kernels that overlap RCCL's send / recv kernels — avoid every 8th / 4th /
 * 2nd CU, which stay free for RCCL; each masked stream takes a hardware queue of its own; read
 * when a communicator's executor / handler is created), "fold_form" (0, default:
 * the N-input fold in its run form from 4 MiB chunks of 7+ inputs, its tile form otherwise; 1 /
 * 2: always the tile / run form), "rccl_min_ctas" / "rccl_max_ctas" (0, default: RCCL's own
 * choice, NCCL_CONFIG_UNDEF_INT; 1..256: ncclConfig_t.minCTAs / maxCTAs of every RCCL
 * communicator created afterwards — ddl_init's ncclCommInitRankConfig, ddl_comm_split's and the
 * keyed data plane's ncclCommSplit — bounding its channel count and with it the p2p channels the
 * direct schedule's concurrent sends and receives spread over; shared tunables),
 * "queue_isolation" (0, default: every engine stream at the default priority; 1: the streams of
 * multi-rank RCCL communicators are created in three stream-priority classes, each of which HIP
 * maps to a pool of in-order hardware queues of its own — the world's direct collectives at the
 * default priority, the world's keyed data plane at the greatest, split communicators at the
 * least — so one communicator's queued RCCL kernels cannot hold another's behind them; env
 * DDL_QUEUE_ISOLATION seeds it; read when a communicator is created; local),
 * "fusion_pipeline_bytes" (keyed fusion plans above this run as a pack / allreduce / unpack
 * pipeline of sub-plans of at most this size; 0 = unpipelined), "one_rank_shortcut" (1: a
 * one-rank world skips the keyed data plane; 0: runs it, for tests), "wire_feedback_epoch" (0,
 * default; per process: a key's error-feedback residual — DDL_ALLREDUCE_WIRE_FEEDBACK, the data-plane
 * section — restarts from zero when this differs from the value it was last written under: raise it
 * after loading a checkpoint or after a change of the loss scale by a large factor),
 * "wire_stochastic_seed" (0, default; per process: the seed of the random bits of
 * DDL_ALLREDUCE_WIRE_STOCHASTIC, the data-plane section; its 64 bits are read when a request is packed;
 * rank-local like "wire_feedback_epoch", not a shared tunable), "pipeline_rounds" (1,
 * default: a completion thread fires a keyed round's done() calls as its plans land while the
 * engine thread negotiates the next round; 0: each round is waited for first), "reference_order" (1,
 * default: every allreduce sum equals the reference's MPI_Allreduce — MPICH 3.3.2 — bit for
 * bit: the direct and one-shot folds add the P inputs in rank order in MPICH's tree, picked by
 * the message size, and "algo" 0 runs as the direct schedule at P > 2; 0: ring order and left
 * folds, within (P-1)·u·Σ|x| of the reference).
 * With "tune" = 1 (default) a communicator of P > 1 ranks picks the schedule (algo, rings,
 * slice size) per bucket-size class (floor(log2 bytes)) the first time it sees that class: a
 * collective timing of a fixed candidate list on scratch buffers, max over ranks, argmin.
 * The shared tunables (algo, slice_bytes, rings, max_slices, fusion_threshold_bytes, tune,
 * fusion_pipeline_bytes, reference_order, host_chunk_bytes, rccl_min_ctas, rccl_max_ctas) must
 * be equal on every rank of a
 * communicator. Direct collectives: the ranks exchange a hash of them at a communicator's first
 * collective and at the next collective after this rank's values changed; a mismatch found there
 * fails that collective on every rank with DDL_STATUS_CONFIG_MISMATCH instead of building
 * different programs. That exchange is itself collective, so it is only matched when EVERY rank
 * changes its shared values between the same two collectives (to equal or different values);
 * changing them on some ranks only, after the first collective, is unsupported — those ranks post
 * an exchange the others never match, and the communicator hangs (there is no per-collective
 * check: it would cost a host-synchronising exchange on every call). Keyed rounds carry each
 * rank's hash in their tokens, so they detect any difference, one-sided included.
 * A change of the shared tunables drops the tuned choices; the other keys are per process. */
int ddl_set_config(const char *key, long long value);
long long ddl_get_config(const char *key);

/* How the ranks of communicator `id` are connected: *kind 0 = one rank (no transport), 1 = RCCL
 * (*ranks = ncclCommCount of its RCCL communicator), 2 = the test transport (*ranks = size). */
int ddl_comm_transport(ddl_communicator_id id, int *kind, int *ranks);

/* ---- reference c_api.h surface ----------------------------------------------------- */
int communicator_rank(ddl_communicator_id id);
int communicator_size(ddl_communicator_id id);
ddl_communicator_id world_communicator(void);
ddl_communicator_id split_communicator(ddl_communicator_id id, int color, int key);
void detach_communicator(ddl_communicator_id id);
void py_info(const char *log_str);
void py_debug(const char *log_str);
void py_error(const char *log_str);

/* ---- data plane ---------------------------------------------------------------------- */
/* The `op` of every allreduce entry point below: DDL_ALLREDUCE_OP_SUM, or DDL_ALLREDUCE_OP_AVG =
 * the SUM result (the same schedules and summation order, already rounded to the dtype) divided
 * by the communicator's size P — what the reference's allreduce_gradient computes with
 * `summed / communicator.size`. The quotient is the correctly rounded IEEE one by (float)P for
 * fp32 and (double)P for fp64; fp16 / bf16 are widened to fp32, divided and rounded to nearest
 * even into the type (numpy's and torch CPU's results, bit for bit). Subnormals are kept, signed
 * zeros and infinities follow IEEE, a NaN stays a NaN. The division is part of the last device
 * write of the result: the fused plans' unpack kernel stores the quotients (also straight into
 * pinned host outputs), every other path divides the result in place with one launch of the same
 * kernel on the caller's stream — no host pass, no launch per tensor. At P = 1 AVG is SUM. AVG on
 * an integer dtype returns DDL_STATUS_UNSUPPORTED_DTYPE and any other op value
 * DDL_STATUS_INVALID_ARGUMENT, from every entry point, before anything is posted. AVG direct
 * collectives (ddl_allreduce, ddl_allreduce_batch) are refused inside a hipGraph capture.
 * SUM against AVG never influences what is communicated: it is a per-request, rank-local property
 * like the output pointer (fusion groups, plans and schedules do not depend on it, and one round,
 * plan or unpack launch may mix SUM and AVG requests). Ranks that disagree about a key's SUM / AVG
 * therefore get different numbers, never a hang.
 *
 * Wire compression: `op` = SUM or AVG, optionally OR-ed with ONE ddl_allreduce_wire flag, on a keyed
 * device request of dtype DDL_FLOAT (ddl_allreduce_submit, _submit_batch, and _submit_mem /
 * _submit_batch_mem with DDL_MEMORY_DEVICE). Definition: every rank's fp32 input is rounded to the
 * wire type (fp16 or bf16) with round-to-nearest-even — overflow becomes +-inf, fp16 subnormals and
 * signed zeros are kept, a NaN stays a NaN (its payload is not pinned); the rounded values are
 * summed in the wire type exactly as a plain DDL_HALF / DDL_BFLOAT16 allreduce of them would be
 * (MPICH's order for the plan's message size with reference_order 1, the message being the plan's
 * unpadded WIRE bytes); the 16-bit sum is widened to fp32, which is exact; with AVG the widened sum
 * is divided by (float)P with the correctly rounded fp32 quotient (one rounding fewer than a 16-bit
 * AVG). Every step is what numpy / torch CPU compute. The conversions are part of the fusion pack
 * and unpack kernels (csrc/pack.hip k_seg<CvtPackOp> / k_seg<CvtUnpackOp>): no extra pass over the
 * tensors; the fusion threshold and the pipeline cuts count wire bytes, and a compressed request
 * always goes through the fusion buffer, also alone in its plan.
 * Unlike SUM / AVG the wire IS communicated: it is a property of a key that every rank must agree
 * on, like its dtype and element count (fp32-over-fp16 requests form a fusion group of their own,
 * after the uncompressed group of the wire dtype, in the same order on every rank). Ranks that
 * disagree about a key's wire flag post different collectives.
 * Refusals, all before anything is registered or posted (the communicator works afterwards): a
 * wire flag on any dtype but DDL_FLOAT returns DDL_STATUS_UNSUPPORTED_DTYPE (a batch takes one
 * `op`, so a non-fp32 entry fails the whole batch: split such batches); both flags together or any
 * other unknown bit, a wire flag with DDL_MEMORY_HOST, and a wire flag on ddl_allreduce,
 * ddl_allreduce_batch or ddl_allreduce_host return DDL_STATUS_INVALID_ARGUMENT.
 * P = 1: with "one_rank_shortcut" 1 nothing is communicated and nothing is compressed — the result
 * is the input, bit for bit; with 0 the data plane runs and the result is the input round-tripped
 * through the wire type.
 *
 * Error feedback (EF-SGD, 1-bit SGD): DDL_ALLREDUCE_WIRE_FEEDBACK, valid only OR-ed with exactly
 * one of WIRE_FP16 / WIRE_BF16 on a keyed DDL_FLOAT device request (ddl_allreduce_submit,
 * _submit_batch, _submit_mem, _submit_batch_mem). The rank keeps what the rounding removed from its
 * own contribution to a key and adds it to the key's next input before rounding again, so nothing
 * small is lost: it accumulates until it registers on the wire. Per element, with r the rank's
 * residual for the key (zero the first time), all arithmetic in fp32, round-to-nearest-even,
 * subnormals kept:
 *     v  = g + r
 *     w  = narrow(v)                          the wire value, the rounding rule above
 *     r' = isfinite(widen(w)) ? v - widen(w) : 0
 * w goes to the wire and r' replaces r; from there on the request is the compressed request above
 * (sum in the wire dtype in MPICH's order for the plan's unpadded wire bytes, widen, AVG's
 * quotient). v - widen(w) is exact in fp32 whenever widen(w) is finite, so the rule has one rounding
 * (g + r) beyond the wire's own. A NaN or inf in v, or an overflow of the narrowing, clears the
 * residual: it can never poison later steps. The rule is part of the fusion pack
 * (csrc/pack.hip k_seg<CvtPackOp<WIRE, true>>): no extra pass, 14 bytes moved per element against 6.
 * The residual is owned by the engine: fp32, the request's element count, in device memory,
 * found by the request's key, kept by the communicator until the communicator is destroyed.
 * EVERY DISTINCT KEY THAT EVER CARRIED THE BIT HOLDS 4 BYTES PER ELEMENT UNTIL THEN: a caller that
 * makes fresh key names per step must not set the bit.
 * The bit changes nothing that is communicated, so it is rank-local like SUM / AVG: it is in no
 * fusion group key, plan cut or negotiation, one pack launch may mix requests with and without it,
 * and ranks that disagree about it get different numbers, never a hang.
 * A key's residual restarts from zero when the key comes back with another element count, and
 * when the per-process config "wire_feedback_epoch" differs from the value under which the
 * residual was last written. A request of the key without the bit leaves the residual untouched
 * and unused. A plan that fails may already have updated its residuals; that is not undone.
 * Refusals, before anything is registered (the communicator works afterwards): the bit without a
 * wire flag, with both wire flags, or on ddl_allreduce, ddl_allreduce_batch or ddl_allreduce_host
 * returns DDL_STATUS_INVALID_ARGUMENT; with host memory or another dtype than DDL_FLOAT the wire
 * flag's own refusals apply.
 * P = 1: with "one_rank_shortcut" 1 nothing is touched and no residual is made; with 0 the data
 * plane runs and the feedback applies.
 *
 * Stochastic rounding: DDL_ALLREDUCE_WIRE_STOCHASTIC, valid only OR-ed with DDL_ALLREDUCE_WIRE_BF16, with
 * op SUM or AVG, on a keyed DDL_FLOAT device request (ddl_allreduce_submit, _submit_batch, and _submit_mem /
 * _submit_batch_mem with DDL_MEMORY_DEVICE), optionally together with DDL_ALLREDUCE_SUMSQ and
 * DDL_ALLREDUCE_SCALE. Round-to-nearest onto bf16's 8 bits is biased for a gradient that changes slowly
 * (a constant 1 + 2^-10 reads 1.0 for ever); with the bit every rank chooses between the two neighbouring
 * bf16 values with probability proportional to the distance, so the expected value of what it sends is
 * exactly its contribution. Against error feedback it keeps no residual, has nothing to reset and moves
 * the plain converting pack's 6 bytes per element; it removes the bias, not the noise.
 * Per element i of the request — i counts from the start of the tensor, never from the start of a piece —
 * with c = g (x) a the contribution behind the prescale (as under "Scale factors"), u the 32 bits of c and
 * r = R(S, i) a 16-bit integer:
 *     c a NaN or an infinity:  w = narrow(c)                       today's round-to-nearest-even rule
 *     otherwise:               w = the upper 16 bits of (u + r) mod 2^32
 * Consequences: the sign never changes and +-0 stays +-0; bf16 subnormals are handled by the same formula;
 * the magnitude goes to the neighbour away from zero with probability (u & 0xffff) / 65536, so for r
 * uniform E[widen(w)] = c exactly; a finite c above the largest bf16 value becomes +-inf with that same
 * probability. From w on the request is today's bf16 request: the same bytes, fusion group, plan cuts,
 * bf16 summation in MPICH's order, widening, AVG quotient, postscale and sum of squares of the final values.
 * R(S, i), the random bits: a stateless function of the 64-bit stream key S and the 64-bit element index i,
 * integer arithmetic only (all 32-bit operations mod 2^32). One 32-bit word per element pair j = i >> 1:
 *     x = fmix32(lo32(j) ^ lo32(S))
 *     x = fmix32(x + hi32(S) + hi32(j) * 0x9e3779b9)
 *     R(S, i) = bits 16 (i & 1) .. 16 (i & 1) + 15 of x
 * with fmix32 MurmurHash3's finaliser: x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35;
 * x ^= x >> 16. Streams whose S differ only in low bits are permutations of each other under R, which is why
 * S comes out of a 64-bit mix:
 * S, the stream key: computed on the host once per request and round from the per-process config
 * "wire_stochastic_seed", the rank in the communicator (the ranks round independently, so the noise of the
 * sum averages down over P), the 64-bit FNV-1a hash h of the key's bytes (offset basis 0xcbf29ce484222325,
 * prime 0x100000001b3) and the key's sequence number n — how many requests of this key with the bit this
 * communicator has packed before (0, 1, 2, ...):
 *     S = mix64(mix64(mix64(mix64(seed) ^ rank) ^ h) ^ n)
 *     mix64(z): z += 0x9e3779b97f4a7c15; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;
 *               z = (z ^ (z >> 27)) * 0x94d049bb133111eb; z ^ (z >> 31)          (one splitmix64 step)
 * tests/_stochastic_helpers.py restates R, the rule and the mix in NumPy, bit for bit.
 * n is kept per key by the communicator until the communicator is destroyed. EVERY DISTINCT KEY THAT EVER
 * CARRIED THE BIT HOLDS ITS NAME AND 8 BYTES UNTIL THEN: a caller that makes fresh key names per step
 * should not set the bit. A plan that fails may already have advanced n; that is not undone.
 * All pieces of a request (plan cuts, pipeline sub-plans) use the same S with their own first element
 * index, and the vector and the element path of the pack (csrc/pack.hip k_seg<CvtPackSrOp>) give the same
 * bits, so the wire values do not depend on "fusion_threshold_bytes" or "fusion_pipeline_bytes", on the
 * tensor's alignment or on what else shares the plan or the launch.
 * The bit changes nothing that is communicated, so it is rank-local like the feedback bit: it is in no
 * fusion group key, plan cut or negotiation, one pack launch may mix bf16 segments with and without it (a
 * segment without it is converted exactly as the plain pack converts it), a launch with no stochastic
 * segment is the kernel it was before, with the same tables and arguments, and ranks that disagree about
 * it get different numbers, never a hang.
 * Refusals, before anything is registered (the communicator works afterwards): the bit without WIRE_BF16,
 * with WIRE_FP16, with WIRE_FEEDBACK, with MIN / MAX, with DDL_MEMORY_HOST, or on ddl_allreduce,
 * ddl_allreduce_batch or ddl_allreduce_host returns DDL_STATUS_INVALID_ARGUMENT; on a dtype other than
 * DDL_FLOAT the wire flag's own refusal applies (DDL_STATUS_UNSUPPORTED_DTYPE). fp16 is deliberately out:
 * its subnormal range needs a different rule (the bit trick does not cross a change of format exponent
 * range), and its practical limit is range, not precision. Feedback and stochastic rounding are
 * alternatives; a request with both has no defined meaning here.
 * P = 1: with "one_rank_shortcut" 1 nothing is rounded and n does not advance; with 0 the data plane runs
 * and the rule applies.
 *
 * The e4m3 wire: DDL_ALLREDUCE_WIRE_E4M3, on a keyed DDL_FLOAT device request with op SUM or AVG, optionally
 * with DDL_ALLREDUCE_SUMSQ and DDL_ALLREDUCE_SCALE. An 8-bit float cannot be summed hop by hop, so this wire
 * is quantized exactly twice whatever P is: every rank's contribution once in the pack, the fp32 sum once in
 * the kernel that folds all P contributions of a chunk (the fold-once schedules: direct, direct-gather,
 * one-shot, gather-fold; a ring at P > 2 becomes the direct schedule, whatever "reference_order" says).
 * tests/_e4m3_helpers.py restates everything below in NumPy / torch, bit for bit.
 * Granule: the wire element is 256 bytes carrying 252 consecutive fp32 elements of one request: bytes 0..251
 * one OCP e4m3fn code per element, bytes 252..255 the bits of an fp32 scale s. A request of n elements is
 * ceil(n / 252) granules; elements past n in the last granule count as +0.0 (code 0x00). Plans, the fusion
 * threshold, plan cuts and pipeline cuts count granules (256 wire bytes = 1008 tensor bytes).
 * Pack, per granule: c = g, or g (x) prescale; amax = the largest |c| over the granule's FINITE elements (0
 * if none); s = the smallest power of two with amax / s <= 448, at least 2^-126 (amax 0: 2^-126; 448 -> 1,
 * 449 -> 2, 1.0 -> 2^-8, 1.75 -> 2^-8, 1.76 -> 2^-7); a finite element becomes RNE_e4m3(c / s) — the division
 * is exact, subnormal codes and -0 are kept, nothing saturates — and a NaN or an infinity 0x7f | sign (e4m3fn
 * has no infinity: an infinity comes back as NaN).
 * Fold: x_r = code_r * s_r in fp32 (exact, fp32 subnormals included), y = ((x_0 (+) x_1) (+) x_2) ... left to
 * right in RANK order 0..P-1 whatever the schedule, its slices or the tuner chose, every add one rounding to
 * nearest even; y is quantized by the pack's rule into the output granule, with ONE DIFFERENCE:
 *     A NaN SUM IS WRITTEN AS 0x7f, WHATEVER ITS SIGN BIT (the pack writes 0x7f | sign).
 * IEEE 754 does not pin the sign of a NaN that an addition produced, so it cannot be part of a bit-exact wire. A
 * NaN code or a NaN scale makes the element NaN; a sum that overflowed to an infinity is 0x7f | its sign. Every
 * rank ends with the same bytes. Requantizing decoded values is lossless, so a step that only copies granules
 * changes no value.
 * Unpack: y = code * s, then AVG's quotient by (float)P, then the postscale, stored as fp32; only the
 * request's n elements are written.
 * The sum of squares is the canonical UNCOMPRESSED order above over each piece of `out` (pieces added in
 * offset order), taken by one read-only pass over the outputs behind the unpack: one extra read of them.
 * Like the other wires the flag is a property of the key that every rank shares; its requests form a fusion
 * group of their own behind the existing compressed groups, and a round without it forms exactly the groups
 * it formed before. Refusals, before anything is registered: another wire flag, WIRE_FEEDBACK or
 * WIRE_STOCHASTIC with it, MIN / MAX, DDL_MEMORY_HOST, ddl_allreduce / ddl_allreduce_batch /
 * ddl_allreduce_host, or a communicator of more than 16 ranks (a fold of more than 16 inputs goes through
 * partials, which would requantize) return DDL_STATUS_INVALID_ARGUMENT; another dtype
 * DDL_STATUS_UNSUPPORTED_DTYPE. P = 1: with "one_rank_shortcut" 1 nothing is quantized.
 *
 * Error feedback of the e4m3 wire: DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK, OR-ed with DDL_ALLREDUCE_WIRE_E4M3 (and
 * optionally DDL_ALLREDUCE_SUMSQ / DDL_ALLREDUCE_SCALE) on the keyed entry points. The wire keeps 3 mantissa bits:
 * within a granule whose amax does not move an element rounds to the same wrong code every step, and an element
 * below 2^-10 of its granule's amax is zero for ever. With the bit the rank keeps what the PACK's quantization
 * removed from its contribution and adds it back at the key's next request. Only the first of the wire's two
 * quantizations is compensated: THE FOLD'S REQUANTIZATION OF THE SUM IS NOT (whichever rank folds a chunk depends
 * on the schedule, the tuner and the cuts, and the fold-everything schedules have no single owner). The P pack
 * errors add up against one fold error, so at P >= 2 the pack side dominates, and once the contributions dither
 * the fold's input no longer sits on the same rounding boundary every step; that is a statement from the
 * arithmetic, nobody has measured it in training.
 * r is the rank's residual for the key: fp32, the request's element count, indexed like the tensor, zero the
 * first time. All arithmetic is fp32, round to nearest even, subnormals kept, every product and sum rounded on
 * its own, never contracted. Per granule of a request that carries the bit:
 *     c  = g, or g (x) prescale                      as without the bit
 *     v  = c (+) r
 *     (codes, s) = the pack's rule above applied to the granule's v (amax over the FINITE v, the same scale
 *                  rule, RNE_e4m3(v / s), 0x7f | sign for a NaN or an infinity)
 *     d  = code * s                                  exact: what the unpack / the fold will read
 *     r' = isfinite(v (-) d) ? v (-) d : +0.0
 * (codes, s) go to the wire, r' replaces r. Elements of the last granule past n have no residual and stay +0.0
 * on the wire. tests/_e4m3_feedback_helpers.py restates the rule in NumPy, bit for bit.
 * Nothing saturates on this wire; a NaN or an infinity in v (d is a NaN then) clears that element's residual and can
 * never poison later steps. The one overflow is the decode's: 2^120 is the largest scale (FLT_MAX / 2^120 < 256), so
 * a finite |v| above 248 * 2^120 rounds to the code of 256, and d = 256 * 2^120 is an infinity in fp32 — for the fold
 * and the unpack too, with or without the bit. There is nothing to keep for what went out as an infinity: v (-) d is
 * not finite and r' is +0.0. Wherever d is finite, v (-) d is exact: 0 is on the code grid, so
 * |v - d| <= |v|, and the grid's quantum — s * 2^-9 at its finest — is never below ulp(v), because |v| <= 448 s.
 * The rule therefore costs one fp32 rounding (c + r) beyond the wire's own (tests/test_e4m3_feedback_model_cpu.py
 * checks the subtraction against fp64). From the wire bytes on the request is the plain e4m3 request: granules,
 * fusion group, plan and pipeline cuts, fold-once schedules, the fold, the unpack, AVG's quotient, the postscale
 * and the sum of squares are unchanged. The residual is in prescaled units, as for the 16-bit wires.
 * The residual has the lifetime and the restarts of the 16-bit one: kept by the communicator until it is
 * destroyed (a failed plan is not undone), restarted from zero on another element count and on another
 * "wire_feedback_epoch"; and also when the key comes back under the other family of wire — e4m3 after a 16-bit
 * wire with DDL_ALLREDUCE_WIRE_FEEDBACK, or the reverse (fp16 <-> bf16 keeps the residual, as before). EVERY
 * DISTINCT KEY THAT EVER CARRIED THE BIT HOLDS 4 BYTES PER ELEMENT UNTIL THEN: never use it with fresh key names
 * per step. A request of the key without the bit leaves the residual untouched and unused. The pack of a segment
 * with a residual moves 4 + 4 + 4 + 256/252 (about 13.0) bytes per element against 5.0 (csrc/pack.hip
 * k_seg<Q8PackOp<SCALE, true>>; the vector and the element path give the same bits, so nothing depends on the
 * tensor's alignment, on "fusion_threshold_bytes" or on "fusion_pipeline_bytes": a piece's residual starts at the
 * piece's first element).
 * The bit is rank-local like the 16-bit feedback bit: it is in no fusion group key, plan cut or negotiation, one
 * pack launch may mix e4m3 segments with and without it (a segment without it is packed exactly as the plain
 * pack packs it), a launch with no feedback segment is the kernel it was, with the same tables and arguments,
 * and ranks that disagree about it get different numbers, never a hang.
 * Refusals, before anything is registered (the communicator works afterwards): the bit without WIRE_E4M3, with
 * WIRE_FP16 or WIRE_BF16, with WIRE_FEEDBACK or WIRE_STOCHASTIC, with MIN / MAX, with DDL_MEMORY_HOST, on
 * ddl_allreduce, ddl_allreduce_batch or ddl_allreduce_host, or on a communicator of more than 16 ranks returns
 * DDL_STATUS_INVALID_ARGUMENT; a dtype other than DDL_FLOAT DDL_STATUS_UNSUPPORTED_DTYPE.
 * P = 1: with "one_rank_shortcut" 1 nothing is touched and no residual is made; with 0 the data plane runs and
 * the rule applies.
 *
 * MIN / MAX: DDL_ALLREDUCE_OP_MIN = 3 and DDL_ALLREDUCE_OP_MAX = 4, on every dtype and every
 * allreduce entry point. Per element over the P inputs: DDL_INT32 / DDL_INT64 in signed order,
 * DDL_UINT64 in unsigned order; DDL_FLOAT / DDL_DOUBLE / DDL_HALF / DDL_BFLOAT16 are IEEE 754-2019
 * `minimum` / `maximum`: if any input is a NaN the result is a quiet NaN (sign and payload not
 * pinned), otherwise it is bit for bit the input that is least / greatest in numeric order with
 * -0 < +0. Subnormals are kept, nothing is rounded (the 16-bit types may be widened internally: the
 * result is the same). This is deliberately not MPICH's `a > b ? a : b`, whose result depends on
 * the order once a NaN or +-0 is present and which lets a NaN hide behind a MAX. The operation is
 * associative and commutative, so the result does not depend on the schedule, the slicing, the fold
 * order, "reference_order" or P, and for non-NaN results every rank holds the same bits. The
 * reduce and fold kernels (csrc/reduce_kernels.hip) take the combine in place of the addition:
 * the same schedules, bytes and launches as SUM, no trailing launch, so MIN / MAX direct
 * collectives can be captured into a hipGraph exactly like SUM. P = 1: the result is the input.
 * Unlike SUM against AVG the reduction kind IS communicated: like the wire flag it is a property of
 * a key that every rank must agree on (MIN and MAX requests form fusion groups of their own, after
 * the SUM / AVG group of the same dtype and memory, MIN before MAX). Ranks that disagree about a
 * key's kind post different collectives.
 * Refusals, before anything is registered: MIN / MAX with a wire flag or DDL_ALLREDUCE_WIRE_FEEDBACK
 * returns DDL_STATUS_INVALID_ARGUMENT; op values 2 and above 4 stay DDL_STATUS_INVALID_ARGUMENT.
 *
 * Sum of squares (DDL_ALLREDUCE_SUMSQ in `op`, `user` a ddl_sumsq_arg): an optional per-request output of a
 * keyed DDL_FLOAT device request with op SUM or AVG (a wire flag and the feedback bit allowed):
 * *sumsq = the fp64 sum of the squares of the fp32 elements written to `out` — the final values,
 * after AVG's quotient and after the wire's widening — stored before `done` fires. It is the
 * squared L2 norm a gradient clip needs, and the finite check of a loss scaler: the square of a
 * finite fp32 value is exact in fp64 and no sum of fewer than 2^64 of them overflows, so *sumsq is
 * FINITE IF AND ONLY IF EVERY ELEMENT IS FINITE (an inf gives +inf, a NaN or inf and NaN give NaN).
 * `out` is bit-identical on every rank and the order of the additions below is fixed, so *sumsq is
 * the same double on every rank: a clip factor derived from it keeps the replicas in step.
 * Order. A request is cut into PIECES at the element offsets where a fusion plan
 * ("fusion_threshold_bytes") or a pipeline sub-plan ("fusion_pipeline_bytes", cuts at 256-byte
 * multiples of the communicated stream) ends inside it — shared tunables and the negotiated round,
 * so every rank cuts alike. For a piece of n elements x[0..n): T = 256 and E = 4 for an
 * uncompressed request, T = 512 and E = 8 for one with a wire flag. The piece has ceil(n / T) tiles;
 * lane l (0..63) of tile t owns elements t*T + l*E .. t*T + l*E + E-1 and computes
 *     s[l] = (((+0.0 + x0*x0) + x1*x1) + ...)       left to right in fp64, x widened to fp64 first,
 * an element at or past n counting as +0.0 (every product is exact, so whether the compiler
 * contracts acc + x*x into a fused multiply-add changes no bit); the lanes combine by the butterfly
 *     for d = 32, 16, 8, 4, 2, 1:  s[l] = s[l] + s[l ^ d]     (all lanes at once)
 * and s[0] is the tile's partial p[t]. The partials are combined in GROUPS of up to 4096 consecutive
 * values: for a group v[0..m), lane l computes q[l] = ((+0.0 + v[l]) + v[l + 64]) + v[l + 128] + ...
 * (missing values +0.0), the same butterfly follows, and q[0] is the group's value. A piece of at
 * most 4096 tiles (1 Mi elements uncompressed) is one group and its value is that group's; a longer
 * piece's group values, in order, form one more group whose value is the piece's (pieces of up to
 * 4096^2 tiles, 16 GiB; longer ones fail with DDL_STATUS_INVALID_ARGUMENT). The request's *sumsq is its
 * pieces' values added in increasing element offset, starting from the first piece's value. n == 0
 * gives +0.0.
 * tests/_sumsq_helpers.py restates this in NumPy, bit for bit.
 * Invariances. The order depends only on an element's index inside its piece, the piece's length
 * and whether the request is compressed — not on the tensor pointer's alignment, not on whether the
 * piece went through the fusion buffer or was read in place, not on which other requests share its
 * plan or unpack launch. No floating-point atomic is used anywhere.
 * Cost. A fused plan takes it inside the unpack launch that writes the elements (csrc/pack.hip
 * k_seg_sumsq: 8 bytes written per 1 KiB tile, plus one small finishing kernel and one async copy
 * per launch): no extra pass over the tensors. A plan of one uncompressed request (reduced in place,
 * no fusion buffer) and the one-rank shortcut pay ONE READ-ONLY PASS over the result with the same
 * kernel. No host synchronisation is added: the values reach pinned host memory by an async copy
 * ahead of the event the completion already waits for.
 * Like SUM against AVG it is rank-local: it is in no fusion group key, plan cut or negotiation, one
 * plan or launch may mix requests with and without it, requests without it run exactly the launches,
 * kernels and tables they ran before, and ranks that disagree about it never hang.
 * P = 1: with "one_rank_shortcut" 1 the value is that of the input moved to `out`, in the
 * uncompressed order also with a wire flag (nothing is compressed); with 0 the data plane runs and
 * the value is its result's. On a failed request the value is unspecified.
 * Refusals, before anything is registered (the communicator works afterwards): a non-NULL sumsq with
 * a dtype other than DDL_FLOAT and DDL_BFLOAT16 returns DDL_STATUS_UNSUPPORTED_DTYPE, with MIN / MAX or with
 * DDL_MEMORY_HOST DDL_STATUS_INVALID_ARGUMENT; the bit with a NULL `user` (`users`, users[i]), and the
 * bit on ddl_allreduce, ddl_allreduce_batch or ddl_allreduce_host, DDL_STATUS_INVALID_ARGUMENT; the
 * op's own refusals apply as without the bit. With every arg->sumsq NULL the request is the one
 * without the bit. No new entry point: the deployment surface is unchanged.
 * bfloat16. A keyed DDL_BFLOAT16 device request with op SUM or AVG (no wire flag: it has none) takes the bit
 * too: *sumsq = the fp64 sum of the squares of widen(e) over the bfloat16 elements e STORED to `out` — after
 * AVG's quotient, the postscale and the one rounding to bfloat16 behind them — so it is finite exactly when
 * every stored element is. The order is the 2-byte layout's, T = 512 and E = 8 (a 1 KiB tile holds 512
 * elements, a lane's 16 bytes 8), pieces cut at 256-byte multiples = 128 elements, everything else as
 * above; a plan of one request and the one-rank shortcut read the result in place in that same order
 * (csrc/pack.hip k_seg_sumsq16). DDL_HALF, DDL_DOUBLE and the integer dtypes stay
 * DDL_STATUS_UNSUPPORTED_DTYPE.
 *
 * Scale factors (DDL_ALLREDUCE_SCALE in `op`, `user` a ddl_scale_arg): two optional fp32 factors of a keyed
 * DDL_FLOAT device request with op SUM or AVG (a wire flag, the feedback bit and DDL_ALLREDUCE_SUMSQ
 * allowed), each finite and > 0, 1.0f meaning "absent". prescale a multiplies every element on its way
 * INTO the reduction, postscale b every result on its way into `out`; both products are taken by the
 * kernels that already move those bytes (csrc/pack.hip, the scaled Ops), so a loss scale's unscale and
 * the division that keeps an fp16 wire's partial sums under 65504 cost no pass over the gradients.
 * All arithmetic is fp32, round to nearest even, subnormals kept; every product is rounded on its own
 * and is never fused with a neighbouring addition. With (x) the product, (+) the sum, (/) the quotient:
 *   contribution of a rank, element g:  c = g (x) a   (a = 1: c = g, the bits untouched, no multiply);
 *     uncompressed c enters the fusion buffer; with a wire flag w = narrow(c); with the feedback bit
 *     v = c (+) r and the rule of the feedback paragraph unchanged — THE RESIDUAL IS IN PRESCALED UNITS:
 *     with prescale = 1 / S for a loss scale S it is in true-gradient units and survives a change of S;
 *   reduction: unchanged — the same bytes, schedules and order of additions;
 *   result, element s of the reduced stream:  y = s (widened from the wire);  AVG: y = y (/) (float)P,
 *     the correctly rounded quotient;  b != 1: y = y (x) b;  y is stored to `out`.
 * The sum of squares, when wanted, is of these final y, in the order above. "*sumsq is finite if and
 * only if every stored element is finite" keeps holding. A NaN stays a NaN (payload unspecified).
 * Like SUM against AVG and the sum of squares the factors are rank-local: they are in no fusion group
 * key, plan cut or negotiation, one plan or launch may mix scaled and unscaled requests (a segment
 * without a factor inside a scaled launch is moved exactly as the unscaled kernel moves it), requests
 * without factors run exactly the launches, kernels and tables they ran before, and ranks that
 * disagree about a factor get different numbers and never hang.
 * Cost. Fused plans: none beyond one multiply per element in the pack / unpack launch. A plan of one
 * uncompressed request keeps its in-place allreduce over exactly the elements it reduces without
 * factors (so ranks that disagree about a factor still post the same collective): a prescale is ONE
 * in-place launch over `out` ahead of it (behind a device copy where out != in), a postscale ONE
 * in-place launch behind it that takes AVG's quotient and the factor together.
 * P = 1: with "one_rank_shortcut" 1, out = (g (x) a) (x) b, each factor skipped when it is 1, no wire
 * rounding; with 0 the data plane runs and defines the value.
 * Refusals, before anything is registered (the communicator works afterwards): a factor that is not
 * finite or is <= 0 returns DDL_STATUS_INVALID_ARGUMENT; a factor other than 1 with a dtype other than
 * DDL_FLOAT and DDL_BFLOAT16 DDL_STATUS_UNSUPPORTED_DTYPE, with MIN / MAX or DDL_MEMORY_HOST DDL_STATUS_INVALID_ARGUMENT;
 * the bit with a NULL `user` (`users`, users[i]), and the bit on ddl_allreduce, ddl_allreduce_batch or
 * ddl_allreduce_host, DDL_STATUS_INVALID_ARGUMENT. If both factors are 1 the request is the one without
 * the bit. No new entry point.
 * bfloat16. A keyed DDL_BFLOAT16 device request with op SUM or AVG (no wire flag) takes the factors too, in
 * fp32 arithmetic as above with widen exact and narrow the round-to-nearest-even fp32 -> bfloat16 of the
 * bf16 wire (overflow gives inf, a NaN stays a NaN, payload unspecified):
 *   contribution:  a != 1: c = narrow(widen(g) (x) a);  a = 1: the bytes are moved untouched;
 *   reduction: the plan's plain bfloat16 allreduce, unchanged;
 *   result, element s of the reduced stream:  y = widen(s);  AVG and P > 1: y = y (/) (float)P;  b != 1:
 *     y = y (x) b;  narrow(y) is stored — ONE bfloat16 rounding, at the end, never one between the quotient
 *     and the factor. With b = 1 these are the bits of the AVG op without factors; SUM with b = 1: bytes.
 * A prescale that is no power of two therefore costs the contribution one extra bfloat16 rounding. A plan
 * of one request takes the prescale in place ahead of its in-place allreduce and quotient and postscale in
 * one in-place launch behind it, as for DDL_FLOAT. DDL_HALF, DDL_DOUBLE and the integer dtypes stay
 * DDL_STATUS_UNSUPPORTED_DTYPE. */
/* recv = SUM over ranks of send (elementwise), bit for bit the reference's MPI_Allreduce (MPICH
 * 3.3.2's order) with reference_order 1. The schedule is the tuned one for the bucket's size
 * class: by default at P > 2 the direct reduce-scatter (slices of every chunk to every peer over
 * RCCL send/recv, one HIP fold per slice in MPICH's tree) + allgather; one-shot / gather-fold for
 * small buckets; at P = 2 the ring. recv may equal send (in place). Stream-ordered: no host
 * synchronisation (except the first bucket of a size class, which the autotuner times). */
int ddl_allreduce(ddl_communicator_id id, const void *send, void *recv, size_t elements,
                  int dtype, int op, void *hip_stream);

/* Grouped form of ddl_allreduce for `count` buckets of one dtype (MI355X extension: a DDP-style
 * bucket list in one call): recvs[b] = SUM over ranks of sends[b] (elements[b] each; in place when
 * recvs[b] == sends[b]); with reference_order 1 (the default) bit for bit what ddl_allreduce
 * gives each bucket on its own (both are MPICH's order for the bucket's own size); with
 * reference_order 0 each bucket is summed in the batch schedule's order (direct: rank-order fold;
 * one-shot: left fold), which may differ in the last bits from the ring or other schedule a solo
 * ddl_allreduce of that bucket's size class was tuned to. One program
 * for all buckets — tick by tick one RCCL group carries every bucket's slices and the folds of up
 * to 8 buckets share a kernel launch — instead of a program, two or more groups and a fold launch
 * per bucket. The schedule is the one tuned for the largest bucket (direct, or one-shot for small
 * buckets). Stream-ordered; collective: every rank passes the same count and element counts. */
int ddl_allreduce_batch(ddl_communicator_id id, int count, const void *const *sends, void *const *recvs,
                        const size_t *elements, int dtype, int op, void *hip_stream);

/* Communicator::broadcast (reference Communicator.h:81-92, MPI_Bcast at MPICommunicator.cc:77-90):
 * root's `elements` of `buf` into every rank's `buf`. Scatter + direct allgather over RCCL
 * send/recv (each xGMI link out of the root carries 2S/P, not S). Stream-ordered. */
int ddl_broadcast(ddl_communicator_id id, void *buf, size_t elements, int dtype, int root, void *hip_stream);
/* Communicator::allgather, per-rank counts (Communicator.h:50-66, MPI_Allgatherv at
 * MPICommunicator.cc:31-60): rank q's recv_counts[q] elements land at recv + displs[q] (in
 * elements) on every rank; send_elements must equal recv_counts[rank]. Stream-ordered. */
int ddl_allgatherv(ddl_communicator_id id, const void *send, size_t send_elements, void *recv,
                   const size_t *recv_counts, const size_t *displs, int dtype, void *hip_stream);
/* Communicator::allgather, equal counts (Communicator.h:68-79): rank q's block at q*recv_elements. */
int ddl_allgather(ddl_communicator_id id, const void *send, size_t send_elements, void *recv,
                  size_t recv_elements, int dtype, void *hip_stream);

/* Host-resident buckets (the reference's deployment case: CPU tensors behind the MPI buffers,
 * MPIRingTokenCommunication.cc:548-733): chunked H2D -> ddl_allreduce -> D2H pipeline on three
 * streams ("host_chunk_bytes", default 32 MiB; 4 chunk slots in HBM in flight). Pageable memory is
 * registered for the call; pinned memory avoids that cost. Synchronous: returns when `recv`
 * holds the result. Collective: every rank calls it with the same element count. */
int ddl_allreduce_host(ddl_communicator_id id, const void *send, void *recv, size_t elements,
                       int dtype, int op);

/* Autotuner record for the size class of `bucket_bytes` on communicator `id`: *chosen = index
 * of the schedule in use (-1 = class not tuned yet), *count = candidates; for the first
 * max_candidates of them configs[4i..4i+3] = {algo, rings, slice_bytes, max_slices} and
 * ms[i] = mean time per allreduce (max over ranks). configs/ms may be NULL. */
int ddl_tune_result(ddl_communicator_id id, size_t bucket_bytes, int *chosen, int *count,
                    long long *configs, float *ms, int max_candidates);
/* Keyed asynchronous request (TF op Allreduce semantics): registered under `key`,
 * negotiated across ranks, fused by dtype in lexicographic key order, then `done` fires.
 * `in`/`out` must stay valid until `done`. Work is ordered after `hip_stream`'s current
 * position; `done` fires once `out` is final.
 * Keyed rounds and direct collectives on one communicator (the reference's MPI_THREAD_MULTIPLE,
 * MPIBackend.cc:77-86): a communicator with a token ring reduces its keyed rounds on a private
 * RCCL communicator, and every round is placed after the same number of the communicator's
 * direct collectives (ddl_allreduce[_batch], ddl_broadcast, ddl_allgather[v], ddl_allreduce_host,
 * split_communicator) on every rank, so both RCCL communicators see their work in one order
 * everywhere. A direct collective issued while a round is being placed waits for the placement
 * (one negotiation). If the communicator's handler stops on an error (a control link lost, a
 * token-protocol fault), its pending requests complete with that status, and from then on every
 * direct collective on the communicator returns it too instead of waiting for a placement that
 * can no longer happen: the communicator is unusable, finalize and re-initialise. */
int ddl_allreduce_submit(ddl_communicator_id id, const char *key, const void *in, void *out,
                         size_t elements, int dtype, int op, void *hip_stream,
                         ddl_done_fn done, void *user);
/* Keyed broadcast (TF op Broadcast, op/tensorflow/BroadcastOp.cc; TensorBroadcastRequest.h:13-40):
 * `out` on every rank receives root's `in`. Negotiated and fused like allreduce requests
 * (dtype groups, plans, MPIRingTokenCommunication.cc:367-419); requests of different roots
 * run as separate groups. */
int ddl_broadcast_submit(ddl_communicator_id id, const char *key, const void *in, void *out, size_t elements,
                         int dtype, int root, void *hip_stream, ddl_done_fn done, void *user);
/* Keyed allgather (TF op Allgather, op/tensorflow/AllgatherOp.cc; TensorAllgatherRequest.h):
 * `in` holds first_dim rows of row_elements; the output holds every rank's rows in rank order
 * (first dims may differ per rank, row_elements may not). Once the gathered first dim is known
 * `alloc(total_rows, bytes, user)` supplies the output buffer, then `done` fires
 * (MPIRingTokenCommunication.cc:160-364). */
int ddl_allgather_submit(ddl_communicator_id id, const char *key, const void *in, size_t first_dim,
                         size_t row_elements, int dtype, void *hip_stream, ddl_alloc_fn alloc,
                         ddl_done_fn done, void *user);
/* Batch form of ddl_allreduce_submit: registers `count` keyed requests at once (one input-ready
 * event on hip_stream, one wake-up of the engine thread); users[i] (or NULL) is passed to done for
 * request i. All-or-nothing: a duplicate key rejects the whole batch. */
int ddl_allreduce_submit_batch(ddl_communicator_id id, int count, const char *const *keys,
                               const void *const *ins, void *const *outs, const size_t *elements,
                               const int *dtypes, int op, void *hip_stream, ddl_done_fn done,
                               void *const *users);
/* The same four submissions with the memory kind of in / out (ddl_memory). Host buffers are
 * ready at submission (no stream wait) and must stay valid until done; a keyed allgather's alloc
 * then returns host memory. Host and device requests of one dtype fuse into separate plans
 * (device groups first); with only host requests the plans are the reference's. */
int ddl_allreduce_submit_mem(ddl_communicator_id id, const char *key, const void *in, void *out, size_t elements,
                             int dtype, int op, int memory, void *hip_stream, ddl_done_fn done, void *user);
int ddl_allreduce_submit_batch_mem(ddl_communicator_id id, int count, const char *const *keys,
                                   const void *const *ins, void *const *outs, const size_t *elements,
                                   const int *dtypes, int op, int memory, void *hip_stream, ddl_done_fn done,
                                   void *const *users);
int ddl_broadcast_submit_mem(ddl_communicator_id id, const char *key, const void *in, void *out, size_t elements,
                             int dtype, int root, int memory, void *hip_stream, ddl_done_fn done, void *user);
int ddl_allgather_submit_mem(ddl_communicator_id id, const char *key, const void *in, size_t first_dim,
                             size_t row_elements, int dtype, int memory, void *hip_stream, ddl_alloc_fn alloc,
                             ddl_done_fn done, void *user);
/* Blocks until every request submitted on `id` so far has completed. */
int ddl_wait_all(ddl_communicator_id id);

/* Completion groups (MI355X extension, csrc/completion.cpp): a native done callback for bindings
 * whose own callbacks are costly — a Python done() per request costs ~10 us of interpreter time,
 * 40-60 ms per 4096-tensor batch. Create a group of `count` slots, pass ddl_completion_done as the
 * ddl_done_fn and slot i's pointer (ddl_completion_slots: `count` of them from `first` into out)
 * as request i's `user`; done() stores the status in slot i and wakes its waiters.
 * ddl_completion_wait blocks (no callback into the binding) until slot `index` completed or
 * `timeout_s` (< 0: no limit; 0: a test) passed: DDL_STATUS_OK with *status = the request's
 * status, or DDL_STATUS_ERROR_UNKNOWN while it is still pending. ddl_completion_poll copies the
 * first `count` slots' statuses (-1: pending; statuses may be NULL when count is 0) and returns
 * how many slots are pending. ddl_completion_destroy is the owner's release: the group is freed
 * once every slot has completed too, so done() calls after it stay safe. */
void *ddl_completion_create(int count);
int ddl_completion_slots(void *group, int first, int count, void **out);
void ddl_completion_done(int status, void *user);
int ddl_completion_wait(void *group, int index, double timeout_s, int *status);
int ddl_completion_poll(void *group, int *statuses, int count);
void ddl_completion_destroy(void *group);

/* With "host_register_cache_bytes" > 0: the host range [ptr, ptr + bytes) is about to be freed —
 * call this BEFORE freeing (munmap / free / the framework's deallocator) any host tensor that was
 * part of a keyed request. Every cached registration overlapping the range is dropped (at once,
 * or — while the engine is posting a host plan — before its next cache lookup), so a later
 * tensor placed at the same address is registered afresh instead of being taken for the old,
 * now unmapped pages (a device access through the stale registration faults). The torch mirror
 * (ddl.torch.tensor_communicate) calls it from a finalizer of every host tensor it submits while
 * the cache is on. A no-op for ranges that are not cached. */
int ddl_host_unregister(const void *ptr, size_t bytes);

/* Measurement: bracket every reduce-kernel launch of ddl_allreduce on `id` with timing
 * events on the engine's compute stream (the stream the kernel runs on). ddl_kernel_stats
 * waits for the recorded events and returns launches, algorithmic HBM bytes (per launch: a
 * two-input ring step 3 * elements * sizeof(T); a fold of nb received inputs
 * (nb + 2) * elements * sizeof(T) — the own input, the nb inputs, one write) and summed kernel
 * milliseconds, then resets. */
int ddl_kernel_timing(ddl_communicator_id id, int on);
int ddl_kernel_stats(ddl_communicator_id id, long long *launches, double *bytes, double *ms);

#ifdef __cplusplus
}
#endif

/* The test / diagnostic entry points (ddl_init_test_transport, ddl_p2p_op, ddl_control_negotiate*,
 * ddl_allreduce_variant, ddl_reduce_*, ddl_pack / ddl_unpack, ddl_local_*, ddl_testing_*,
 * ddl_rccl_loopback_*, the schedule introspection) are declared in ddl_amd_testing.h and exported
 * only by lib/libddl_amd_testing.so (the same engine objects plus the harness); lib/libddl_amd.so
 * exports exactly this header. Define DDL_AMD_WITH_TESTING_API before including this header to
 * get both (and link the testing library). ddl_init_test_transport also needs
 * DDL_ALLOW_TEST_TRANSPORT=1 in the environment. */
#ifdef DDL_AMD_WITH_TESTING_API
#include "ddl_amd_testing.h"
#endif

#endif /* DDL_AMD_H */
