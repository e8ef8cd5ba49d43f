/*
 * esr_hip.h -- C ABI of libesr_hip.so, the MI355X (gfx950) embedding-training hot path.
 *
 * The reference (BBischof/ESRecsys) has no plugin / operator / FFI boundary: its
 * hot path is a handful of Python functions executed by XLA through JAX/Flax/Optax
 * (SURVEY.md section 8b).  This header is therefore the boundary a maintainer
 * would bind from the reference's Python (ctypes -- see INTEGRATION.md); each
 * entry point cites the reference lines whose arithmetic it replaces.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - returns ESR_OK (0) or a negative ESR_E* code; never throws.  esr_last_error()
 *     returns a thread-local message for the last failing call on this thread.
 *   - every pointer is DEVICE memory owned by the caller unless marked "host".
 *     The library never allocates, frees or synchronises; work is enqueued on
 *     `stream` (a hipStream_t passed as void*; NULL = the null stream).
 *   - scratch memory is passed explicitly: `workspace` of at least the size the
 *     matching esr_*_workspace_bytes() query returns (16-byte aligned).
 *   - tables are row-major [V, D]; ids are int32 in [0, V).  Rows are processed
 *     in 16-byte chunks when D * sizeof(elt) is a multiple of 16, else scalar.
 *   - re-entrant across streams/threads; no global mutable state.
 */
#ifndef ESR_HIP_H_
#define ESR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESR_OK 0
#define ESR_EINVAL (-1)     /* bad argument (null pointer, negative size, unsupported D/k/...) */
#define ESR_ELAUNCH (-2)    /* HIP launch / runtime error (message has hipGetErrorString) */
#define ESR_EWORKSPACE (-3) /* workspace too small or misaligned */
#define ESR_ENODEVICE (-4)  /* no gfx950 device visible */

#define ESR_F32 0
#define ESR_BF16 1

#define ESR_GLOVE_REFERENCE 0 /* (B,B)-broadcast loss of wikipedia/train_cooccurence.py:83 */
#define ESR_GLOVE_DIAGONAL 1  /* textbook per-pair GloVe loss (build-defined option) */
/* OR-ed into esr_glove_fwd_bwd's `mode` / esr_triplet_fwd_bwd's `with_reg`: the gradient of the occurrence that read
 * table row r is written at output row r instead of at its occurrence index.  For "tables" that are a private copy
 * of the looked-up rows with one row per occurrence (the row-sharded step: rows in exchange order, ids = the inverse
 * routing permutation) this emits the gradients directly in exchange order; the three triplet gradient pointers may
 * then alias one buffer. */
#define ESR_GRADS_AT_IDS 0x100

typedef void* esr_stream_t;

const char* esr_last_error(void);
int esr_version(void);
/* host out-params; arch_len bytes at arch receive e.g. "gfx950". */
int esr_device_info(int* cu_count, int* wave_size, size_t* hbm_bytes, char* arch, int arch_len);

/* ---- measurement: per-kernel launch durations ("GPU kernel times ... from rocprofv3"; bench.py's
 * `roofline.achieved` wants the dominant kernel's duration measured live with HIP events on the stream the kernel is
 * launched on -- the kernels are launched inside the library, so the events are recorded here).  The reference has no
 * counterpart (it never measures: wikipedia/train_cooccurence.py:185-186 logs the loss only).
 * esr_kernel_timing(1): from now on the instrumented launch sites record a HIP event pair around their launch (the
 * in-batch head's kernels, the one-pass GloVe / triplet update kernels, the retrieval GEMM and selects); (0): stop.
 * Either call drops unread records.  Off by default: one load per launch site.
 * esr_kernel_timing_read: the ONE entry point that synchronises (it waits for the recorded events): writes
 * "name\tcalls\ttotal_ms\tmin_ms\tmax_ms\n" per kernel name to the HOST buffer `buf` (NUL-terminated, truncated to cap)
 * and clears the records; returns the bytes the whole text needs. */
int esr_kernel_timing(int enable);
long esr_kernel_timing_read(char* buf, size_t cap);
/* rocprofv3 markers ("tracing / profiling": absent in the reference -- only a commented-out
 * jax_debug_nans toggle, spotify/train_spotify.py:162-163): esr_trace_markers(1), or ESR_ROCTX=1 in the environment when the
 * library is loaded, makes every instrumented launch site and every step entry point a roctx range (push / pop on the
 * calling thread), so `rocprofv3 --marker-trace --kernel-trace` shows which phase of which step a kernel belongs to;
 * (0): off, the default (one load per site).  ESR_ENODEVICE when no roctx library can be loaded. */
int esr_trace_markers(int enable);

/* ---- G2 / S1: embedding-row gather ------------------------------------------------------
 * nn.Embed lookup == jnp.take(table, ids, axis=0): wikipedia/models.py:31-34 (and the id towers
 * that replace pinterest/models.py:64-70).  out[i, :] = table[ids[i], :], bit-exact. */
int esr_gather_rows(const void* table, int dtype, int64_t V, int D, const int32_t* ids, int64_t n,
                    void* out, esr_stream_t stream);

/* Debug screen for DEVICE-resident ids (the hot path trusts them: a host-side check would force a sync per step).
 * report is device int64 [2], initialised by the caller to {0, INT64_MAX}: report[0] += number of ids outside
 * [0, V), report[1] = min(position of such an id).  jnp.take clamps out-of-range ids silently
 * (wikipedia/models.py:31-34 [upstream jax]); here they would be wild reads / read-modify-writes, so the Python
 * layer runs this screen on every device id tensor when ESR_CHECK_IDS=1 and raises IndexError. */
int esr_check_ids(const int32_t* ids, int64_t n, int64_t V, int64_t* report, esr_stream_t stream);

/* ---- G2: Glove.__call__ pieces -- wikipedia/models.py:30-37 ------------------------------
 * dot[j] = E[t1[j]] . E[t2[j]],  s[i] = Bias[t1[i]] + Bias[t2[i]];  the (B,B) output is
 * dot[None,:] + s[:,None].  inputs is int32 [2, B] row-major (cooccurrence_matrix.py:103-104). */
int esr_glove_forward(const float* emb, const float* bias, int64_t V, int D, const int32_t* inputs,
                      int64_t B, float* dot, float* s, esr_stream_t stream);

/* ---- G3: apply_model / glove_loss value_and_grad -- wikipedia/train_cooccurence.py:76-89 ---
 * Fused gather + dot + weighted log10 loss + per-occurrence row gradients.
 *   loss[0]                       scalar loss
 *   grad_rows [2B, D]             occurrence j   : dL/ddot_j * E[t2[j]]   (row id t1[j])
 *                                 occurrence B+j : dL/ddot_j * E[t1[j]]   (row id t2[j])
 *   grad_bias [2B]                occurrence i and B+i: dL/ds_i
 * The occurrence ids are simply inputs[0..2B) read as a flat array. */
size_t esr_glove_workspace_bytes(int64_t B);
int esr_glove_fwd_bwd(const float* emb, const float* bias, int64_t V, int D, const int32_t* inputs,
                      const float* target, int64_t B, int mode, float* loss, float* grad_rows,
                      float* grad_bias, void* workspace, size_t workspace_bytes, esr_stream_t stream);

/* ---- G3 + G4 in one pass: loss, gradients and the sparse Adagrad update of BOTH tables ------------------------
 * (wikipedia/train_cooccurence.py:71-101 with the build's row-sparse Adagrad in place of dense optax.adam.)
 * No gradient row is ever written to memory: the update kernel walks the sorted occurrences of every distinct row,
 * re-reads each occurrence's partner row, forms gdot and accumulates gdot * partner on chip, then does the row's one
 * read-modify-write.  Reading partner rows while other rows are being rewritten is made safe by DOUBLE-BUFFERING
 * the embedding table: `emb` and `emb_shadow` are two [V, D] buffers and emb_loc [V] holds one STAMPED byte per row:
 * bit 0 = the buffer with the row's current value, bits 1..7 = the stamp of the step that last moved the row (0 = long
 * ago).  The step reads every row where it lived when the step began -- a byte that already carries THIS step's stamp
 * says "moved during this step, the old value is in the other buffer" -- writes each updated row into the other
 * buffer and stamps its byte.  `stamp`: 1 .. 127, a value no byte of the table carries from an EARLIER step: count the
 * steps on a table 1, 2, ... 127 and call esr_rows_restamp (one pass over V bytes, clears the stamps) before starting
 * over at 1.  Callers that need a plain [V, D] table run esr_rows_consolidate (copies the rows that live in `shadow`
 * into `primary`, zeroes every byte).  A fresh state is emb_loc = 0.
 * Same sort, same cut points and the same association of every row sum as esr_glove_fwd_bwd +
 * esr_sparse_adagrad_scatter: tables and accumulators agree with that path to an f32 rounding (bias sums are carried
 * in fp64 here; the bias statistics sum s, sum s^2 of K_A in exact integer arithmetic).
 * loss [1]; bias / bias_accum [V] are updated in place (every bias read of a step precedes its bias writes).
 * presorted_ids / presorted_perm (both or neither): the output of esr_segment_sort_ids on inputs[0 .. 2B) -- the sort
 * depends on the ids only, so a training loop runs it ahead; NULL = sort here.  plan (optional, needs the presorted
 * arrays): esr_glove_plan's record of this batch, made ahead as well -- it holds what the step needs from ids and
 * counts alone and the zeroed accumulators of ONE step (a plan feeds exactly one esr_glove_train_step); NULL = made
 * here.  long_runs: 0 = the caller knows from esr_glove_plan's hint that no run of equal ids outgrows a 32-position
 * chunk, and the long-run launch is skipped; anything else = launched (it returns at once when nothing was parked).
 * Launches per step with a plan and uniform ids: update, finalize.  blocks_per_cu > 0 caps the update kernel's
 * residency (experiment knob); 0 = fill the chip.  start_flag (optional, device uint32): the update kernel's first
 * workgroup stores start_value there as it starts -- a second stream gated on the word (esr_stream_gate: the id sort
 * of a coming batch) is released while that kernel runs, i.e. arrives after it has taken its wave slots, and the main
 * queue carries no event marker for it.
 * dtype (round 6): the embedding rows' type -- ESR_F32, or ESR_BF16 (BASELINE config 4's dtype: both buffers bf16 [V, D],
 * fp32 accumulator, fp32 bias tables): rows are widened on the load (exact), stepped in f32 and rounded to nearest even on
 * their one store; ~7 200 instead of 10 292 bytes per pair at D = 256. */
size_t esr_glove_step_workspace_bytes(int64_t B, int D);
int esr_glove_train_step(void* emb, void* emb_shadow, uint8_t* emb_loc, float* emb_accum, float* bias,
                         float* bias_accum, int64_t V, int dtype, int D, const int32_t* inputs, const float* target, int64_t B,
                         int mode, float lr, float eps, uint32_t stamp, const int32_t* presorted_ids,
                         const int32_t* presorted_perm, void* plan, int long_runs, int blocks_per_cu,
                         uint32_t* start_flag, uint32_t start_value, float* loss, void* workspace,
                         size_t workspace_bytes, esr_stream_t stream);
/* Holds `stream` (one sleeping wave) until the device word *flag has reached `value` -- sequence numbers, compared
 * wrap-safe as (int32)(*flag - value) >= 0 -- or timeout_us have passed (then the stream goes on: the gate orders work
 * for speed and for producers that are certain to run; it never hangs a queue).  The cheap cross-stream edge of the
 * training loops: no event marker on the producing stream, whose kernel announces itself with one store
 * (esr_glove_train_step's start_flag).  Build-defined: the reference's loops are single-stream JAX dispatch
 * (wikipedia/train_cooccurence.py:103-112). */
int esr_stream_gate(const uint32_t* flag, uint32_t value, uint32_t timeout_us, esr_stream_t stream);
/* The steps of nbatch <= 8 planned batches issued by ONE call (a training loop's per-step host work is then one
 * foreign call per group: at the reference's batch of 2048 pairs a step is ~20 us of kernels, less than a ctypes call
 * with 25 arguments plus the Python around it).  inputs / targets / sorted_ids / perm / plans as esr_glove_plan took and
 * made them; stamps first_stamp, first_stamp + 1, ... (all <= 127); long_runs: host int32 [nbatch] (0 / 1 / -1 as above)
 * or NULL = unknown; losses [nbatch]. */
int esr_glove_train_steps(void* emb, void* emb_shadow, uint8_t* emb_loc, float* emb_accum, float* bias,
                          float* bias_accum, int64_t V, int dtype, int D, int nbatch, const int32_t* const* inputs,
                          const float* const* targets, int64_t B, int mode, float lr, float eps, uint32_t first_stamp,
                          const int32_t* sorted_ids, const int32_t* perm, void* plans, const int32_t* long_runs,
                          float* losses, void* workspace, size_t workspace_bytes, esr_stream_t stream);
/* Plans of nbatch <= 8 coming batches of B pairs in one launch: inputs[b] = int32 [2, B], targets[b] = f32 [B],
 * sorted_ids / perm = [nbatch, 2B] (esr_segment_sort_ids_batched layout, or one esr_segment_sort_ids result with
 * nbatch = 1), plans = nbatch x esr_glove_plan_bytes(B) bytes, 256-byte aligned.  hints (optional) [nbatch]:
 * hints[b] = gen when a run of equal ids in list b is longer than 32 positions -- compare with `gen` (any value the
 * caller has not passed for this array before) after the stream has passed the call; words need no clearing. */
size_t esr_glove_plan_bytes(int64_t B);
int esr_glove_plan(const int32_t* const* inputs, const float* const* targets, int nbatch, int64_t B,
                   const int32_t* sorted_ids, const int32_t* perm, void* plans, int32_t* hints, int32_t gen,
                   esr_stream_t stream);
/* The hint alone, for lists whose steps resolve their records themselves (more than 32 768 ids: esr_glove_train_step
 * then ignores `plan`): hint[0] = gen when sorted_ids [n] has a run of equal ids longer than `chunk` positions (32 for
 * the GloVe step, 8 for the triplet step).  `hint` may be device memory or pinned host memory. */
int esr_long_run_hint(const int32_t* sorted_ids, int64_t n, int chunk, int32_t* hint, int32_t gen, esr_stream_t stream);
int esr_rows_consolidate(void* primary, const void* shadow, uint8_t* loc, int64_t V, int dtype, int D,
                         esr_stream_t stream);
/* loc[r] &= 1 for every row: forget the stamps, keep the locations (see esr_glove_train_step's `stamp`). */
int esr_rows_restamp(uint8_t* loc, int64_t V, esr_stream_t stream);

/* ---- S1-S3: STL score head + triplet loss -- pinterest/models.py:67-72,
 * pinterest/train_shop_the_look.py:93-122 --------------------------------------------------
 * Towers are id-embedding tables; pos and neg rows may come from different tables (pass the product
 * table twice for the id towers).  ids == NULL means "row b of the table", so the three (B,D)
 * embedding matrices of the reference head can be passed directly as scene/pos/neg tables.
 *   loss = (sum_b relu(1 + neg_b - pos_b) + regularization * sum_b reg) / batch_size   (train)
 *   eval_step (:118) = the same call with with_reg = 0, batch_size = 1 and g_* = NULL.
 * pos_score / neg_score [B] may be NULL.  g_scene/g_pos/g_neg [B, D] per-occurrence gradients. */
size_t esr_triplet_workspace_bytes(int64_t B);
int esr_triplet_fwd_bwd(const float* scene_table, int64_t Vs, const float* pos_table, int64_t Vp,
                        const float* neg_table, int64_t Vn, int D, const int32_t* scene_ids, const int32_t* pos_ids,
                        const int32_t* neg_ids, int64_t B, float regularization, float batch_size,
                        int with_reg, float* loss, float* pos_score, float* neg_score,
                        float* g_scene, float* g_pos, float* g_neg, void* workspace,
                        size_t workspace_bytes, esr_stream_t stream);

/* ---- S2 in one pass: train_step (pinterest/train_shop_the_look.py:93-109) = loss + gradients + sparse Adagrad ----
 * on both id towers, no [3B, D] gradient in memory: the update kernel walks the sorted occurrences of every distinct row
 * and forms each occurrence's gradient row on chip from the two OTHER rows of its triplet (both partner rows give the
 * pos / neg scores and the hinge mask; the own row gives the regulariser term).  Both towers are DOUBLE-BUFFERED with
 * stamped location bytes as in esr_glove_train_step (`scene` / `scene_shadow` + scene_loc [Vs], `product` /
 * `product_shadow` + product_loc [Vp]; one `stamp` per step for both; esr_rows_restamp / esr_rows_consolidate per
 * table).  Occurrence ids are the virtual rows [scene_ids ; Vs + pos_ids ; Vs + neg_ids]; presorted_ids /
 * presorted_perm (both or neither) = their esr_segment_sort_ids_multi output computed ahead, NULL = sort here; plan /
 * long_runs as for esr_glove_train_step (esr_triplet_plan; chunks of 8 positions here).  With a plan and uniform ids a
 * step is ONE launch: the loss leaves the update kernel through an exact integer reduction (a mean loss beyond 2048
 * comes out +inf).  Same element arithmetic (trip_grad, adagrad_elem), same sort and the same association of every row
 * sum as esr_triplet_fwd_bwd + esr_sparse_adagrad_scatter_multi.
 * loss [1] = (sum_b relu(1 + neg_b - pos_b) + regularization * reg) / batch_size.
 *
 * DIRECT mode (round 4, the default; ESR_TRIPLET_STEP=stamped keeps the walk described above): one row group per TRIPLET
 * reads its three rows once and steps every row that occurs once in the batch IN PLACE (row + accumulator read and
 * written once: the fused minimum of 4 row transfers per row, against 6 per occurrence for the stamped walk); a row with
 * 2 .. 8 occurrences is stepped by whichever of its triplets finishes last (gradient rows parked at their sorted
 * positions, one atomic arrival per occurrence); longer runs by a second launch, made only when the plan's hint says
 * one exists.  Nothing is double-buffered: the *_shadow / *_loc arguments and `stamp` are ignored and may be NULL / 0,
 * rows never leave `scene` / `product`.  Same sums, same association as the stamped walk and the six-launch path.
 * dtype (round 6): ESR_F32, or ESR_BF16 -- bf16 table rows [V, D] with fp32 accumulators (BASELINE config 4's dtype;
 * direct mode only): a row is widened on the load (exact), stepped in f32 and rounded to nearest even on its one store,
 * as esr_sparse_adagrad_scatter does; 5 376 instead of 7 680 bytes per triplet at D = 128. */
size_t esr_triplet_step_workspace_bytes(int64_t B, int D);
int esr_triplet_train_step(void* scene, void* scene_shadow, uint8_t* scene_loc, float* scene_accum, int64_t Vs,
                           void* product, void* product_shadow, uint8_t* product_loc, float* product_accum,
                           int64_t Vp, int dtype, int D, const int32_t* scene_ids, const int32_t* pos_ids,
                           const int32_t* neg_ids, int64_t B, float regularization, float batch_size, float lr,
                           float eps, uint32_t stamp, const int32_t* presorted_ids, const int32_t* presorted_perm,
                           void* plan, int long_runs, float* loss, void* workspace, size_t workspace_bytes,
                           esr_stream_t stream);
/* The steps of nbatch <= 8 planned batches by one call (see esr_glove_train_steps): ids[3 b + {0, 1, 2}] as for
 * esr_triplet_plan, losses [nbatch]. */
int esr_triplet_train_steps(void* scene, void* scene_shadow, uint8_t* scene_loc, float* scene_accum, int64_t Vs,
                            void* product, void* product_shadow, uint8_t* product_loc, float* product_accum,
                            int64_t Vp, int dtype, int D, int nbatch, const int32_t* const* ids, int64_t B, float regularization,
                            float batch_size, float lr, float eps, uint32_t first_stamp, const int32_t* sorted_ids,
                            const int32_t* perm, void* plans, const int32_t* long_runs, float* losses, void* workspace,
                            size_t workspace_bytes, esr_stream_t stream);
/* Plans of nbatch <= 8 coming batches of B triplets in one launch: ids[3 b + {0, 1, 2}] = scene / pos / neg id lists
 * of batch b, sorted_ids / perm = [nbatch, 3B] (esr_segment_sort_ids_batched layout), plans = nbatch x
 * esr_triplet_plan_bytes(B) bytes, 256-byte aligned; hints / gen as for esr_glove_plan (runs longer than 8 positions).
 * Direct mode: gen != 0 also tags the plan's long-run counter with the full 32-bit value (a count left in the buffer by
 * an earlier plan call is replaced, no fill launch): pass a generation that differs from the one the buffer was last
 * planned with (a counter that grows by one per call does), and ZERO a plan buffer before its first use.  gen == 0: the
 * counter is cleared by a fill in front of the launch.  A direct-mode plan is left as planned by the step it feeds
 * (the arrival that completes a run clears the run's counter), so it may feed another step of the SAME batch; a
 * stamped-mode plan (ESR_TRIPLET_STEP=stamped) feeds exactly one step. */
size_t esr_triplet_plan_bytes(int64_t B);
int esr_triplet_plan(const int32_t* const* ids, int nbatch, int64_t B, int64_t Vs, const int32_t* sorted_ids,
                     const int32_t* perm, void* plans, int32_t* hints, int32_t gen, esr_stream_t stream);

/* ---- north_star: in-batch-negative sampled softmax on the dense B x B score matrix --------
 * (build-defined; the closest reference precedent is spotify/models.py:74-87).
 *   S = scale * Q C^T (FP32 MFMA), ce_i = logsumexp_j S_ij - S_ii,
 *   loss = (sum_i ce_i + regularization * sum_i [reg(q_i) + reg(c_i)]) / batch_size
 *   gQ = scale * (softmax(S) - I) C / batch_size + dreg ; gC likewise with S^T.
 * Q, C, gQ, gC are [B, D] row-major, any B >= 1 (tiles of 32 rows; a ragged last tile is masked out of every
 * softmax); D is 32, 64 or 128. */
size_t esr_inbatch_workspace_bytes(int64_t B, int D);
int esr_inbatch_softmax_fwd_bwd(const float* Q, const float* C, int64_t B, int D, float scale,
                                float regularization, float batch_size, float* loss, float* lse,
                                float* gQ, float* gC, void* workspace, size_t workspace_bytes,
                                esr_stream_t stream);

/* Same contract with FP32-EQUIVALENT products on the bf16 matrix cores: every operand is split exactly
 * into three bf16 planes and a product is the six leading cross terms (dropped terms <= 2^-23 |a||b|),
 * 2.67x fewer matrix-pipe cycles than v_mfma_f32_32x32x2_f32.  D <= 128 and a multiple of 4 (narrower rows are
 * zero-padded into the 128-column tiles), B a multiple of 128. */
size_t esr_inbatch3_workspace_bytes(int64_t B, int D);
int esr_inbatch_softmax_fwd_bwd_bf16x3(const float* Q, const float* C, int64_t B, int D, float scale,
                                       float regularization, float batch_size, float* loss, float* lse,
                                       float* gQ, float* gC, void* workspace, size_t workspace_bytes,
                                       esr_stream_t stream);
/* The whole in-batch step head without materialised Q / C: row i of Q is query_table[query_ids[i]], row i of C is
 * cand_table[cand_ids[i]] (tables f32 or bf16, dtype = ESR_F32 / ESR_BF16; the id-embedding towers that replace
 * pinterest/models.py:64-70).  The gather is folded into the bf16-plane split and into the merge kernels; gQ / gC
 * are the per-occurrence gradient rows [B, 128].  gq_rows / gc_rows (optional, may be NULL): gradient row i is
 * written at gQ[gq_rows[i]] / gC[gc_rows[i]] instead of row i -- the row-sharded step passes the bucket positions
 * of the occurrences, with gQ == gC == the buffer that goes straight into the gradient all-to-all.
 * Same workspace as above. */
int esr_inbatch_towers_fwd_bwd_bf16x3(const void* query_table, int64_t Vq, const void* cand_table, int64_t Vc,
                                      int dtype, int D, const int32_t* query_ids, const int32_t* cand_ids,
                                      const int32_t* gq_rows, const int32_t* gc_rows, int64_t B, float scale,
                                      float regularization, float batch_size, float* loss, float* lse,
                                      float* gQ, float* gC, void* workspace, size_t workspace_bytes,
                                      esr_stream_t stream);

/* Same two contracts with the products formed from TWO fp16 planes per operand (x * 2^e = x1 + x2 to 2^-24 relative with
 * round-to-nearest planes; a.b ~= a2 b1 + a1 b2 + a1 b1, dropped term <= 2^-24 |a||b|): three v_mfma_f32_32x32x16_f16 per
 * product instead of six bf16 ones, i.e. half the matrix-core work of the bf16x3 entry points at the same f32-grade
 * error (the kernels run at the chip's power limit, so fewer MFMAs is what shortens the step).  fp16's narrow range is
 * handled inside: a per-matrix power-of-two scale from the batch's largest |element|, and an exponent reference tied
 * to the true row maximum.  Pass C reads the B x B probabilities pass Q stored (as the two fp16 planes pass Q forms for
 * its own product; their per-row factors ride on per-split scaled copies of Q -- esr_inbatch2h_pass_c_forms): D <= 128 and a multiple of 4 (narrower
 * rows are zero-padded into the 128-column tiles; gQ / gC are [B, D]), B a multiple of 128 and <= 16384 (workspace ~ 4 B^2 bytes); esr_inbatch2h_workspace_bytes returns 256 for a B it cannot serve.
 * GUARANTEED ERROR (tests/test_gpu_kernels.py): an operand element x of a matrix whose largest |element| is M enters the
 * products as x (1 + d) + a with |d| <= 2^-24 and |a| <= 2^-26 M 2^-16 -- relative for elements within 2^-16 of M,
 * absolute below.  Consequences that are asserted against the fp64 oracle: loss, lse and norm-wise gradients within 1e-5
 * (every shape / range test); every gradient entry within 1e-4 of max(|entry|, 1e-3 of the largest entry) at C2 size;
 * with row norms spread over FOUR decades inside each matrix (a few hot rows 100 x the median) every 128-row block of
 * gQ / gC within 2e-5 of the block's own largest entry and every row within 1e-4 of its own (measured 1.6e-6 / 1.7e-6,
 * the exact-f32 MFMA path measures 1.5e-6 / 3.5e-6); a 20-step training trajectory at C2 size within 1e-5 on every loss
 * and norm-wise on tables and accumulators (measured 1e-6).  A matrix whose rows span MORE than ~2^16 in magnitude should
 * take the bf16x3 entry points, whose three planes are an exact split of every element. */
size_t esr_inbatch2h_workspace_bytes(int64_t B, int D);
int esr_inbatch_softmax_fwd_bwd_f16x2(const float* Q, const float* C, int64_t B, int D, float scale,
                                      float regularization, float batch_size, float* loss, float* lse,
                                      float* gQ, float* gC, void* workspace, size_t workspace_bytes,
                                      esr_stream_t stream);
int esr_inbatch_towers_fwd_bwd_f16x2(const void* query_table, int64_t Vq, const void* cand_table, int64_t Vc,
                                     int dtype, int D, const int32_t* query_ids, const int32_t* cand_ids,
                                     const int32_t* gq_rows, const int32_t* gc_rows, int64_t B, float scale,
                                     float regularization, float batch_size, float* loss, float* lse,
                                     float* gQ, float* gC, void* workspace, size_t workspace_bytes,
                                     esr_stream_t stream);
/* Which form pass C of the LAST f16x2 call on `workspace` took, per pass-Q split (forms[8], device memory, copied on
 * `stream`): 0 = the scaled copy of Q for that split fed the matrix cores as stored (round 6: dC_j = sum_i P'_ij (f_is q_i),
 * the stored fp16 planes of P' are the MFMA operand, no VALU work on probabilities), non-zero = some row of the copy lay
 * more than ~17 binades under the copy's largest element and the workgroups of that split applied the factors to the
 * probabilities in registers instead (the general form; also taken for every split when B / 32 / splits is not a
 * multiple of 8, where the words stay 0).  Diagnostics and tests; no reference counterpart. */
int esr_inbatch2h_pass_c_forms(const void* workspace, size_t workspace_bytes, int64_t B, int32_t* forms,
                               esr_stream_t stream);

/* The whole in-batch training step of the two towers as ONE call (fp16 x 2 score path + the build's row-sparse Adagrad;
 * what train_step(state, scene, pos, None, ...) of esrecsys_amd/pinterest/train_shop_the_look.py issues per batch):
 * gather + split -> pass Q -> [merge<Q> -> Adagrad on the query tower] beside [factors -> pass C -> merge<C> -> Adagrad on
 * the candidate tower].  side_stream (optional): a second stream of the same device; the first bracket then runs on it
 * while the second runs on `stream` (pass C needs only the factors of merge<Q>: 14 + 6 us of the step leave its critical
 * path at B = 8192), joined before the call returns control of `stream`; NULL: everything in order on `stream`.  Both
 * forms run the same kernels on the same values -- tables, accumulators, loss and lse are bit-identical to
 * esr_inbatch_towers_fwd_bwd_f16x2 + esr_sparse_adagrad_scatter_multi on the occurrence list [query ids ; Vq + cand ids].
 * presorted_vids / presorted_perm [2B] (both or neither): that list sorted by esr_segment_sort_ids_multi /
 * _batched ahead of the call (offsets {0, Vq}); NULL: sorted here.  long_runs: 0 = the caller knows (esr_long_run_hint) that
 * no id occurs more than 32 times, else -1.  lse [B] optional.  Tables f32 or bf16 [V, D] with fp32 accumulators, D <= 128
 * (a multiple of 4), B a multiple of 128, <= 16384.  Workspace: esr_inbatch_train_step_workspace_bytes, 256-byte aligned. */
size_t esr_inbatch_train_step_workspace_bytes(int64_t B, int D);
int esr_inbatch_train_step_f16x2(void* query_table, float* query_accum, int64_t Vq, void* cand_table, float* cand_accum,
                                 int64_t Vc, int dtype, int D, const int32_t* query_ids, const int32_t* cand_ids,
                                 int64_t B, float scale, float regularization, float batch_size, float lr, float eps,
                                 const int32_t* presorted_vids, const int32_t* presorted_perm, int long_runs, float* loss,
                                 float* lse, void* workspace, size_t workspace_bytes, esr_stream_t stream,
                                 esr_stream_t side_stream);

/* ---- G4 (build's production optimizer): sort + segment-reduce + sparse Adagrad -----------
 * Replaces the dense V x D gradient + dense optimizer sweep of
 * wikipedia/train_cooccurence.py:86-101 with a row-sparse update.
 * esr_segment_sort_ids: stable sort of occurrence ids; perm[k] = original occurrence index.  Every size runs this
 * library's own kernels (one-workgroup bitonic sort, tile sort + rank merge, 11-bit LSD radix passes; no device-library
 * sort): n up to 2^30 ids.
 * The scatter entry points below may OVERWRITE grad_rows: runs of equal ids that cross a 32-position boundary are
 * summed chunk-wise, the partial sums parked in the gradient rows themselves, and combined in a fixed order. */
size_t esr_segment_sort_workspace_bytes(int64_t n);
int esr_segment_sort_ids(const int32_t* ids, int64_t n, int64_t V, int32_t* sorted_ids,
                         int32_t* perm, void* workspace, size_t workspace_bytes,
                         esr_stream_t stream);
/* The same sort over a list given as up to four segments [ids_k + offsets[k]] (the towers of one step as virtual rows
 * offsets[k] + id of their concatenation): read in place, no concatenated copy.  Same workspace query with
 * n = the sum of the counts. */
int esr_segment_sort_ids_multi(const int32_t* const* ids, const int64_t* counts, const int64_t* offsets, int nseg,
                               int64_t V, int32_t* sorted_ids, int32_t* perm, void* workspace,
                               size_t workspace_bytes, esr_stream_t stream);
/* The lists of `nbatch` (<= 8) coming batches sorted in ONE launch sequence: a training loop knows the ids of the next
 * batches before it needs them (the reference's loop draws them from its data iterator,
 * pinterest/train_shop_the_look.py:195-204), and at the reference's batch sizes the two-launch sort is latency, not
 * work -- eight lists cost what one does.  ids[b * nseg + k] = segment k of list b; counts / offsets are the same for
 * every list (n = their sum); sorted_ids / perm are [nbatch][n], list b exactly what esr_segment_sort_ids_multi would
 * give for it (perm indexes list b's own occurrences).  Up to 2 048 ids: one launch for all lists; up to 32 768: two;
 * up to 2 097 152 (and V < 2^33: at most three 11-bit digits): three per radix pass; beyond that the lists are sorted
 * one after the other. */
size_t esr_segment_sort_batched_workspace_bytes(int64_t n, int nbatch);
int esr_segment_sort_ids_batched(const int32_t* const* ids, const int64_t* counts, const int64_t* offsets, int nseg,
                                 int nbatch, int64_t V, int32_t* sorted_ids, int32_t* perm, void* workspace,
                                 size_t workspace_bytes, esr_stream_t stream);
/* For each distinct id: G = sum of its grad rows (occurrence order); acc += G*G;
 * p -= lr * G * rsqrt(acc + eps).  table dtype f32 or bf16 (fp32 accumulator either way). */
int esr_sparse_adagrad_scatter(void* table, int dtype, float* accum, int64_t V, int D,
                               const int32_t* sorted_ids, const int32_t* perm, int64_t n,
                               float* grad_rows, float lr, float eps, esr_stream_t stream);
/* Several tables (same D, same dtype) updated from ONE sorted occurrence list: ids are virtual rows
 * vid = row_offsets[t] + id of the concatenation of <= 4 tables, so a two-tower step needs one sort chain
 * and one update launch.  tables / accums / row_offsets (ntables + 1 entries) are HOST arrays of device
 * pointers / int64.  esr_concat_offset_ids builds the virtual ids: out = [ids[0] + offsets[0] ; ids[1] + ...]
 * (ids / counts / offsets are host arrays; the id buffers are device memory).
 * esr_sparse_adagrad_scatter_multi's long_runs: 0 = the caller knows (esr_long_run_hint with chunk = 32 on the sorted
 * list) that no id fills a whole 32-position block and the next position, and the launch that combines the chunk
 * partials of such runs is skipped; anything else = launched (on a list without them it only screens the boundaries). */
int esr_concat_offset_ids(const int32_t* const* ids, const int64_t* counts, const int64_t* offsets, int nseg,
                          int32_t* out, esr_stream_t stream);
/* out[i, :] = tables[t][vids[i] - row_offsets[t], :] (row bytes must be a multiple of 16). */
int esr_gather_rows_multi(const void* const* tables, const int64_t* row_offsets, int ntables, int dtype, int D,
                          const int32_t* vids, int64_t n, void* out, esr_stream_t stream);
int esr_sparse_adagrad_scatter_multi(void* const* tables, float* const* accums, const int64_t* row_offsets,
                                     int ntables, int dtype, int D, const int32_t* sorted_vids,
                                     const int32_t* perm, int64_t n, float* grad_rows, float lr, float eps,
                                     int long_runs, esr_stream_t stream);
/* Row-sparse SGD (p -= lr * G), same segment reduction. */
int esr_sparse_sgd_scatter(void* table, int dtype, int64_t V, int D, const int32_t* sorted_ids,
                           const int32_t* perm, int64_t n, float* grad_rows, float lr,
                           esr_stream_t stream);
/* Reference-faithful dense gradient: dense[V, D] = 0 then dense[id] = segment sum
 * (the scatter-add JAX's autodiff performs for nn.Embed, train_cooccurence.py:86-87). */
int esr_rows_to_dense(float* dense, int64_t V, int D, const int32_t* sorted_ids,
                      const int32_t* perm, int64_t n, float* grad_rows, esr_stream_t stream);
/* out[id, :] = the left-to-right sum of the gradient rows of the occurrences with sorted id `id`, for every id that
 * occurs -- esr_rows_to_dense without the zero fill, for callers whose ids cover [0, rows_out) (the distinct-row index
 * of esr_unique_by_owner: the per-occurrence gradient rows of a batch become ONE row per distinct row before they cross
 * the exchange).  May overwrite grad_rows (chunk partials of long runs are parked there). */
int esr_segment_sum_rows(float* out, int64_t rows_out, int D, const int32_t* sorted_ids, const int32_t* perm, int64_t n,
                         float* grad_rows, esr_stream_t stream);
/* optax.adam over every element -- wikipedia/train_cooccurence.py:99-101,171.
 * step = the 1-based count AFTER this update. */
int esr_dense_adam(float* param, float* mu, float* nu, const float* grad, int64_t numel, float lr,
                   float b1, float b2, float eps, int64_t step, esr_stream_t stream);

/* Lazy optax.adam: the dense trajectory without a whole-table pass per step.  A row that gets no gradient still moves
 * (mu *= b1 ; nu *= b2 ; p -= lr (mu ibc1) / (sqrt(nu ibc2) + eps)) -- a function of (p, mu, nu, t) alone -- so it is
 * moved when it is next read.  last[row] (int32 [V]) = the step the row is current with (0 for a fresh table: every
 * row current with step 0).  A step t >= 1 is: esr_adam_catchup_rows2 on the ids the step will read (rows brought up to
 * step t - 1 and stamped so), the forward / backward on current rows, then esr_sparse_adam_step_lazy (the touched rows
 * caught up if they were not, one whole Adam step with the run-summed gradient, marked t).  esr_adam_flush brings EVERY
 * row up to step t -- before a dense step, a checkpoint, or anybody reading the whole tables.
 *
 * Exactness contract, against esr_dense_adam stepped on the same gradients (the dense gradient of esr_rows_to_dense):
 *   - a touched row, and a row whose gap is <= 8 steps (ESR_ADAM_EXACT_STEPS), is bit-identical in p, mu and nu: the
 *     same per-element operations, the same fp32 bias corrections (computed on the host in fp64, as esr_dense_adam);
 *   - a longer gap of n steps is applied in closed form in fp64: mu and nu within 1e-6 relative of an fp64 replay of
 *     the n zero-gradient steps, p within 1e-6 |dp| + 2 ulp(p) of it (dp = that replay's displacement);
 *   - a row with mu = nu = 0 never moves (bit-identical).
 * fp32 tables only.  D <= 1024 (D % 4 == 0) or D <= 256; table / mu / nu 16-byte aligned, last / ids 4-byte aligned. */
#define ESR_ADAM_EXACT_STEPS 8
/* Rows ids0[i] % modulus0 (modulus 0: ids0[i]) of table 0 and ids1[i] % modulus1 of table 1 up to step - 1 (ids outside
 * [0, V) are skipped).  Table 1 is optional (table1 = NULL); the two may differ in width and row count.  One launch. */
int esr_adam_catchup_rows2(float* table0, float* mu0, float* nu0, int32_t* last0, int64_t V0, int D0, const int32_t* ids0,
                           int64_t n0, int modulus0, float* table1, float* mu1, float* nu1, int32_t* last1, int64_t V1,
                           int D1, const int32_t* ids1, int64_t n1, int modulus1, int step, float lr, float b1, float b2,
                           float eps, esr_stream_t stream);
/* Step `step` on the touched rows of one or two same-width tables addressed by virtual rows (row_offsets[0] = 0,
 * row_offsets[t + 1] = row_offsets[t] + V_t; sorted_vids / perm from esr_segment_sort_ids, grad_rows [n, D]).  Duplicates
 * are summed exactly as esr_rows_to_dense sums them.  May overwrite grad_rows (partials of long runs). */
int esr_sparse_adam_step_lazy(float* const* tables, float* const* mus, float* const* nus, int32_t* const* lasts,
                              const int64_t* row_offsets, int ntables, int D, const int32_t* sorted_vids, const int32_t* perm,
                              int64_t n, float* grad_rows, float lr, float b1, float b2, float eps, int step,
                              esr_stream_t stream);
/* The owner side of a row-sharded lookup under lazy Adam, in one pass: catch up and serve.  sorted_rows / perm =
 * esr_segment_sort_ids of the n virtual rows asked of this rank (row_offsets as esr_sparse_adam_step_lazy, one or two
 * same-width tables).  Every distinct row is brought up to step - 1 if last < step - 1 (p, mu, nu stored back, last =
 * step - 1) and written to served[perm[j]] ([n, D] fp32) for every j of its run; duplicate requests get the same bytes.
 * One launch; a second, copy-only one serves the positions of runs longer than the row group (Zipf batches).
 * served = NULL: catch up only (perm may then be NULL).  Rows outside [0, row_offsets[ntables]) are skipped.
 * Exactness: served rows, p, mu, nu and last are bit-identical to esr_adam_catchup_rows2 on each table's rows followed
 * by esr_gather_rows_multi on sorted_rows, for short and long gaps alike (the same per-row geometry and arithmetic).
 * served 16-byte aligned (4-byte when D % 4 != 0), sorted_rows / perm 4-byte aligned; tables as above. */
int esr_adam_catchup_gather(float* const* tables, float* const* mus, float* const* nus, int32_t* const* lasts,
                            const int64_t* row_offsets, int ntables, int D, const int32_t* sorted_rows, const int32_t* perm,
                            int64_t n, float* served, int step, float lr, float b1, float b2, float eps,
                            esr_stream_t stream);
/* Every row with last < step up to `step`; last = step afterwards. */
int esr_adam_flush(float* table, float* mu, float* nu, int32_t* last, int64_t V, int D, int step, float lr, float b1,
                   float b2, float eps, esr_stream_t stream);

/* ---- G6: Glove.score_all + find_knn -- wikipedia/models.py:50-55, train_cooccurence.py:91-97
 * scores[v, t] = E[v] . E[token[t]]  ([V, T] row-major, no bias);
 * indices = stable ascending argsort of every column ([V, T] int32). */
int esr_score_all(const float* emb, int64_t V, int D, const int32_t* token, int T, float* scores,
                  esr_stream_t stream);
/* The k last rows of that argsort without sorting the columns (what dump_knn reads: train_cooccurence.py:114-126 takes
 * indices[-10:]): a radix select per column, k <= 1024.  out_indices / out_scores [T, k], best first:
 * out_indices[t][j] = argsort(scores[:, t])[V - 1 - j], ties exactly as the stable ascending argsort leaves them. */
int esr_topk_columns(const float* scores, int64_t V, int T, int k, float* out_scores, int32_t* out_indices,
                     esr_stream_t stream);
size_t esr_argsort_columns_workspace_bytes(int64_t V, int T);
int esr_argsort_columns(const float* scores, int64_t V, int T, int32_t* indices, void* workspace,
                        size_t workspace_bytes, esr_stream_t stream);

/* ---- find_top_k -- pinterest/make_recommendations.py:49-65 --------------------------------
 * scores[q, n] = queries[q] . candidates[n]; top-k per query, descending, ties -> lower index. */
size_t esr_score_topk_workspace_bytes(int64_t nq, int64_t N, int k);
int esr_score_topk(const float* queries, const float* candidates, int64_t nq, int64_t N, int D,
                   int k, float* out_scores, int32_t* out_indices, void* workspace,
                   size_t workspace_bytes, esr_stream_t stream);

/* ---- N3 / config 5: batched brute-force retrieval ------------------------------------------
 * find_top_k (pinterest/make_recommendations.py:49-65) for a BATCH of queries -- the scenes loop of
 * :123-132 in one call -- and the eval of spotify/train_spotify.py:120 (top_k(500) over every track):
 *   scores[q, n] = queries[q] . candidates[n];  per query the k best, descending, ties -> lower index.
 * queries f32 [nq, D], candidates f32 [N, D], k <= min(N, 1024).  The reported index of local candidate
 * n is index_base + n * index_step (row-sharded candidates: base = rank, step = world); index_base >= 0, index_step > 0,
 * and the last index index_base + (N - 1) * index_step at most 2^31 - 1.
 * mode ESR_RETRIEVE_EXACT: products from three exact bf16 planes per operand (six MFMA cross terms,
 *   f32 accumulate) -- f32-equivalent scores, the brute-force answer.
 * mode ESR_RETRIEVE_BF16: one bf16 plane per operand -- the approximate candidate stage; follow with
 *   esr_rescore_candidates + esr_topk_merge for an exact re-rank of k' > k candidates.
 * mode ESR_RETRIEVE_F16X2: products from two fp16 planes of x * 2^e per operand (e per matrix, from its largest
 *   |element|; three MFMA cross terms, f32 accumulate) -- f32-grade scores (<= ~3 * 2^-24 |a||b| per elementary product)
 *   at half the matrix-core work of ESR_RETRIEVE_EXACT; one extra read of both matrices for the scales.
 * mode ESR_RETRIEVE_F16R (round 6): the EXACT top-k of the f32 scores from a ONE-term filter.  Every candidate is scored
 *   with the hi fp16 plane alone (one MFMA term instead of three); that score is off by at most b = 2^-10 (1 + 2 %) |q|
 *   max |c| (two roundings to 11 bits, Cauchy-Schwarz; row norms from the scaling pass), so the true top-k lies among
 *   the candidates whose one-term score reaches (k-th best one-term score) - 2 b: k of them have true scores >= that
 *   k-th best - b, and a member of the true top-k cannot score lower than those in truth.  The filter keeps exactly that
 *   band per query; the survivors (~1.2 k at N = 1 M, D = 512, k = 500) are re-scored as f32 dot products and selected.
 *   A query whose band outgrows its list (near-equal scores for thousands of candidates) is switched to exact scores on
 *   the spot and filtered against (exact k-th best) - b from then on: the answer never depends on the band being small.
 *   Scores are the f32 dot products (fmaf over 16 lanes + tree), ties -> lower index, like ESR_RETRIEVE_EXACT. */
#define ESR_RETRIEVE_EXACT 0
#define ESR_RETRIEVE_BF16 1
#define ESR_RETRIEVE_F16X2 2
#define ESR_RETRIEVE_F16R 3
size_t esr_retrieve_workspace_bytes(int64_t nq, int64_t N, int D, int k, int mode);
int esr_retrieve_topk(const float* queries, const float* candidates, int64_t nq, int64_t N, int D, int k,
                      int mode, int32_t index_base, int32_t index_step, float* out_scores,
                      int32_t* out_indices, void* workspace, size_t workspace_bytes, esr_stream_t stream);
/* A PREPARED corpus (round 6; every mode): everything a call does with the candidates before it looks at a query -- the
 * statistics pass (exponent, largest row norm: the scaled fp16 modes) and the split into the mode's planes, up to
 * 2 x 4 N D bytes of reads and 2 P N D of writes -- done ONCE for a corpus that serves many calls (the reference scores every batch of
 * scenes against the same product embeddings: pinterest/make_recommendations.py:123-132).  esr_retrieve_prepare fills
 * `prepared` (esr_retrieve_prepared_bytes(N, D, mode) bytes, 256-byte aligned, the caller's; valid while the candidate
 * matrix is unchanged; made for ONE mode); esr_retrieve_topk_prepared is esr_retrieve_topk of that mode with those passes
 * left out -- the same products, filter, band, re-score (from the f32 `candidates`, still an argument) and answer, bit for
 * bit. */
size_t esr_retrieve_prepared_bytes(int64_t N, int D, int mode);
int esr_retrieve_prepare(const float* candidates, int64_t N, int D, int mode, void* prepared, size_t prepared_bytes,
                         esr_stream_t stream);
int esr_retrieve_topk_prepared(const float* queries, const float* candidates, const void* prepared, int64_t nq, int64_t N,
                               int D, int k, int mode, int32_t index_base, int32_t index_step, float* out_scores,
                               int32_t* out_indices, void* workspace, size_t workspace_bytes, esr_stream_t stream);
/* scores[q, j] = queries[q] . candidates[(indices[q, j] - index_base) / index_step] in f32 (fmaf chain per
 * lane, wave reduction); indices < 0 give -inf.  indices int32 [nq, kc]. */
int esr_rescore_candidates(const float* queries, const float* candidates, int64_t nq, int64_t N, int D,
                           const int32_t* indices, int kc, int32_t index_base, int32_t index_step,
                           float* scores, esr_stream_t stream);
/* top-k of per-query (score, index) lists [nq, n] -> [nq, k], descending, ties -> lower index: the merge
 * of the shards' answers (after an all-gather) and of re-scored candidate lists. */
int esr_topk_merge(const float* scores, const int32_t* indices, int64_t nq, int n, int k,
                   float* out_scores, int32_t* out_indices, esr_stream_t stream);
/* hits[0] = sum over queries of |{j : exact[q, j] occurs in approx[q, :]}| (the word is zeroed by the call): recall@k of an
 * approximate answer against the brute-force one is hits / (nq * ke).  approx int32 [nq, ka], exact int32 [nq, ke], ka <=
 * 8192; O(ka + ke) per query (a hash set in LDS).  Build-defined: the reference has no ANN path to measure. */
int esr_recall_at_k(const int32_t* approx, int64_t nq, int ka, const int32_t* exact, int ke, unsigned long long* hits,
                    esr_stream_t stream);

/* ---- config 5's ANN leg: IVF search (build-defined; the reference has no ANN index -- esr_retrieve_topk stays the exact
 * answer and the yardstick for recall).  The index (esrecsys_amd/ivf.py builds it with the kernels above): candidates
 * grouped by coarse centroid -- cands_sorted [N, D] list after list, list_off int32 [nlist + 1], orig int32 [N] = the
 * row each one has in the caller's matrix, max_list = the longest list.  probe_lists int32 [nq, nprobe]: the lists each
 * query looks into, best first (the nprobe best centroids: esr_retrieve_topk of the queries against the centroids).
 * Scores inside the probed lists are exact f32 (grouped GEMM on the FP32 matrix cores, one 64 x 64 tile per workgroup)
 * and the answer is the exact top-k of the probed lists: the first probe slots are scored densely and give every query
 * a threshold (its k-th best so far), the others pass through a filtered epilogue in rounds of eight slots with a
 * compacting select in between -- the scheme of esr_retrieve_topk.  out [nq, k], best first, entries a query's lists
 * could not fill: score -inf, index -1.  k <= 1024. */
size_t esr_ivf_search_workspace_bytes(int64_t nq, int nlist, int max_list, int nprobe, int k);
int esr_ivf_search(const float* queries, int64_t nq, int D, const float* cands_sorted, const int32_t* list_off,
                   const int32_t* orig, int nlist, int max_list, const int32_t* probe_lists, int nprobe, int k,
                   float* out_scores, int32_t* out_indices, void* workspace, size_t workspace_bytes, esr_stream_t stream);
/* Index build helpers (esrecsys_amd/ivf.py).  esr_run_offsets: list_off[v] = first position of the ASCENDING list
 * sorted [n] whose value is >= v, for v = 0 .. nvalues (int32 [nvalues + 1]: the inverted lists' boundaries from the sorted
 * assignments); max_len (optional, int32 [1]) = the longest run.  esr_ivf_centroids: centroids[v] = the unit vector of
 * sums[v] [nlist, D] where list v has members (list_off[v + 1] > list_off[v]; list_off NULL: every list), else of training
 * row fallback_rows[v] -- the centroid step of spherical k-means. */
int esr_run_offsets(const int32_t* sorted, int64_t n, int nvalues, int32_t* list_off, int32_t* max_len, esr_stream_t stream);
int esr_ivf_centroids(const float* sums, const int32_t* list_off, const float* train, const int32_t* fallback_rows,
                      int nlist, int D, float* centroids, esr_stream_t stream);

/* ---- N1: Spotify id-embedding two-tower -- spotify/models.py:27-90, spotify/train_spotify.py:77-131 ----
 * A track embeds as concat(album_table[album mod n_album_rows], artist_table[artist]) ([.., 2F]).  One call is one
 * playlist: album_ids / artist_ids are int32 [n + m + o] = context, next, neg occurrences in that order (raw ids:
 * the +0.1 isin boosts of models.py:76-81 compare un-hashed ids).  n <= 32, 2F <= 256. */
size_t esr_spotify_workspace_bytes(int n, int m, int o, int F);
/* SpotifyModel.get_embeddings (models.py:37-51): out [count, 2F] = concat(album row (hashed), artist row); l2 [count]. */
int esr_spotify_get_embeddings(const float* album_table, int64_t n_album_rows, const float* artist_table,
                               int64_t n_artists, int F, const int32_t* album_ids, const int32_t* artist_ids,
                               int64_t count, float* out, float* l2, esr_stream_t stream);
/* SpotifyModel.__call__: pos [m], neg [o], the three flipped self-affinity matrices [n,n] [m,m] [o,o], l2 [n+m+o]. */
int esr_spotify_forward(const float* album_table, int64_t n_album_rows, const float* artist_table,
                        int64_t n_artists, int F, const int32_t* album_ids, const int32_t* artist_ids, int n,
                        int m, int o, float* pos, float* neg, float* ctx_self, float* next_self,
                        float* neg_self, float* l2, void* workspace, size_t workspace_bytes,
                        esr_stream_t stream);
/* value_and_grad of train_step's loss_fn (train_spotify.py:78-109): loss [1]; the gradient as per-occurrence rows
 * g_album_rows / g_artist_rows [n+m+o, F] (occurrence r -> album row album_rows[r] = hashed id, artist row
 * artist_ids[r]).  max / min split their cotangent evenly over ties; relu'(0) = 0 [upstream jax]. */
int esr_spotify_fwd_bwd(const float* album_table, int64_t n_album_rows, const float* artist_table,
                        int64_t n_artists, int F, const int32_t* album_ids, const int32_t* artist_ids, int n,
                        int m, int o, float regularization, float* loss, int32_t* album_rows,
                        float* g_album_rows, float* g_artist_rows, void* workspace, size_t workspace_bytes,
                        esr_stream_t stream);
/* eval_step's result[1] (train_spotify.py:113-119): affinity [T] of every track of the corpus to the n context
 * tracks (row max over the context + boosts). */
int esr_spotify_affinity_all(const float* album_table, int64_t n_album_rows, const float* artist_table,
                             int64_t n_artists, int F, const int32_t* ctx_album, const int32_t* ctx_artist,
                             int n, const int32_t* all_albums, const int32_t* all_artists, int64_t T,
                             float* affinity, esr_stream_t stream);
/* eval_step's top_k over every track (train_spotify.py:113-131) for P playlists at once (the eval loop of :270-281):
 * ctx_album / ctx_artist [P * n] raw ids (n context tracks per playlist), out_scores / out_indices [P * k], best first,
 * ties to the lower track index.  Every score has the bits esr_spotify_affinity_all gives that playlist, so the result
 * equals its top-k.  1 <= n <= 32, 2F <= 256, P >= 1, 1 <= k <= min(T, 1024).  The workspace holds no [P, T] scores:
 * the first chunk of tracks is scored densely, later chunks append only what reaches each playlist's running
 * k-th best (lists of ~1 GiB in all; ESR_SPOTIFY_EVAL_CHUNK sets the tracks per chunk). */
size_t esr_spotify_topk_batch_workspace_bytes(int64_t P, int n, int64_t T, int F, int k);
int esr_spotify_topk_batch(const float* album_table, int64_t n_album_rows, const float* artist_table,
                           int64_t n_artists, int F, const int32_t* ctx_album, const int32_t* ctx_artist, int64_t P,
                           int n, const int32_t* all_albums, const int32_t* all_artists, int64_t T, int k,
                           float* out_scores, int32_t* out_indices, void* workspace, size_t workspace_bytes,
                           esr_stream_t stream);
/* optax.sgd(lr, momentum) [upstream] in two halves: the decay over the whole table (trace *= momentum;
 * p -= lr * trace) and the row-sparse gradient (trace[row] += g; p[row] -= lr * g, duplicates summed in
 * occurrence order first).  Together: trace' = g + momentum * trace, p' = p - lr * trace'. */
int esr_dense_momentum_decay(float* param, float* trace, int64_t count, float lr, float momentum,
                             esr_stream_t stream);
int esr_sparse_momentum_scatter(float* table, float* trace, int64_t V, int D, const int32_t* sorted_ids,
                                const int32_t* perm, int64_t n, float* grad_rows, float lr,
                                esr_stream_t stream);
/* Lazy form of the same optimizer (row-sparse steps): no dense decay pass.  last [V] (int32, zero for a fresh state) is
 * the step each row is up to date with.  A step t >= 1 is: esr_momentum_catchup_rows on the ids the step will read
 * (ids[i] % modulus when modulus > 0: the album hash of spotify/models.py:37-41; duplicates welcome) -- the rows are
 * brought up to step t - 1 (n missed steps of trace *= momentum ; p -= lr * trace: one by one up to 2048, the closed form
 * beyond) and marked t -- then the forward / backward on current rows, then esr_sparse_momentum_step: trace = g +
 * momentum * trace ; p -= lr * trace on the touched rows (optax's order).  esr_momentum_flush brings EVERY row up to
 * `step` (before an eval, a checkpoint, any read of the whole table). */
int esr_momentum_catchup_rows(float* table, float* trace, int32_t* last, int64_t V, int D, const int32_t* ids, int64_t n,
                              int modulus, int step, float lr, float momentum, esr_stream_t stream);
int esr_sparse_momentum_step(float* table, float* trace, int64_t V, int D, const int32_t* sorted_ids,
                             const int32_t* perm, int64_t n, float* grad_rows, float lr, float momentum,
                             esr_stream_t stream);
int esr_momentum_flush(float* table, float* trace, int32_t* last, int64_t V, int D, int step, float lr, float momentum,
                       esr_stream_t stream);
int esr_momentum_catchup_rows2(float* table0, float* trace0, int32_t* last0, const int32_t* ids0, int modulus0,
                               float* table1, float* trace1, int32_t* last1, const int32_t* ids1, int modulus1, int D,
                               int64_t n, int step, float lr, float momentum, esr_stream_t stream);
int esr_sparse_momentum_step_multi(float* const* tables, float* const* traces, const int64_t* row_offsets, int ntables,
                                   int D, const int32_t* sorted_vids, const int32_t* perm, int64_t n, float* grad_rows,
                                   float lr, float momentum, esr_stream_t stream);
/* spotify/train_spotify.py:77-111 + 238-241 as ONE call (N1): catch-up of the playlist's rows (both tables, one launch),
 * esr_spotify_fwd_bwd, one sort of the virtual rows [album mod rows ; n_album_rows + artist], the whole momentum step on
 * the touched rows of both tables.  album_last / artist_last, step, lr, momentum as for esr_momentum_catchup_rows;
 * loss [1]. */
size_t esr_spotify_train_step_workspace_bytes(int n, int m, int o, int F);
int esr_spotify_train_step(float* album_table, float* album_trace, int32_t* album_last, int64_t n_album_rows,
                           float* artist_table, float* artist_trace, int32_t* artist_last, int64_t n_artists, int F,
                           const int32_t* album_ids, const int32_t* artist_ids, int n, int m, int o, float regularization,
                           int step, float lr, float momentum, float* loss, void* workspace, size_t workspace_bytes,
                           esr_stream_t stream);
/* sample_negative (train_spotify.py:139-150) on the device: the o negatives of global step `step` >= 1 are a function
 * of (seed, step) alone.  Negative i takes word i & 3 of Philox4x32-10 (Random123) with counter (i >> 2, step, 0, 0) and
 * key (seed & 0xffffffff, seed >> 32); its track index is (word * (T - 1)) >> 32 -- like the reference, the last track is
 * never drawn; multiply-high is biased by at most (T - 1) / 2^32 relative (5.3e-4 at the reference's 2 262 292 tracks).
 * neg_index / neg_album / neg_artist [o] (each may be NULL, not all): the index, all_albums[index], all_artists[index].
 * 2 <= T <= 2^31, 1 <= o <= 2^24.  One launch, no workspace. */
int esr_spotify_sample_negatives(const int32_t* all_albums, const int32_t* all_artists, int64_t T, uint64_t seed, int step,
                                 int o, int32_t* neg_index, int32_t* neg_album, int32_t* neg_artist, esr_stream_t stream);
/* K train steps in ONE call (the loop of train_spotify.py:255-259 over a group of playlists): one launch draws the
 * negatives of steps first_step .. first_step + K - 1 (as esr_spotify_sample_negatives) and assembles every step's id
 * lists, then each step j runs exactly the launch sequence of esr_spotify_train_step with shape (n, m_j, o) and
 * step = first_step + j, and writes losses[j].  Never synchronises, never allocates.
 * ctx_album / ctx_artist: device int32 [K * n]; next_album / next_artist: device int32, the K next lists packed;
 * next_offsets: HOST int64 [K + 1] (next_offsets[0] = 0, list j = [next_offsets[j], next_offsets[j + 1]), m_j >= 1) and
 * next_offsets_dev: the same K + 1 values in device memory (the caller uploads them, e.g. with the id lists: the call
 * copies nothing from the host); neg_index: device int32 [K * o] or NULL.  K (n + o) + next_offsets[K] <= 2^24.
 * The workspace begins with the assembled lists, int32: step j's block [album ids R_j][artist ids R_j] (context, next,
 * neg; R_j = n + m_j + o) starts at int  roundup(2 (j (n + o) + next_offsets[j]), 64) + 64 j,  i.e. 256-byte aligned.
 * Workspace query: max_m = the longest next list, total_next = next_offsets[K]. */
size_t esr_spotify_train_steps_workspace_bytes(int n, int max_m, int o, int F, int K, int64_t total_next);
int esr_spotify_train_steps(float* album_table, float* album_trace, int32_t* album_last, int64_t n_album_rows,
                            float* artist_table, float* artist_trace, int32_t* artist_last, int64_t n_artists, int F,
                            int n, int o, int K, const int32_t* ctx_album, const int32_t* ctx_artist,
                            const int32_t* next_album, const int32_t* next_artist, const int64_t* next_offsets,
                            const int64_t* next_offsets_dev, const int32_t* all_albums, const int32_t* all_artists,
                            int64_t T, uint64_t seed, int first_step, float regularization, float lr, float momentum,
                            float* losses, int32_t* neg_index, void* workspace, size_t workspace_bytes,
                            esr_stream_t stream);

/* ---- 8e: row-shard routing (owner = id mod world, local row = id div world) ---------------
 * Stable bucket of ids by owner: local_rows[k] = ids[perm[k]] / world, counts[g] = #ids owned by g
 * (int64, device); inverse (optional, may be NULL): inverse[perm[k]] = k, the bucket position of occurrence i.
 * Build-defined; the reference is single-device. */
size_t esr_bucket_workspace_bytes(int64_t n);
int esr_bucket_ids_by_owner(const int32_t* ids, int64_t n, int world, int32_t* local_rows,
                            int32_t* perm, int32_t* inverse, int64_t* counts, void* workspace,
                            size_t workspace_bytes, esr_stream_t stream);
/* The same bucket over a list given as up to four segments [ids_k + offsets[k]] (the lookups of one step as virtual
 * rows of the concatenated tables), read in place; perm / inverse index the concatenation.  ids / seg_counts /
 * offsets are host arrays as in esr_concat_offset_ids; workspace query with n = the sum of the counts. */
int esr_bucket_ids_by_owner_multi(const int32_t* const* ids, const int64_t* seg_counts, const int64_t* offsets,
                                  int nseg, int world, int32_t* local_rows, int32_t* perm, int32_t* inverse,
                                  int64_t* counts, void* workspace, size_t workspace_bytes, esr_stream_t stream);
/* The lists of `nbatch` (<= 8) coming batches bucketed in ONE launch pair (row-sharded loops make the routing plans of
 * several batches at once: esrecsys_amd/sharded.py begin_plans).  ids[b * nseg + k] = segment k of list b; seg_counts /
 * offsets are common to the lists (n = their sum); local_rows / perm / inverse are [nbatch][n], counts [nbatch][world]:
 * list b exactly what esr_bucket_ids_by_owner_multi gives for it. */
size_t esr_bucket_batched_workspace_bytes(int64_t n, int nbatch);
int esr_bucket_ids_by_owner_batched(const int32_t* const* ids, const int64_t* seg_counts, const int64_t* offsets,
                                    int nseg, int nbatch, int world, int32_t* local_rows, int32_t* perm,
                                    int32_t* inverse, int64_t* counts, void* workspace, size_t workspace_bytes,
                                    esr_stream_t stream);
/* The same routing with every DISTINCT row asked for once (esr_shard.hip): the occurrence list given as segments (as
 * esr_bucket_ids_by_owner_multi) -> ulocal [<= n]: the distinct local rows, owner-major and ascending inside an owner
 * (slice o, ucounts[o] entries, is what this rank asks of owner o and the order the rows come back in); ucounts [world]
 * (int64, device); uidx [n]: occurrence i reads row uidx[i] of the rows that came back; sorted_uidx / perm [n]: the
 * occurrences grouped by distinct row (sorted_uidx ascending; perm[p] = the occurrence) for esr_segment_sum_rows.
 * local_rows = the owner-local row space (max over owners of virtual rows div world, e.g. ceil(total / world)).
 * Owners need nothing new: they serve the list they are sent and segment-reduce what comes back by row. */
size_t esr_unique_by_owner_workspace_bytes(int64_t n);
int esr_unique_by_owner(const int32_t* const* ids, const int64_t* seg_counts, const int64_t* offsets, int nseg, int world,
                        int64_t local_rows, int32_t* ulocal, int32_t* uidx, int32_t* sorted_uidx, int32_t* perm,
                        int64_t* ucounts, void* workspace, size_t workspace_bytes, esr_stream_t stream);
/* The plan phase of the overlapped row-sharded loop (esrecsys_amd/sharded.py begin_stale_sets), batched over nlists lists:
 * esr_sorted_membership: flags[l][j] = 1 iff cur[l][j] != sentinel and it occurs in the ascending list seq[l][0 .. m)
 *   (cur int32 [nlists][n], seq int32 [nlists][m], flags uint8 [nlists][n]).
 * esr_flagged_first: out[l][0 .. c_l) = the flagged entries of values[l] (values NULL: their positions) in order -- a
 *   stable partition, only the flagged prefix is written -- and counts[l * counts_stride_list + g * counts_stride_slice]
 *   = flagged entries inside the g-th of G consecutive slices of lengths slice_len[l][g] (int64 [nlists][G], device; G
 *   <= 64); the count words are zeroed by the call.  Workspace: esr_flagged_first_workspace_bytes. */
int esr_sorted_membership(const int32_t* cur, int64_t n, const int32_t* seq, int64_t m, int nlists, int32_t sentinel,
                          uint8_t* flags, esr_stream_t stream);
size_t esr_flagged_first_workspace_bytes(int64_t n, int nlists);
int esr_flagged_first(const uint8_t* flags, const int32_t* values, int64_t n, int nlists, const int64_t* slice_len, int G,
                      int32_t* out, int64_t* counts, int64_t counts_stride_list, int64_t counts_stride_slice,
                      void* workspace, size_t workspace_bytes, esr_stream_t stream);
/* out[perm[k], :] = rows[k, :]  (undo the bucket order for rows that came back). */
int esr_unpermute_rows(const void* rows, int dtype, int D, const int32_t* perm, int64_t n, void* out,
                       esr_stream_t stream);

/* out[perm[k], :] = (float) rows_bf16[k, :] (perm == NULL: identity).  Requester side of a sharded lookup on a
 * bf16 table (BASELINE config 4): rows cross xGMI as bf16, the loss kernels consume f32.  D % 4 == 0. */
int esr_unpermute_rows_bf16_to_f32(const void* rows_bf16, int D, const int32_t* perm, int64_t n, float* out,
                                   esr_stream_t stream);

/* ---- 8e: the exchange itself -- all-to-all(v) of ids / rows / gradient rows over RCCL (xGMI) -------------------
 * Build-defined (the reference is single-device).  RCCL is bound at run time with dlopen: the library
 * has no link-time dependency on it.  An exchange is ncclGroupStart ; per peer ncclSend + ncclRecv ; ncclGroupEnd
 * enqueued on `stream`, i.e. in stream order with the kernels around it (no internal stream, no hand-over events);
 * on the xGMI full mesh every peer slice rides its own direct link.
 *   esr_comm_load       host: bind librccl (path NULL/"" = the librccl.so.1 already loaded in the process, else the
 *                       loader path).  Optional: the other entry points call it with NULL on first use.
 *   esr_comm_unique_id  host: 128 bytes of ncclUniqueId (rank 0 calls it and hands the bytes to every rank).
 *   esr_comm_init       COLLECTIVE over the `world` ranks, on the calling thread's current HIP device.
 *   esr_comm_count      host out-params: what RCCL itself reports for this communicator.
 *   esr_comm_async_error  ESR_OK or ESR_ELAUNCH when RCCL has recorded an asynchronous failure.
 *   esr_comm_abort / esr_comm_destroy  free the communicator (abort also terminates enqueued operations).
 * send_counts / recv_counts are HOST int64 [world] arrays: slice p of the send buffer (send_counts[p] ids / rows)
 * goes to peer p, slice p of the receive buffer comes from peer p.  Arguments are validated before the group opens
 * and the group is always closed, so a failing call never leaves peers inside an open group. */
typedef void* esr_comm_t;
int esr_comm_load(const char* librccl_path);
int esr_comm_unique_id(void* uid128);
int esr_comm_init(const void* uid128, int world, int rank, esr_comm_t* comm);
int esr_comm_count(esr_comm_t comm, int* world, int* rank);
int esr_comm_async_error(esr_comm_t comm);
int esr_comm_abort(esr_comm_t comm);
int esr_comm_destroy(esr_comm_t comm);
int esr_alltoall_bytes(esr_comm_t comm, const void* send, const int64_t* send_bytes, void* recv,
                       const int64_t* recv_bytes, esr_stream_t stream);
/* n_ops all-to-all(v)s as ONE RCCL group: operation o sends slice p of send[o] (send_bytes[o * world + p] bytes, host
 * arrays) to peer p and receives slice p of recv[o] from it.  The ids exchanges of a group of routing plans. */
int esr_alltoall_bytes_multi(esr_comm_t comm, int n_ops, const void* const* send, const int64_t* send_bytes,
                             void* const* recv, const int64_t* recv_bytes, esr_stream_t stream);
/* All-gather of equal blocks: block r of `recv` (world x bytes) = rank r's `send` (bytes).  The replicated-table mode
 * gathers every rank's ids and gradient rows with it; the sharded retrieval its queries. */
int esr_allgather_bytes(esr_comm_t comm, const void* send, int64_t bytes, void* recv, esr_stream_t stream);
/* int32 virtual local rows -> their owners (step 2 of SURVEY 8e). */
int esr_alltoall_ids(esr_comm_t comm, const int32_t* send_ids, const int64_t* send_counts, int32_t* recv_ids,
                     const int64_t* recv_counts, esr_stream_t stream);
/* looked-up rows [n, D] in the table dtype, owners -> requesters (step 3). */
int esr_alltoall_rows(esr_comm_t comm, const void* send_rows, int dtype, int D, const int64_t* send_counts,
                      void* recv_rows, const int64_t* recv_counts, esr_stream_t stream);
/* fp32 gradient rows [n, D], requesters -> owners (step 5). */
int esr_alltoall_grads(esr_comm_t comm, const float* send_grads, int D, const int64_t* send_counts,
                       float* recv_grads, const int64_t* recv_counts, esr_stream_t stream);

/* ---- a row-sharded step's exchange halves as ONE call each (esr_shard_step.hip; the loss kernel sits between them) ----
 * The steps being sharded: pinterest/train_shop_the_look.py:93-109, wikipedia/train_cooccurence.py:71-101 (the reference
 * is single-device and has no counterpart).  Count arrays are host int64 [world], peer-major, as in esr_alltoall_*:
 *   asked_counts[p]  rows peer p asks of THIS rank (their virtual local rows: asked_rows, concatenated peer by peer)
 *   ask_counts[p]    rows this rank asks of peer p (the routing plan's send counts)
 * esr_sharded_lookup: gather asked_rows from this rank's shards (esr_gather_rows_multi) into `served`
 *   [sum asked_counts, D], exchange (esr_alltoall_rows) into `back` [sum ask_counts, D], both in the tables' dtype.
 * esr_sharded_update: unique plans (sorted_uidx / occ_perm of esr_unique_by_owner non-NULL): ONE summed row per distinct
 *   row (esr_segment_sum_rows into `summed` [sum ask_counts, D]; grad_rows [n_occ, D] may be overwritten), else grad_rows
 *   are already one row per exchanged row; rows to their owners (esr_alltoall_grads into recv_grads [sum asked_counts,
 *   D]); the owner's fused segment-reduce + Adagrad (esr_sparse_adagrad_scatter_multi) with the sort of asked_rows the
 *   plan phase made (owner_sorted / owner_perm).  grad_dtype ESR_BF16: the rows cross the exchange as bf16 (rounded to
 *   nearest-even after the per-row sum into send_bf16 [sum ask_counts, D], received into recv_raw, widened into
 *   recv_grads; element error <= 2^-9 relative; D % 8 == 0) -- SURVEY 8d's config-4 budget of bf16-sized gradients.
 * world == 1 (comm may be NULL): nothing is exchanged or copied -- the gather writes into `back`, the update reads the
 * asker's rows in place; served / recv_grads / send_bf16 / recv_raw are not touched. */
/* rows [n, D] f32 -> bf16, round to nearest even (NaN stays NaN); D % 8 == 0.  The narrowing half of the bf16 gradient
 * exchange (esr_unpermute_rows_bf16_to_f32 with perm = NULL is the widening half). */
int esr_rows_f32_to_bf16(const float* rows, int64_t n, int D, void* rows_bf16, esr_stream_t stream);
int esr_sharded_lookup(esr_comm_t comm, int world, const void* const* tables, const int64_t* row_offsets, int ntables,
                       int dtype, int D, const int32_t* asked_rows, const int64_t* asked_counts,
                       const int64_t* ask_counts, void* served, void* back, esr_stream_t stream);
int esr_sharded_update(esr_comm_t comm, int world, void* const* tables, float* const* accums,
                       const int64_t* row_offsets, int ntables, int dtype, int D, float* grad_rows, int64_t n_occ,
                       const int32_t* sorted_uidx, const int32_t* occ_perm, float* summed, const int64_t* ask_counts,
                       const int64_t* asked_counts, int grad_dtype, void* send_bf16, void* recv_raw, float* recv_grads,
                       const int32_t* owner_sorted, const int32_t* owner_perm, float lr, float eps, int long_runs,
                       esr_stream_t stream);

/* ---- a whole row-sharded step -- lookup, loss kernel, update -- as ONE call (esr_shard_step.hip) -----------------------
 * A group = the same-width tables a step looks up and updates together, as this rank holds them (host struct of host
 * arrays of device pointers); a routing plan = what esrecsys_amd/sharded.py's plan phase made for one batch: */
typedef struct {
  esr_comm_t comm;              /* esr_comm_init's communicator; may be NULL at world 1 */
  int world;
  void* const* tables;          /* [ntables] this rank's shards */
  float* const* accums;         /* [ntables] their Adagrad accumulators */
  const int64_t* row_offsets;   /* [ntables + 1] virtual LOCAL row boundaries of the concatenated shards */
  int ntables;
  int dtype;                    /* ESR_F32 / ESR_BF16 (whole steps: ESR_F32) */
  int D;
  int grad_dtype;               /* ESR_F32, or ESR_BF16: gradient rows cross the exchange as bf16 (esr_sharded_update) */
} esr_shard_group_t;
typedef struct {
  const int32_t* asked_rows;    /* device [sum asked_counts]: virtual local rows the peers ask of this rank */
  const int64_t* asked_counts;  /* host [world] */
  const int64_t* ask_counts;    /* host [world]: rows this rank asks of each peer */
  const int32_t* index;         /* device [occurrences]: occurrence i reads row index[i] of the rows that come back */
  const int32_t* sorted_uidx;   /* device [occurrences] -- esr_unique_by_owner's grouping of the occurrences by distinct */
  const int32_t* occ_perm;      /*   row; both NULL for a per-occurrence plan (index = the inverse bucket permutation) */
  const int32_t* owner_sorted;  /* device [sum asked_counts]: esr_segment_sort_ids of asked_rows ... */
  const int32_t* owner_perm;    /*   ... and its permutation, for the owner-side update */
  int long_runs;                /* esr_sparse_adagrad_scatter_multi's hint (-1: unknown) */
} esr_routing_plan_t;
/* esr_sharded_triplet_step: the reference triplet loss (pinterest/train_shop_the_look.py:93-109) on row-sharded towers
 * (group = [scene table, product table]; occurrences = [scene ; pos ; neg] ids, 3 B of them): esr_sharded_lookup ->
 * esr_triplet_fwd_bwd on the rows where they landed -> esr_sharded_update.  loss [1] = this rank's share (a sum over
 * triplets / batch_size: all-reduce for the global value).
 * esr_sharded_glove_step: wikipedia/train_cooccurence.py:71-101 on a row-sharded embedding table and its [V, 1] bias table
 * (two single-table groups, ONE plan: same ids, same sharding; occurrences = inputs [2, B] flattened): both lookups ->
 * esr_glove_fwd_bwd -> both updates.  The loss is over the local batch.
 * Workspace: caller-owned, 256-byte aligned, at least the *_workspace_bytes of the SAME group(s), plan and B. */
size_t esr_sharded_triplet_step_workspace_bytes(const esr_shard_group_t* towers, const esr_routing_plan_t* plan,
                                                int64_t B);
int esr_sharded_triplet_step(const esr_shard_group_t* towers, const esr_routing_plan_t* plan, int64_t B,
                             float regularization, float batch_size, float lr, float eps, float* loss, void* workspace,
                             size_t workspace_bytes, esr_stream_t stream);
size_t esr_sharded_glove_step_workspace_bytes(const esr_shard_group_t* emb, const esr_shard_group_t* bias,
                                              const esr_routing_plan_t* plan, int64_t B);
int esr_sharded_glove_step(const esr_shard_group_t* emb, const esr_shard_group_t* bias, const esr_routing_plan_t* plan,
                           const float* target, int64_t B, int mode, float lr, float eps, float* loss, void* workspace,
                           size_t workspace_bytes, esr_stream_t stream);

/* ---- the same steps with the NEXT batch's lookup overlapped (build-defined) ---------------------------------
 * A training loop knows its coming batches (the plans are made a group ahead), so batch k + 1's gather + rows exchange
 * need not wait for batch k: call k issues them on `side` with the second communicator `comm2` right after batch k's own
 * rows are in place -- they run under batch k's loss kernel, gradient exchange and update -- and call k + 1 receives the
 * buffers as `back`.  Rows that batch k's update writes were fetched too early; which ones is a function of the ids alone
 * (owner side: the rows of batch k + 1's asked list that are in batch k's; esrecsys_amd/sharded.py begin_stale_sets),
 * and call k + 1 serves exactly those again on the main stream before its loss kernel: gather stale_rows -> rows
 * exchange (first communicator; counts stale_asked / stale_ask) -> scatter to rows stale_pos of `back`.  The results
 * equal the plain steps' bit for bit (tests/test_gpu_sharded.py, tests/test_sharded_gloo.py).
 * One struct per call; `ready` / `next_ready` hand the side stream's completion event from call to call (the consumer
 * releases it; esr_sharded_overlap_release for one that is never consumed).  Buffers in next_back / next_served belong to
 * the caller and must stay untouched until the call that takes them as `back` has been issued. */
typedef struct {
  void* back[2];                /* in: THIS batch's rows per group (GloVe: embedding, bias) = the previous call's next_back;
                                   NULL: look them up in line (first step of a loop) */
  void* ready;                  /* in: the previous call's next_ready (waited for on `stream`, then released), or NULL */
  const int32_t* stale_rows;    /* device [sum stale_asked]: virtual local rows this rank serves again, asker by asker */
  const int64_t* stale_asked;   /* host [world] */
  const int32_t* stale_pos;     /* device [sum stale_ask]: the rows of `back` that come again, owner by owner */
  const int64_t* stale_ask;     /* host [world] */
  const esr_routing_plan_t* next_plan; /* the NEXT batch's plan, or NULL (last step) */
  void* next_back[2];           /* per group: [sum next ask_counts, D], filled on `side` */
  void* next_served[2];         /* per group: scratch [sum next asked_counts, D] (world > 1) */
  esr_comm_t comm2;             /* a second esr_comm_init communicator over the same ranks (may be NULL at world 1) */
  esr_stream_t side;            /* the stream the next lookup runs on */
  void* next_ready;             /* out: recorded on `side` behind the next lookup (NULL when next_plan is NULL) */
} esr_step_overlap_t;
/* extra workspace of ONE group for its stale rows (add it to the step's *_workspace_bytes for every group of the step) */
size_t esr_sharded_step_overlap_workspace_bytes(const esr_shard_group_t* group, const esr_step_overlap_t* overlap);
void esr_sharded_overlap_release(void* ready);
/* overlap == NULL: exactly esr_sharded_triplet_step / esr_sharded_glove_step */
int esr_sharded_triplet_step_overlapped(const esr_shard_group_t* towers, const esr_routing_plan_t* plan,
                                        esr_step_overlap_t* overlap, int64_t B, float regularization, float batch_size,
                                        float lr, float eps, float* loss, void* workspace, size_t workspace_bytes,
                                        esr_stream_t stream);
int esr_sharded_glove_step_overlapped(const esr_shard_group_t* emb, const esr_shard_group_t* bias,
                                      const esr_routing_plan_t* plan, esr_step_overlap_t* overlap, const float* target,
                                      int64_t B, int mode, float lr, float eps, float* loss, void* workspace,
                                      size_t workspace_bytes, esr_stream_t stream);

/* ---- GloVe co-occurrence matrix from token-id streams (esr_cooccur.hip; the reference's wikipedia/make_cooccurrence.py) ----
 * Position i of a document pairs with j in [max(0, i - W), min(n, i + W)) and adds 1 / |i - j| to the entry
 * (index = t[i], other = t[j]) when t[i] > t[j]; nothing crosses a document boundary.  Sums are kept in fixed point
 * (units of 1 / lcm(1 .. W), uint64), so they do not depend on the order of the atomics or on how the corpus is cut into
 * calls; 1 <= W <= 22.
 * The table is device memory of esr_cooccur_table_bytes(capacity) bytes, 16-byte aligned, capacity a power of two >= 2:
 * a 256-byte header -- uint64 word 0: occupied slots, word 1: failure bits (1: a probe wrapped the whole table, 2: a
 * negative token id, 4: doc_offsets[0] / doc_offsets[ndocs] outside [0, N], 8: finalize's nnz below the table's, 16:
 * esr_dice_accumulate met a document above esr_dice_max_doc()) --
 * then keys uint64[capacity] (index << 32 | other, all ones = empty) and sums uint64[capacity].  The caller reads the
 * header and must keep capacity >= occupied + (tok_end - tok_begin) * W before a call: a full table raises failure bit 1,
 * it never spins and never drops an increment silently.
 *   accumulate  the pairs whose LATER position lies in [tok_begin, tok_end) (any cut of [0, N) into such ranges gives
 *               the same table); tokens int32[N] >= 0, doc_offsets int64[ndocs + 1] in CSR form (device memory; empty
 *               documents allowed).
 *   rehash      new_table (initialised here) receives every occupied slot of table: same keys, same sums.
 *   finalize    nnz = the header's occupied count, num_ids > every id: (index, other, count) ascending by (index, other),
 *               count = (float)((double)sum / lcm(1 .. W)). */
size_t esr_cooccur_table_bytes(int64_t capacity);
int esr_cooccur_table_init(void* table, int64_t capacity, esr_stream_t stream);
int esr_cooccur_accumulate(const int32_t* tokens, int64_t N, const int64_t* doc_offsets, int64_t ndocs,
                           int64_t tok_begin, int64_t tok_end, int context_window, void* table, int64_t capacity,
                           esr_stream_t stream);
int esr_cooccur_rehash(const void* table, int64_t capacity, void* new_table, int64_t new_capacity,
                       esr_stream_t stream);
size_t esr_cooccur_finalize_workspace_bytes(int64_t nnz);
int esr_cooccur_finalize(void* table, int64_t capacity, int64_t nnz, int64_t num_ids, int context_window,
                         int32_t* index, int32_t* other, float* count, void* workspace, size_t workspace_bytes,
                         esr_stream_t stream);

/* ---- Set co-occurrence (Dice) matrix from id sets (esr_dice.hip; the reference's wikipedia/make_dice.py) ----
 * A document is the SET of indices[doc_offsets[d] .. doc_offsets[d + 1]); with u = its sorted distinct ids every i < j adds
 * 1 to the entry (index = u[i], other = u[j]) of an esr_cooccur_* pair table -- index < other, the opposite orientation to
 * the windowed matrix -- and every distinct id adds 1 to the diagonal key id << 32 | id, which no pair makes: the number
 * of documents that hold the id.  Counts are uint64: nothing depends on the order of the atomics or on how the documents
 * are cut into calls.  esr_cooccur_rehash grows the table; esr_cooccur_finalize with context_window = 1 returns pairs and
 * diagonal together, ascending by (index, other), count = (float)sum.
 *   accumulate  the documents [doc_begin, doc_end) of doc_offsets int64[ndocs + 1] (CSR over indices int32[N] >= 0, device
 *               memory; empty documents allowed), at most 2^31 - 1 of them.  The caller keeps capacity >= occupied +
 *               sum over those documents of n (n - 1) / 2 + n (n = the document's length).  A document longer than
 *               esr_dice_max_doc() (its sort lives in LDS) raises failure bit 16 and adds nothing: check lengths on the host.
 *               workspace: esr_dice_workspace_bytes(N) bytes, 16-byte aligned (the work list of the long documents). */
int esr_dice_max_doc(void);
size_t esr_dice_workspace_bytes(int64_t N);
int esr_dice_accumulate(const int32_t* indices, int64_t N, const int64_t* doc_offsets, int64_t ndocs,
                        int64_t doc_begin, int64_t doc_end, void* table, int64_t capacity, void* workspace,
                        size_t workspace_bytes, esr_stream_t stream);

/* ---- Term statistics, dictionary lookup and tf-idf documents from token-id streams (esr_terms.hip; the reference's
 * wikipedia/make_dictionary.py:67-117, token_dictionary.py:58-64, count_terms.py:32-74) ----
 * All tables are esr_cooccur_* pair tables (same header, same failure bits, grown by esr_cooccur_rehash); all counts uint64.
 *   accumulate   the tokens [tok_begin, tok_end) = the whole documents [doc_begin, doc_end) of doc_offsets int64[ndocs + 1]
 *                (both ranges given: the device's offsets must agree with the host's plan, else failure bit 4) add 1 to
 *                the SCRATCH key (document - doc_begin) << 32 | id, so its sum is the term frequency.  id = the raw token
 *                id, or with `lookup` (a table made by lookup_build) the value stored for it -- a raw id the lookup does
 *                not hold adds nothing.  The caller keeps scratch capacity >= 2 (tok_end - tok_begin).  A negative id
 *                raises failure bit 2.
 *   fold         every occupied scratch slot (document, id, tf) adds tf to key id << 32 | 0 and 1 to key id << 32 | 1 of
 *                `table`: frequency and document frequency.  The scratch table's failure bits are carried over.  The
 *                caller keeps capacity >= occupied + 2 x the scratch table's occupied count.
 *   stats        n_ids = occupied / 2: the ids of `table` with both sums, in slot order (sort with esr_segment_sort_ids).
 *                counter: 8 bytes of device memory, zeroed by the call.
 *   lookup_build table (initialised by esr_cooccur_table_init, capacity >= 2 K) receives key = keys[i], sum = values[i];
 *                the keys are distinct.
 *   lookup       mode 0: out[i] = the value of tokens[i], -1 when absent.  mode 1: out[i] = 1 + value, and when absent
 *                1 + size + bucket with bucket = oov_bucket[i] (or tokens[i] & 0xFFFF when oov_bucket is NULL).  fail: a
 *                uint64 device word the CALLER zeroes; bit 2 = a negative token, bit 32 = a bucket outside [0, 65536).
 *   tfidf_rows   index int32[nnz] = the dictionary indices of the scratch keys in (document, index) order (esr_cooccur_finalize
 *                with context_window = 1), row_off int32[nrows + 1] their rows (esr_run_offsets): tfidf[i] =
 *                float(tf idf[index] / sqrt(sum over the row of (tf idf)^2)), 0 where that sum is 0; tf is read back from
 *                the scratch table as uint64, the arithmetic is fp64, the row sum one wave's fixed-order reduction. */
int esr_terms_accumulate(const int32_t* tokens, int64_t N, const int64_t* doc_offsets, int64_t ndocs, int64_t doc_begin,
                         int64_t doc_end, int64_t tok_begin, int64_t tok_end, const void* lookup,
                         int64_t lookup_capacity, void* scratch, int64_t capacity, esr_stream_t stream);
int esr_terms_fold(const void* scratch, int64_t scratch_capacity, void* table, int64_t capacity, esr_stream_t stream);
int esr_terms_stats(void* table, int64_t capacity, int64_t n_ids, int32_t* ids, int64_t* frequency,
                    int64_t* doc_frequency, void* counter, esr_stream_t stream);
int esr_terms_lookup_build(const int32_t* keys, const int32_t* values, int64_t K, void* table, int64_t capacity,
                           esr_stream_t stream);
int esr_terms_lookup(const int32_t* tokens, int64_t N, const void* lookup, int64_t lookup_capacity, int mode,
                     int32_t size, const int32_t* oov_bucket, int32_t* out, void* fail, esr_stream_t stream);
int esr_terms_tfidf_rows(const void* scratch, int64_t capacity, const int32_t* index, const int32_t* row_off,
                         int64_t nrows, int64_t nnz, const double* idf, int64_t K, float* tfidf, esr_stream_t stream);

/* ---- Item-to-item neighbours and the item-kNN recommender (esr_neighbours.hip; the reference's wikipedia/dump_dice.py:33-51
 * ranks a row's partners by Dice score) ----
 * Entries index / other int32[nnz], count float[nnz] as esr_cooccur_finalize returns them without the diagonal (either
 * orientation, any order); ids int32[u] ascending and distinct, df float[u] their document frequencies (score 1 only).
 * Row r = item ids[r]: both = 0 the entries with index == ids[r] (partner = other), both = 1 those with index == ids[r] or
 * other == ids[r] (partner = the other end).  score 0: the joint count; score 1: count / (df[other] + df[index]), f32, no
 * factor 2.  Per row the k best by (score descending, partner id ascending) -- a total order, so the result does not depend
 * on atomic order or on the grid: out_neighbours int32[u, k] (-1 behind the row's end), out_scores / out_counts float[u, k]
 * (0 there), out_lengths int32[u] = min(k, row length).  1 <= k <= 1024, nnz < 2^30.  An entry with an end that ids lacks is
 * left out and raises bit 64 of the failure word = the first uint64 of the workspace (the caller reads it after the call).
 * workspace: esr_neighbours_workspace_bytes(nnz, u, both) bytes, 16-byte aligned.
 * esr_neighbours_plan_bounds: the row lengths at which the select changes class, ascending, into bounds[0 .. capacity);
 * returns their number (3): rows of at most bounds[0] entries share a wave four at a time, at most bounds[1] take a wave,
 * at most bounds[2] a workgroup's LDS, longer ones a radix select over global memory.
 *   recommend   the table is what esr_neighbours_topk wrote (table_ids = ids, width = its k).  Query q has the history
 *               history[offsets[q] .. offsets[q + 1]) (offsets int64[nq + 1] over history int32[N], device memory).  The score
 *               of candidate c = the f32 sum of table_scores[row(h_p), j] over the (p, j) with table_neighbours[row(h_p), j]
 *               == c, added left to right in ascending history position p; ids the table lacks add nothing; with
 *               exclude_history candidates that occur in the history are dropped.  out_ids int32[nq, k] (-1 padded),
 *               out_scores float[nq, k] (0 padded), out_lengths int32[nq]: the k best by (score descending, id ascending).
 *               A query may gather at most esr_itemknn_max_entries() = history length x width entries (one workgroup sorts
 *               them in LDS): the caller checks that; the kernel answers such a query with length -1, never truncated. */
size_t esr_neighbours_workspace_bytes(int64_t nnz, int64_t u, int both);
int esr_neighbours_plan_bounds(int32_t* bounds, int capacity);
int esr_neighbours_topk(const int32_t* index, const int32_t* other, const float* count, int64_t nnz, const int32_t* ids,
                        const float* df, int64_t u, int k, int both, int score, int32_t* out_neighbours,
                        float* out_scores, float* out_counts, int32_t* out_lengths, void* workspace,
                        size_t workspace_bytes, esr_stream_t stream);
int esr_itemknn_max_entries(void);
int esr_itemknn_recommend(const int32_t* table_ids, const int32_t* table_neighbours, const float* table_scores,
                          const int32_t* table_lengths, int64_t u, int width, const int32_t* history, int64_t N,
                          const int64_t* offsets, int64_t nq, int k, int exclude_history, int32_t* out_ids,
                          float* out_scores, int32_t* out_lengths, esr_stream_t stream);

/* ---- Ranking metrics of recommended lists against held-out truth sets (esr_eval.hip; the reference holds out all but the
 * first tracks of a playlist, spotify/make_training.py:74-98, and reports the recall of the next tracks among the 500 best,
 * train_spotify.py:113-131) ----
 * Query q: the list rec_ids[q * rec_pitch .. + width) (int32, -1 behind a row's end; rec_lengths int32[nq] or NULL = width
 * everywhere) against the truth ids truth[truth_offsets[q] .. truth_offsets[q + 1]) (int32[n] with int64[nq + 1] offsets, the
 * CSR layout of the builders).  All of these are device memory; ks is HOST memory -- int32[nk], 1 <= nk <= 8, strictly
 * ascending, ks[0] >= 1 -- because it is validated before the launch and travels with the kernel's arguments.
 * With kmax = min(ks[nk - 1], width): position r (0-based) < min(rec_lengths[q], kmax) is a HIT if its id is a truth id and
 * (count_repeats or no earlier position holds the same id).  c(k) = the hits at positions < k; walking the hits in ascending
 * 1-based rank r with c = the hits so far: ap_sum += (double)c / r, dcg += disc[r - 1].  n_rel = the DISTINCT truth ids of
 * the query (listed_size 0) or truth_offsets[q + 1] - truth_offsets[q] (listed_size 1).  Outputs, [nq, nk] unless stated:
 *   hits int32 = c(k);  first_hit int32[nq] = the 1-based rank of the first hit within kmax, 0 if none;
 *   precision = c / k;  recall = c / n_rel;  rr = 1 / first_hit if first_hit <= k else 0;
 *   ap = ap_sum / min(k, n_rel);  ndcg = dcg / cum_disc[min(k, n_rel)];  valid int32[nq] = (n_rel > 0).
 * Each float is that one fp64 expression rounded once to float; a query with n_rel == 0 gets zeros.  With count_repeats ap
 * and ndcg are not defined (hits may exceed n_rel): they are not written and may be NULL.
 * disc double[kmax]: disc[r - 1] = 1 / log2(r + 1); cum_disc double[kideal + 1] = [0, cumsum(disc)] continued to kideal =
 * min(ks[nk - 1], max_truth) -- the ideal DCG at a cutoff above the width still counts min(k, n_rel) items.  Both are made by
 * the caller in float64: the device evaluates no logarithm.
 * max_truth: the caller's bound on truth_offsets[q + 1] - truth_offsets[q]; it sizes the table in LDS.  A query may hold at
 * most esr_eval_max_truth() DISTINCT truth ids and width is at most esr_eval_max_width(): the caller checks both, nothing
 * is ever truncated.  fail: a uint64 device word, zeroed by the call; bit 2 = a negative truth id (left out), bit 4 = truth
 * offsets outside [0, n], falling or a set above max_truth (the query gets zeros), bit 8 = more distinct truth ids than the
 * table takes.  nq == 0 is a no-op. */
int esr_eval_max_truth(void);
int esr_eval_max_width(void);
int esr_eval_ranking(const int32_t* rec_ids, int64_t rec_pitch, int width, const int32_t* rec_lengths,
                     const int32_t* truth, int64_t n, const int64_t* truth_offsets, int64_t nq, int max_truth,
                     const int32_t* ks, int nk, const double* disc, const double* cum_disc, int count_repeats,
                     int listed_size, int32_t* hits, int32_t* first_hit, int32_t* valid, float* precision, float* recall,
                     float* rr, float* ap, float* ndcg, unsigned long long* fail, esr_stream_t stream);

/* ---- Explicit ratings: Pearson user similarity and the user-kNN affinity (esr_ratings.hip; the collaborative-filtering job
 * of the reference's book, chapter 5 "Data Processing": USim from the deviations of the co-rated items, Aff over the nearest
 * users) ----
 * The WIDE pair table: esr_usersim_table_bytes(capacity) bytes, 16-byte aligned, capacity a power of two >= 2 -- the
 * 256-byte header of the esr_cooccur_* table (word 0: occupied slots, word 1: failure bits), keys uint64[capacity]
 * (index << 32 | other, all ones = empty), then FOUR planes sums uint64[4][capacity]: n, P, Qa, Qb.  A slot is claimed once
 * by a compare-and-swap on its key; the four sums are integer atomic adds, so nothing depends on their order.  Failure bits
 * as there, and 128: the users of an item are not strictly ascending (a (user, item) given twice).
 *   accumulate  ratings as CSR by item: item r of [item_begin, item_end) has the raters users[item_offsets[r] ..
 *               item_offsets[r + 1]) (int32 >= 0, strictly ascending) with the fixed-point deviations dev (int32) and the id
 *               item_ids[r] (only screened: a negative one raises bit 2).  Every p < q of an item adds n += 1, P += dev_p
 *               dev_q (two's complement), Qa += dev_p^2, Qb += dev_q^2 to the key users[p] << 32 | users[q].  The work unit is
 *               a T x T tile of an item's triangle, T = esr_usersim_tile(): with C = ceil(n / T) an item of n >= 2 raters
 *               has C (C + 1) / 2 tiles, an item below two raters none; tile_prefix int64[nitems + 1] is the exclusive
 *               prefix of those counts over ALL items (made by the caller, device memory) and ntiles =
 *               tile_prefix[item_end] - tile_prefix[item_begin] (a prefix that disagrees raises bit 4 and adds nothing).
 *               The caller keeps capacity >= occupied + sum over the range of n (n - 1) / 2, and m^2 * (items in all
 *               calls) < 2^53 with m = the largest |dev|, so that every sum is exact in a double.
 *   rehash      new_table (initialised here) receives every occupied slot with its four sums, and the failure word.
 *   finalize    nnz = the header's occupied count, num_ids > every user id.  Per entry sim = float(double(P) /
 *               (sqrt(double(Qa)) * sqrt(double(Qb)))), each fp64 operation rounded once; entries with Qa == 0 or Qb == 0
 *               (counted in counts[1]), with n < min_overlap, or -- has_min_similarity -- with sim <= min_similarity are
 *               dropped.  The kept rows go to index / other / sim / overlap [nnz] ascending by (index, other), index <
 *               other; counts int64[2] (device) = {rows kept, entries dropped as flat}.
 *               workspace: esr_usersim_finalize_workspace_bytes(nnz) bytes, 16-byte aligned.
 * User-kNN over a neighbour table made by esr_neighbours_topk from (index, other, sim) with score 0 (table_ids, width = its
 * k) and the ratings as CSR by user: users int32[nu] ascending, row_offsets int64[nu + 1] over items int32[R] (ascending and
 * distinct inside a row) and ratings float[R]; mean double[nu] the users' mean ratings.  For the query user A with table row
 * (U_j, s_j), j < length, the columns COUNTED for item i are those whose U_j rated i, taken in ascending j:
 *   num = sum s_j (double(r[U_j, i]) - c_j), c_j = mean[A] (center 0) or mean[U_j] (center 1);
 *   den = sum |s_j| over the counted columns (denominator 0) or sum s_j over the whole row (denominator 1);
 *   affinity = float(mean[A] + num / den), or float(mean[A]) when no column counts or den == 0; -0 is written as +0.
 * All of it fp64, each operation rounded once.  support = the number of counted columns.
 *   predict     (query_users[q], query_items[q]) -> out_affinity float[nq], out_support int32[nq]; a user that table_ids or
 *               users lacks gets (NaN, 0).
 *   recommend   per query user the k best items among those its neighbours rated -- without the user's own with
 *               exclude_rated, without those of support < min_support -- by (affinity descending, item ascending): out_ids
 *               int32[nq, k] (-1 padded), out_scores float[nq, k] (0 padded), out_lengths int32[nq].  The affinity is
 *               predict's bit for bit.  A query gathers the sum of its neighbours' row lengths, at most
 *               esr_userknn_max_entries() (one workgroup sorts them in LDS): the caller checks that; the kernel answers
 *               such a query with length -1, never truncated.  A user the table lacks gets length 0. */
int esr_usersim_tile(void);
size_t esr_usersim_table_bytes(int64_t capacity);
int esr_usersim_table_init(void* table, int64_t capacity, esr_stream_t stream);
int esr_usersim_rehash(const void* table, int64_t capacity, void* new_table, int64_t new_capacity, esr_stream_t stream);
int esr_usersim_accumulate(const int32_t* users, const int32_t* dev, int64_t N, const int64_t* item_offsets,
                           const int32_t* item_ids, const int64_t* tile_prefix, int64_t nitems, int64_t item_begin,
                           int64_t item_end, int64_t ntiles, void* table, int64_t capacity, esr_stream_t stream);
size_t esr_usersim_finalize_workspace_bytes(int64_t nnz);
int esr_usersim_finalize(void* table, int64_t capacity, int64_t nnz, int64_t num_ids, int min_overlap,
                         int has_min_similarity, float min_similarity, int32_t* index, int32_t* other, float* sim,
                         int32_t* overlap, int64_t* counts, void* workspace, size_t workspace_bytes,
                         esr_stream_t stream);
int esr_userknn_max_entries(void);
int esr_userknn_predict(const int32_t* table_ids, const int32_t* table_neighbours, const float* table_scores,
                        const int32_t* table_lengths, int64_t u, int width, const int32_t* users, int64_t nu,
                        const int64_t* row_offsets, const int32_t* items, const float* ratings, int64_t R,
                        const double* mean, const int32_t* query_users, const int32_t* query_items, int64_t nq,
                        int center, int denominator, float* out_affinity, int32_t* out_support, esr_stream_t stream);
int esr_userknn_recommend(const int32_t* table_ids, const int32_t* table_neighbours, const float* table_scores,
                          const int32_t* table_lengths, int64_t u, int width, const int32_t* users, int64_t nu,
                          const int64_t* row_offsets, const int32_t* items, const float* ratings, int64_t R,
                          const double* mean, const int32_t* query_users, int64_t nq, int k, int exclude_rated,
                          int min_support, int center, int denominator, int32_t* out_ids, float* out_scores,
                          int32_t* out_lengths, esr_stream_t stream);

/* ---- Matrix factorisation of explicit ratings by alternating least squares (esr_als.hip) ----
 * The model is r[u, i] ~ c[u] + x_u . y_i over factor tables float[n, rank], rank in [1, the max-rank query] (64).
 *   geometry    chunk (even, >= 2): the ratings of a row are taken in CSR order and cut into chunks of that many;
 *               chunks_per_workgroup: rows up to one chunk are solved by a wave, rows up to chunk * chunks_per_workgroup by
 *               a workgroup, longer rows through partials in the workspace and a second launch.
 *   solve_rows  one half-sweep over the rows [row_begin, row_end) of one side.  row_offsets int64[row_end + 1] is HOST
 *               memory (ascending, >= 0): the call sorts the rows into the three classes from it; cols int32 (positions into
 *               other_factors float[n_other, rank]) and targets float are device memory of row_offsets[row_end] entries.
 *               Row r with n ratings (c_k, d_k) gets the solution of
 *                   (sum_k y_k y_k^T + lam I) x = sum_k d_k y_k,  y_k = other_factors[c_k],  lam = reg * (weighted ? n : 1)
 *               in out_factors[r], a row without ratings the zero vector.  Order: per chunk the Gram entries are the
 *               k-ordered f32 fmaf chain from 0 of v_mfma_f32_32x32x2_f32, the right-hand side is the chain over the even
 *               ratings plus the chain over the odd ones; chunk partials are added in ascending chunk order in f32; then lam
 *               on the diagonal, an f32 Cholesky and two triangular solves.  The output row depends on its own ratings,
 *               other_factors, reg and weighted only -- not on the row range, the grid or the other rows.  No floating-point
 *               atomics.  failed (int32 word, device, zeroed by the caller): bit 30 is set by a column outside [0, n_other)
 *               (never dereferenced; its rating counts as absent), and 1 is added per row whose pivot is not finite and
 *               positive or whose solution is not finite -- that output row stays as it was.  out_factors must not overlap
 *               other_factors.  workspace: the workspace-bytes query of (row_end - row_begin, the ratings of the range,
 *               rank), 16-byte aligned; the call waits for the stream once (its row lists are copied from host memory).
 *   predict     out[q] = float(offset[u] + sum_d double(x_u[d]) * double(y_i[d])), the sum in fp64 in ascending d from 0,
 *               u = user_pos[q], i = item_pos[q] (positions; NaN where either is outside its table); offset double[nu] or
 *               null (0).  With targets float[nq] (residual mode): out[q] = float(double(targets[q]) - that value).
 *               predict is a per-pair loop that needs no rank x rank matrix: it takes rank in [1, the predict-max-rank
 *               query] (128, the widest row of the float4 row-group models), above what the solves and the Gram take. */
int esr_als_max_rank(void);
int esr_als_predict_max_rank(void);
int esr_als_geometry(int* chunk, int* chunks_per_workgroup);
size_t esr_als_solve_workspace_bytes(int64_t n_rows, int64_t nnz, int rank);
int esr_als_solve_rows(const float* other_factors, int64_t n_other, int rank, const int64_t* row_offsets, const int32_t* cols,
                       const float* targets, int64_t row_begin, int64_t row_end, float reg, int weighted, float* out_factors,
                       int32_t* failed, void* workspace, size_t workspace_bytes, esr_stream_t stream);
int esr_als_predict(const float* user_factors, int64_t nu, const float* item_factors, int64_t ni, int rank,
                    const int32_t* user_pos, const int32_t* item_pos, const double* offset, const float* targets, int64_t nq,
                    float* out, esr_stream_t stream);

/* ---- Implicit-feedback ALS (Hu, Koren, Volinsky 2008; esr_als.hip) ----
 * Every (row, column) cell is fitted: preference 1 on a row's entries and 0 elsewhere, confidence 1 + w_k on the entries and 1
 * elsewhere.  A row with n entries solves (G + sum_k w_k y_k y_k^T + lam I) x = sum_k c_k y_k, G = Y^T Y of the other side's
 * whole table, c_k = float(1 + w_k), lam = reg * (weighted ? n : 1).
 *   gram        out_gram float[rank, rank] = factors^T factors of a float table [n, rank]: the full symmetric matrix (the upper
 *               triangle holds the bits of the lower).  The table is cut into segments of `segment` consecutive rows (the
 *               geometry query); a segment's entry is ONE k-ordered f32 fmaf chain from 0 (v_mfma_f32_32x32x2_f32, both operands
 *               the same register), the segment partials are added per entry in fp64 in ascending segment order and rounded
 *               once.  A function of the table alone: not of the grid, not of trailing all-zero rows; n = 0 gives zeros.  No
 *               floating-point atomics.  workspace: the gram workspace-bytes query of (n, rank), 16-byte aligned.
 *   solve_rows_implicit   the arguments of solve_rows with weights float[nnz] (w_k >= 0) in the place of targets and gram (device,
 *               float[rank, rank], what gram wrote for other_factors).  Order: the entries in CSR order in chunks of the
 *               geometry's chunk; within a chunk the lower-triangle entry (i, j), i >= j, is the k-ordered chain
 *               acc = fmaf(float(w_k * y_k[i]), y_k[j], acc) from 0 and the right-hand side is fmaf(c_k, y_k[d], acc) over the
 *               chunk's even entries plus the same chain over its odd ones; chunk partials are added in ascending order in f32;
 *               then G[i][j] is added; then lam on the diagonal; then the Cholesky and the two solves of solve_rows.  The same
 *               three row classes and the same workspace query.  A row without entries gets the zero vector.  failed: bit 30
 *               and the count as solve_rows; a weight that is negative or not finite counts as absent and sets bit 29.
 *               out_factors must overlap neither other_factors nor gram. */
int esr_als_gram_geometry(int* segment);
size_t esr_als_gram_workspace_bytes(int64_t n, int rank);
int esr_als_gram(const float* factors, int64_t n, int rank, float* out_gram, void* workspace, size_t workspace_bytes,
                 esr_stream_t stream);
int esr_als_solve_rows_implicit(const float* other_factors, int64_t n_other, int rank, const float* gram,
                                const int64_t* row_offsets, const int32_t* cols, const float* weights, int64_t row_begin,
                                int64_t row_end, float reg, int weighted, float* out_factors, int32_t* failed, void* workspace,
                                size_t workspace_bytes, esr_stream_t stream);

/* ---- Bayesian Personalised Ranking (Rendle et al., UAI 2009; esr_bpr.hip) ----
 * -log sigmoid(x_u . y_i - x_u . y_j) over sampled (user, seen item, unseen item) triples.  No workspace.
 *   geometry    max_tries = the negative candidates tried per triple (15); the fwd_bwd kernel takes D that is a multiple of
 *               rank_multiple (4) and at most max_rank (128).
 *   sample      K steps of B triples in one launch, outputs int32 [K, B] row-major, row k = global step step0 + k (mod
 *               2^32).  The seen pairs are a CSR by user: row_offsets int64[nu + 1], row_upos / row_ipos int32[nnz], item
 *               positions ascending within a row, pairs distinct.  The rule is esr_bpr_sample.h's bpr_sample_triple: Philox
 *               block b = philox4x32_10((t, s, b, 0), (seed low, seed high)); word 0 of block 0 picks the pair by
 *               multiply-high; the next 15 words are the negative candidates in order, the first one not in the user's row
 *               (binary search) wins; if all are seen the last one is written with valid = 0.  A triple is a function of
 *               (seed, s, t, the CSR) alone.  dropped int32[K] = the exact count of valid == 0 per step (zeroed by the call;
 *               integer atomics).  1 <= nnz, ni, nu, K, B <= 2^31 - 1.
 *   fwd_bwd     per triple t with x = user_table[u[t]], yi = item_table[i[t]], yj = item_table[j[t]] (f32 tables):
 *               d = sum_k x[k] (yi[k] - yj[k]) in f32 in the order esr_bpr.hip states (a function of D alone),
 *               loss_t[t] = max(-d, 0) + log1pf(expf(-|d|)), diff_t[t] = d (diff_t may be null), g = sigmoid(-d), and into
 *               grads float[3 B, D] = [user rows ; positive rows ; negative rows] in occurrence order
 *                 g_u = -g (yi - yj) + reg x,  g_i = -g x + reg yi,  g_j = g x + reg yj.
 *               grads null: forward only.  valid int32[B] or null (all valid): a triple with valid = 0 writes three zero
 *               rows, loss_t = 0 and diff_t = 0 and reads no row.  A u, i or j outside its table does the same and sets bit
 *               30 of *failed (the caller zeroes and reads it).  No reduction across triples: an output depends on its own
 *               triple, reg and D only.  Tables and grads 16-byte aligned. */
int esr_bpr_geometry(int* max_tries, int* max_rank, int* rank_multiple);
int esr_bpr_sample(const int64_t* row_offsets, const int32_t* row_upos, const int32_t* row_ipos, int64_t nu, int64_t ni,
                   int64_t nnz, uint64_t seed, uint32_t step0, int64_t K, int64_t B, int32_t* out_u, int32_t* out_i,
                   int32_t* out_j, int32_t* out_valid, int32_t* dropped, esr_stream_t stream);
int esr_bpr_fwd_bwd(const float* user_table, int64_t nu, const float* item_table, int64_t ni, int D, const int32_t* u,
                    const int32_t* i, const int32_t* j, const int32_t* valid, int64_t B, float reg, float* loss_t,
                    float* diff_t, float* grads, int32_t* failed, esr_stream_t stream);

/* ---- WARP (Weston, Bengio, Usunier, IJCAI 2011; esr_warp.hip) ----
 * The rank-weighted margin loss over (user, seen item, violating unseen item) triples: one fused call that samples the pair,
 * scores the positive, searches the candidate stream for a negative that violates the margin, weights the step by the rank
 * estimate and writes the loss and the gradient rows.  No workspace.  The rule of a slot is stated in full in
 * esrecsys_amd/csrc/esr_warp_sample.h (warp_slot), the text the kernel's pieces and a stand-alone host program compile.
 *   geometry    max_trials = the most candidates a search may walk (255); D is a multiple of rank_multiple (4) and at most
 *               max_rank (128).
 *   step        B slots of global step `step` under `seed`.  The CSR, the Philox stream and the candidates are those of
 *               esr_bpr_sample (for c < 15 the candidates are BPR's).  s_i = x_u . y_i and every s_j = x_u . y_j in f32 in the
 *               order esr_bpr.hip states for one row; a candidate in u's row is skipped and not counted; otherwise
 *               trials += 1 and d = s_i - s_j; the first candidate with d < margin (strict) within max_trials candidates is
 *               the negative.  Then r = max(1, (ni - len_u) / trials), w = rank_weight[r] (rank_weight float[ni + 1]),
 *               loss_t = w (margin - d), diff_t = d (may be null) and into grads float[3 B, D] = [user rows ; positive
 *               rows ; negative rows]  g_u = reg x - w (yi - yj),  g_i = reg yi - w x,  g_j = reg yj + w x.  grads null:
 *               forward only.  A slot without a violating candidate has out_valid = 0, out_j = the last candidate walked,
 *               out_trials = its count of unseen candidates (may be 0) and zeros in loss_t, diff_t and its three rows.  An
 *               item position outside the table (ill-formed CSR) sets bit 30 of *failed (the caller zeroes and reads it);
 *               that slot reads no row and writes j = 0, valid = 0, trials = 0 and zeros.  A slot is a function of (seed,
 *               step, slot, CSR, tables, max_trials, margin, reg, rank_weight) alone: not of B or the launch.  1 <= nnz, ni,
 *               nu, B <= 2^31 - 1; 1 <= max_trials <= 255; margin finite; reg finite and not negative.  Tables and grads
 *               16-byte aligned. */
int esr_warp_geometry(int* max_trials, int* max_rank, int* rank_multiple);
int esr_warp_step(const float* user_table, int64_t nu, const float* item_table, int64_t ni, int D, const int64_t* row_offsets,
                  const int32_t* row_upos, const int32_t* row_ipos, int64_t nnz, const float* rank_weight, uint64_t seed,
                  uint32_t step, int64_t B, int max_trials, float margin, float reg, int32_t* out_u, int32_t* out_i,
                  int32_t* out_j, int32_t* out_valid, int32_t* out_trials, float* loss_t, float* diff_t, float* grads,
                  int32_t* failed, esr_stream_t stream);

/* ---- Bag tables (Kula, LightFM, 2015; esr_bag.hip) ----
 * A user or an item of the hybrid model is the weighted sum of the embedding rows of its features.  A bag table is a CSR
 * over entities: bag_offsets int64[n_bags + 1], bag_feat int32[nnz] (row positions into table float[nf, D]) and bag_weight
 * float[nnz] or null (every weight 1).  The rule of both calls is stated in esrecsys_amd/csrc/esr_bag_rule.h, the text the
 * kernels and a stand-alone host program compile.  No workspace; the calls never synchronise.
 *   geometry    D is a multiple of rank_multiple (4) and at most max_rank (128): esr_bpr_fwd_bwd's geometry.
 *   sum         out float[n, D]: row r is bag b = rows[r] (rows int32[n], any order, repeats allowed) or b = r (rows null,
 *               n <= n_bags): out[r, c] = acc after acc = fmaf(w[k], table[feat[k], c], acc) for k = off[b] .. off[b + 1] - 1
 *               ascending, from +0.0f.  An empty bag gives a zero row.  An element depends on its own bag and column only:
 *               not on n, the launch or the bags beside it.
 *   expand      the transpose for the optimiser.  grad_rows float[n, D] are the composed rows' gradients, valid int32[n] or
 *               null (all valid), out_offsets int64[n + 1] the exclusive scan of the selected bags' lengths (computed by the
 *               caller), M = out_offsets[n] the rows of out_feat int32[M] / out_grads float[M, D].  Occurrence k of
 *               selected bag r is output row p = out_offsets[r] + (k - off[b]):  out_feat[p] = feat[k],
 *               out_grads[p, c] = fmaf(w[k], grad_rows[r, c], reg * table[feat[k], c]); with valid[r] == 0 the row is zeros
 *               and the table is not read.  Every output row of [out_offsets[r], out_offsets[r + 1]) (clamped into [0, M])
 *               is written; an output row depends on its own occurrence only.
 * Refusals on the device: a bag number outside [0, n_bags) or a feature position outside [0, nf) sets bit 30 of *failed (the
 * caller zeroes and reads it), reads no row and writes zeros -- the whole row of sum; the one output row of expand, with
 * out_feat = 0, as does an output row that the bag has no occurrence for.  The row bounds off[b], off[b + 1] are clamped into
 * [0, nnz]: an ill-formed CSR gives a wrong row, never a read outside the arrays.
 * 1 <= nf, nnz, n_bags <= 2^31 - 1; 0 <= n, M <= 2^31 - 1 (n = 0: nothing is launched); reg finite and not negative.
 * table, grad_rows, out and out_grads 16-byte aligned, the int64 arrays 8-byte aligned. */
int esr_bag_geometry(int* max_rank, int* rank_multiple);
int esr_bag_sum(const float* table, int64_t nf, int D, const int64_t* bag_offsets, const int32_t* bag_feat,
                const float* bag_weight, int64_t nnz, int64_t n_bags, const int32_t* rows, int64_t n, float* out,
                int32_t* failed, esr_stream_t stream);
int esr_bag_expand(const float* table, int64_t nf, int D, const int64_t* bag_offsets, const int32_t* bag_feat,
                   const float* bag_weight, int64_t nnz, int64_t n_bags, const int32_t* rows, const float* grad_rows,
                   const int32_t* valid, const int64_t* out_offsets, int64_t n, int64_t M, float reg, int32_t* out_feat,
                   float* out_grads, int32_t* failed, esr_stream_t stream);

/* ---- Factorised Personalised Markov Chain (Rendle, Freudenthaler, Schmidt-Thieme, WWW 2010; esr_fpmc.hip) ----
 * Next-item ranking trained with the BPR step: score(u, event, i) = U_u . A_i + m . Bn_i over four f32 tables of one rank D,
 * user_table [nu, D] and item_table (A), next_table (Bn), prev_table (P) [ni, D].  The users' sequences are a CSR in time
 * order with repeats kept: seq_offsets int64[nu + 1], seq_upos / seq_ipos int32[nnz_seq].  The context of event e is the
 * c <= window <= 8 events e - c .. e - 1 of the same user, oldest first, and m their bag by the rule of esr_bag_rule.h with
 * every weight w = 1.0f / c:  m = fmaf(w, P[l], m) from +0.0f in that order (c = 0: zeros).  No workspace; the calls
 * never synchronise.
 *   geometry    max_window (8); D is a multiple of rank_multiple (4) and at most max_rank (128).
 *   sample      K steps of B slots in one launch, outputs int32 [K, B] row-major, row k = global step step0 + k (mod 2^32).
 *               The rule is esr_fpmc_sample.h's fpmc_sample_slot: esr_bpr_sample's Philox stream; word 0 of block 0 picks
 *               the event e by multiply-high over nnz_seq, u = seq_upos[e], i = seq_ipos[e], c = min(e - seq_offsets[u],
 *               window); the next 15 words are esr_bpr_sample's negative candidates, tested against u's row of the seen
 *               CSR (row_offsets int64[nu + 1], row_ipos int32[nnz_seen], ascending and distinct within a row); if all are
 *               seen the last one is written with valid = 0.  A slot is a function of (seed, step, slot, the CSRs, window)
 *               alone.  dropped int32[K] = the exact count of valid == 0 per step (zeroed by the call; integer atomics).
 *   fwd_bwd     per slot t (u, e, c, i, j int32[B]; valid int32[B] or null = all valid) with x = U[u], the context ids
 *               l_n = seq_ipos[e - c + n] and m as above:  d = x . (A_i - A_j) + m . (Bn_i - Bn_j) in f32 in the order
 *               esr_fpmc.hip states (a function of D alone), loss_t[t] = max(-d, 0) + log1pf(expf(-|d|)), diff_t[t] = d
 *               (may be null), g = sigmoid(-d), and into grads float[5 B + M, D] = [U rows ; A_i rows ; A_j rows ; Bn_i rows ;
 *               Bn_j rows ; context occurrences]
 *                 g_u = reg x - g (A_i - A_j),  g_ai = reg A_i - g x,  g_aj = reg A_j + g x,
 *                 g_bi = reg Bn_i - g m,  g_bj = reg Bn_j + g m,  g_m = -g (Bn_i - Bn_j),
 *                 occurrence n: fmaf(w, g_m, reg * P[l_n]) per element, at row 5 B + ctx_offsets[t] + n,
 *               with ctx_ids[ctx_offsets[t] + n] = l_n.  ctx_offsets int64[B + 1] is the exclusive scan of c and M =
 *               ctx_offsets[B], both computed by the caller (esr_bag_expand's convention).  grads null: forward only,
 *               ctx_offsets and ctx_ids are not read.  valid[t] == 0 writes zero rows, loss_t = 0 and diff_t = 0 and
 *               reads no table row, but its c occurrences keep their ids: the layout depends on the draw alone.  A u, i,
 *               j or context id outside its table, an e outside [0, nnz_seq), a c outside [0, min(8, e)] or a range of
 *               ctx_offsets that is not c rows long sets bit 30 of *failed (the caller zeroes and reads it) whatever valid
 *               says; that slot reads no table row and writes zeros, and every row of its (clamped) range gets ctx_ids = 0
 *               where the id was refused.  No reduction across slots: an output depends on its own slot, reg and D only.
 * 1 <= nu, ni, nnz_seq, nnz_seen, K, B <= 2^31 - 1; nu + 3 ni <= 2^31 - 1 (the virtual row space of the update over the four
 * tables); 0 <= M <= 2^31 - 1; 1 <= window <= 8; reg finite and not negative.  Tables and grads 16-byte aligned, the int64
 * arrays 8-byte aligned. */
int esr_fpmc_geometry(int* max_window, int* max_rank, int* rank_multiple);
int esr_fpmc_sample(const int64_t* seq_offsets, const int32_t* seq_upos, const int32_t* seq_ipos, int64_t nnz_seq,
                    const int64_t* row_offsets, const int32_t* row_ipos, int64_t nnz_seen, int64_t nu, int64_t ni, int window,
                    uint64_t seed, uint32_t step0, int64_t K, int64_t B, int32_t* out_u, int32_t* out_e, int32_t* out_c,
                    int32_t* out_i, int32_t* out_j, int32_t* out_valid, int32_t* dropped, esr_stream_t stream);
int esr_fpmc_fwd_bwd(const float* user_table, int64_t nu, const float* item_table, const float* next_table,
                     const float* prev_table, int64_t ni, int D, const int32_t* seq_ipos, int64_t nnz_seq, const int32_t* u,
                     const int32_t* e, const int32_t* c, const int32_t* i, const int32_t* j, const int32_t* valid, int64_t B,
                     const int64_t* ctx_offsets, int64_t M, float reg, float* loss_t, float* diff_t, float* grads,
                     int32_t* ctx_ids, int32_t* failed, esr_stream_t stream);

/* ---- Skip-gram with negative sampling (Mikolov et al., NIPS 2013; item2vec, Barkan and Koenigstein 2016; esr_sgns.hip) ----
 * Item or word vectors trained straight from id sequences: two f32 tables of ni rows and one rank D, in_table (the centre
 * vectors v) and out_table (the context vectors w); no user table.  The documents are a CSR in order with repeats kept:
 * seq_offsets int64[nd + 1], seq_upos (the document of an event) / seq_ipos (its item position) int32[nnz_seq].  The noise
 * distribution is an alias table: noise_keep uint32[ni], noise_alias int32[ni]; column n yields item n for a 32-bit word
 * below noise_keep[n] and noise_alias[n] otherwise (a full column: noise_alias[n] == n).  No workspace; the calls never
 * synchronise.
 *   geometry    max_window (32), max_negatives (16); D is a multiple of rank_multiple (4) and at most max_rank (128).
 *   sample      K steps of B slots in one launch, outputs int32 row-major: c, e, o, valid [K, B], neg [K, B, negatives];
 *               row k = global step step0 + k (mod 2^32).  The rule is esr_sgns_sample.h's sgns_sample_slot over
 *               esr_bpr_sample's counter layout (t, s, block, 0): word 0 of block 0 picks the event e by multiply-high
 *               over nnz_seq, c = seq_ipos[e]; word 1 the distance d in [1, window] with weight window - d + 1; the top
 *               bit of word 2 the side; o = seq_ipos[e +- d] when that event lies in e's document, else valid = 0 and
 *               o = c.  Noise item k takes words 2 (k & 1), 2 (k & 1) + 1 of block 1 + (k >> 1): the column by
 *               multiply-high over ni, then the column's own item or its alias.  A slot is a function of (seed, step,
 *               slot, the CSR, window, negatives, the noise table) alone.  dropped int32[K] = the exact count of
 *               valid == 0 per step (zeroed by the call; integer atomics).
 *   fwd_bwd     per slot t (c, o int32[B], neg int32[B, negatives]; valid int32[B] or null = all valid) with v = in[c],
 *               s_o = v . out[o], s_k = v . out[n_k] in f32 in the order esr_sgns.hip states (a function of D alone) and
 *               m_k = (n_k != o):  loss_t[t] = softplus(-s_o) + sum_k m_k softplus(s_k);  diff_t float[B, 1 + negatives]
 *               (may be null) = [s_o, s_0, ..];  grads float[(2 + negatives) B, D] (may be null: forward only) =
 *               [centre rows ; positive rows ; noise rows k-major], noise item k of slot t at row (2 + k) B + t:
 *                 g_c = (sigmoid(s_o) - 1) out[o] + sum_k m_k sigmoid(s_k) out[n_k] + reg v   (positive, then k ascending),
 *                 g_o = (sigmoid(s_o) - 1) v + reg out[o],   g_n_k = m_k (sigmoid(s_k) v + reg out[n_k]).
 *               valid[t] == 0 writes zero rows, loss_t = 0 and zero scores and reads no table row.  A c, o or n_k outside
 *               [0, ni) sets bit 30 of *failed (the caller zeroes and reads it) whatever valid says; that slot reads no
 *               table row and writes zeros.  No reduction across slots: an output depends on its own slot, reg and D only.
 * 1 <= nd, ni, nnz_seq, K, B <= 2^31 - 1; 2 ni <= 2^31 - 1 (the virtual row space of the update over the two tables);
 * (2 + negatives) B <= 2^31 - 1; 1 <= window <= 32; 1 <= negatives <= 16; reg finite and not negative.  Tables and grads
 * 16-byte aligned, seq_offsets 8-byte aligned. */
int esr_sgns_geometry(int* max_window, int* max_negatives, int* max_rank, int* rank_multiple);
int esr_sgns_sample(const int64_t* seq_offsets, const int32_t* seq_upos, const int32_t* seq_ipos, int64_t nnz_seq, int64_t nd,
                    int64_t ni, int window, int negatives, const uint32_t* noise_keep, const int32_t* noise_alias,
                    uint64_t seed, uint32_t step0, int64_t K, int64_t B, int32_t* out_c, int32_t* out_e, int32_t* out_o,
                    int32_t* out_valid, int32_t* out_neg, int32_t* dropped, esr_stream_t stream);
int esr_sgns_fwd_bwd(const float* in_table, const float* out_table, int64_t ni, int D, const int32_t* c, const int32_t* o,
                     const int32_t* neg, const int32_t* valid, int64_t B, int negatives, float reg, float* loss_t,
                     float* diff_t, float* grads, int32_t* failed, esr_stream_t stream);

/* ---- Diversity re-ranking (MMR, Carbonell and Goldstein 1998; intra-list similarity, Ziegler et al. 2005; esr_rerank.hip) ----
 * rows float[ni, D] are the items' rows (D a multiple of 4 in [4, 128]), cand int32[nq, width] item POSITIONS into rows,
 * rel float[nq, width], lengths int32[nq] or null (full rows), 1 <= width <= 1024.  The rule of both calls is stated in
 * esrecsys_amd/csrc/esr_rerank_rule.h, the text the kernels and a stand-alone host program compile.  sim(a, b) is the dot
 * product of two rows in the summation order of esr_bpr_fwd_bwd.  No workspace; the calls never synchronise.
 *   geometry    for (D, width): the limits (max_rank 128, rank_multiple 4, max_width 1024, max_cutoffs 8), the staging budget
 *               stage_bytes, the grid cap, whether this shape stages the query's rows in LDS (width * D * 4 <= stage_bytes)
 *               and the dynamic LDS of its launch.  Both forms give the same bits.
 *   mmr         per query n_out (1 .. width) greedy rounds over the candidates c < L = clamp(lengths[q], 0, width): the pick of
 *               round t maximises v[c] = fmaf(lam, rel[c], -((1.0f - lam) * m[c])), m[c] = the greatest sim of c to a row
 *               picked before (0.0f in round 0), ties to the smallest c; out_pos / out_item / out_rel / out_value [nq, n_out]
 *               receive c, cand[c], rel[c] and v[c], out_length[q] the picks, and the slots behind -1 / -1 / 0 / 0.  lam in
 *               [0, 1]; lam = 1 is the stable sort by rel descending.
 *   ils         at nk (1 .. 8) strictly ascending cutoffs ks (HOST array): ils float[nq, nk] = the mean sim over the pairs of
 *               present candidates among the first min(k, L), summed in fp64 in ascending (i, j < i) order and rounded once;
 *               valid int32[nq, nk] = 0 (and ils = 0) with fewer than two present candidates.
 * Refusals on the device: a position outside [0, ni) sets bit 30 of *failed, a rel that is not finite bit 29 (the caller zeroes
 * and reads the word); such a candidate is absent: never picked, never counted, its row never read.
 * 1 <= ni <= 2^31 - 1; 0 <= nq <= 2^31 - 1 (nq = 0: nothing is launched).  rows 16-byte aligned. */
int esr_rerank_geometry(int D, int width, int* max_rank, int* rank_multiple, int* max_width, int* max_cutoffs,
                        int* stage_bytes, int* grid_cap, int* staged, int* lds_bytes);
int esr_rerank_mmr(const float* rows, int64_t ni, int D, const int32_t* cand, const float* rel, const int32_t* lengths,
                   int64_t nq, int width, int n_out, float lam, int32_t* out_pos, int32_t* out_item, float* out_rel,
                   float* out_value, int32_t* out_length, int32_t* failed, esr_stream_t stream);
int esr_rerank_ils(const float* rows, int64_t ni, int D, const int32_t* cand, const int32_t* lengths, int64_t nq, int width,
                   const int32_t* ks, int nk, float* ils, int32_t* valid, int32_t* failed, esr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ESR_HIP_H_ */
