/*
 * pllhip.h -- engine-specific additions to the libpll-2 style C ABI of
 * include/pll.h.  Nothing here exists in the reference; these entry points
 * cover what a device-resident engine needs on top of the reference interface:
 *
 *   - device selection and introspection,
 *   - explicit materialisation of device-resident arrays into the host mirrors
 *     that pll-modules' msa/binary code reads (partition->clv[i],
 *     partition->scale_buffer[i], partition->pmatrix[i]):
 *     src/binary/binary_io_operations.c:286-296, src/msa/pll_msa.c:114-124,
 *     test/src/optimize/blopt-minimal.c:96 (pll_show_pmatrix),
 *   - a ready-made implementation of the reference's only parallelism hook,
 *       void (*parallel_reduce_cb)(void *ctx, double *data, size_t n, int op)
 *     (src/tree/pll_tree.h:274-276, ops SUM/MAX/MIN = 0/1/2 at
 *     src/pllmod_common.h:29-31), backed by RCCL over xGMI with one process
 *     per GPU.
 */
#ifndef PLLHIP_H_INCLUDED
#define PLLHIP_H_INCLUDED

#include "pll.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what pllhip_sync_to_host materialises */
#define PLLHIP_SYNC_PMATRIX  (1 << 0)   /* all P-matrices -> partition->pmatrix   */
#define PLLHIP_SYNC_CLV      (1 << 1)   /* all CLVs       -> partition->clv[i]    */
#define PLLHIP_SYNC_SCALERS  (1 << 2)   /* all scalers    -> partition->scale_buffer[i] */
#define PLLHIP_SYNC_TIPS     (1 << 3)   /* pllhip_sync_to_device only: tip codes, tip map, pattern weights, invariant sites */
#define PLLHIP_SYNC_ALL      15

/* pll_partition_create attribute (above PLL_ATTRIB_MASK): allocate the host mirrors
   partition->clv[i] / scale_buffer[i] up front, so that code which FILLS them -- the
   reference's binary loader, src/binary/pll_binary.c:346-500 -- finds memory there;
   pllhip_sync_to_device() then moves the contents to the GPU.  pllhip_sync_to_host()
   sets the bit on the partition, so a dump carries it into the file and the loader
   passes it back to pll_partition_create. */
#define PLLHIP_ATTRIB_HOST_MIRRORS (1u << 30)

/* reduce-callback operation codes (src/pllmod_common.h:29-31) */
#define PLLHIP_REDUCE_SUM 0
#define PLLHIP_REDUCE_MAX 1
#define PLLHIP_REDUCE_MIN 2

/* number of visible HIP devices (0 if none); never initialises a context */
PLL_EXPORT int pllhip_device_count(void);

/* device used by partitions created afterwards on this thread (default 0,
   or the value of the PLLHIP_DEVICE environment variable) */
PLL_EXPORT int pllhip_set_device(int device);
PLL_EXPORT int pllhip_get_device(void);

/* ---- one partition over several GPUs (engine-internal sharding, SURVEY.md 8e topology i) ----
 * Partitions created afterwards on this thread are split into `count` contiguous site ranges,
 * one per device (devices[i]; NULL: device i modulo the visible ones): every device holds all
 * nodes' CLVs of its range and a replica of the model; pll_update_partials /
 * pll_update_prob_matrices / pll_update_sumtable fan out without communication, the scalar
 * calls add the devices' sums on the host in a fixed order.  The caller -- an unmodified
 * pll-modules client with ONE treeinfo and no parallel_reduce_cb -- sees one pll_partition_t.
 * count <= 1 switches it off.  The environment variable PLLHIP_SHARD_DEVICES="0,1,2,3" does the
 * same for clients that cannot call this.  Partitions with fewer than 64 sites per device, and
 * partitions with ascertainment-bias correction, stay on one device. */
PLL_EXPORT int pllhip_set_sharding(unsigned int count, const int * devices);
/* number of devices `partition` is spread over (1: an ordinary partition) */
PLL_EXPORT unsigned int pllhip_shard_count(const pll_partition_t * partition);

/* ---- parsimony (pll_fastparsimony_init objects; INTEGRATION.md, "Parsimony") ----
 * The Fitch cost of `tree` over the `count` partitions of `list` (same tip count): sum over partitions and sites
 * of pattern weight x empty intersections.  The tree is any binary unrooted tree whose tip clv_index values are
 * tip indices of the partitions.  PLL_ERROR_STEPWISE_TIPS: different tip counts or fewer than 3 tips;
 * PLL_ERROR_TREE_INVALID: a non-binary tree or an unknown tip. */
PLL_EXPORT int pllhip_parsimony_tree_score(pll_parsimony_t * const * list, unsigned int count,
                                           const pll_utree_t * tree, unsigned int * score);

/* gfx architecture name of a device, e.g. "gfx950" */
PLL_EXPORT int pllhip_device_arch(int device, char * out, size_t out_len);

/* host-only: eigen-decomposition of the reversible rate matrix built from
   `subst_params` (upper triangle, row-major) and `frequencies`, normalised to
   mean rate 1, Q = V L V^-1.  Storage follows libpll-2: inv_eigenvecs[i*Sp+k] = V[i][k],
   eigenvecs[k*Sp+j] = V^-1[k][j], i.e. P(t) = inv_eigenvecs * diag(exp(L t)) * eigenvecs.
   This is what pll_update_prob_matrices runs when eigen_decomp_valid[i] == 0. */
PLL_EXPORT int pllhip_eigen_decompose(unsigned int states, unsigned int states_padded,
                                      const double * subst_params,
                                      const double * frequencies,
                                      double * eigenvecs, double * inv_eigenvecs,
                                      double * eigenvals);

/* copy device-resident arrays into the host mirrors of the partition
   (allocating partition->clv[i] / scale_buffer[i] on first use) */
PLL_EXPORT int pllhip_sync_to_host(pll_partition_t * partition, unsigned int what);

/* the opposite direction: host mirrors (filled by a checkpoint loader) -> device.
   CLVs / scalers whose mirror is NULL are skipped. */
PLL_EXPORT int pllhip_sync_to_device(pll_partition_t * partition, unsigned int what);

/* single-array variants, caller-provided output.  Layouts are the partition's:
   CLV [site][rate][states_padded]; a tip stored as codes is expanded to 0/1. */
PLL_EXPORT int pllhip_get_clv(pll_partition_t * partition, unsigned int clv_index,
                              double * out);
PLL_EXPORT int pllhip_get_scaler(pll_partition_t * partition, unsigned int scaler_index,
                                 unsigned int * out);
PLL_EXPORT int pllhip_get_sumtable(pll_partition_t * partition,
                                   const double * sumtable_key, double * out);

/* host -> device for an inner CLV / scaler (checkpoint restore path of
   src/binary; also lets tests inject states) */
PLL_EXPORT int pllhip_set_clv(pll_partition_t * partition, unsigned int clv_index,
                              const double * clv);
PLL_EXPORT int pllhip_set_scaler(pll_partition_t * partition, unsigned int scaler_index,
                                 const unsigned int * scaler);

/* block until all work queued on the partition's stream has finished */
PLL_EXPORT int pllhip_synchronize(pll_partition_t * partition);

/* the partition's HIP stream (hipStream_t as void*), for callers that time
   kernels with events or enqueue their own work */
PLL_EXPORT void * pllhip_stream(pll_partition_t * partition);

/* per-partition work counters (engine-side analogue of treeinfo->counter,
   src/tree/treeinfo.c:1017) */
typedef struct pllhip_counters
{
  unsigned long long partial_ops;        /* operations executed                */
  unsigned long long partial_launches;   /* kernel launches for them           */
  unsigned long long site_updates;       /* ops * sites * rate_cats            */
  unsigned long long pmatrix_updates;      /* matrices requested               */
  unsigned long long pmatrix_launches;     /* kernel launches that served them */
  unsigned long long lnl_calls;
  unsigned long long sumtable_calls;
  unsigned long long derivative_calls;   /* sumtable scans                     */
  unsigned long long derivative_points;  /* trial branch lengths evaluated by them */
  unsigned long long model_uploads;      /* host->device re-syncs of model state */
} pllhip_counters_t;

PLL_EXPORT int pllhip_get_counters(const pll_partition_t * partition,
                                   pllhip_counters_t * out);
PLL_EXPORT void pllhip_reset_counters(pll_partition_t * partition);

/* live timing of the pll_update_partials kernel launches with HIP events on the
   partition's stream.  While enabled, every launch is bracketed by two events;
   pllhip_profile_read() synchronises, sums the elapsed times, reports them with
   the algorithmic byte count of those launches and
   resets the accumulators. */
typedef struct pllhip_profile
{
  unsigned long long launches;
  unsigned long long ops;
  double kernel_ms;
  double algorithmic_bytes;
  double algorithmic_flops;   /* 2*S*S per non-tip child matvec + S products, per site-update */
  double minimum_bytes;       /* what the schedule has to move: as algorithmic_bytes, but a child vector (and its
                                 scaler counts) that an operation chain hands over in registers is not read */
} pllhip_profile_t;

PLL_EXPORT int pllhip_profile_partials(pll_partition_t * partition, int enable);

/* PLL_ATTRIB_SITE_REPEATS (libpll-2's site repeats; the reference's test harness selects it,
   test/src/common.c:31): what the engine did with it since the partition was created.  The vector of a cherry
   (a tip x tip operation) is computed per class of sites -- a pair of tip codes -- and not per site, and so is the
   vector of every node whose two children are known per class (4- and 20-state families, coded tips). */
typedef struct pllhip_repeat_stats
{
  unsigned long long cherries;         /* operations kept per class (the name is the first step's: cherries only) */
  unsigned long long classes;          /* classes of those operations, summed */
  unsigned long long sites;            /* sites they cover, summed (classes / sites = the share computed) */
  unsigned long long expansions;       /* class nodes expanded to the site-indexed form on demand */
} pllhip_repeat_stats_t;
PLL_EXPORT int pllhip_repeat_stats(const pll_partition_t * partition, pllhip_repeat_stats_t * out);
PLL_EXPORT int pllhip_profile_read(pll_partition_t * partition, pllhip_profile_t * out);

/* What the scheduler made of the last operation list that went through a resident schedule (operation chains in
   device memory; all zero when the partition has none).  An operation chain hands its vector on in registers; the
   vector next to it comes back from memory -- except a lone cherry (a tip x tip operation), which the 20-state
   family builds in registers inside the chain that reads it, from the two tip tables ("folded"; per-site scalers,
   coded tips, no site repeats; PLLHIP_FOLD=0 in the environment plans without folds).  A folded cherry's scaler
   counts are stored like any other's; its vector is stored when somebody needs it (pllhip_deferred_stats). */
typedef struct pllhip_schedule_stats
{
  unsigned int chains;                 /* operation chains of the schedule */
  unsigned int operations;             /* operations in them, folded cherries included */
  unsigned int inner_reads;            /* inner vectors that the chains read from memory */
  unsigned int folded_cherries;        /* cherries built in registers by the operation that reads them */
  unsigned int lookup_children;        /* cherries and cherry x tip subtrees that the operation above them reads through a
                                          table of their classes of tip codes instead of the stored vector (inner_reads
                                          counts neither these nor the folded cherries) */
} pllhip_schedule_stats_t;
PLL_EXPORT int pllhip_schedule_stats(const pll_partition_t * partition, pllhip_schedule_stats_t * out);

/* Evaluate-only traversals.  The model-parameter optimisers of pll-modules evaluate the whole tree after every
   parameter poke (src/algorithm/algo_callback.c:338, 465, 568, 678: pllmod_treeinfo_compute_loglh(treeinfo, 0);
   src/optimize/opt_algorithms.c:734-773: nmax + 1 of them per L-BFGS-B iteration): every vector is recomputed by
   the next evaluation and never read in between, yet two thirds of what such an evaluation moves are stores.
   While the mode is on, an operation list with the shape of a tree traversal (pll_update_partials /
   pllhip_update_partials_batch, resident schedules of the 4-, 2..32- and 20-state families) hands the vectors
   inside its operation chains on in registers WITHOUT storing them; the last vector of every chain and all scaler
   counts are stored as always.  Nothing observable changes: a vector that was not stored stays recomputable (the
   engine keeps its operation) and is stored
     - for the first reader that needs it (a later operation list, an edge / root log-likelihood, a sumtable,
       pllhip_get_clv, pllhip_sync_to_host, ...), and
     - before one of its inputs changes (a P-matrix it was computed with, a tip, a child vector or scaler buffer
       that a later list overwrites),
   with the very operations that made it, so every later result is bit-identical to the mode being off.
   pllhip_discard_transient declares the vectors that were not stored dead (a caller that is about to change the
   model and evaluate the whole tree again: nothing is recomputed for the P-matrix updates that follow);
   reading one of them afterwards without recomputing it is the caller's error, as after any invalidation.
   PLLHIP_TRANSIENT=1 in the environment switches the mode on for every partition (the test suite under it). */
typedef struct pllhip_transient_stats
{
  unsigned long long skipped;          /* vectors a traversal did not store */
  unsigned long long materialized;     /* ... that were recomputed and stored for a reader or before a change */
  unsigned long long discarded;        /* ... that were declared dead or overwritten before anybody asked */
} pllhip_transient_stats_t;
PLL_EXPORT int pllhip_set_transient(pll_partition_t * partition, int enable);
PLL_EXPORT int pllhip_discard_transient(pll_partition_t * partition);
PLL_EXPORT int pllhip_transient_stats(const pll_partition_t * partition, pllhip_transient_stats_t * out);

/* Deferred stores.  A storing traversal of the 20-state family (the mode above being off; partitions of 122 880 sites
   and more, PLLHIP_DEFER=1 in the environment: of any size) leaves out the stores of vectors that none of its
   operations reads from memory and that coded tips alone recompute: folded cherries, and the one or two operations of a
   cherry / cherry x tip subtree that the operation above reads through its class table; and, while the caller keeps
   evaluating without reading such vectors (two such lists in a row of which none was stored later; PLLHIP_DEFER=3: always),
   the tip-only run at the bottom of every operation chain -- the cherry a chain starts with and the "that vector x
   coded tip" operations above it whose result the next operation takes in registers (PLLHIP_DEFER_DEPTH=D: the
   first D operations of a run); and, once four such lists in a row have gone unread
   (PLLHIP_DEFER=4: always), every vector inside a chain that the next operation of the chain takes in registers and
   that no other operation of the list reads, whatever its children are: from the fifth
   evaluation of a row on only the last vector of each chain and the vectors at the root edge are stored.  The first
   deferred vector that is stored for a reader takes the following lists back to the first level.  Their scaler
   counts are stored as always.  Such a vector is kept as its operation, exactly like a vector the mode above left
   out, and is stored for its first reader or before one of its inputs -- a P-matrix, a tip, a child vector, a scaler
   buffer -- changes, by a launch of its own (deferred vectors that stand next to each other in a chain: by one
   launch for all of them from the reader's upwards; PLLHIP_DEFER_GROUP=0: one per reader), which costs two to three
   times what leaving the store out of the traversal saved.  A caller observes nothing but
   timing: whatever it reads is bit-identical to PLLHIP_DEFER=0 in the environment (which plans every store).
   pllhip_discard_transient leaves these vectors alone (the caller never asked for them to be left out);
   pllhip_transient_stats does not count them. */
typedef struct pllhip_deferred_stats
{
  unsigned long long deferred;         /* stores that storing traversals left out */
  unsigned long long stored_later;     /* ... that were made up for: a reader needed the vector, or an input changed */
  unsigned long long given_up;         /* ... that never happened: the vector was overwritten before anybody asked */
} pllhip_deferred_stats_t;
PLL_EXPORT int pllhip_deferred_stats(const pll_partition_t * partition, pllhip_deferred_stats_t * out);

/* kernel family actually used for pll_update_partials on this partition:
   "s4-valu", "s20-mfma", "generic" ... (for tests that must prove the
   specialised path ran) */
PLL_EXPORT const char * pllhip_partials_kernel_name(const pll_partition_t * partition);

/* ---- multi-GPU: one process per GPU, RCCL all-reduce ---------------- */

#define PLLHIP_COMM_ID_BYTES 128

/* rank 0 creates an id and ships it to the other ranks by any side channel
   (bench.py uses the torch.distributed store) */
PLL_EXPORT int pllhip_comm_get_unique_id(unsigned char id[PLLHIP_COMM_ID_BYTES]);

typedef struct pllhip_comm pllhip_comm_t;

PLL_EXPORT pllhip_comm_t * pllhip_comm_create(const unsigned char id[PLLHIP_COMM_ID_BYTES],
                                              int rank, int nranks, int device);
PLL_EXPORT void pllhip_comm_destroy(pllhip_comm_t * comm);

PLL_EXPORT int pllhip_comm_rank(const pllhip_comm_t * comm);
PLL_EXPORT int pllhip_comm_size(const pllhip_comm_t * comm);

/* drop-in value for treeinfo's parallel_reduce_cb with ctx = pllhip_comm_t*.  The payload is
   a host array (the library calls before it have returned doubles), staged through one pinned
   buffer.  On a HIP / RCCL failure the payload is set to NaN and pll_errno is set: the
   callback has no error channel, and a rank must not continue with its local value. */
PLL_EXPORT void pllhip_reduce_cb(void * ctx, double * data, size_t n, int op);

/* ---- several trial branch lengths per sumtable scan ------------------------
 * pll_compute_likelihood_derivatives at `count` (1..8) branch lengths in ONE pass over the
 * sumtable (src/optimize/pll_optimize.c:1223-1287 scans it once per Newton-Raphson
 * iteration).  d_f[i], dd_f[i] are bit-identical to what the single-length call returns
 * for branch_lengths[i], whatever else shares the launch. */
PLL_EXPORT int pllhip_compute_likelihood_derivatives_multi(pll_partition_t * partition,
                                                           int parent_scaler_index,
                                                           int child_scaler_index,
                                                           const double * branch_lengths,
                                                           unsigned int count,
                                                           const unsigned int * params_indices,
                                                           const double * sumtable,
                                                           double * d_f, double * dd_f);

/* how many trial lengths one scan of this partition's sumtable evaluates at (about) the
   price of one: 4 where the scan runs on the matrix cores (20- and 61-state families: the
   lengths are rows of an MFMA operand and the scan stays HBM-bound), 1 elsewhere (the
   4-state scan is bound by its per-site divisions).  Callers that speculate on trial
   lengths (include/pllhip_eval.h) use it to decide whether speculation is free. */
PLL_EXPORT unsigned int pllhip_free_trial_lengths(const pll_partition_t * partition);

/* Newton-Raphson on one branch, entirely on the device: the loop the reference runs around
   pll_compute_likelihood_derivatives (src/optimize/opt_algorithms.c:133-261: evaluate {f, f'} at the iterate,
   bracket, clamp the step to +-bl_max / max_newton and to the bracket, stop at |f| or |step| < tolerance; the
   target function is src/optimize/pll_optimize.c:1223-1287) for ONE partition whose sumtable is current
   (pll_update_sumtable), in ONE launch: scan, in-launch reduction, step rule, next scan.  The iterates are the
   host loop's, bit for bit (same scan, same summation order, the same fp64 expressions without contraction).
   max_newton: 1 ... PLLHIP_NEWTON_MAX_ITERATIONS; a loop makes at most max_newton + 2 scans, the last of which finds
   the limit exceeded.  Any two loops may follow one another on a partition, whatever their limits and however they
   ended.
   Returns PLL_SUCCESS with *length = the length the loop ended at and *iterations = scans made; `trail`
   (NULL, or room for 96 doubles) receives the iterate after each of the first min(*iterations, 96) scans -- of a
   longer loop the later iterates are not kept, *length and *iterations are complete.  PLL_FAILURE with pll_errno =
   PLLHIP_ERROR_NEWTON_LIMIT (more than max_newton iterations; *iterations = max_newton + 2) /
   PLLHIP_ERROR_NEWTON_DERIVATIVES (a non-finite derivative) -- the reference's two failure modes; *length,
   *iterations and `trail` are set as on success -- or PLLHIP_ERROR_NEWTON_UNSUPPORTED: this partition cannot
   run the loop on the device (4-state / generic kernel family, ascertainment-bias correction, a partition spread
   over devices, a scan grid larger than the chip holds at once, max_newton 0 or above
   PLLHIP_NEWTON_MAX_ITERATIONS); the caller then iterates itself.
   PLLHIP_ERROR_NEWTON_STUCK: the workgroups of the loop wait for one another inside the launch, so all of them
   have to be on the chip at once; the grid is sized for a device this partition has to itself, and other work on
   the device (another process, another stream) can keep a workgroup out.  Every wait is bounded: the launch then
   ends with this code after the bound (about a second), the engine's reduction state is reset, nothing was
   changed -- the caller iterates itself (pllhip_eval does, and stops asking for the device loop). */
#define PLLHIP_ERROR_NEWTON_LIMIT        910
#define PLLHIP_ERROR_NEWTON_DERIVATIVES  911
#define PLLHIP_ERROR_NEWTON_UNSUPPORTED  912
#define PLLHIP_ERROR_NEWTON_STUCK        913
#define PLLHIP_NEWTON_MAX_ITERATIONS     65536        /* 2^16 */
PLL_EXPORT int pllhip_newton_branch(pll_partition_t * partition,
                                    int parent_scaler_index, int child_scaler_index,
                                    const unsigned int * params_indices, const double * sumtable,
                                    double start, double bl_min, double bl_max, double tolerance,
                                    unsigned int max_newton,
                                    double * length, unsigned int * iterations, double * trail);

/* The same loop for SEVERAL partitions that share the branch length -- linked lengths, or scaled ones (partition p
   sees length_scalers[p] * x; NULL: all 1) --: the reference's multi-partition derivative function
   (src/optimize/pll_optimize.c:1223-1287: f = sum s_p f_p, f' = sum s_p^2 f'_p, added in partition order) inside
   the loop.  Every partition runs its own instance of the loop on its own stream (its family's kernel, its own scan
   grid: its totals are those of its blocking derivative call); the instances meet on the device after every scan.
   All partitions live on ONE device and none is remote (a sum over workers needs the host loop); at most 8.
   The partitions run as ONE launch (every partition a run of its workgroups, every family its own loop) when their scan
   grids fit the chip together under that kernel's occupancy; else one launch per partition.
   Same results and error codes as pllhip_newton_branch; PLLHIP_ERROR_NEWTON_UNSUPPORTED also when the partitions'
   scan grids do not fit the chip together, or -- one launch per partition -- the process was not started with
   GPU_MAX_HW_QUEUES >= 8 in its environment: those launches wait for one another on the device, the HIP runtime runs streams that share a
   hardware queue one after the other, and it has four queues unless told otherwise before its first call (the library
   does not ask for more: they slow evaluations of many partitions down).  The caller iterates from the host then. */
PLL_EXPORT int pllhip_newton_branch_multi(pll_partition_t * const * partitions, unsigned int count,
                                          int parent_scaler_index, int child_scaler_index,
                                          const unsigned int * const * params_indices,
                                          const double * const * sumtables, const double * length_scalers,
                                          double start, double bl_min, double bl_max, double tolerance,
                                          unsigned int max_newton,
                                          double * length, unsigned int * iterations, double * trail);

/* pll_update_partials for several partitions that are evaluated on ONE tree: the result is what
   pll_update_partials(partitions[i], operations, count) stores for every non-NULL partitions[i], bit for
   bit.  pll-modules walks the partitions of an analysis one after the other
   (src/tree/treeinfo.c:1020-1056, src/optimize/pll_optimize.c:748-775); partitions of one kernel family on
   one device share their launches here (the chains of a round of every partition are grid rows of one
   launch), which is what keeps data sets with one small partition per gene -- and the per-GPU share of a
   partitioned analysis on eight GPUs -- off the launch-latency floor.  NULL entries (partitions another
   worker owns, src/tree/treeinfo.c:1024-1031) are skipped.  PLLHIP_BATCH=0: per-partition calls. */
PLL_EXPORT int pllhip_update_partials_batch(pll_partition_t * const * partitions,
                                            unsigned int partition_count,
                                            const pll_operation_t * operations,
                                            unsigned int count);

/* ---- deferred scalar results -----------------------------------------------
 * pll_compute_edge_loglikelihood and pll_compute_likelihood_derivatives hand a double back
 * to the host: one wait per call and partition, and with several workers a host-side
 * reduce after it.  A result group collects the totals of several such computations -- the
 * partitions of an evaluation (src/tree/treeinfo.c:1040-1067), the trial lengths of a
 * Newton-Raphson round (src/optimize/pll_optimize.c:1240-1286) -- in device-resident slots:
 * the pllhip_results_* calls only enqueue work; pllhip_results_fetch() all-reduces the slots
 * in place over the communicator (when there is one), publishes them to mapped host memory
 * and waits ONCE.  Slots nobody deposited to since the last fetch (partitions another worker
 * owns) count as the identity of `op`.  One fetch completes all deposits made since the
 * previous one.  Same numbers, bit for bit, as the blocking calls. */
typedef struct pllhip_results pllhip_results_t;

PLL_EXPORT pllhip_results_t * pllhip_results_create(pllhip_comm_t * comm /* or NULL */,
                                                    unsigned int slots);
PLL_EXPORT void pllhip_results_destroy(pllhip_results_t * results);

/* 1 slot: the edge log-likelihood of `partition` */
PLL_EXPORT int pllhip_results_edge_loglikelihood(pllhip_results_t * results, unsigned int slot,
                                                 pll_partition_t * partition,
                                                 unsigned int parent_clv_index, int parent_scaler_index,
                                                 unsigned int child_clv_index, int child_scaler_index,
                                                 unsigned int matrix_index,
                                                 const unsigned int * freqs_indices);

/* 2 * count slots: d_f[0], dd_f[0], d_f[1], dd_f[1], ... */
PLL_EXPORT int pllhip_results_derivatives(pllhip_results_t * results, unsigned int slot,
                                          pll_partition_t * partition,
                                          int parent_scaler_index, int child_scaler_index,
                                          const double * branch_lengths, unsigned int count,
                                          const unsigned int * params_indices,
                                          const double * sumtable);

/* out[i] = reduce over all workers of slot first + i; NaN in every out[i] and PLL_FAILURE on error.
   Failure handling (no worker is left inside a collective; the process is expected to exit or to start a
   fresh child -- the library never re-executes anything):
     * a deposit that failed on this worker (or pllhip_results_poison) makes the fetch contribute NaN to
       every slot and still take part in the all-reduce: every worker gets NaN and PLL_FAILURE in this call;
     * an RCCL / HIP error in the collective path, or no result within PLLHIP_COLLECTIVE_TIMEOUT_S seconds
       (default 120: a peer that died never joins), aborts the communicator (ncclCommAbort), sets pll_errno
       (PLL_ERROR_HIP_RUNTIME / PLL_ERROR_HIP_TIMEOUT) and returns NaN; every later collective on that
       communicator fails at once with PLL_ERROR_HIP_COMM_ABORTED.  pllhip_reduce_cb behaves the same way.
   The group itself is reset on every path and can take new deposits. */
PLL_EXPORT int pllhip_results_fetch(pllhip_results_t * results, unsigned int first,
                                    unsigned int count, int op, double * out);

/* this worker cannot contribute to the pending fetch (a local failure outside the deposits) */
PLL_EXPORT void pllhip_results_poison(pllhip_results_t * results);

/* give a pllhip_eval driver (include/pllhip_eval.h) a result group over `comm` (NULL: this
   process only) sized for its partitions; the driver then reduces its lnL and
   {df, ddf} on the device */
struct pllhip_eval;
PLL_EXPORT int pllhip_eval_attach_comm(struct pllhip_eval * ev, pllhip_comm_t * comm);

/* device time of this thread's last successful pll_compress_site_patterns[_msa] call, in ms between HIP events on the
   call's stream: rows up; the kernels (table set-up, hash, insert, numbering, then gather: two device segments, without
   the host's read of the pattern count and its allocation of the output between them); results down.  Any pointer
   may be NULL.  (tools/gpu_compress.py) */
PLL_EXPORT void pllhip_compress_last_times(double * upload_ms, double * kernel_ms, double * download_ms);
/* work of the hash table in that call: slots passed over (probe steps beyond a site's first slot) and full column
   compares.  With all 64 hash bits the first is about 0.3 per site at most and the second the number of sites that
   joined a group; PLLHIP_COMPRESS_HASH_BITS=0 turns every site's walk into one chain from slot 0. */
PLL_EXPORT void pllhip_compress_last_counts(unsigned long long * probe_steps, unsigned long long * compares);

/* ---- empirical parameters and alignment statistics ("Empirical parameters and alignment
 * statistics") ----
 * What pll-modules' src/msa/pll_msa.c computes on the host, from tips that live on the device: one pass over the
 * tips fills 64-bit integer tables, the host makes the few divisions, so results do not depend on summation order
 * and are the same from run to run.  Arrays are malloc()ed; the caller frees them.
 *
 * Partition forms (any partition of 2 .. 64 states, sharded ones included; only partition->sites patterns count):
 *   frequencies [states]: every character adds w / popcount(mask) to each state of its mask, gaps included; over
 *     sum(w) * tips (pllmod_msa_empirical_frequencies).  Tips set through pll_set_tip_clv with entries other than
 *     0 and 1 add w * v[k] / sum(v) instead: the one floating-point sum, made in a fixed order.
 *   subst_rates [states * (states - 1) / 2]: per column cnt[k] = characters that are no gap and contain k,
 *     pair[i][j] += cnt[i] * cnt[j] * w; over pair[S-2][S-1] (1 if 0), clamped to [0.01, 50], last entry 1
 *     (pllmod_msa_empirical_subst_rates, with the counts reset for every column -- the reference resets half).
 *   invariant_sites: weighted share of invariant[n] > -1 (pll_update_invariant_sites runs if it has not: a column
 *     whose characters share any state, so an all-gap column counts); -INFINITY on failure. */
PLL_EXPORT double * pllhip_empirical_frequencies(pll_partition_t * partition);
PLL_EXPORT double * pllhip_empirical_subst_rates(pll_partition_t * partition);
PLL_EXPORT double pllhip_empirical_invariant_sites(pll_partition_t * partition);

/* Alignment form (pllmod_msa_compute_stats): raw characters and a character -> state map.  Bit values and the
 * result's fields are those of PLLMOD_MSA_STATS_* / pllmod_msa_stats_t (src/msa/pll_msa.h:29-66).  The gap state is
 * the full mask of `states` bits; frequencies ignore gaps; an invariant column is one whose masks' AND has exactly one
 * bit (an all-gap column is not); weights == NULL means 1.  A character that maps to 0 fails the call with
 * PLL_ERROR_MSA_MAP_INVALID, the message naming the first such character in sequence-major order.  A mask that
 * asks only for duplicates is host work and touches no device. */
#define PLLHIP_MSA_STATS_NONE        (0ul)
#define PLLHIP_MSA_STATS_DUP_TAXA    (1ul<<0)
#define PLLHIP_MSA_STATS_DUP_SEQS    (1ul<<1)
#define PLLHIP_MSA_STATS_GAP_PROP    (1ul<<2)
#define PLLHIP_MSA_STATS_GAP_SEQS    (1ul<<3)
#define PLLHIP_MSA_STATS_GAP_COLS    (1ul<<4)
#define PLLHIP_MSA_STATS_INV_PROP    (1ul<<5)
#define PLLHIP_MSA_STATS_INV_COLS    (1ul<<6)
#define PLLHIP_MSA_STATS_FREQS       (1ul<<7)
#define PLLHIP_MSA_STATS_SUBST_RATES (1ul<<8)
#define PLLHIP_MSA_STATS_ALL         (~0ul)

typedef struct pllhip_msa_stats
{
  unsigned int states;

  unsigned long dup_taxa_pairs_count;
  unsigned long * dup_taxa_pairs;      /* (first occurrence, later copy), by first occurrence, then by copy */

  unsigned long dup_seqs_pairs_count;
  unsigned long * dup_seqs_pairs;

  double gap_prop;
  unsigned long gap_seqs_count;
  unsigned long * gap_seqs;
  unsigned long gap_cols_count;
  unsigned long * gap_cols;

  double inv_prop;
  unsigned long inv_cols_count;
  unsigned long * inv_cols;

  double * freqs;
  double * subst_rates;
} pllhip_msa_stats_t;

PLL_EXPORT pllhip_msa_stats_t * pllhip_msa_compute_stats(const pll_msa_t * msa, unsigned int states,
                                                         const pll_state_t * tipmap, const unsigned int * weights,
                                                         unsigned long stats_mask);
PLL_EXPORT void pllhip_msa_destroy_stats(pllhip_msa_stats_t * stats);

/* device time of this thread's last successful statistics call, in ms between HIP events: rows up (alignment form;
   0 for a partition), the kernels (summed over shards).  Any pointer may be NULL.  (tools/gpu_msa_stats.py) */
PLL_EXPORT void pllhip_msa_stats_last_times(double * upload_ms, double * kernel_ms);

/* ---- tree sets: splits, RF distances, bootstrap support ("Split support and tree distances") ----
 * A set of B binary unrooted trees over the same T tips (4 .. 65535), and what pll-modules' src/tree computes from
 * such trees on one host thread: pllmod_utree_split_create, pllmod_utree_split_rf_distance, Felsenstein support and
 * pllmod_utree_tbe_naive.  Integer work on the device; every result is exact and the same from run to run.
 *
 * Tip ids: with labels, the index of a tip's label in `labels` (copied); without, the tip's node_index, which must be
 *   a permutation of 0 .. T-1 (what pllmod_utree_consistency_set arranges).  Trees are only read, and nothing of them
 *   is kept.
 * Split: ceil(T/32) words per inner edge, bit id%32 of word id/32 set for the tips on one side, normalised so that
 *   bit 0 of word 0 is set, unused high bits clear; a tree's T-3 splits ascending by words compared as unsigned, word
 *   0 first (content and order of pllmod_utree_split_create).
 * RF(a, b) = 2 * (T - 3 - common splits).  FBP support of a reference split = trees that hold it / B.
 * TBE support: with p the size of the split's lighter side and delta = min(p - 1, min over the nodes v of a tree of
 *   min(d, T - d)), d = |split xor tips below v|, the support is 1 - sum(delta) / (B * (p - 1)); the sum is a 64-bit
 *   integer and the quotient (B * (p - 1) - sum) / (B * (p - 1)) is rounded once.
 *
 * pllhip_treeset_create and _add touch no device.  The other calls run on the device pllhip_get_device() names, on a
 * stream of their own, and return when done.  PLL_FAILURE / NULL with pll_errno PLL_ERROR_PARAM_INVALID (NULL
 * arguments, T outside 4 .. 65535, a bad index, an empty set, tip ids or labels that are unknown, duplicate or
 * missing), PLL_ERROR_TREE_INVALID (not binary, not T tips), PLL_ERROR_MEM_ALLOC, PLL_ERROR_HIP_NODEVICE,
 * PLL_ERROR_HIP_RUNTIME; a failed call leaves the set as it was.
 * PLLHIP_TREESET_BATCH=<trees> fixes how many trees' splits are built at a time (default: from free device memory);
 * PLLHIP_SPLIT_HASH_BITS=<0..64> keeps that many bits of the split hash.  Neither changes a result. */
typedef struct pllhip_treeset pllhip_treeset_t;

#define PLLHIP_SUPPORT_FBP 0
#define PLLHIP_SUPPORT_TBE 1

PLL_EXPORT pllhip_treeset_t * pllhip_treeset_create(unsigned int tip_count, const char * const * labels);
PLL_EXPORT void pllhip_treeset_destroy(pllhip_treeset_t * ts);
PLL_EXPORT unsigned int pllhip_treeset_count(const pllhip_treeset_t * ts);
PLL_EXPORT int pllhip_treeset_add(pllhip_treeset_t * ts, const pll_utree_t * tree);
/* the (T-3) * ceil(T/32) words of tree `index` */
PLL_EXPORT int pllhip_treeset_splits(pllhip_treeset_t * ts, unsigned int index, unsigned int * out);
/* out [B * B]: symmetric, zero diagonal */
PLL_EXPORT int pllhip_treeset_rf_matrix(pllhip_treeset_t * ts, unsigned int * out);
/* out [B]: RF distance of every tree to `ref` */
PLL_EXPORT int pllhip_treeset_rf_to(pllhip_treeset_t * ts, const pll_utree_t * ref, unsigned int * out);
/* support [T-3]: entry i belongs to the i-th split of `ref` in the order above (the index pllmod_utree_split_create
   gives on the same tree); split_to_node_map [T-3] or NULL: a record of that edge in the caller's tree, so that
   pllmod_utree_draw_support(ref, support, map, NULL) works unchanged */
PLL_EXPORT int pllhip_treeset_support(pllhip_treeset_t * ts, const pll_utree_t * ref, int kind, double * support,
                                      pll_unode_t ** split_to_node_map);
/* the integers behind this thread's last support call: trees that hold split i (FBP) or sum(delta) (TBE).  Copies
   min(count, T-3) of them and returns T-3. */
PLL_EXPORT unsigned int pllhip_treeset_last_sums(unsigned long long * out, unsigned int count);
/* what the host made of tree `index` (host only; csrc/treeset_plan.h): order [T-1] tip ids depth first from tip 0's
   neighbour, lo/hi [T-3] the inner edges as intervals of it, program [2 * (2T-3)] (kind, argument) pairs with kind 0 =
   push tip, 1 = combine the two top entries into a node of `argument` tips, and the deepest stack the program reaches
   (never more than 1 + floor(log2(T))).  Any pointer may be NULL. */
PLL_EXPORT int pllhip_treeset_plan(const pllhip_treeset_t * ts, unsigned int index, unsigned int * order,
                                   unsigned int * lo, unsigned int * hi, unsigned int * program,
                                   unsigned int * max_stack);
/* device time of this thread's last successful tree-set query, in ms between HIP events: plans, programs and the
   reference up; kernels; results down.  Trees added since the last query are brought to the device by the next one
   and count towards it.  pllhip_treeset_last_counts: slots passed over and full bit-vector compares of the split
   table while the last such trees were inserted. */
PLL_EXPORT void pllhip_treeset_last_times(double * upload_ms, double * kernel_ms, double * download_ms);
PLL_EXPORT void pllhip_treeset_last_counts(unsigned long long * probe_steps, unsigned long long * compares);

/* ---- consensus of a tree set ("Split support and tree distances") ----
 * What pllmod_utree_weight_consensus with equal weights computes: threshold 1.0 is the strict consensus, 0.5 majority
 * rule, 0.0 extended majority rule; a value outside [0, 1] fails with PLL_ERROR_PARAM_INVALID, an empty set as every
 * other query does.  With B trees and c the number of trees that hold a split:
 *   need_major  c = B for threshold 1.0; 2c > B for max(threshold, 0.5) = 0.5; otherwise the smallest c for which the
 *               one correctly rounded quotient (double)c / (double)B is greater than the threshold.  Every split with
 *               c >= need_major is in.
 *   need_minor  for a threshold below 0.5 the splits with c / B > threshold (every split for 0.0; the same rounded
 *               comparison) are candidates of the greedy extension: in rank order, each one that is compatible with
 *               everything taken so far is taken, until T-3 splits are held.
 *   rank        c descending, then the bit vector ascending (words as unsigned, word 0 first).  The output is in this
 *               order, in the normal form of pllhip_treeset_splits.  The result is that of the sequential definition,
 *               whatever PLLHIP_CONSENSUS_BLOCK=<1..2048> (candidates per round on the device, default 1024) says.
 * out_words [(T-3) * ceil(T/32)], out_trees [T-3] (c), out_support [T-3] ((double)c / (double)B, rounded once); any may
 * be NULL.  *out_count = K, the number of splits (0 .. T-3).  The arrays are what a pll_split_system_t holds (splits
 * row by row, support, split_count, max_support = 1.0).  pllhip_treeset_last_times covers both calls. */
PLL_EXPORT int pllhip_treeset_consensus(pllhip_treeset_t * ts, double threshold, unsigned int * out_count,
                                        unsigned int * out_words, unsigned int * out_trees, double * out_support);
/* The unrooted, possibly multifurcating tree of that split system, built on the host; destroy it with
   pll_utree_destroy(tree, NULL).  Tips carry the set's labels (none for an unlabelled set) and node_index = clv_index =
   tip id; vroot is tip 0's neighbour; K = 0 gives the star.  The support of a split is the label of the inner node on
   the side of its edge away from tip 0, as the shortest decimal that reads back as the same double (all records of
   the node share the string, as in a cloned tree): pll_utree_export_newick(tree->vroot, NULL) prints it in the place
   of a bootstrap value, and a callback finds it in node->label of every record with node->next != NULL. */
PLL_EXPORT pll_utree_t * pllhip_treeset_consensus_tree(pllhip_treeset_t * ts, double threshold);
/* The same builder for any `count` pairwise compatible, distinct, non-trivial splits in normal form (host only; support
   may be NULL: no inner labels).  NULL with PLL_ERROR_PARAM_INVALID when the splits are not such a system. */
PLL_EXPORT pll_utree_t * pllhip_treeset_tree_from_splits(const pllhip_treeset_t * ts, unsigned int count,
                                                         const unsigned int * words, const double * support);
/* need_major and need_minor of `tree_count` trees (host only) */
PLL_EXPORT int pllhip_consensus_needs(unsigned int tree_count, double threshold, unsigned int * need_major,
                                      unsigned int * need_minor);
/* this thread's last consensus call: splits of the accepted set that candidates were tested against, and pairs of
   candidates of one round tested against each other */
PLL_EXPORT void pllhip_treeset_last_consensus_counts(unsigned long long * accepted_tests, unsigned long long * pair_tests);

/* ---- marginal ancestral states of many nodes ("Ancestral states") ----
 * The value of pll_compute_node_ancestral (scaler counts and p-inv ignored; a site whose sum is 0 keeps an all-zero
 * row), computed into a device staging buffer, plus the summary most callers want per site: states[n] = the smallest
 * state index with the largest probability of row n (0 for an all-zero row), state_probs[n] = that probability --
 * both taken from the very doubles `probs` would hold, so states[n] == argmax(probs[n]) holds exactly.
 * The staging buffer is allocated once per batch; when the entries do not fit PLLHIP_ANC_STAGING_BYTES (environment,
 * read at the call; default 1 GiB, never less than one entry) they go through it in chunks with one wait and one
 * round of copies per chunk.  Results do not depend on the chunk size, nor on PLLHIP_ANC_BLOCKS (environment, read at
 * the call; unset or 0: no cap), a cap on the workgroups of each of its launches that the tests use. */
#define PLLHIP_ANC_PROBS (1u << 0)   /* also return the full sites x states table */

/* One (node, other, matrix) triple per entry, same meaning as the arguments of pll_compute_node_ancestral.
   Enqueues everything, waits once.  states[k], state_probs[k] (and probs[k] with PLLHIP_ANC_PROBS, else probs may be
   NULL) are host arrays of partition->sites (x states) elements per entry. */
PLL_EXPORT int pllhip_node_ancestral_batch(pll_partition_t * partition, unsigned int count,
                                           const unsigned int * node_clv, const unsigned int * other_clv,
                                           const unsigned int * matrix_indices, const unsigned int * freqs_indices,
                                           unsigned int flags,
                                           unsigned char * const * states, double * const * state_probs,
                                           double * const * probs);

/* The same batch entry by entry, for callers whose vectors are not all valid at the same time (a re-rooting loop:
   pllhip_eval_compute_ancestral).  add() prepares both vectors as pll_compute_node_ancestral does and enqueues the
   entry's kernel, which writes into the staging buffer in stream order: whatever the caller enqueues next on the
   partition may overwrite the two vectors.  The host waits only when a staging chunk is full, and in finish().  The
   result arrays of an entry are complete after finish() (a full chunk delivers earlier).  `expected`: the number of
   entries to come, which bounds the staging buffer (0: size it by the budget alone).  After a failed add() no
   further entry is taken; finish() must still be called, releases everything and reports the failure. */
typedef struct pllhip_anc_batch pllhip_anc_batch_t;
PLL_EXPORT pllhip_anc_batch_t * pllhip_node_ancestral_begin(pll_partition_t * partition, unsigned int flags,
                                                            unsigned int expected);
PLL_EXPORT int pllhip_node_ancestral_add(pllhip_anc_batch_t * batch, unsigned int node_clv_index,
                                         unsigned int other_clv_index, unsigned int matrix_index,
                                         const unsigned int * freqs_indices, unsigned char * states,
                                         double * state_probs, double * probs);
PLL_EXPORT int pllhip_node_ancestral_finish(pllhip_anc_batch_t * batch);
/* the batch this thread finished last: device time of its kernels in ms between HIP events (summed over the devices
   of a sharded partition), and its staging chunks (the largest count of any device) */
PLL_EXPORT void pllhip_node_ancestral_last_times(double * kernel_ms, unsigned long long * chunks);

/* ---- site categories: per-site posteriors of the rate categories / mixture components, site rates and the EM fit of
 * the category weights ("Site categories") ----
 * A set holds, on one device, the table of an edge kept per category: for site n and category r
 *     l[n][r] = sum_i pi_r[i] parent[n, r, i] sum_j P_r[i][j] child[n, r, j]      (pi_r, q_r: those of freqs_indices[r])
 * under the scaling and p-inv rules of pll_compute_edge_loglikelihood, as rate part A = (1 - q_r) l, invariant part
 * B = q_r pi_r[invariant[n]] and scaler count c[n]; g = A + B.  With weights w: T[n] = sum_r w_r g[n][r],
 * lnl[n] = log T[n] - c[n] 256 ln 2 (the per-site value of the edge log-likelihood, up to rounding),
 * post[n][r] = w_r A[n][r] / T[n], inv[n] = sum_r w_r B[n][r] / T[n], rate[n] = sum_r post[n][r] rates[r],
 * category[n] = the smallest r with the largest post[n][r] and category_prob[n] that very double,
 * expected[r] = sum_n m_n w_r g[n][r] / T[n] with the pattern weights m.  A site with T[n] = 0 has all-zero rows, rate 0,
 * category 0 and lnl = -inf, and adds nothing to `expected`.
 * The vectors do not depend on the weights, so with the table resident the weights are fitted by EM with no further
 * traversal: w'_r = expected[r] / sum_n m_n, one pass over the table per iteration (the divisor is taken as
 * sum_r expected[r], the same number up to rounding, so that the new weights add up to 1 to `cats` roundings).
 * PLLHIP_SITECAT_BLOCKS (environment, read at the call; unset or 0: no cap) caps the workgroups of every launch of
 * these calls; per-site results do not depend on it, sums are bit-identical from run to run at a given cap. */
typedef struct pllhip_sitecat pllhip_sitecat_t;

/* The table of an edge (arguments as for pll_compute_edge_loglikelihood).  Snapshots the partition's category weights,
   p-inv, rates and pattern weights; owns its buffers on the partition's device and stays valid after the partition has
   changed or gone.  Changes nothing in the partition (vectors that exist as their operation only are stored, as for
   any reader).  NULL on error: NULL arguments, an index out of range, a partition spread over devices. */
PLL_EXPORT pllhip_sitecat_t * pllhip_sitecat_edge(pll_partition_t * partition, unsigned int parent_clv_index,
                                                  int parent_scaler_index, unsigned int child_clv_index,
                                                  int child_scaler_index, unsigned int matrix_index,
                                                  const unsigned int * freqs_indices);
/* A set from a host table g[sites][cats] (non-negative, finite), on the device of pllhip_get_device(): the EM fit and
   the posteriors of any mixture (no invariant parts, no rates: `rate` and `invariant_prob` of its posteriors are NULL).
   pattern_weights NULL: 1 each; weights NULL: 1 / cats each.  At most 256 categories. */
PLL_EXPORT pllhip_sitecat_t * pllhip_sitecat_from_table(unsigned int sites, unsigned int cats, const double * g,
                                                        const unsigned int * pattern_weights, const double * weights);
PLL_EXPORT void pllhip_sitecat_destroy(pllhip_sitecat_t * set);
PLL_EXPORT unsigned int pllhip_sitecat_sites(const pllhip_sitecat_t * set);
PLL_EXPORT unsigned int pllhip_sitecat_categories(const pllhip_sitecat_t * set);
/* rate_part / inv_part [sites][cats] (A and B above), counts [sites]; any may be NULL */
PLL_EXPORT int pllhip_sitecat_table(pllhip_sitecat_t * set, double * rate_part, double * inv_part,
                                    unsigned int * counts);

#define PLLHIP_SITECAT_POSTERIORS (1u << 0)   /* also the full post[sites][cats] */
typedef struct pllhip_site_posteriors
{
  unsigned int sites, cats;
  double * rate;                 /* [sites]; NULL for a set made from a host table */
  unsigned char * category;      /* [sites] */
  double * category_prob;        /* [sites] */
  double * invariant_prob;       /* [sites]; NULL for a set made from a host table */
  double * lnl;                  /* [sites] */
  double * posterior;            /* [sites][cats]; NULL without PLLHIP_SITECAT_POSTERIORS */
  double * expected;             /* [cats] */
  double loglh;                  /* sum_n m_n lnl[n] (-inf if a site with m_n > 0 has T = 0) */
} pllhip_site_posteriors_t;

/* weights NULL: the set's own.  Weights must be finite, non-negative and not all zero.  NULL on error. */
PLL_EXPORT pllhip_site_posteriors_t * pllhip_sitecat_posteriors(pllhip_sitecat_t * set, const double * weights,
                                                                unsigned int flags);
PLL_EXPORT void pllhip_site_posteriors_destroy(pllhip_site_posteriors_t * posteriors);

typedef struct pllhip_sitecat_em_params
{
  const double * start;          /* NULL: the set's own weights */
  double epsilon;                /* stop once an iteration gains less than this in sum_n m_n lnl[n] */
  unsigned int max_iterations;
} pllhip_sitecat_em_params_t;

#define PLLHIP_SITECAT_TRAIL_MAX 64
/* EM on the weights (rates, p-inv and vectors fixed).  Iteration i (from 0) evaluates the table at w_i, which gives
   L_i = sum_n m_n lnl[n] and w_(i+1); it stops at the first i > 0 with L_i - L_(i-1) < epsilon, or at
   i = max_iterations.  Out: weights = w_i, *loglh = L_i, *iterations = i (the updates made).  trail_weights [64][cats]
   and trail_loglh [64] (or NULL) receive w_i and L_i of the first 64 evaluations, the final one included.
   The set's own weights are not changed.  Fails with PLL_ERROR_PARAM_INVALID for a set made from a partition with an
   ascertainment-bias correction (the correction depends on the weights), and when a site with m_n > 0 has T = 0 (the
   message names the site). */
PLL_EXPORT int pllhip_sitecat_em_weights(pllhip_sitecat_t * set, const pllhip_sitecat_em_params_t * params,
                                         double * weights, double * loglh, unsigned int * iterations,
                                         double * trail_weights, double * trail_loglh);
/* this thread's last calls: device time of the table kernel, of the last pllhip_sitecat_posteriors (posterior and
   reduction kernels) and of the last EM fit (all its iterations, host waits included) in ms */
PLL_EXPORT void pllhip_sitecat_last_times(double * table_ms, double * posterior_ms, double * em_ms);

/* ---- substitution mapping: posterior expectations per branch ("Substitution mapping"; DESIGN.md
 * section 31) ----
 * Given the data, the expected joint states at the two ends of an edge (endpoint pairs); from them, on the host
 * (pllhip_substmap_counts, include/pllhip_eval.h), the expected number of a -> b substitutions along the edge and the
 * expected time spent in each state.  Notation of the site-category block above: A[n][r], B[n][r], c[n] and
 * T[n] = sum_r w_r (A + B) are the site-category table of the same edge, q_r and pi_r those of freqs_indices[r], m_n
 * the pattern weights.  For site n, category r, parent-side state i and child-side state j:
 *     s[n][r]       = w_r (1 - q_r) d[n][r] / T[n]     d: the descaling the table applied to l[n][r] -- the rate factor
 *                                                      and, for a site with an invariant term and c > 0, 2^(-256 c) or
 *                                                      0; s = 0 where T[n] = 0
 *     J[n][r][i][j] = s[n][r] pi_r[i] parent[n,r,i] P_r[i][j] child[n,r,j]
 *                     so that sum_ij J[n][r] = post[n][r] = w_r A[n][r] / T[n] up to rounding
 *     F[r][i][j]    = sum_n m_n s[n][r] pi_r[i] parent[n,r,i] child[n,r,j]      (no P: nothing is ever divided by P)
 *     pairs[r][i][j] = F[r][i][j] P_r[i][j]                                     (= sum_n m_n J)
 *     posterior[r]  = sum_ij pairs[r][i][j]
 *     differ[n]     = sum_r sum_(i != j) J[n][r][i][j]
 * differ is summed over the off-diagonal entries themselves (the table of the edge under matrices with a zeroed
 * diagonal), never as 1 - same, which cancels on short branches.  A coded parent contributes parent[n,r,i] = bit i of
 * tipmap[code], a coded child child[n,r,j] = bit j of its mask.  A site with T[n] = 0 adds nothing and has differ = 0;
 * `dropped` counts such sites with m_n > 0.  The invariant component contributes to neither table.  With an
 * ascertainment-bias correction the expectations are those of the OBSERVED sites: nothing is corrected.
 * The call accepts the partitions pllhip_sitecat_edge accepts (not one spread over devices: PLL_ERROR_PARAM_INVALID),
 * changes nothing in the partition (vectors that exist as their operation only are stored, as for any reader), and
 * waits once.  F is summed without floating-point atomics: bit-identical from run to run at a given grid.
 * PLLHIP_SUBSTMAP_BLOCKS (environment, read at the call; unset or 0: no cap) caps the workgroups of the scale kernel
 * and of the pair kernel, whose grid decides the order in which F is summed; differ does not depend on it.  The two
 * table launches of the scale pass obey PLLHIP_SITECAT_BLOCKS, as in pllhip_sitecat_edge (per-site values: no effect
 * on the results); the launches over the matrices and the reduction have fixed grids. */
#define PLLHIP_SUBST_SITES (1u << 0)       /* also differ[sites] */
typedef struct pllhip_edge_pairs
{
  unsigned int states, cats, sites;
  double * F;                    /* [cats][states][states] */
  double * pairs;                /* [cats][states][states] */
  double * posterior;            /* [cats]: sum_ij pairs[r] */
  double * differ;               /* [sites]; NULL without PLLHIP_SUBST_SITES */
  double weight_sum;             /* sum_n m_n */
  unsigned long long dropped;    /* sites with m_n > 0 and T = 0 */
} pllhip_edge_pairs_t;

/* arguments as for pll_compute_edge_loglikelihood; NULL on error: NULL arguments, an index out of range, unknown flags,
   a partition spread over devices */
PLL_EXPORT pllhip_edge_pairs_t * pllhip_substmap_edge(pll_partition_t * partition, unsigned int parent_clv_index,
                                                      int parent_scaler_index, unsigned int child_clv_index,
                                                      int child_scaler_index, unsigned int matrix_index,
                                                      const unsigned int * freqs_indices, unsigned int flags);
PLL_EXPORT void pllhip_edge_pairs_destroy(pllhip_edge_pairs_t * pairs);
/* this thread's last call: device time of the scale pass (both tables and the scale kernel), of the pair kernel and of
   the reduction in ms between HIP events */
PLL_EXPORT void pllhip_substmap_last_times(double * scale_ms, double * pairs_ms, double * reduce_ms);

/* ---- simulated alignments: the parametric bootstrap ("Simulated alignments") ----
 * Replicates of an alignment drawn from the partition's own model -- rate categories and their weights, p-inv and
 * frequencies of params_indices[category], and the transition matrices as pll_update_prob_matrices left them -- along
 * a tree given as edges (parent -> child, matrix).  The distribution is the one the edge log-likelihood evaluates.
 * Every draw is a counter-based number of (seed, replicate, stream, absolute site), stream = 3 + matrix index for an
 * edge: the bytes are a function of (seed, replicate, site, model, tree with its matrix indices, root) alone, not of
 * the order of the edge list, of the site or replicate range a call asks for, of chunks or grids.  Edges that share a
 * matrix index share their draws.
 * The calls change nothing in the partition (no vector, scaler or result); queued matrix requests are flushed first.
 * A sharded partition is served from its first shard's matrices.  Partitions with an ascertainment-bias attribute are
 * refused.  The output goes through a device staging buffer of PLLHIP_SIM_STAGING_BYTES (environment, read at the
 * call; default 1 GiB, never less than one chunk of 1024 sites of every row), in chunks over replicates and site
 * ranges; PLLHIP_SIM_BLOCKS (environment, read at the call; unset or 0: no cap) caps the workgroups of a launch.
 * Results depend on neither. */
#define PLLHIP_SIM_INNER (1u << 0)   /* also return the rows of the inner nodes (the true ancestors) */

typedef struct pllhip_sim_params
{
  unsigned long long seed;
  unsigned long long first_site;     /* absolute number of column 0 */
  unsigned int sites;                /* columns per replicate */
  unsigned int first_replicate;      /* absolute number of replicate 0; first_replicate + replicates <= 2^32 */
  unsigned int replicates;
  unsigned int flags;                /* PLLHIP_SIM_* */
  const char * alphabet;             /* NULL: the output holds state indices; else at least `states` characters and the
                                        output holds alphabet[state] (ready for pll_set_tip_states) */
} pllhip_sim_params_t;

/* Nodes are numbered like CLVs (< partition->tips: a tip), all < node_count; edges in any order; root_node is an inner
   node.  out[replicate][row][site], one byte each, row = node index: partition->tips rows, node_count rows with
   PLLHIP_SIM_INNER (rows of nodes the list does not name are 0xFF).  PLL_ERROR_PARAM_INVALID, with nothing written to
   `out`, for sites or replicates of 0, an index out of range, a list that is not a tree over the nodes it names (a
   node reached twice, a tip used as a parent, a node never reached from the root), a missing tip, an alphabet shorter
   than the states, or an ascertainment-bias attribute. */
PLL_EXPORT int pllhip_simulate_edges(pll_partition_t * partition, const pllhip_sim_params_t * params,
                                     unsigned int root_node, unsigned int edge_count, const unsigned int * parent,
                                     const unsigned int * child, const unsigned int * matrix_indices,
                                     const unsigned int * params_indices, unsigned int node_count, unsigned char * out);
/* The same for a tree walked from `root` (an inner node): rows are clv_index, matrices pmatrix_index, node_count =
   tips + clv_buffers.  update_matrices != 0: every edge's matrix is first requested from its `length`
   (pll_update_prob_matrices with params_indices). */
PLL_EXPORT int pllhip_simulate_utree(pll_partition_t * partition, const pllhip_sim_params_t * params,
                                     const pll_unode_t * root, const unsigned int * params_indices, int update_matrices,
                                     unsigned char * out);
/* this thread's last simulation: device time of the table kernel and of the evolve kernels in ms between HIP events,
   the copies (device to pinned memory, and from there into `out`) in ms, and the staging chunks */
PLL_EXPORT void pllhip_simulate_last_times(double * tables_ms, double * kernel_ms, double * copy_ms,
                                           unsigned long long * chunks);

/* ---- sampled ancestral states ("Sampled ancestral states") ----
 * One coherent draw of all unobserved nodes from their joint posterior given the data: per pattern and replicate a
 * component (rate category, invariant or not) and a state for every node of the edge list, by the process
 * INTEGRATION.md spells out -- the component from the site-category table of the root edge, the root state from both
 * sides of that edge, then every edge downwards from Pr(child = j | parent = a, r, data below) ~ P_r[a][j] child[n,r,j].
 * Draws are those of the simulation contract (stream 0: component, 2: root state, 3 + matrix index: an edge) with the
 * pattern index as the site counter, so the bytes are a function of (seed, replicate, pattern, the doubles the engine
 * holds, the edge list with its matrix indices, the root edge) alone.  The caller guarantees that every named vector
 * points away from its listed parent and root_node's away from other_node: the state after pll_update_partials
 * towards that edge.  Nothing in the partition changes (a vector that exists as its operation or class table only is
 * stored, as for any reader); queued matrix requests are launched first.  An ascertainment attribute is ignored.
 * Environment, read at the call, none of which shows in the results: PLLHIP_ANCS_STAGING_BYTES (device staging buffer,
 * default 1 GiB), PLLHIP_ANCS_REPLICATES (replicates per pass, at most 8), PLLHIP_ANCS_BLOCKS (workgroups, 0: no cap). */
#define PLLHIP_ANCS_TIPS      (1u << 0)   /* tip rows are written too: a state compatible with the tip's code */
#define PLLHIP_ANCS_COMPONENT (1u << 1)   /* fill `component` */

typedef struct pllhip_ancsample_params
{
  unsigned long long seed;
  unsigned int first_replicate;      /* absolute number of replicate 0; first_replicate + replicates <= 2^32 */
  unsigned int replicates;
  unsigned int flags;                /* PLLHIP_ANCS_* */
  const char * alphabet;             /* NULL: state indices; else at least `states` characters.  0xFF stays 0xFF */
} pllhip_ancsample_params_t;

/* Nodes are numbered like CLVs (< partition->tips: a tip), all < node_count; the edge list
   (parent -> child, matrix) is a tree from root_node and holds the edge root_node -> other_node exactly once, with the
   root matrix.  out[replicate][node_count][partition->sites], one byte each: rows not named, and tip rows without
   PLLHIP_ANCS_TIPS, hold 0xFF.  component[replicate][sites] (with PLLHIP_ANCS_COMPONENT, else ignored): r, or 0x80 | r
   for an invariant draw, on which every row holds invariant[site].  A site whose table total is not > 0 or not finite
   is dropped: 0xFF in every row and in `component`; *dropped (may be NULL) counts those with a pattern weight, once.
   PLL_ERROR_PARAM_INVALID, with nothing written: NULLs, zero replicates, unknown flags, an index out of range, a list
   simplan rejects (a node reached twice, a tip as a parent, a node never reached), no or several root edges in the
   list, a tip as root_node, a short alphabet, a sharded partition, weights that are negative, not finite or all 0, a
   vector that cannot be stored beside the others. */
PLL_EXPORT int pllhip_sample_ancestral_edges(pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                                             unsigned int root_node, int root_scaler, unsigned int other_node,
                                             int other_scaler, unsigned int edge_count, const unsigned int * parent,
                                             const unsigned int * child, const unsigned int * matrix_indices,
                                             const unsigned int * freqs_indices, unsigned int node_count,
                                             unsigned char * out, unsigned char * component,
                                             unsigned long long * dropped);
/* The same for a tree walked from `root` (an inner node; the root edge is root -- root->back): rows are clv_index,
   matrices pmatrix_index, scalers scaler_index, node_count = tips + clv_buffers.  Touches neither matrices nor vectors. */
PLL_EXPORT int pllhip_sample_ancestral_utree(pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                                             const pll_unode_t * root, const unsigned int * freqs_indices,
                                             unsigned char * out, unsigned char * component,
                                             unsigned long long * dropped);
/* this thread's last call: device time of the table kernel and of the walk kernels in ms between HIP events, the
   copies (device to pinned memory, and from there into `out`) in ms, and the staging chunks */
PLL_EXPORT void pllhip_ancsample_last_times(double * table_ms, double * kernel_ms, double * copy_ms,
                                            unsigned long long * chunks);

/* ---- sampled substitution histories ("Sampled substitution histories") ----
 * Stochastic mapping: after the ancestral draw above, a path of substitutions along every edge, drawn by
 * uniformization conditioned on the sampled component and the sampled states at both ends of the edge -- a jump count
 * from the Poisson table of (matrix, category) weighted by Rpow[k][a][c], a chain of states through the uniformized
 * matrix R, and event times from the order statistics of 32-bit draws.  The tables come from the host stage
 * (include/pllhip_eval.h, pllhip_history_*), built from branch_lengths[edge] -- the lengths the caller promises the
 * matrices were made from -- and the model of params_indices[category].  Draws are those of the simulation contract on
 * the streams 0x40000000 + (matrix << 11) + i (i = 0: jump count, 1 .. 1023: chain steps) and + 1024 + i (event
 * times).  Every accumulated number is a 64-bit integer, so all outputs are a function of (seed, replicate, pattern,
 * the doubles the engine holds and the tables, the edge list with its matrix indices and lengths) alone.
 * counts[replicate][edge][states][states]: pattern-weighted number of a -> b substitutions.
 * units[replicate][edge][cats][states]: pattern-weighted time in a state under category r, in units of 2^-32 tau_r
 *   (two's complement; every final cell is >= 0).  pllhip_history_summary turns both into doubles.
 * changes[replicate][edge][sites] (with PLLHIP_HIST_SITES, else ignored): substitutions of the site on the edge,
 *   saturating at 254; 0xFF: the site, or this edge of it, was dropped.
 * dropped_edges[replicate][edge]: sites with a pattern weight whose jump-count table had no mass (the sampled ends
 *   cannot be joined within the table), which add nothing.  Edges are in the order of the caller's list.
 * out, component (either may be NULL) hold what pllhip_sample_ancestral_edges returns for the same seed and flags.
 * PLL_ERROR_PARAM_INVALID with nothing written: whatever pllhip_sample_ancestral_edges refuses, a NULL, negative or
 * non-finite length, a Poisson table of more than 1024 entries (mu tau of roughly 760 and more), a matrix index of 2^19
 * or more, pattern weights that add up to 2^31 or more, unknown flags.  The partition is left as it was.
 * Environment, read at the call, none of which shows in the results: PLLHIP_HIST_BLOCKS (workgroups of the history
 * kernel, 0: no cap), PLLHIP_HIST_REPLICATES (replicates per staging chunk, 0: no cap), and the PLLHIP_ANCS_* above. */
#define PLLHIP_HIST_SITES (1u << 8)       /* fill `changes` */
#define PLLHIP_HIST_MAX_TABLE 1024u       /* entries of a Poisson table, at most */

PLL_EXPORT int pllhip_sample_histories_edges(pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                                             unsigned int root_node, int root_scaler, unsigned int other_node,
                                             int other_scaler, unsigned int edge_count, const unsigned int * parent,
                                             const unsigned int * child, const unsigned int * matrix_indices,
                                             const unsigned int * freqs_indices, unsigned int node_count,
                                             const unsigned int * params_indices, const double * branch_lengths,
                                             unsigned char * out, unsigned char * component,
                                             unsigned long long * dropped, unsigned long long * counts,
                                             unsigned long long * units, unsigned char * changes,
                                             unsigned long long * dropped_edges);
/* The same for a tree walked from `root`: the edge list of pllhip_sample_ancestral_utree in its order, which is the
   order of counts, units, changes and dropped_edges (*edge_count receives its length and edge_matrix[tips +
   clv_buffers] the pmatrix_index of every edge; either may be NULL), lengths from node->length. */
PLL_EXPORT int pllhip_sample_histories_utree(pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                                             const pll_unode_t * root, const unsigned int * freqs_indices,
                                             const unsigned int * params_indices, unsigned char * out,
                                             unsigned char * component, unsigned long long * dropped,
                                             unsigned long long * counts, unsigned long long * units,
                                             unsigned char * changes, unsigned long long * dropped_edges,
                                             unsigned int * edge_count, unsigned int * edge_matrix);
/* this thread's last call: device time of the site-category table, of the walk kernels and of the history kernels in
   ms between HIP events, and the copies in ms */
PLL_EXPORT void pllhip_history_last_times(double * table_ms, double * walk_ms, double * history_ms, double * copy_ms);

/* ---- topology tests and bootstrap weights ("Topology tests and bootstrap weights"; DESIGN.md
 *      section 20) ----
 * A site-likelihood set holds, on the device pllhip_get_device() names at its creation, a matrix L[trees][patterns]
 * of per-pattern log-likelihoods -- unweighted, what `persite_lnl` of pll_compute_edge_loglikelihood holds -- and the
 * pattern weights w (NULL: all 1).  `patterns` is the caller's concatenation of all partitions.  The ascertainment
 * correction is not a per-site quantity and is in no row. */
typedef struct pllhip_sitelh pllhip_sitelh_t;
PLL_EXPORT pllhip_sitelh_t * pllhip_sitelh_create(unsigned int patterns, const unsigned int * weights);
PLL_EXPORT void pllhip_sitelh_destroy(pllhip_sitelh_t * set);
PLL_EXPORT unsigned int pllhip_sitelh_count(const pllhip_sitelh_t * set);
/* row `tree` -> out[patterns] */
PLL_EXPORT int pllhip_sitelh_get(pllhip_sitelh_t * set, unsigned int tree, double * out);
/* appends row[patterns] from the host; returns the tree index, or -1 (PLL_ERROR_PARAM_INVALID for a non-finite value) */
PLL_EXPORT int pllhip_sitelh_add(pllhip_sitelh_t * set, const double * row);
/* pll_compute_edge_loglikelihood of `partition` with its partition->sites per-pattern values left in row `tree` at
   `offset`, device to device (through the host for a sharded partition or one on another device).  tree == count opens
   a new row, whose other patterns are 0 until written.  *lnl (may be NULL) = the value the edge function returns, the
   ascertainment correction included; the row does not hold that correction.  A non-finite value written this way is
   found when the set is used: pllhip_sitelh_rell then fails and names row and pattern. */
PLL_EXPORT int pllhip_sitelh_add_edge(pllhip_sitelh_t * set, unsigned int tree, unsigned int offset,
                                      pll_partition_t * partition, unsigned int parent_clv_index,
                                      int parent_scaler_index, unsigned int child_clv_index, int child_scaler_index,
                                      unsigned int matrix_index, const unsigned int * freqs_indices, double * lnl);

#define PLLHIP_RELL_REPLICATES (1u << 0)   /* also return the replicates x trees matrix of replicate log-likelihoods */

typedef struct pllhip_rell_params
{
  unsigned int replicates;      /* B, 1 .. 2^24 - 1 */
  unsigned long long seed;
  unsigned int flags;
  unsigned int batch;           /* replicates per pass (rounded up to 16); 0: chosen from the free device memory */
} pllhip_rell_params_t;

/* Replicate b draws N = sum of w patterns with the counter-based generator INTEGRATION.md defines (N < 2^40);
   R[b][t] = sum_s C[b][s] L[t][s].  lnl[t] = sum_s w[s] L[t][s]; best = argmax lnl (lowest index on ties);
   bp_count / kh_count / sh_count = numerators of the RELL bootstrap proportion and of the one-sided KH and the SH
   p-values (denominator: replicates); elw = expected likelihood weights.  R, and with it every field, is bit-identical
   across runs and across `batch`. */
typedef struct pllhip_rell_result
{
  unsigned int trees;
  unsigned int replicates;
  unsigned int best;
  unsigned int batch;           /* the batch used */
  double * lnl;                 /* [trees] */
  unsigned int * bp_count;      /* [trees] */
  unsigned int * kh_count;      /* [trees] */
  unsigned int * sh_count;      /* [trees] */
  double * elw;                 /* [trees] */
  double * replicate_lnl;       /* [replicates][trees] with PLLHIP_RELL_REPLICATES, else NULL */
} pllhip_rell_result_t;

PLL_EXPORT pllhip_rell_result_t * pllhip_sitelh_rell(pllhip_sitelh_t * set, const pllhip_rell_params_t * params);
PLL_EXPORT void pllhip_rell_destroy(pllhip_rell_result_t * result);
/* the last pllhip_sitelh_rell of this thread: device time of its stages in ms between HIP events */
PLL_EXPORT void pllhip_rell_last_times(double * draw_ms, double * product_ms, double * stats_ms);

/* the count vectors of replicates first .. first + count - 1 for (weights, seed) -- the very vectors
   pllhip_sitelh_rell uses -- as out[count][patterns], each ready for pll_set_pattern_weights; weights NULL: all 1 */
PLL_EXPORT int pllhip_bootstrap_weights(const unsigned int * weights, unsigned int patterns, unsigned long long seed,
                                        unsigned int first, unsigned int count, unsigned int * out);

/* The approximately unbiased (AU) test from multiscale bootstrap replicates ("Multiscale replicates
   and the AU test").  Scale k draws n_k = floor(r_k N + 0.5) sites per replicate from a stream
   of its own; bp_count[k][t] counts the replicates of scale k that tree t wins; per tree, z_k = -Phi^-1(bp_count / B)
   is fitted by d sqrt(n_k / N) + c / sqrt(n_k / N) with weighted least squares over the scales with
   0 < bp_count < B, and p_au = 1 - Phi(d - c).  With fewer than two such scales no fit is made: d = c = se = rss = 0
   and p_au is the proportion of the scale whose n_k is nearest to N.  Every field is bit-identical across runs and
   across `batch`. */
#define PLLHIP_AU_REPLICATES (1u << 0)   /* also return R[scales][replicates][trees] */

typedef struct pllhip_au_params
{
  unsigned int replicates;        /* B per scale, 1 .. 2^24 - 1 */
  unsigned int scales;            /* K, 2 .. 64; ignored when scale == NULL (then 10) */
  const double * scale;           /* r_k, or NULL: 0.5, 0.6, ... 1.4 */
  unsigned long long seed;
  unsigned int flags;
  unsigned int batch;             /* rows (scale, replicate) per pass, as in pllhip_rell_params_t */
} pllhip_au_params_t;

typedef struct pllhip_au_result
{
  unsigned int trees, replicates, scales, best, batch;
  double * lnl;                   /* [trees] */
  unsigned long long * draws;     /* [scales]  n_k */
  unsigned int * bp_count;        /* [scales][trees] */
  double * p_au, * d, * c, * se, * rss;   /* [trees] */
  unsigned int * used;            /* [trees]  scales with 0 < bp_count < B */
  double * replicate_lnl;         /* [scales][replicates][trees] with PLLHIP_AU_REPLICATES, else NULL */
} pllhip_au_result_t;

PLL_EXPORT pllhip_au_result_t * pllhip_sitelh_au(pllhip_sitelh_t * set, const pllhip_au_params_t * params);
PLL_EXPORT void pllhip_au_destroy(pllhip_au_result_t * result);
/* the last pllhip_sitelh_au of this thread: device time of its stages in ms between HIP events (stats = proportions
   and fit) */
PLL_EXPORT void pllhip_au_last_times(double * draw_ms, double * product_ms, double * stats_ms);

/* the count vectors of replicates first .. first + count - 1 of scale `scale_index` (< 64) with `draws` = n_k draws each,
   for (weights, seed) -- the very vectors pllhip_sitelh_au uses -- as out[count][patterns] */
PLL_EXPORT int pllhip_multiscale_weights(const unsigned int * weights, unsigned int patterns, unsigned long long seed,
                                         unsigned int scale_index, unsigned long long draws,
                                         unsigned int first, unsigned int count, unsigned int * out);

/* ---- pairwise distances and neighbour joining ("Pairwise distances and neighbour joining";
 *      DESIGN.md section 23) ----
 * Every character becomes a code: its state where its mask has exactly one bit, "nothing" otherwise (gaps and
 * ambiguities: pairwise deletion).  N[i][j][a][b] = sum over sites of w * [code_i = a] * [code_j = b], 32-bit integers
 * made by an integer matrix product, so they are exact and the same from run to run; n_ij = sum over a, b of N_ij is
 * the number of compared sites.  Distances (fp64, symmetric, zero diagonal) come from the counts:
 *   PLLHIP_DIST_P    (n - tr N) / n
 *   PLLHIP_DIST_JC   -b log(1 - p / b), b = (S - 1) / S; max_dist where p >= b
 *   PLLHIP_DIST_ML   (partition form) the maximiser over [min_dist, max_dist] of
 *                    sum_ab N_ab log(pi_a ((1 - pinv) sum_r w_r P^r_ab(t) + pinv [a = b])), P^r(t) what
 *                    pll_update_prob_matrices gives for length t and rate r with parameter set 0; within
 *                    1e-8 d + 1e-10 of the exact maximiser
 * A pair without a compared site gets max_dist and is counted (pllhip_distmat_no_overlap).  The calls fail with
 * PLL_ERROR_PARAM_INVALID for a sharded partition, a tip vector with an entry other than 0 and 1, a sum of weights of
 * 2^31 or more, PLLHIP_DIST_ML with more than one rate matrix, and PLLHIP_DIST_KEEP_COUNTS where the whole table
 * exceeds the budget; a character that maps to 0 fails as in pllhip_msa_compute_stats. */
#define PLLHIP_DIST_P  0
#define PLLHIP_DIST_JC 1
#define PLLHIP_DIST_ML 2
#define PLLHIP_DIST_KEEP_COUNTS (1u << 0)   /* keep N on the device for pllhip_distmat_counts */

typedef struct pllhip_dist_params
{
  int method;                      /* PLLHIP_DIST_* */
  unsigned int flags;
  double min_dist;                 /* 0: 1e-6 */
  double max_dist;                 /* 0: 10 */
  unsigned long long budget_bytes; /* device memory for one band of counts; 0: PLLHIP_DIST_BUDGET_MB or 1 GiB */
  unsigned int chunk_columns;      /* staged columns per workgroup (rounded up to 64); 0: chosen from the shape */
} pllhip_dist_params_t;

typedef struct pllhip_distmat pllhip_distmat_t;

PLL_EXPORT pllhip_distmat_t * pllhip_distances_partition(pll_partition_t * partition,
                                                         const pllhip_dist_params_t * params);
/* raw characters and a character -> state map; weights NULL: all 1; PLLHIP_DIST_P and PLLHIP_DIST_JC only */
PLL_EXPORT pllhip_distmat_t * pllhip_distances_msa(const pll_msa_t * msa, unsigned int states,
                                                   const pll_state_t * tipmap, const unsigned int * weights,
                                                   const pllhip_dist_params_t * params);
/* matrix[T][T], finite, T >= 3; only neighbour joining reads it (no counts, compared = 0) */
PLL_EXPORT pllhip_distmat_t * pllhip_distmat_from_host(unsigned int T, const double * matrix);
PLL_EXPORT void pllhip_distmat_destroy(pllhip_distmat_t * dm);
PLL_EXPORT unsigned int pllhip_distmat_size(const pllhip_distmat_t * dm);
PLL_EXPORT int pllhip_distmat_get(const pllhip_distmat_t * dm, double * out /* [T][T] */);
PLL_EXPORT int pllhip_distmat_compared(const pllhip_distmat_t * dm, unsigned int * out /* [T][T]: n_ij */);
/* N_ij -> out[S][S]; needs PLLHIP_DIST_KEEP_COUNTS */
PLL_EXPORT int pllhip_distmat_counts(const pllhip_distmat_t * dm, unsigned int i, unsigned int j, int * out);
PLL_EXPORT unsigned long long pllhip_distmat_no_overlap(const pllhip_distmat_t * dm);
/* Neighbour joining on the device by the rules of INTEGRATION.md (tests/nj_reference.py restates them): the join
 * order is a function of the matrix alone.  Tips carry clv_index = taxon index and labels[i] (NULL: no labels);
 * negative lengths are clamped to 0 in the tree only.  T = 3 gives the star. */
PLL_EXPORT pll_utree_t * pllhip_distmat_nj(pllhip_distmat_t * dm, const char * const * labels);
/* the joins of that run (made on demand): T - 3 rounds (slot i, slot j, l_i, l_j), then the last three slots and
 * their lengths: slots[2 (T - 3) + 3], lengths[2 (T - 3) + 3], not clamped */
PLL_EXPORT int pllhip_distmat_nj_joins(pllhip_distmat_t * dm, unsigned int * slots, double * lengths);
/* this thread's last distance / neighbour-joining calls, in ms: rows and site list up, the code kernel, the integer
 * product, the distance kernels (between HIP events); neighbour joining (host clock, its launches included) */
PLL_EXPORT void pllhip_distances_last_times(double * upload_ms, double * codes_ms, double * counts_ms,
                                            double * estimate_ms, double * nj_ms);

#ifdef __cplusplus
}
#endif

#endif /* PLLHIP_H_INCLUDED */
