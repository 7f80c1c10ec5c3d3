/*
 * pllhip_eval.h -- a small C driver on top of include/pll.h for machines where
 * pll-modules itself is not available (the GPU box): tree + partitions +
 * validity flags -> likelihood evaluations and Newton-Raphson branch-length
 * optimisation, issuing the same libpll call sequences as the reference's
 * upper layers.  It is NOT a re-implementation of pll-modules: clients that
 * have pll-modules link it unchanged against libpll_hip.so (INTEGRATION.md,
 * tests/test_dropin_modules.py); this driver exists so that those call
 * patterns can be exercised, tested and timed where the reference cannot go.
 *
 * What each entry point mirrors (behaviour, not code):
 *   pllhip_eval_loglh              treeinfo_compute_loglh, src/tree/treeinfo.c:946-1079
 *                                  (full / partial post-order traversal, per-partition
 *                                  loop that skips NULL = remote partitions, SUM reduce)
 *   pllhip_eval_invalidate_*       src/tree/treeinfo.c:872-944 (one CLV slot per inner
 *                                  node: validating one direction invalidates the other two)
 *   pllhip_eval_optimize_branches  pllmod_opt_optimize_branch_lengths_local_multi with
 *                                  linked branch lengths and PLLMOD_OPT_BLO_NEWTON_FAST,
 *                                  src/optimize/pll_optimize.c:1395-1951; Newton-Raphson
 *                                  step rule of pllmod_opt_minimize_newton_multi,
 *                                  src/optimize/opt_algorithms.c:133-261
 *   pllhip_eval_spr_round          pllmod_algo_spr_round, src/algorithm/algo_search.c:1052-1484
 * One deliberate difference: P-matrix updates of an evaluation go out in one
 * pll_update_prob_matrices call per partition (count = number of invalid
 * branches) unless PLLHIP_EVAL_PMATRIX_PER_BRANCH is set, which reproduces the
 * reference's one-call-per-branch pattern (src/tree/treeinfo.c:845-865).
 */
#ifndef PLLHIP_EVAL_H_INCLUDED
#define PLLHIP_EVAL_H_INCLUDED

#include "pll.h"
#include "pllhip.h"   /* pllhip_site_posteriors_t */

#ifdef __cplusplus
extern "C" {
#endif

#define PLLHIP_EVAL_PMATRIX_PER_BRANCH (1 << 0)
/* Newton-Raphson trial lengths.  The reference evaluates the current iterate per sumtable
   scan (src/optimize/pll_optimize.c:1223-1287).  Where a scan evaluates several lengths
   at the price of one (pllhip_free_trial_lengths() of EVERY partition of every worker,
   agreed through one MIN reduce) the driver also evaluates the iterates the step rule can
   produce by CLAMPING (+-dxmax, the bracket ends: known before the derivatives are), and
   an iteration whose point was already evaluated costs no scan.  The iterate sequence
   and every result are bit-identical either way.
   NO_SPECULATION: never; ALWAYS_SPECULATE: even where extra lengths cost time (tests). */
#define PLLHIP_EVAL_NO_SPECULATION     (1 << 1)
#define PLLHIP_EVAL_ALWAYS_SPECULATE   (1 << 2)

#define PLLHIP_EVAL_RADIUS_ALL (-1)   /* PLLMOD_OPT_BRLEN_OPTIMIZE_ALL, src/optimize/pll_optimize.h:102 */

/* error codes of the reference's optimiser that this driver reports
   (src/optimize/pll_optimize.h:88-99) */
#define PLLHIP_EVAL_ERROR_NEWTON_DERIV 2210
#define PLLHIP_EVAL_ERROR_NEWTON_LIMIT 2220
#define PLLHIP_EVAL_ERROR_NEWTON_WORSE 2240

/* branch-length linkage across partitions (PLLMOD_COMMON_BRLEN_*, src/pllmod_common.h:25-27):
   LINKED    one length per branch, the tree's;
   SCALED    the tree's length times a per-partition scaler (src/tree/treeinfo.c:849-852,
             chain rule in the derivatives: src/optimize/pll_optimize.c:1240-1262);
   UNLINKED  every partition has its own length per branch (src/tree/treeinfo.c:176-183);
             Newton-Raphson then runs one function per partition with its own bracket and
             convergence flag (src/optimize/opt_algorithms.c:133-261), the lengths of
             partitions other workers own arrive through a MAX reduce
             (src/optimize/pll_optimize.c:1431-1442). */
#define PLLHIP_EVAL_BRLEN_LINKED   0
#define PLLHIP_EVAL_BRLEN_SCALED   1
#define PLLHIP_EVAL_BRLEN_UNLINKED 2

typedef struct pllhip_eval pllhip_eval_t;

typedef void (*pllhip_reduce_fn)(void * ctx, double * data, size_t n, int op);

/* `tree` is borrowed (not destroyed); its records need unique node_index values
   (as produced by pll_utree_parse_newick* / pll_utree_reset_template_indices) */
PLL_EXPORT pllhip_eval_t * pllhip_eval_create(pll_utree_t * tree, unsigned int partition_count,
                                              unsigned int flags);
PLL_EXPORT void pllhip_eval_destroy(pllhip_eval_t * ev);

/* partition == NULL marks a partition that another worker owns */
PLL_EXPORT int pllhip_eval_set_partition(pllhip_eval_t * ev, unsigned int index,
                                         pll_partition_t * partition,
                                         const unsigned int * params_indices);

PLL_EXPORT void pllhip_eval_set_parallel_context(pllhip_eval_t * ev, void * ctx,
                                                 pllhip_reduce_fn reduce_cb);

/* Deferred scalar results (include/pllhip.h, pllhip_results_*): with such a table the
   driver enqueues the edge log-likelihoods / derivative scans of ALL its partitions,
   then fetches once -- one wait per evaluation or Newton-Raphson round instead of one per
   partition, and the sum over the workers happens on the device (RCCL) inside the fetch.
   It replaces the reduce callback for these two reductions.  The driver owns `results`
   and calls destroy() on it.  libpll_hip.so provides pllhip_eval_attach_comm() to fill
   this in; the table keeps this driver free of device code. */
typedef struct pllhip_eval_fused
{
  void * results;
  int (*edge_loglikelihood)(void * results, unsigned int slot, pll_partition_t * partition,
                            unsigned int parent_clv_index, int parent_scaler_index,
                            unsigned int child_clv_index, int child_scaler_index,
                            unsigned int matrix_index, const unsigned int * freqs_indices);
  int (*derivatives)(void * results, unsigned int slot, pll_partition_t * partition,
                     int parent_scaler_index, int child_scaler_index,
                     const double * branch_lengths, unsigned int count,
                     const unsigned int * params_indices, const double * sumtable);
  int (*fetch)(void * results, unsigned int first, unsigned int count, int op, double * out);
  void (*destroy)(void * results);
  /* a local failure before the fetch (this worker could not compute or enqueue its part): the next fetch
     contributes NaN and reports failure, so that all workers fail in the same call instead of one of them
     leaving the others inside the collective.  May be NULL. */
  void (*poison)(void * results);
} pllhip_eval_fused_t;

PLL_EXPORT void pllhip_eval_set_fused(pllhip_eval_t * ev, const pllhip_eval_fused_t * fused);

/* linkage mode (default LINKED).  UNLINKED copies the tree's current lengths into every
   partition's own array, like pllmod_treeinfo_create does (src/tree/treeinfo.c:1266-1277). */
PLL_EXPORT int pllhip_eval_set_brlen_linkage(pllhip_eval_t * ev, int linkage);
PLL_EXPORT int pllhip_eval_set_brlen_scaler(pllhip_eval_t * ev, unsigned int partition, double scaler);
PLL_EXPORT double pllhip_eval_get_brlen_scaler(const pllhip_eval_t * ev, unsigned int partition);
/* the length partition `partition` sees on `edge` before scaling: its own (UNLINKED) or the tree's */
PLL_EXPORT double pllhip_eval_get_partition_branch_length(const pllhip_eval_t * ev, unsigned int partition,
                                                          const pll_unode_t * edge);
/* UNLINKED only (src/tree/treeinfo.c:456-472) */
PLL_EXPORT int pllhip_eval_set_partition_branch_length(pllhip_eval_t * ev, unsigned int partition,
                                                       const pll_unode_t * edge, double length);

PLL_EXPORT int pllhip_eval_set_root(pllhip_eval_t * ev, pll_unode_t * root);
PLL_EXPORT pll_unode_t * pllhip_eval_root(const pllhip_eval_t * ev);

PLL_EXPORT void pllhip_eval_invalidate_all(pllhip_eval_t * ev);
PLL_EXPORT void pllhip_eval_invalidate_pmatrix(pllhip_eval_t * ev, const pll_unode_t * edge);
PLL_EXPORT void pllhip_eval_invalidate_clv(pllhip_eval_t * ev, const pll_unode_t * node);

/* log-likelihood at the current root edge; incremental != 0 recomputes only
   invalid P-matrices and CLVs.  NaN on error (pll_errno set). */
PLL_EXPORT double pllhip_eval_loglh(pllhip_eval_t * ev, int incremental);

/* Evaluate-only traversals (include/pllhip.h, pllhip_set_transient) for FULL evaluations -- the call the
   reference's model-parameter optimisers make after every parameter change
   (pllmod_treeinfo_compute_loglh(treeinfo, 0): src/algorithm/algo_callback.c:338, 465, 568, 678;
   nmax + 1 of them per L-BFGS-B iteration: src/optimize/opt_algorithms.c:734-773).  A full evaluation declares
   every vector invalid first, so what an earlier one did not store is given up (pllhip_discard_transient), and
   the vectors inside the operation chains of this one stay in registers.  Whatever reads a vector later
   (an incremental evaluation from another root, a branch-length optimisation, an SPR round) gets it recomputed on
   demand: results are bit-identical in every mode.
     OFF   never (default: pll_update_partials stores every vector, like the reference)
     ON    every full evaluation
     AUTO  a full evaluation that directly follows a full evaluation (the optimiser pattern) */
#define PLLHIP_EVAL_TRANSIENT_OFF  0
#define PLLHIP_EVAL_TRANSIENT_ON   1
#define PLLHIP_EVAL_TRANSIENT_AUTO 2
PLL_EXPORT void pllhip_eval_set_transient(pllhip_eval_t * ev, int mode);

/* change a branch length and invalidate what depends on it */
PLL_EXPORT void pllhip_eval_set_branch_length(pllhip_eval_t * ev, pll_unode_t * edge, double length);

/* returns the NEGATIVE log-likelihood after optimisation (like the reference);
   CLVs need not be valid on entry.  0 on error. */
PLL_EXPORT double pllhip_eval_optimize_branches(pllhip_eval_t * ev, double min_brlen, double max_brlen,
                                                double lh_epsilon, int max_iters, int radius);

/* work counters: operations and P-matrices handed to libpll so far */
/* ---------------------------------------------------------------------------
 * One SPR round: the counterpart of pllmod_algo_spr_round
 * (src/algorithm/algo_search.c:1052-1484, linked branch lengths, no topological
 * constraint, incremental CLV updates) on this driver, for machines where
 * pll-modules cannot go.  Same decision procedure, so the same moves on the same
 * data:
 *   scan   every inner record p, in the reference's post-order (algo_search.c:94-121),
 *          is pruned and scored at every branch within [radius_min, radius_max]
 *          of the pruning point (breadth-first, descent stopped by the lnL cutoff;
 *          algo_search.c:603-899).  A placement that beats the current best by
 *          more than 1e-6 is applied at once and remembered for undo; otherwise
 *          it competes for the list of the ntopol_keep (x3 in fast mode) best
 *          placements (algo_search.c:905-1050).
 *   rescore all branches are optimised (smoothings/4 passes), then every
 *          remembered topology -- applied moves undone one by one, listed
 *          placements re-applied -- gets the same optimisation; the best one
 *          (by more than 0.01 lnL units) is restored (algo_search.c:1233-1445).
 * The reference's second, "thorough" scan of the listed nodes in fast mode is
 * unreachable there (its guard reads a counter that is never advanced,
 * algo_search.c:1193) and is therefore not built.
 * Returns the final log-likelihood (checked against a full re-evaluation to 1e-6,
 * algo_search.c:1453-1457); 0 on error (pll_errno set).
 * ------------------------------------------------------------------------- */
typedef struct pllhip_spr_params
{
  unsigned int radius_min;          /* >= 1 */
  unsigned int radius_max;
  unsigned int ntopol_keep;
  int thorough;                     /* optimise the three branches at every insertion */
  double bl_min, bl_max;
  int smoothings;
  double epsilon;                   /* lnL epsilon of the whole-tree optimisations */
  double subtree_cutoff;            /* multiplier of the average lnL loss -> next round's cutoff */
  double lh_epsilon_brlen_triplet;
} pllhip_spr_params_t;

/* carried from round to round (cutoff_info_t, src/algorithm/pllmod_algorithm.h:41-47) */
typedef struct pllhip_spr_cutoff
{
  double lh_start;
  double lh_cutoff;
  double lh_dec_sum;
  int lh_dec_count;
} pllhip_spr_cutoff_t;

#define PLLHIP_SPR_LOG_MAX 256

typedef struct pllhip_spr_stats
{
  unsigned long prunings;           /* subtrees pruned and scanned */
  unsigned long insertions;         /* placements scored */
  unsigned long moves_applied;      /* improving moves applied during the scan */
  unsigned long rescored;           /* topologies that got a whole-tree optimisation */
  double lnl_start, lnl_scan, lnl_final;
  unsigned int log_count;           /* applied moves, in order: node_index of p and of r */
  unsigned int log_prune[PLLHIP_SPR_LOG_MAX];
  unsigned int log_regraft[PLLHIP_SPR_LOG_MAX];
} pllhip_spr_stats_t;

PLL_EXPORT double pllhip_eval_spr_round(pllhip_eval_t * ev, const pllhip_spr_params_t * params,
                                        pllhip_spr_cutoff_t * cutoff, pllhip_spr_stats_t * stats);

/* ---------------------------------------------------------------------------
 * Marginal ancestral states of every inner node: the counterpart of pllmod_treeinfo_compute_ancestral
 * (src/tree/treeinfo.c:1611-1718) on this driver.  Node order is the reference's: a full post-order
 * pll_utree_traverse from the tree's vroot, inner nodes kept, so probs[i] lines up element for element with
 * pllmod_ancestral_t::probs[i].  The driver's own tree is used (no clone, no labels invented); per node the root is
 * set to the node's record, the invalid P-matrices and vectors of that root are computed, and the triple
 * (node->clv_index, node->back->clv_index, node->pmatrix_index) of every local partition gives the node's rows.
 * The root is restored before returning.
 * Per site: states = the smallest state index with the largest probability (0 for an all-zero row), state_probs =
 * that probability; with PLLHIP_ANC_PROBS (include/pllhip.h) also the full table.  Scaler counts and p-inv are
 * ignored, as pll_compute_node_ancestral ignores them.
 * On the HIP engine every entry goes through pllhip_node_ancestral_begin / _add / _finish: the host never waits
 * between nodes, only once per staging chunk.  Where the library has no such call (the CPU oracle) the driver calls
 * pll_compute_node_ancestral per node and partition and derives the summary on the host by the same rule.
 * NULL on error (pll_errno set; everything freed, the root restored).
 * ------------------------------------------------------------------------- */
typedef struct pllhip_ancestral
{
  unsigned int node_count;             /* inner nodes of the tree */
  unsigned int partition_count;        /* local (non-NULL) partitions */
  pll_unode_t ** nodes;                /* records of the driver's tree, in the reference's order */
  unsigned int * partition_indices;
  size_t * site_offset;                /* partition_count + 1: first site of each local partition in a node's row */
  size_t * prob_offset;                /* partition_count + 1: same for the sites x states rows */
  unsigned char ** states;             /* [node][site_offset[partition_count]] */
  double ** state_probs;
  double ** probs;                     /* [node][prob_offset[partition_count]], NULL without PLLHIP_ANC_PROBS */
} pllhip_ancestral_t;

PLL_EXPORT pllhip_ancestral_t * pllhip_eval_compute_ancestral(pllhip_eval_t * ev, unsigned int flags);
PLL_EXPORT void pllhip_eval_destroy_ancestral(pllhip_ancestral_t * anc);

/* ---------------------------------------------------------------------------
 * Site categories (include/pllhip.h, "site categories"): which rate category or mixture component every site
 * belongs to, its empirical-Bayes rate, and the EM fit of the category weights -- what IQ-TREE writes to .rate and
 * .siteprob, and the E-step of a free-rate (+R) or mixture-weight fit.
 * pllhip_eval_site_rates evaluates incrementally at the current root edge and returns one pllhip_site_posteriors_t
 * per local partition, in partition order, behind a NULL entry; flags: PLLHIP_SITECAT_POSTERIORS for the full
 * sites x categories table.  NULL on error (pll_errno set).
 * pllhip_eval_optimize_rate_weights evaluates likewise, fits the category weights of one local partition by EM from
 * its current weights (rates, p-inv and vectors fixed: no traversal per iteration), installs them with
 * pll_set_category_weights and returns the log-likelihood of the whole driver afterwards; NaN on error.  It does NOT
 * renormalise sum_r w_r rate_r = 1 nor rescale the branch lengths: a +R fit does both after its rate step, and that
 * stays the caller's.  pllhip_eval_rate_weights_trail copies what the last fit evaluated -- the weights
 * [evaluations][categories] and the partition's log-likelihood at them, the first 64 -- and returns their number.
 * On the HIP engine the table, the posteriors and the EM run on the device (pllhip_sitecat_*).  Where the library has
 * no such calls (the CPU oracle) the driver computes the same definitions on the host from the partition's own arrays
 * (clv, tipchars / tipmap, pmatrix, scale_buffer, invariant).
 * ------------------------------------------------------------------------- */
PLL_EXPORT pllhip_site_posteriors_t ** pllhip_eval_site_rates(pllhip_eval_t * ev, unsigned int flags);
PLL_EXPORT void pllhip_eval_destroy_site_rates(pllhip_site_posteriors_t ** rates);
PLL_EXPORT double pllhip_eval_optimize_rate_weights(pllhip_eval_t * ev, unsigned int partition, double epsilon,
                                                    unsigned int max_iterations);
PLL_EXPORT unsigned int pllhip_eval_rate_weights_trail(const pllhip_eval_t * ev, double * weights, double * loglh);

/* ---------------------------------------------------------------------------
 * Substitution mapping (include/pllhip.h, "substitution mapping"): per branch and given the data, the expected joint
 * states at its two ends, the expected number of a -> b substitutions along it and the expected time spent in each
 * state -- what Bio++ mapnh and HyPhy call substitution mapping, PAML's changes per branch, and the E-step of
 * Holmes-Rubin EM for a rate matrix (counts[a][b] / dwell[a] is the update of q_ab).
 *
 * pllhip_substmap_counts is the host stage for ONE category: pure C, no device.  From F_r [states][states] (row-major,
 * not padded; pairs = F o P) and the eigen system in libpll's storage, P = inv_eigenvecs diag(exp(lambda tau)) eigenvecs
 * (V = inv_eigenvecs, V^-1 = eigenvecs, both [states][states_padded]; tau_r = rates[r] t / (1 - q_r)):
 *     K[k][l] = tau e^(lambda_l tau) phi((lambda_k - lambda_l) tau),  phi(x) = expm1(x) / x, phi(0) = 1   (symmetric)
 *     G = V^T F V^-T,   M = V^-T (G o K) V^T
 *     counts[a][b] = q_ab M[a][b]  (a != b, q = V Lambda V^-1),  counts[a][a] = 0,   dwell[a] = M[a][a]
 * dwell is rate-scaled time: sum_a dwell[a] = tau posterior[r].  tau = 0 gives all zeros.  Reversible models only (real
 * eigenvalues).
 *
 * pllhip_eval_substitution_map evaluates incrementally, then visits every branch once by the re-rooting walk of
 * pllhip_eval_optimize_branches and returns, for every local partition and every branch (by pmatrix_index), the record
 * below: counts and dwell summed over the categories (the invariant component contributes to neither), total =
 * sum_ab counts, posterior_weight = sum_r sum_ij pairs (sum_n m_n less the invariant share), flags: PLLHIP_SUBST_SITES
 * for differ[sites].  tau comes from the driver's own branch length and linkage mode.  The root, the branch lengths,
 * the vectors and the log-likelihood are afterwards what they were.  On the HIP engine the pair tables come from
 * pllhip_substmap_edge; where the library has no such call (the CPU oracle) the driver computes them on the host from
 * the partition's own arrays.  NULL on error: unknown flags, no local partition.
 * ------------------------------------------------------------------------- */
PLL_EXPORT int pllhip_substmap_counts(unsigned int states, unsigned int states_padded, const double * eigenvecs,
                                      const double * inv_eigenvecs, const double * eigenvals, double tau,
                                      const double * F, double * counts, double * dwell);

typedef struct pllhip_branch_subst
{
  pll_unode_t * node;            /* orientation: i on node's side, j on node->back's side */
  double * pairs;                /* [cats][states][states] */
  double * counts;               /* [states][states] */
  double * dwell;                /* [states] */
  double * differ;               /* [sites]; NULL without PLLHIP_SUBST_SITES */
  double total, posterior_weight;
  unsigned long long dropped;    /* sites with m_n > 0 and likelihood 0 */
  unsigned int states, cats, sites;
} pllhip_branch_subst_t;

typedef struct pllhip_substitution_map
{
  unsigned int partition_count;          /* local partitions */
  unsigned int branch_count;
  unsigned int * partition_indices;      /* [partition_count] */
  pllhip_branch_subst_t ** branches;     /* [partition_count][branch_count], by pmatrix_index */
} pllhip_substitution_map_t;

PLL_EXPORT pllhip_substitution_map_t * pllhip_eval_substitution_map(pllhip_eval_t * ev, unsigned int flags);
PLL_EXPORT void pllhip_eval_destroy_substitution_map(pllhip_substitution_map_t * map);

/* ---------------------------------------------------------------------------
 * Sampled ancestral states (include/pllhip.h, "sampled ancestral states"; the process: INTEGRATION.md): one coherent
 * draw of a rate category and a state for every node of every site from their joint posterior given the data -- the
 * first step of stochastic mapping, posterior-predictive checks, alternative ancestors, imputation at the tips
 * (PLLHIP_ANCS_TIPS).
 * pllhip_eval_sample_ancestral evaluates the whole tree at the current root edge with evaluate-only mode off (every
 * vector stored; the mode of later evaluations is what it was), then draws params->replicates replicates for every
 * local partition with its own params_indices.  Rows are clv_index (node_count = tips + clv_buffers, the largest of the
 * local partitions); `component` is always filled.  The root, the branch lengths and the log-likelihood are afterwards
 * what they were.  On the HIP engine the draw is pllhip_sample_ancestral_edges; where the library has no such call (the
 * CPU oracle) the driver runs the same contract in plain C from the partition's own arrays (clv, tipchars / tipmap,
 * pmatrix, scale_buffer, invariant) and its host site-category table.  NULL on error (pll_errno set): NULL parameters,
 * zero replicates, unknown flags, more than 256 states or 128 categories, a short alphabet, invalid category weights,
 * no local partition, a root edge between two tips.
 * ------------------------------------------------------------------------- */
typedef struct pllhip_sampled_ancestral
{
  unsigned int partition_count;          /* local partitions */
  unsigned int node_count;               /* rows per replicate */
  unsigned int replicates;
  unsigned int * partition_indices;      /* [partition_count] */
  unsigned int * sites;                  /* [partition_count] */
  unsigned int * clv_index;              /* [node_count]: the clv_index of every row */
  unsigned char ** out;                  /* [partition_count][replicate][node_count][sites] */
  unsigned char ** component;            /* [partition_count][replicate][sites] */
  unsigned long long * dropped;          /* [partition_count] */
} pllhip_sampled_ancestral_t;

PLL_EXPORT pllhip_sampled_ancestral_t * pllhip_eval_sample_ancestral(pllhip_eval_t * ev,
                                                                     const pllhip_ancsample_params_t * params);
PLL_EXPORT void pllhip_eval_destroy_sampled_ancestral(pllhip_sampled_ancestral_t * sa);

/* ---------------------------------------------------------------------------
 * Sampled substitution histories (include/pllhip.h, "sampled substitution histories"; the process: INTEGRATION.md):
 * stochastic mapping by uniformization, conditioned on the sampled component and states at both ends of every branch.
 *
 * The host stage is pure C, no device:
 * pllhip_history_rate_table: from the eigen system in libpll's storage (V = inv_eigenvecs, V^-1 = eigenvecs, both
 *   [states][states_padded]) Q[a][b] = sum_k V[a][k] lambda_k V^-1[k][b] (a != b, negative values clamped to 0),
 *   Q[a][a] = -sum_(b != a) Q[a][b], *mu = max_a -Q[a][a], R = I + Q / mu (diagonal 1 - sum of the row's others, clamped
 *   at 0; mu = 0: R = I) and Rpow[k] = Rpow[k - 1] R, Rpow[0] = I, k < K, each [states][states] row-major, a plain
 *   triple loop.  Rpow[1] is R.  PLL_FAILURE for K = 0 or without memory.
 * pllhip_history_poisson: pois[k] = exp(k log lambda - lambda - lgamma(k + 1)) (lambda = 0: pois[0] = 1) for k < *K,
 *   *K the first k > lambda with pois[k] < 2^-70 sum_(i<k) pois[i].  PLL_FAILURE (pll_errno PLL_ERROR_PARAM_INVALID)
 *   where lambda is negative or not finite or the table would need more than PLLHIP_HIST_MAX_TABLE entries.
 * pllhip_history_summary: counts as doubles, dwell[c] = sum_r (tau[r] 2^-32) units[r][c] with r ascending (rate-scaled
 *   time, as in the substitution map; units are two's complement), *total = sum counts.
 *
 * pllhip_eval_sample_histories evaluates the tree as pllhip_eval_sample_ancestral does, draws the ancestral states and
 * then a history on every branch, for every local partition with its own params_indices, the driver's own branch
 * lengths and linkage mode.  params->flags: PLLHIP_ANCS_* and PLLHIP_HIST_SITES.  Branches are indexed by
 * pmatrix_index.  The root, the branch lengths, the vectors and the log-likelihood are afterwards what they were.  On
 * the HIP engine the draw is pllhip_sample_histories_edges; where the library has no such call (the CPU oracle) the
 * driver runs the same contract in plain C.  NULL on error (pll_errno set): what pllhip_eval_sample_ancestral refuses,
 * a Poisson table beyond the cap, pattern weights that add up to 2^31 or more, 2^19 or more branches.
 * ------------------------------------------------------------------------- */
PLL_EXPORT int pllhip_history_rate_table(unsigned int states, unsigned int states_padded, const double * eigenvecs,
                                         const double * inv_eigenvecs, const double * eigenvals, unsigned int K,
                                         double * mu, double * Rpow);
PLL_EXPORT int pllhip_history_poisson(double lambda, double * pois, unsigned int * K);
PLL_EXPORT int pllhip_history_summary(unsigned int states, unsigned int cats, const double * tau,
                                      const unsigned long long * counts_int, const unsigned long long * units,
                                      double * counts, double * dwell, double * total);

typedef struct pllhip_sampled_histories
{
  unsigned int partition_count;          /* local partitions */
  unsigned int node_count;               /* rows per replicate of `out` */
  unsigned int replicates;
  unsigned int branch_count;
  unsigned int * partition_indices;      /* [partition_count] */
  unsigned int * sites, * states, * cats;/* [partition_count] */
  unsigned int * clv_index;              /* [node_count]: the clv_index of every row */
  unsigned char ** out;                  /* [partition_count][replicate][node_count][sites], as pllhip_sampled_ancestral_t */
  unsigned char ** component;            /* [partition_count][replicate][sites] */
  unsigned long long * dropped;          /* [partition_count]: dropped sites */
  unsigned long long ** counts;          /* [partition_count][replicate][branch][states][states] */
  unsigned long long ** units;           /* [partition_count][replicate][branch][cats][states] */
  double ** dwell;                       /* [partition_count][replicate][branch][states] */
  double ** total;                       /* [partition_count][replicate][branch] */
  unsigned long long ** dropped_edges;   /* [partition_count][replicate][branch] */
  unsigned char ** changes;              /* [partition_count][replicate][branch][sites]; NULL without PLLHIP_HIST_SITES */
} pllhip_sampled_histories_t;

PLL_EXPORT pllhip_sampled_histories_t * pllhip_eval_sample_histories(pllhip_eval_t * ev,
                                                                     const pllhip_ancsample_params_t * params);
PLL_EXPORT void pllhip_eval_destroy_sampled_histories(pllhip_sampled_histories_t * sh);

PLL_EXPORT unsigned long pllhip_eval_ops(const pllhip_eval_t * ev);
PLL_EXPORT unsigned long pllhip_eval_pmatrix_updates(const pllhip_eval_t * ev);
PLL_EXPORT unsigned long pllhip_eval_derivative_calls(const pllhip_eval_t * ev);   /* sumtable scans */
PLL_EXPORT unsigned long pllhip_eval_newton_iterations(const pllhip_eval_t * ev);  /* iterates consumed */

#ifdef __cplusplus
}
#endif

#endif /* PLLHIP_EVAL_H_INCLUDED */
