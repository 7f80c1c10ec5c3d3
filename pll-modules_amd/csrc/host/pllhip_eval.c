/*
 * pllhip_eval.c -- evaluation driver on top of include/pll.h (see
 * include/pllhip_eval.h for scope and the reference functions it mirrors).
 * Plain C, no device code: everything below is calls into the libpll-style
 * interface, so the same file serves the HIP library and the CPU oracle.
 */
#include "pllhip_eval_internal.h"
#include "pllhip.h"
#include "pllhip_history.h"
#pragma weak pllhip_eval_attach_comm   /* HIP engine only (pllhip_comm.hip) */
#pragma weak pllhip_newton_branch      /* HIP engine only (pll_core.hip) */
#pragma weak pllhip_newton_branch_multi
#pragma weak pllhip_set_transient      /* HIP engine only: the CPU oracle stores every vector */
#pragma weak pllhip_discard_transient
#pragma weak pllhip_node_ancestral_batch   /* HIP engine only: the CPU oracle computes node by node */
#pragma weak pllhip_node_ancestral_begin
#pragma weak pllhip_node_ancestral_add
#pragma weak pllhip_node_ancestral_finish
#pragma weak pllhip_sitecat_edge          /* HIP engine only: with the CPU oracle the driver computes the table itself */
#pragma weak pllhip_sitecat_posteriors
#pragma weak pllhip_sitecat_em_weights
#pragma weak pllhip_sitecat_destroy
#pragma weak pllhip_substmap_edge         /* HIP engine only: with the CPU oracle the driver computes the pair table itself */
#pragma weak pllhip_edge_pairs_destroy
#pragma weak pllhip_sample_ancestral_edges   /* HIP engine only: with the CPU oracle the driver walks the tree itself */
#pragma weak pllhip_sample_histories_edges   /* HIP engine only: with the CPU oracle the driver samples the paths itself */
#include <stdarg.h>

static __thread pllhip_eval_t * cb_self;   /* pll_utree_traverse callbacks carry no user pointer */

void pllhip_eval_error(int code, const char * fmt, ...)
{
  va_list ap;
  pll_errno = code;
  va_start(ap, fmt);
  vsnprintf(pll_errmsg, 200, fmt, ap);
  va_end(ap);
}

pllhip_eval_t * pllhip_eval_create(pll_utree_t * tree, unsigned int partition_count, unsigned int flags)
{
  unsigned int i;
  if (!tree || !tree->binary || !partition_count)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "pllhip_eval_create needs a binary tree and >= 1 partition");
    return NULL;
  }
  pllhip_eval_t * ev = (pllhip_eval_t *)calloc(1, sizeof(*ev));
  if (!ev) goto nomem;
  ev->tree = tree;
  ev->tips = tree->tip_count;
  ev->inner = tree->inner_count;
  ev->records = ev->tips + 3 * ev->inner;
  ev->edges = tree->edge_count;
  ev->nparts = partition_count;
  ev->flags = flags;
  ev->parts = (pll_partition_t **)calloc(partition_count, sizeof(*ev->parts));
  ev->params = (unsigned int **)calloc(partition_count, sizeof(*ev->params));
  ev->sumtables = (double **)calloc(partition_count, sizeof(*ev->sumtables));
  ev->part_lnl = (double *)calloc(partition_count, sizeof(double));
  ev->clv_valid = (char *)calloc(ev->records, 1);
  ev->pmat_valid = (char *)calloc(ev->edges, 1);
  ev->trav = (pll_unode_t **)calloc(ev->tips + ev->inner, sizeof(*ev->trav));
  ev->ops = (pll_operation_t *)calloc(ev->inner, sizeof(*ev->ops));
  ev->brlens = (double *)calloc((size_t)2 * ev->edges, sizeof(double));   /* tree lengths | one partition's view */
  ev->midx = (unsigned int *)calloc(ev->edges, sizeof(unsigned int));
  ev->slot_buf = (double *)calloc((size_t)partition_count * 2 * PLLHIP_EVAL_MAX_TRIALS, sizeof(double));
  ev->brlen_scalers = (double *)calloc(partition_count, sizeof(double));
  ev->nr_x = (double *)calloc((size_t)partition_count * 6, sizeof(double));
  ev->nr_converged = (int *)calloc(partition_count, sizeof(int));
  if (ev->nr_x)
  {
    ev->nr_xl = ev->nr_x + partition_count;      ev->nr_xh = ev->nr_xl + partition_count;
    ev->nr_f = ev->nr_xh + partition_count;      ev->nr_df = ev->nr_f + partition_count;
    ev->nr_orig = ev->nr_df + partition_count;
  }
  for (i = 0; ev->brlen_scalers && i < partition_count; ++i) ev->brlen_scalers[i] = 1.0;
  if (!ev->brlen_scalers || !ev->nr_x || !ev->nr_converged || !ev->slot_buf || !ev->parts || !ev->params || !ev->sumtables || !ev->part_lnl || !ev->clv_valid ||
      !ev->pmat_valid || !ev->trav || !ev->ops || !ev->brlens || !ev->midx)
    goto nomem;
  /* indices must address the flag arrays */
  for (i = 0; i < ev->tips + ev->inner; ++i)
  {
    pll_unode_t * n = tree->nodes[i], * s = n;
    do
    {
      if (s->node_index >= ev->records || s->pmatrix_index >= ev->edges)
      {
        pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "node/pmatrix index out of range in tree record");
        pllhip_eval_destroy(ev);
        return NULL;
      }
      s = s->next;
    } while (s && s != n);
  }
  ev->root = tree->vroot->next ? tree->vroot : tree->vroot->back;
  {
    const char * env = getenv("PLLHIP_EVAL_DEVICE_NEWTON");
    ev->device_newton = (pllhip_newton_branch && (!env || atoi(env))) ? 1 : 0;
    env = getenv("PLLHIP_EVAL_TRANSIENT");          /* 0 / 1 / 2: pllhip_eval_set_transient for every evaluator */
    if (env) ev->transient = atoi(env);
  }
  /* Several partitions: leave every partition's lnL / derivative totals on the device and wait ONCE per
     evaluation / Newton round (include/pllhip.h, pllhip_results_*) instead of once per partition -- the
     reference's per-partition loop (src/tree/treeinfo.c:1020-1056) with the waits taken out.  Only where the
     library has such result groups (the HIP engine; the CPU oracle does not export the symbol).
     A reduce callback set later replaces it (pllhip_eval_set_parallel_context).  PLLHIP_EVAL_DEFERRED=0: off. */
  if (partition_count > 1 && pllhip_eval_attach_comm)
  {
    const char * env = getenv("PLLHIP_EVAL_DEFERRED");
    if (!env || atoi(env))
    {
      if (pllhip_eval_attach_comm(ev, NULL)) ev->fused_auto = 1;
      else pll_errno = 0;
    }
  }
  return ev;
nomem:
  pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate evaluator");
  pllhip_eval_destroy(ev);
  return NULL;
}

void pllhip_eval_destroy(pllhip_eval_t * ev)
{
  unsigned int p;
  if (!ev) return;
  for (p = 0; p < ev->nparts; ++p)
  {
    if (ev->params) free(ev->params[p]);
    if (ev->sumtables) free(ev->sumtables[p]);   /* pll_aligned_alloc memory is free()-able */
  }
  free(ev->parts); free(ev->params); free(ev->sumtables); free(ev->part_lnl);
  free(ev->clv_valid); free(ev->pmat_valid); free(ev->trav); free(ev->ops);
  free(ev->brlens); free(ev->midx); free(ev->slot_buf);
  free(ev->brlen_scalers); free(ev->nr_x); free(ev->nr_converged); free(ev->em_trail_w);
  if (ev->part_brlens)
  {
    for (p = 0; p < ev->nparts; ++p) free(ev->part_brlens[p]);
    free(ev->part_brlens);
  }
  if (ev->fused.destroy && ev->fused.results) ev->fused.destroy(ev->fused.results);
  free(ev);
}

int pllhip_eval_set_partition(pllhip_eval_t * ev, unsigned int index, pll_partition_t * partition,
                              const unsigned int * params_indices)
{
  unsigned int r;
  if (index >= ev->nparts)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "partition index %u out of range", index);
    return PLL_FAILURE;
  }
  if (partition)
  {
    if (partition->tips != ev->tips || partition->clv_buffers < ev->inner ||
        partition->prob_matrices < ev->edges)
    {
      pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "partition %u does not fit the tree", index);
      return PLL_FAILURE;
    }
    free(ev->params[index]);
    ev->params[index] = (unsigned int *)calloc(partition->rate_cats, sizeof(unsigned int));
    if (!ev->params[index])
    {
      pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate params indices");
      return PLL_FAILURE;
    }
    for (r = 0; params_indices && r < partition->rate_cats; ++r) ev->params[index][r] = params_indices[r];
  }
  ev->parts[index] = partition;
  ev->spec_trials = 0;
  pllhip_eval_invalidate_all(ev);
  return PLL_SUCCESS;
}

void pllhip_eval_set_parallel_context(pllhip_eval_t * ev, void * ctx, pllhip_reduce_fn reduce_cb)
{
  /* sums go through the caller's hook from now on, not through the local result group of pllhip_eval_create */
  if (reduce_cb && ev->fused_auto) pllhip_eval_set_fused(ev, NULL);
  ev->ctx = ctx;
  ev->reduce_cb = reduce_cb;
  ev->spec_trials = 0;
}

void pllhip_eval_set_fused(pllhip_eval_t * ev, const pllhip_eval_fused_t * fused)
{
  if (ev->fused.destroy && ev->fused.results) ev->fused.destroy(ev->fused.results);
  memset(&ev->fused, 0, sizeof(ev->fused));
  ev->fused_auto = 0;
  if (fused) ev->fused = *fused;
}

int pllhip_eval_set_brlen_linkage(pllhip_eval_t * ev, int linkage)
{
  unsigned int p, i;
  if (linkage < PLLHIP_EVAL_BRLEN_LINKED || linkage > PLLHIP_EVAL_BRLEN_UNLINKED)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "unknown branch-length linkage %d", linkage);
    return PLL_FAILURE;
  }
  if (linkage == PLLHIP_EVAL_BRLEN_UNLINKED && !ev->part_brlens)
  {
    ev->part_brlens = (double **)calloc(ev->nparts, sizeof(double *));
    for (p = 0; ev->part_brlens && p < ev->nparts; ++p)
      if (!(ev->part_brlens[p] = (double *)calloc(ev->edges, sizeof(double)))) break;
    if (!ev->part_brlens || p < ev->nparts)
    {
      pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate per-partition branch lengths");
      return PLL_FAILURE;
    }
    /* every partition starts from the tree's lengths */
    for (i = 0; i < ev->tips + ev->inner; ++i)
    {
      const pll_unode_t * n = ev->tree->nodes[i], * s2 = n;
      do
      {
        for (p = 0; p < ev->nparts; ++p) ev->part_brlens[p][s2->pmatrix_index] = s2->length;
        s2 = s2->next;
      } while (s2 && s2 != n);
    }
  }
  ev->linkage = linkage;
  if (linkage != PLLHIP_EVAL_BRLEN_SCALED)
    for (p = 0; p < ev->nparts; ++p) ev->brlen_scalers[p] = 1.0;
  pllhip_eval_invalidate_all(ev);
  return PLL_SUCCESS;
}

int pllhip_eval_set_brlen_scaler(pllhip_eval_t * ev, unsigned int partition, double scaler)
{
  if (partition >= ev->nparts || ev->linkage != PLLHIP_EVAL_BRLEN_SCALED || !(scaler > 0.0))
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "branch-length scalers need SCALED linkage, a valid "
                      "partition and a positive value");
    return PLL_FAILURE;
  }
  ev->brlen_scalers[partition] = scaler;
  pllhip_eval_invalidate_all(ev);
  return PLL_SUCCESS;
}

double pllhip_eval_get_brlen_scaler(const pllhip_eval_t * ev, unsigned int partition)
{
  return partition < ev->nparts ? ev->brlen_scalers[partition] : 0.0;
}

double pllhip_eval_get_partition_branch_length(const pllhip_eval_t * ev, unsigned int partition,
                                               const pll_unode_t * edge)
{
  if (partition >= ev->nparts) return 0.0;
  return ev->part_brlens ? ev->part_brlens[partition][edge->pmatrix_index] : edge->length;
}

int pllhip_eval_set_partition_branch_length(pllhip_eval_t * ev, unsigned int partition,
                                            const pll_unode_t * edge, double length)
{
  if (partition >= ev->nparts || ev->linkage != PLLHIP_EVAL_BRLEN_UNLINKED || !(length >= 0.0))
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "per-partition branch lengths need UNLINKED linkage");
    return PLL_FAILURE;
  }
  ev->part_brlens[partition][edge->pmatrix_index] = length;
  ev->pmat_valid[edge->pmatrix_index] = 0;
  memset(ev->clv_valid, 0, ev->records);
  return PLL_SUCCESS;
}

/* the branch length partition p's P-matrix of branch m is computed for */
static double effective_length(const pllhip_eval_t * ev, unsigned int p, unsigned int m, double tree_length)
{
  const double t = ev->part_brlens ? ev->part_brlens[p][m] : tree_length;
  return (ev->linkage == PLLHIP_EVAL_BRLEN_SCALED) ? t * ev->brlen_scalers[p] : t;
}

int pllhip_eval_set_root(pllhip_eval_t * ev, pll_unode_t * root)
{
  if (!root || !root->next)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "the root must be an inner node record");
    return PLL_FAILURE;
  }
  ev->root = root;
  return PLL_SUCCESS;
}

pll_unode_t * pllhip_eval_root(const pllhip_eval_t * ev) { return ev->root; }

void pllhip_eval_invalidate_all(pllhip_eval_t * ev)
{
  memset(ev->clv_valid, 0, ev->records);
  memset(ev->pmat_valid, 0, ev->edges);
}

void pllhip_eval_invalidate_pmatrix(pllhip_eval_t * ev, const pll_unode_t * edge)
{
  ev->pmat_valid[edge->pmatrix_index] = 0;
}

void pllhip_eval_invalidate_clv(pllhip_eval_t * ev, const pll_unode_t * node)
{
  ev->clv_valid[node->node_index] = 0;
}

void pllhip_eval_set_branch_length(pllhip_eval_t * ev, pll_unode_t * edge, double length)
{
  unsigned int p;
  edge->length = edge->back->length = length;
  for (p = 0; ev->part_brlens && p < ev->nparts; ++p) ev->part_brlens[p][edge->pmatrix_index] = length;
  ev->pmat_valid[edge->pmatrix_index] = 0;
  /* every CLV that looks across this edge depends on it: all records on the far
     side pointing this way.  Conservative and cheap: drop all CLV flags. */
  memset(ev->clv_valid, 0, ev->records);
}

/* the CLV slot of an inner node is shared by its three records */
static void mark_clv_valid(pllhip_eval_t * ev, const pll_unode_t * node)
{
  ev->clv_valid[node->node_index] = 1;
  ev->clv_valid[node->next->node_index] = 0;
  ev->clv_valid[node->next->next->node_index] = 0;
}

static int cb_all(pll_unode_t * node) { (void)node; return 1; }

static int cb_invalid_only(pll_unode_t * node)
{
  if (!node->next) return 0;
  return !cb_self->clv_valid[node->node_index];
}

static int update_pmatrices(pllhip_eval_t * ev)
{
  unsigned int n = 0, i, k = 0, p;
  if (!pll_utree_traverse(ev->root, PLL_TREE_TRAVERSE_POSTORDER, cb_all, ev->trav, &n)) return PLL_FAILURE;
  for (i = 0; i < n; ++i)
  {
    const pll_unode_t * node = ev->trav[i];
    if (ev->pmat_valid[node->pmatrix_index]) continue;
    ev->pmat_valid[node->pmatrix_index] = 1;
    ev->midx[k] = node->pmatrix_index;
    ev->brlens[k++] = node->length;
  }
  if (!k) return PLL_SUCCESS;
  for (p = 0; p < ev->nparts; ++p)
  {
    double * bl = ev->brlens;
    if (!ev->parts[p]) continue;
    if (ev->linkage != PLLHIP_EVAL_BRLEN_LINKED)
    {
      /* this partition's own view of the invalid branches (scaled or unlinked lengths) */
      bl = ev->brlens + ev->edges;
      for (i = 0; i < k; ++i) bl[i] = effective_length(ev, p, ev->midx[i], ev->brlens[i]);
    }
    if (ev->flags & PLLHIP_EVAL_PMATRIX_PER_BRANCH)
    {
      for (i = 0; i < k; ++i)
        if (!pll_update_prob_matrices(ev->parts[p], ev->params[p], &ev->midx[i], &bl[i], 1))
          return PLL_FAILURE;
    }
    else if (!pll_update_prob_matrices(ev->parts[p], ev->params[p], ev->midx, bl, k))
      return PLL_FAILURE;
  }
  ev->n_pmat += k;
  return PLL_SUCCESS;
}

/* A worker that fails locally must not leave its peers inside the reduction: it still takes part, with NaN,
   so that every worker fails in the same call (include/pllhip.h, pllhip_results_fetch).  `failed`: this
   worker could not bring its vectors up to date. */
static void poison_and_reduce(pllhip_eval_t * ev, double * buf, unsigned int n)
{
  unsigned int i;
  const int code = pll_errno;
  char msg[200];
  memcpy(msg, pll_errmsg, sizeof(msg));
  if (ev->fused.fetch)
  {
    if (ev->fused.poison) ev->fused.poison(ev->fused.results);
    (void)ev->fused.fetch(ev->fused.results, 0, n, 0 /* SUM */, buf);
  }
  else if (ev->reduce_cb)
  {
    for (i = 0; i < n; ++i) buf[i] = NAN;
    ev->reduce_cb(ev->ctx, buf, n, 0 /* SUM */);
  }
  for (i = 0; i < n; ++i) buf[i] = NAN;
  if (code) { pll_errno = code; memcpy(pll_errmsg, msg, sizeof(msg)); }    /* the cause, not the consequence */
}

static double edge_loglh(pllhip_eval_t * ev, const pll_unode_t * e, int failed)
{
  unsigned int p;
  double total = 0.0;
  if (failed)
  {
    poison_and_reduce(ev, ev->part_lnl, ev->nparts);
    return NAN;
  }
  if (ev->fused.fetch)
  {
    /* every partition's kernel is enqueued, then ONE fetch: all-reduce on the device, one wait */
    for (p = 0; p < ev->nparts; ++p)
      if (ev->parts[p] &&
          !ev->fused.edge_loglikelihood(ev->fused.results, p, ev->parts[p], e->clv_index, e->scaler_index,
                                        e->back->clv_index, e->back->scaler_index, e->pmatrix_index,
                                        ev->params[p]))
      {
        poison_and_reduce(ev, ev->part_lnl, ev->nparts);
        return NAN;
      }
    if (!ev->fused.fetch(ev->fused.results, 0, ev->nparts, 0 /* SUM */, ev->part_lnl)) return NAN;
  }
  else
  {
    for (p = 0; p < ev->nparts; ++p)
    {
      ev->part_lnl[p] = 0.0;
      if (!ev->parts[p]) continue;
      ev->part_lnl[p] = pll_compute_edge_loglikelihood(ev->parts[p], e->clv_index, e->scaler_index,
                                                       e->back->clv_index, e->back->scaler_index,
                                                       e->pmatrix_index, ev->params[p], NULL);
    }
    if (ev->reduce_cb) ev->reduce_cb(ev->ctx, ev->part_lnl, ev->nparts, 0 /* SUM */);
  }
  for (p = 0; p < ev->nparts; ++p) total += ev->part_lnl[p];
  return total;
}

/* PLLHIP_EVAL_FAULT=N (+ PLLHIP_EVAL_FAULT_RANK is up to the caller: set the variable on one worker only):
   the N-th evaluation of this process fails before its reduction -- for the tests of the path above.
   Evaluators of several host threads come through here at once: the variable is read until one thread has
   published its value (all of them would publish the same), the evaluations of the process are counted atomically */
static int injected_fault(void)
{
  static long at = -1, n = 0;
  long a = __atomic_load_n(&at, __ATOMIC_RELAXED);
  if (a < 0)
  {
    const char * e = getenv("PLLHIP_EVAL_FAULT");
    a = e ? atol(e) : 0;
    if (a < 0) a = 0;
    __atomic_store_n(&at, a, __ATOMIC_RELAXED);
  }
  if (a > 0 && __atomic_add_fetch(&n, 1, __ATOMIC_RELAXED) == a)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "injected evaluation failure");
    return 1;
  }
  return 0;
}

void pllhip_eval_set_transient(pllhip_eval_t * ev, int mode)
{
  ev->transient = mode;
  ev->last_was_full = 0;
}

/* mode of the partitions' engines for the operation list that follows */
static void partitions_transient(pllhip_eval_t * ev, int on, int discard)
{
  unsigned int p;
  if (!pllhip_set_transient || !pllhip_discard_transient) return;
  for (p = 0; p < ev->nparts; ++p)
  {
    if (!ev->parts[p]) continue;
    if (discard) (void)pllhip_discard_transient(ev->parts[p]);
    (void)pllhip_set_transient(ev->parts[p], on);
  }
}

/* P-matrices and vectors of the current root up to date (the invalid ones only); 0 if that failed */
static int update_vectors(pllhip_eval_t * ev, int failed)
{
  unsigned int n = 0, nops = 0, i;
  if (!failed && !update_pmatrices(ev)) failed = 1;
  cb_self = ev;
  if (!failed && !pll_utree_traverse(ev->root, PLL_TREE_TRAVERSE_POSTORDER, cb_invalid_only, ev->trav, &n))
    failed = 1;
  if (!failed) pll_utree_create_operations(ev->trav, n, NULL, NULL, ev->ops, NULL, &nops);
  if (!failed && nops)
  {
    /* every partition walks the same list (src/tree/treeinfo.c:1020-1056): one call, so that partitions
       of one kernel family can share their launches */
    if (!pllhip_update_partials_batch(ev->parts, ev->nparts, ev->ops, nops) || pll_errno) failed = 1;
    else
    {
      for (i = 0; i < n; ++i)
        if (ev->trav[i]->next) mark_clv_valid(ev, ev->trav[i]);
      ev->n_ops += nops;
    }
  }
  return !failed;
}

double pllhip_eval_loglh(pllhip_eval_t * ev, int incremental)
{
  int failed = 0;
  /* a full evaluation recomputes every vector: what the last one kept in registers only is given up BEFORE the
     P-matrices change (nothing is recomputed for them), and this one may keep its own in registers */
  const int transient = !incremental && (ev->transient == PLLHIP_EVAL_TRANSIENT_ON ||
                                         (ev->transient == PLLHIP_EVAL_TRANSIENT_AUTO && ev->last_was_full));
  ev->last_was_full = !incremental;
  if (!incremental) pllhip_eval_invalidate_all(ev);
  pll_errno = 0;
  if (!incremental && ev->transient != PLLHIP_EVAL_TRANSIENT_OFF) partitions_transient(ev, transient, 1);
  failed = !update_vectors(ev, injected_fault());
  if (transient) partitions_transient(ev, 0, 0);
  return edge_loglh(ev, ev->root, failed);
}

/* ---------------------------------------------------------------------- */
/* Marginal ancestral states of every inner node                          */
/* (pllmod_treeinfo_compute_ancestral, src/tree/treeinfo.c:1611-1718)      */
/* ---------------------------------------------------------------------- */

void pllhip_eval_destroy_ancestral(pllhip_ancestral_t * anc)
{
  unsigned int i;
  if (!anc) return;
  for (i = 0; i < anc->node_count; ++i)
  {
    if (anc->states) free(anc->states[i]);
    if (anc->state_probs) free(anc->state_probs[i]);
    if (anc->probs) free(anc->probs[i]);
  }
  free(anc->nodes); free(anc->partition_indices); free(anc->site_offset); free(anc->prob_offset);
  free(anc->states); free(anc->state_probs); free(anc->probs);
  free(anc);
}

/* first index of the row maximum (0 for an all-zero row) and the maximum: the rule of the device summary */
static void summarise_rows(const double * probs, size_t sites, unsigned int states, unsigned char * st, double * sp)
{
  size_t n;
  unsigned int i;
  for (n = 0; n < sites; ++n)
  {
    const double * row = probs + n * states;
    double best = row[0];
    unsigned int idx = 0;
    for (i = 1; i < states; ++i)
      if (row[i] > best) { best = row[i]; idx = i; }
    st[n] = (unsigned char)idx;
    sp[n] = best;
  }
}

pllhip_ancestral_t * pllhip_eval_compute_ancestral(pllhip_eval_t * ev, unsigned int flags)
{
  unsigned int i, p, k, n = 0, local = 0;
  int failed = 0;
  pll_unode_t * const old_root = ev->root;
  pllhip_ancestral_t * anc = NULL;
  pllhip_anc_batch_t ** batches = NULL;     /* [local]: one device batch per partition (the product) */
  double * scratch = NULL;                  /* the oracle without PLLHIP_ANC_PROBS: one node's table */
  const int device = pllhip_node_ancestral_batch && pllhip_node_ancestral_begin && pllhip_node_ancestral_add &&
                     pllhip_node_ancestral_finish;
  const int want_probs = (flags & PLLHIP_ANC_PROBS) != 0;

  pll_errno = 0;
  if (flags & ~PLLHIP_ANC_PROBS)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "unknown flags for the ancestral states");
    return NULL;
  }
  for (p = 0; p < ev->nparts; ++p)
    if (ev->parts[p])
    {
      if (ev->parts[p]->states > 256)
      {
        pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "partition %u: more than 256 states do not fit the state array", p);
        return NULL;
      }
      ++local;
    }
  anc = (pllhip_ancestral_t *)calloc(1, sizeof(*anc));
  if (!anc) goto nomem;
  anc->node_count = ev->inner;
  anc->partition_count = local;
  anc->nodes = (pll_unode_t **)calloc(ev->inner ? ev->inner : 1, sizeof(*anc->nodes));
  anc->partition_indices = (unsigned int *)calloc(local ? local : 1, sizeof(unsigned int));
  anc->site_offset = (size_t *)calloc((size_t)local + 1, sizeof(size_t));
  anc->prob_offset = (size_t *)calloc((size_t)local + 1, sizeof(size_t));
  anc->states = (unsigned char **)calloc(ev->inner ? ev->inner : 1, sizeof(*anc->states));
  anc->state_probs = (double **)calloc(ev->inner ? ev->inner : 1, sizeof(*anc->state_probs));
  if (want_probs) anc->probs = (double **)calloc(ev->inner ? ev->inner : 1, sizeof(*anc->probs));
  if (!anc->nodes || !anc->partition_indices || !anc->site_offset || !anc->prob_offset || !anc->states ||
      !anc->state_probs || (want_probs && !anc->probs))
    goto nomem;
  for (p = 0, k = 0; p < ev->nparts; ++p)
  {
    if (!ev->parts[p]) continue;
    anc->partition_indices[k] = p;
    anc->site_offset[k + 1] = anc->site_offset[k] + ev->parts[p]->sites;
    anc->prob_offset[k + 1] = anc->prob_offset[k] + (size_t)ev->parts[p]->sites * ev->parts[p]->states;
    ++k;
  }
  /* the reference's order: a full post-order traversal from the tree's vroot, inner nodes kept */
  if (!pll_utree_traverse(ev->tree->vroot, PLL_TREE_TRAVERSE_POSTORDER, cb_all, ev->trav, &n)) goto fail;
  for (i = 0, k = 0; i < n; ++i)
    if (ev->trav[i]->next)
    {
      if (k == anc->node_count)
      {
        pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "the tree holds more inner nodes than it declares");
        goto fail;
      }
      anc->nodes[k++] = ev->trav[i];
    }
  if (k != anc->node_count)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "the traversal from vroot does not reach every inner node");
    goto fail;
  }
  for (i = 0; i < anc->node_count; ++i)
  {
    const size_t ns = anc->site_offset[local], np = anc->prob_offset[local];
    anc->states[i] = (unsigned char *)calloc(ns ? ns : 1, 1);
    anc->state_probs[i] = (double *)calloc(ns ? ns : 1, sizeof(double));
    if (want_probs) anc->probs[i] = (double *)calloc(np ? np : 1, sizeof(double));
    if (!anc->states[i] || !anc->state_probs[i] || (want_probs && !anc->probs[i])) goto nomem;
  }
  if (device)
  {
    batches = (pllhip_anc_batch_t **)calloc(local ? local : 1, sizeof(*batches));
    if (!batches) goto nomem;
    for (k = 0; k < local; ++k)
    {
      batches[k] = pllhip_node_ancestral_begin(ev->parts[anc->partition_indices[k]], flags, anc->node_count);
      if (!batches[k]) goto fail;
    }
  }
  else if (!want_probs)
  {
    size_t widest = 1;
    for (k = 0; k < local; ++k)
      if (anc->prob_offset[k + 1] - anc->prob_offset[k] > widest) widest = anc->prob_offset[k + 1] - anc->prob_offset[k];
    scratch = (double *)calloc(widest, sizeof(double));
    if (!scratch) goto nomem;
  }

  /* per node: root at its record, the invalid vectors and P-matrices of that root, one entry per partition.  On the
     device nothing waits here: an entry's kernel reads the two vectors in stream order, before the next re-rooting
     overwrites their slots. */
  ev->last_was_full = 0;
  for (i = 0; i < anc->node_count && !failed; ++i)
  {
    const pll_unode_t * node = anc->nodes[i];
    ev->root = anc->nodes[i];
    if (!update_vectors(ev, 0)) { failed = 1; break; }
    for (k = 0; k < local && !failed; ++k)
    {
      pll_partition_t * part = ev->parts[anc->partition_indices[k]];
      const unsigned int * params = ev->params[anc->partition_indices[k]];
      unsigned char * st = anc->states[i] + anc->site_offset[k];
      double * sp = anc->state_probs[i] + anc->site_offset[k];
      double * pr = want_probs ? anc->probs[i] + anc->prob_offset[k] : NULL;
      if (device)
      {
        if (!pllhip_node_ancestral_add(batches[k], node->clv_index, node->back->clv_index, node->pmatrix_index,
                                       params, st, sp, pr))
          failed = 1;
      }
      else
      {
        double * table = want_probs ? pr : scratch;
        if (!pll_compute_node_ancestral(part, node->clv_index, node->scaler_index, node->back->clv_index,
                                        node->back->scaler_index, node->pmatrix_index, params, table))
          failed = 1;
        else summarise_rows(table, part->sites, part->states, st, sp);
      }
    }
  }
  if (batches)
  {
    /* one wait per staging chunk: here for the last one.  Every batch is finished, also after a failure. */
    const int code = pll_errno;
    char msg[200];
    memcpy(msg, pll_errmsg, sizeof(msg));
    for (k = 0; k < local; ++k)
      if (batches[k] && !pllhip_node_ancestral_finish(batches[k]) && !failed)
      {
        failed = 1;
        memcpy(msg, pll_errmsg, sizeof(msg));
      }
    if (failed && code) { pll_errno = code; memcpy(pll_errmsg, msg, sizeof(msg)); }
    free(batches);
    batches = NULL;
  }
  if (failed) goto fail;
  free(scratch);
  ev->root = old_root;
  return anc;

nomem:
  pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the ancestral states");
fail:
  if (batches)
  {
    const int code = pll_errno;
    char msg[200];
    memcpy(msg, pll_errmsg, sizeof(msg));
    for (k = 0; k < local; ++k)
      if (batches[k]) (void)pllhip_node_ancestral_finish(batches[k]);
    free(batches);
    pll_errno = code;
    memcpy(pll_errmsg, msg, sizeof(msg));
  }
  if (!pll_errno) pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "ancestral states: the traversal failed");
  free(scratch);
  pllhip_eval_destroy_ancestral(anc);
  ev->root = old_root;
  return NULL;
}

/* ---------------------------------------------------------------------- */
/* Site categories: posteriors of the rate categories, site rates, and the */
/* EM fit of the category weights (include/pllhip.h, "site categories")    */
/* ---------------------------------------------------------------------- */

#define SC_LN_SCALE 177.445678223345993274     /* 256 ln 2 */
#define SC_RATE_MAXDIFF 4                      /* libpll-2's PLL_SCALE_RATE_MAXDIFF */

/* element (n, r, j) of a vector as the host arrays hold it: a coded tip through tipchars / tipmap */
static double sc_elem(const pll_partition_t * p, unsigned int clv, size_t n, unsigned int r, unsigned int j)
{
  if ((p->attributes & PLL_ATTRIB_PATTERN_TIP) && clv < p->tips)
    return (double)((p->tipmap[p->tipchars[clv][n]] >> j) & 1);
  return p->clv[clv][(n * p->rate_cats + r) * p->states_padded + j];
}

static unsigned int sc_count(const pll_partition_t * p, int ps, int cs, size_t x)
{
  return (ps == PLL_SCALE_BUFFER_NONE ? 0u : p->scale_buffer[ps][x]) + (cs == PLL_SCALE_BUFFER_NONE ? 0u : p->scale_buffer[cs][x]);
}

/* The definitions of include/pllhip.h in plain C from the partition's host arrays: A, B [sites][cats], c [sites].
   The second implementation of the table kernels (kernels_sitecat.hpp), for libraries that keep host arrays. */
/* ... and, where D is not NULL, D[n][r] = (1 - q_r) d[n][r]: what the table did to l = 1 (the substitution map's scale) */
static void sc_host_table_scaled(const pll_partition_t * p, unsigned int pc, int ps, unsigned int cc, int cs, unsigned int m,
                                 const unsigned int * fi, double * A, double * B, unsigned int * c, double * D)
{
  const unsigned int S = p->states, Sp = p->states_padded, R = p->rate_cats;
  const int per_rate = (p->attributes & PLL_ATTRIB_RATE_SCALERS) != 0;
  size_t n;
  unsigned int r, i, j;
  for (n = 0; n < p->sites; ++n)
  {
    unsigned int cnt = per_rate ? ~0u : sc_count(p, ps, cs, n);
    const int state = p->invariant ? p->invariant[n] : -1;
    double binv = 0.0;
    int descale;
    for (r = 0; per_rate && r < R; ++r)
      if (sc_count(p, ps, cs, n * R + r) < cnt) cnt = sc_count(p, ps, cs, n * R + r);
    for (r = 0; r < R; ++r)
      if (p->prop_invar[fi[r]] > 0.0 && state >= 0)
        binv += p->rate_weights[r] * p->prop_invar[fi[r]] * p->frequencies[fi[r]][state];
    descale = binv > 0.0 && cnt > 0;
    for (r = 0; r < R; ++r)
    {
      const double * pi = p->frequencies[fi[r]], q = p->prop_invar[fi[r]];
      const double * P = p->pmatrix[m] + (size_t)r * S * Sp;
      double l = 0.0, one = 1.0;
      for (i = 0; i < S; ++i)
      {
        double a = 0.0;
        for (j = 0; j < S; ++j) a += P[i * Sp + j] * sc_elem(p, cc, n, r, j);
        l += pi[i] * sc_elem(p, pc, n, r, i) * a;
      }
      if (per_rate)
      {
        unsigned int d = sc_count(p, ps, cs, n * R + r) - cnt;
        if (d > SC_RATE_MAXDIFF) d = SC_RATE_MAXDIFF;
        if (d) { l *= ldexp(1.0, -256 * (int)d); one *= ldexp(1.0, -256 * (int)d); }
      }
      if (descale) { l = (cnt <= 3) ? ldexp(l, -256 * (int)cnt) : 0.0; one = (cnt <= 3) ? ldexp(one, -256 * (int)cnt) : 0.0; }
      A[n * R + r] = (q > 0.0) ? (1.0 - q) * l : l;
      if (D) D[n * R + r] = (q > 0.0) ? (1.0 - q) * one : one;
      B[n * R + r] = (q > 0.0 && state >= 0) ? q * pi[state] : 0.0;
    }
    c[n] = descale ? 0u : cnt;
  }
}

static void sc_host_table(const pll_partition_t * p, unsigned int pc, int ps, unsigned int cc, int cs, unsigned int m,
                          const unsigned int * fi, double * A, double * B, unsigned int * c)
{
  sc_host_table_scaled(p, pc, ps, cc, cs, m, fi, A, B, c, NULL);
}

/* T[n], and what follows from it: any of the outputs may be NULL.  Returns sum_n m_n lnl[n]. */
static double sc_host_posteriors(size_t N, unsigned int R, const double * A, const double * B, const unsigned int * c,
                                 const unsigned int * m, const double * w, const double * rho,
                                 pllhip_site_posteriors_t * po, double * expected)
{
  size_t n;
  unsigned int r;
  double loglh = 0.0;
  for (r = 0; r < R; ++r) expected[r] = 0.0;
  for (n = 0; n < N; ++n)
  {
    const double * a = A + n * R, * b = B + n * R;
    double T = 0.0, rate = 0.0, inv = 0.0, best = 0.0, lnl;
    unsigned int idx = 0;
    for (r = 0; r < R; ++r) T += w[r] * (a[r] + b[r]);
    lnl = log(T) - (double)c[n] * SC_LN_SCALE;
    for (r = 0; r < R; ++r)
    {
      const double post = (T > 0.0) ? (w[r] * a[r]) / T : 0.0;
      if (po && po->posterior) po->posterior[n * R + r] = post;
      rate += post * rho[r];
      inv += w[r] * b[r];
      if (post > best) { best = post; idx = r; }
      if (T > 0.0 && m[n]) expected[r] += (double)m[n] * ((w[r] * (a[r] + b[r])) / T);
    }
    if (m[n]) loglh += (double)m[n] * lnl;
    if (!po) continue;
    po->rate[n] = rate;
    po->category[n] = (unsigned char)idx;
    po->category_prob[n] = best;
    po->invariant_prob[n] = (T > 0.0) ? inv / T : 0.0;
    po->lnl[n] = lnl;
  }
  return loglh;
}

static void sc_destroy_one(pllhip_site_posteriors_t * po)
{
  if (!po) return;
  free(po->rate); free(po->category); free(po->category_prob); free(po->invariant_prob); free(po->lnl);
  free(po->posterior); free(po->expected);
  free(po);
}

void pllhip_eval_destroy_site_rates(pllhip_site_posteriors_t ** rates)
{
  unsigned int k;
  if (!rates) return;
  for (k = 0; rates[k]; ++k) sc_destroy_one(rates[k]);
  free(rates);
}

static pllhip_site_posteriors_t * sc_alloc_posteriors(size_t N, unsigned int R, int full)
{
  pllhip_site_posteriors_t * po = (pllhip_site_posteriors_t *)calloc(1, sizeof(*po));
  if (!po) return NULL;
  po->sites = (unsigned int)N;
  po->cats = R;
  po->rate = (double *)calloc(N ? N : 1, sizeof(double));
  po->category = (unsigned char *)calloc(N ? N : 1, 1);
  po->category_prob = (double *)calloc(N ? N : 1, sizeof(double));
  po->invariant_prob = (double *)calloc(N ? N : 1, sizeof(double));
  po->lnl = (double *)calloc(N ? N : 1, sizeof(double));
  if (full) po->posterior = (double *)calloc(N ? N * R : 1, sizeof(double));
  po->expected = (double *)calloc(R, sizeof(double));
  if (po->rate && po->category && po->category_prob && po->invariant_prob && po->lnl && (!full || po->posterior) && po->expected)
    return po;
  sc_destroy_one(po);
  return NULL;
}

static int sc_check_partition(const pll_partition_t * part, unsigned int p)
{
  if (part->rate_cats <= 256) return 1;
  pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "partition %u: more than 256 categories do not fit the category array", p);
  return 0;
}

/* the host table of partition `part` at the current root edge (vectors up to date); 0: out of memory */
static int sc_host_root_table(pllhip_eval_t * ev, unsigned int p, double ** A, double ** B, unsigned int ** c)
{
  const pll_partition_t * part = ev->parts[p];
  const pll_unode_t * e = ev->root;
  const size_t cells = (size_t)part->sites * part->rate_cats;
  *A = (double *)calloc(cells ? cells : 1, sizeof(double));
  *B = (double *)calloc(cells ? cells : 1, sizeof(double));
  *c = (unsigned int *)calloc(part->sites ? part->sites : 1, sizeof(unsigned int));
  if (!*A || !*B || !*c)
  {
    free(*A); free(*B); free(*c);
    pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the site-category table");
    return 0;
  }
  sc_host_table(part, e->clv_index, e->scaler_index, e->back->clv_index, e->back->scaler_index, e->pmatrix_index,
                ev->params[p], *A, *B, *c);
  return 1;
}

pllhip_site_posteriors_t ** pllhip_eval_site_rates(pllhip_eval_t * ev, unsigned int flags)
{
  const int device = pllhip_sitecat_edge && pllhip_sitecat_posteriors && pllhip_sitecat_destroy;
  const pll_unode_t * e;
  pllhip_site_posteriors_t ** out;
  unsigned int p, k = 0, local = 0;
  pll_errno = 0;
  if (flags & ~PLLHIP_SITECAT_POSTERIORS)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "unknown flags for the site rates");
    return NULL;
  }
  for (p = 0; p < ev->nparts; ++p)
    if (ev->parts[p])
    {
      if (!sc_check_partition(ev->parts[p], p)) return NULL;
      ++local;
    }
  ev->last_was_full = 0;
  if (!update_vectors(ev, 0))
  {
    if (!pll_errno) pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "site rates: the traversal failed");
    return NULL;
  }
  e = ev->root;
  out = (pllhip_site_posteriors_t **)calloc((size_t)local + 1, sizeof(*out));
  if (!out) goto nomem;
  for (p = 0; p < ev->nparts; ++p)
  {
    pll_partition_t * part = ev->parts[p];
    if (!part) continue;
    if (device)
    {
      pllhip_sitecat_t * set = pllhip_sitecat_edge(part, e->clv_index, e->scaler_index, e->back->clv_index,
                                                   e->back->scaler_index, e->pmatrix_index, ev->params[p]);
      if (!set) goto fail;
      out[k] = pllhip_sitecat_posteriors(set, NULL, flags);
      pllhip_sitecat_destroy(set);
      if (!out[k]) goto fail;
    }
    else
    {
      double * A, * B;
      unsigned int * c;
      out[k] = sc_alloc_posteriors(part->sites, part->rate_cats, (flags & PLLHIP_SITECAT_POSTERIORS) != 0);
      if (!out[k]) goto nomem;
      if (!sc_host_root_table(ev, p, &A, &B, &c)) goto fail;
      out[k]->loglh = sc_host_posteriors(part->sites, part->rate_cats, A, B, c, part->pattern_weights, part->rate_weights,
                                         part->rates, out[k], out[k]->expected);
      free(A); free(B); free(c);
    }
    ++k;
  }
  return out;
nomem:
  pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the site rates");
fail:
  pllhip_eval_destroy_site_rates(out);
  return NULL;
}

unsigned int pllhip_eval_rate_weights_trail(const pllhip_eval_t * ev, double * weights, double * loglh)
{
  if (weights && ev->em_evals) memcpy(weights, ev->em_trail_w, sizeof(double) * ev->em_evals * ev->em_cats);
  if (loglh && ev->em_evals) memcpy(loglh, ev->em_trail_l, sizeof(double) * ev->em_evals);
  return ev->em_evals;
}

double pllhip_eval_optimize_rate_weights(pllhip_eval_t * ev, unsigned int partition, double epsilon,
                                         unsigned int max_iterations)
{
  const int device = pllhip_sitecat_edge && pllhip_sitecat_em_weights && pllhip_sitecat_destroy;
  pll_partition_t * part;
  const pll_unode_t * e;
  double w[256], L = 0.0;
  unsigned int R, r, its = 0;
  pll_errno = 0;
  ev->em_evals = 0;
  if (partition >= ev->nparts || !ev->parts[partition])
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "rate weights: partition %u is not local", partition);
    return NAN;
  }
  part = ev->parts[partition];
  R = part->rate_cats;
  if (!sc_check_partition(part, partition)) return NAN;
  if (!(epsilon >= 0.0))
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "rate weights: epsilon is negative or not a number");
    return NAN;
  }
  ev->last_was_full = 0;
  if (!update_vectors(ev, 0))
  {
    if (!pll_errno) pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "rate weights: the traversal failed");
    return NAN;
  }
  e = ev->root;
  ev->em_cats = R;
  free(ev->em_trail_w);
  ev->em_trail_w = (double *)calloc((size_t)PLLHIP_SITECAT_TRAIL_MAX * R, sizeof(double));
  if (!ev->em_trail_w)
  {
    pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the weight trail");
    return NAN;
  }
  if (device)
  {
    pllhip_sitecat_em_params_t prm;
    int ok;
    pllhip_sitecat_t * set = pllhip_sitecat_edge(part, e->clv_index, e->scaler_index, e->back->clv_index,
                                                 e->back->scaler_index, e->pmatrix_index, ev->params[partition]);
    if (!set) return NAN;
    prm.start = NULL;
    prm.epsilon = epsilon;
    prm.max_iterations = max_iterations;
    ok = pllhip_sitecat_em_weights(set, &prm, w, &L, &its, ev->em_trail_w, ev->em_trail_l);
    pllhip_sitecat_destroy(set);
    if (!ok) return NAN;
  }
  else
  {
    double * A, * B, expected[256], Lprev = 0.0, msum = 0.0, esum;
    unsigned int * c;
    size_t n;
    if (part->attributes & PLL_ATTRIB_AB_MASK)
    {
      pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "rate weights: the partition has an ascertainment-bias correction, which depends on the weights");
      return NAN;
    }
    for (n = 0; n < part->sites; ++n) msum += (double)part->pattern_weights[n];
    for (r = 0; r < R; ++r) w[r] = part->rate_weights[r];
    if (!(msum > 0.0))
    {
      pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "rate weights: the pattern weights add up to 0");
      return NAN;
    }
    if (!sc_host_root_table(ev, partition, &A, &B, &c)) return NAN;
    for (its = 0;; ++its)
    {
      L = sc_host_posteriors(part->sites, R, A, B, c, part->pattern_weights, w, part->rates, NULL, expected);
      if (its < PLLHIP_SITECAT_TRAIL_MAX)
      {
        memcpy(ev->em_trail_w + (size_t)its * R, w, sizeof(double) * R);
        ev->em_trail_l[its] = L;
      }
      if (!(L > -INFINITY))
      {
        for (n = 0; n < part->sites; ++n)
        {
          double T = 0.0;
          for (r = 0; r < R; ++r) T += w[r] * (A[n * R + r] + B[n * R + r]);
          if (part->pattern_weights[n] && !(T > 0.0)) break;
        }
        free(A); free(B); free(c);
        pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "rate weights: site %zu has a pattern weight and likelihood 0 under the weights of iteration %u", n, its);
        return NAN;
      }
      if ((its > 0 && L - Lprev < epsilon) || its == max_iterations) break;
      /* (sum_r expected[r] is sum_n m_n up to rounding; as the divisor it makes the new weights add up to 1 to R roundings) */
      for (r = 0, esum = 0.0; r < R; ++r) esum += expected[r];
      for (r = 0; r < R; ++r) w[r] = expected[r] / esum;
      Lprev = L;
    }
    free(A); free(B); free(c);
  }
  ev->em_evals = (its + 1 < PLLHIP_SITECAT_TRAIL_MAX) ? its + 1 : PLLHIP_SITECAT_TRAIL_MAX;
  pll_set_category_weights(part, w);
  /* (the vectors are per category and do not depend on the weights: the edge log-likelihood alone is new) */
  return pllhip_eval_loglh(ev, 1);
}

/* ---------------------------------------------------------------------- */
/* Newton-Raphson branch-length optimisation, linked branch lengths        */
/* ---------------------------------------------------------------------- */

typedef struct
{
  pllhip_eval_t * ev;
  double bl_min, bl_max, tolerance;
  unsigned int max_newton;
} blo_t;

static int ensure_sumtables(pllhip_eval_t * ev)
{
  unsigned int p;
  for (p = 0; p < ev->nparts; ++p)
  {
    const pll_partition_t * part = ev->parts[p];
    if (!part || ev->sumtables[p]) continue;
    /* sized and aligned exactly as the reference does it (src/tree/treeinfo.c:333-340) */
    size_t len = (size_t)part->sites * part->rate_cats * part->states_padded;
    ev->sumtables[p] = (double *)pll_aligned_alloc((len ? len : 1) * sizeof(double), part->alignment);
    if (!ev->sumtables[p])
    {
      pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate sumtable");
      return PLL_FAILURE;
    }
  }
  return PLL_SUCCESS;
}

/* first and second derivative of -lnL over all partitions at `count` trial branch
   lengths from ONE scan of every partition's sumtable (and one reduce over the workers).
   SCALED linkage: partition p is evaluated at s_p t and contributes s_p df, s_p^2 ddf (chain
   rule, src/optimize/pll_optimize.c:1240-1262). */
static int derivatives(pllhip_eval_t * ev, const pll_unode_t * e, const double * t, unsigned int count,
                       double * f, double * df)
{
  unsigned int p, k;
  double * buf = ev->slot_buf;
  double tp[PLLHIP_EVAL_MAX_TRIALS];
  for (k = 0; k < count; ++k) f[k] = df[k] = 0.0;
  if (ev->fused.fetch)
  {
    for (p = 0; p < ev->nparts; ++p)
    {
      if (!ev->parts[p]) continue;
      for (k = 0; k < count; ++k) tp[k] = ev->brlen_scalers[p] * t[k];
      if (!ev->fused.derivatives(ev->fused.results, p * 2 * count, ev->parts[p], e->scaler_index,
                                 e->back->scaler_index, tp, count, ev->params[p], ev->sumtables[p]))
      {
        poison_and_reduce(ev, buf, ev->nparts * 2 * count);
        return PLL_FAILURE;
      }
    }
    if (!ev->fused.fetch(ev->fused.results, 0, ev->nparts * 2 * count, 0 /* SUM */, buf)) return PLL_FAILURE;
    for (p = 0; p < ev->nparts; ++p)
    {
      const double sc = ev->brlen_scalers[p];
      for (k = 0; k < count; ++k)
      {
        f[k] += sc * buf[(p * count + k) * 2];
        df[k] += sc * sc * buf[(p * count + k) * 2 + 1];
      }
    }
  }
  else
  {
    double a[PLLHIP_EVAL_MAX_TRIALS], b[PLLHIP_EVAL_MAX_TRIALS];
    for (p = 0; p < ev->nparts; ++p)
    {
      const double sc = ev->brlen_scalers[p];
      int ok;
      if (!ev->parts[p]) continue;
      for (k = 0; k < count; ++k) tp[k] = sc * t[k];
      if (count == 1)
        ok = pll_compute_likelihood_derivatives(ev->parts[p], e->scaler_index, e->back->scaler_index, tp[0],
                                                ev->params[p], ev->sumtables[p], &a[0], &b[0]);
      else
        ok = pllhip_compute_likelihood_derivatives_multi(ev->parts[p], e->scaler_index,
                                                         e->back->scaler_index, tp, count, ev->params[p],
                                                         ev->sumtables[p], a, b);
      if (!ok)
      {
        poison_and_reduce(ev, buf, 2 * count);
        return PLL_FAILURE;
      }
      for (k = 0; k < count; ++k) { f[k] += sc * a[k]; df[k] += sc * sc * b[k]; }
    }
    if (ev->reduce_cb)
    {
      /* {df, ddf} of every trial length in one message (src/optimize/pll_optimize.c:1281-1284) */
      for (k = 0; k < count; ++k) { buf[2 * k] = f[k]; buf[2 * k + 1] = df[k]; }
      ev->reduce_cb(ev->ctx, buf, 2 * count, 0 /* SUM */);
      for (k = 0; k < count; ++k) { f[k] = buf[2 * k]; df[k] = buf[2 * k + 1]; }
    }
  }
  ev->n_deriv++;
  return PLL_SUCCESS;
}

/* UNLINKED: every partition at its own length x[p]; f[p], df[p] stay per partition
   (src/optimize/pll_optimize.c:1229-1279; one message of 2 P values here) */
static int derivatives_unlinked(pllhip_eval_t * ev, const pll_unode_t * e, const double * x,
                                double * f, double * df)
{
  unsigned int p;
  double * buf = ev->slot_buf;
  if (ev->fused.fetch)
  {
    for (p = 0; p < ev->nparts; ++p)
      if (ev->parts[p] &&
          !ev->fused.derivatives(ev->fused.results, 2 * p, ev->parts[p], e->scaler_index,
                                 e->back->scaler_index, &x[p], 1, ev->params[p], ev->sumtables[p]))
      {
        poison_and_reduce(ev, buf, 2 * ev->nparts);
        return PLL_FAILURE;
      }
    if (!ev->fused.fetch(ev->fused.results, 0, 2 * ev->nparts, 0 /* SUM */, buf)) return PLL_FAILURE;
  }
  else
  {
    for (p = 0; p < ev->nparts; ++p)
    {
      buf[2 * p] = buf[2 * p + 1] = 0.0;
      if (ev->parts[p] &&
          !pll_compute_likelihood_derivatives(ev->parts[p], e->scaler_index, e->back->scaler_index, x[p],
                                              ev->params[p], ev->sumtables[p], &buf[2 * p], &buf[2 * p + 1]))
      {
        poison_and_reduce(ev, buf, 2 * ev->nparts);
        return PLL_FAILURE;
      }
    }
    if (ev->reduce_cb) ev->reduce_cb(ev->ctx, buf, 2 * ev->nparts, 0 /* SUM */);
  }
  for (p = 0; p < ev->nparts; ++p) { f[p] = buf[2 * p]; df[p] = buf[2 * p + 1]; }
  ev->n_deriv++;
  return PLL_SUCCESS;
}

/* trial lengths per scan: every worker must scan with the same number (the reduce payloads
   have to match), so the local minimum over the partitions goes through one MIN reduce */
static unsigned int speculation_width(pllhip_eval_t * ev)
{
  unsigned int p;
  double v = PLLHIP_EVAL_SPECULATE_MAX;
  if (ev->spec_trials) return ev->spec_trials;
  if (ev->flags & PLLHIP_EVAL_NO_SPECULATION) v = 1;
  else if (!(ev->flags & PLLHIP_EVAL_ALWAYS_SPECULATE))
  {
    for (p = 0; p < ev->nparts; ++p)
      if (ev->parts[p]) v = PLL_MIN(v, (double)pllhip_free_trial_lengths(ev->parts[p]));
    if (ev->reduce_cb) ev->reduce_cb(ev->ctx, &v, 1, 2 /* MIN */);
    if (v < 3) v = 1;             /* the current iterate + both clamped outcomes, or nothing */
  }
  ev->spec_trials = (unsigned int)v;
  return ev->spec_trials;
}

/* the step rule of the reference's minimiser (opt_algorithms.c:208-240) clamps a Newton
   step to +-dxmax and to the bracket [xl, xh]: those outcomes are known BEFORE the
   derivatives are.  Returns the iterate a clamped step upwards (dir > 0) / downwards leads
   to from x, computed with the step rule's own expressions so that it is that iterate bit
   for bit. */
static double clamped_iterate(const blo_t * b, double x, double xl, double xh, double dxmax, int dir)
{
  double dx = dir > 0 ? dxmax : -dxmax;
  if (x + dx < xl) dx = xl - x;
  if (x + dx > xh) dx = xh - x;
  x += dx;
  return PLL_MAX(PLL_MIN(x, b->bl_max), b->bl_min);
}

static unsigned int add_trial(double * t, unsigned int n, double v)
{
  unsigned int i;
  for (i = 0; i < n; ++i) if (t[i] == v) return n;
  if (n < PLLHIP_EVAL_MAX_TRIALS) t[n++] = v;
  return n;
}

/* one-dimensional Newton-Raphson with bracketing: step rule of the reference's
   multi-function minimiser for a single function (opt_algorithms.c:133-261).  Each scan
   of the sumtables evaluates the current iterate and the iterates clamped steps would
   lead to (two levels); an iteration whose point is among the ones already evaluated
   costs no scan.  Same iterates, same results as one scan per iteration. */
static int newton(const blo_t * b, const pll_unode_t * e, double * x)
{
  pllhip_eval_t * ev = b->ev;
  const double dxmax = b->bl_max / b->max_newton;
  const unsigned int width = speculation_width(ev);     /* UNLINKED runs newton_unlinked instead */
  const int speculate = width > 1;
  double xl = b->bl_min, xh = b->bl_max, f, df, dx;
  double t[PLLHIP_EVAL_MAX_TRIALS], tf[PLLHIP_EVAL_MAX_TRIALS], tdf[PLLHIP_EVAL_MAX_TRIALS];
  unsigned int nt = 0, k, iter = 0;
  /* Every partition on this worker, one length per branch (linked, or scaled by a per-partition factor): the whole
     loop runs on the device (include/pllhip.h, pllhip_newton_branch / _multi: the same iterates, one wait per branch
     instead of one per iterate).  With other workers the sums of the derivatives have to meet on the host between
     two iterates: the loop below. */
  /* (a result group with a communicator installs the reduce callback too: pllhip_eval_attach_comm) */
  /* (PLLHIP_EVAL_ALWAYS_SPECULATE asks for the host loop's trial lengths: tests) */
  if (ev->device_newton && !ev->reduce_cb && !ev->part_brlens && !(ev->flags & PLLHIP_EVAL_ALWAYS_SPECULATE) &&
      (ev->nparts == 1 ? (ev->parts[0] && ev->brlen_scalers[0] == 1.0)
                       : (pllhip_newton_branch_multi != NULL && ev->nparts <= 8)))
  {
    unsigned int its = 0, p;
    double len = *x;
    int ok, local = 1;
    for (p = 0; p < ev->nparts; ++p) if (!ev->parts[p]) local = 0;
    if (!local) ok = 0, pll_errno = PLLHIP_ERROR_NEWTON_UNSUPPORTED;
    else if (ev->nparts == 1)
      ok = pllhip_newton_branch(ev->parts[0], e->scaler_index, e->back->scaler_index, ev->params[0], ev->sumtables[0],
                                *x, b->bl_min, b->bl_max, b->tolerance, b->max_newton, &len, &its, NULL);
    else
      ok = pllhip_newton_branch_multi(ev->parts, ev->nparts, e->scaler_index, e->back->scaler_index,
                                      (const unsigned int * const *)ev->params, (const double * const *)ev->sumtables,
                                      ev->brlen_scalers, *x, b->bl_min, b->bl_max, b->tolerance, b->max_newton,
                                      &len, &its, NULL);
    if (ok)
    {
      *x = len;
      ev->n_newton += its;
      ev->n_deriv += its;
      return PLL_SUCCESS;
    }
    if (pll_errno == PLLHIP_ERROR_NEWTON_LIMIT)
    {
      /* (counted like the loop below: it gives up BEFORE the evaluation that would exceed the limit, the device
         loop after it) */
      if (its) { ev->n_newton += its - 1; ev->n_deriv += its - 1; }
      pllhip_eval_error(PLLHIP_EVAL_ERROR_NEWTON_LIMIT, "Exceeded maximum number of iterations");
      return PLL_FAILURE;
    }
    if (pll_errno == PLLHIP_ERROR_NEWTON_DERIVATIVES)
    {
      ev->n_newton += its;
      ev->n_deriv += its;
      pllhip_eval_error(PLLHIP_EVAL_ERROR_NEWTON_DERIV, "Wrong likelihood derivatives");
      return PLL_FAILURE;
    }
    /* UNSUPPORTED: this partition cannot; STUCK: the device is shared and the loop's workgroups did not all get
       onto it (nothing was changed): either way this branch -- and the ones after it -- iterate on the host */
    if (pll_errno != PLLHIP_ERROR_NEWTON_UNSUPPORTED && pll_errno != PLLHIP_ERROR_NEWTON_STUCK) return PLL_FAILURE;
    pll_errno = 0;
    ev->device_newton = 0;
  }
  *x = PLL_MAX(PLL_MIN(*x, b->bl_max), b->bl_min);
  for (;;)
  {
    if (iter++ > b->max_newton)
    {
      pllhip_eval_error(PLLHIP_EVAL_ERROR_NEWTON_LIMIT, "Exceeded maximum number of iterations");
      return PLL_FAILURE;
    }
    for (k = 0; k < nt; ++k) if (t[k] == *x) break;
    if (k == nt)
    {
      nt = 0;
      t[nt++] = *x;
      if (speculate)
      {
        const double up = clamped_iterate(b, *x, xl, xh, dxmax, 1);
        const double dn = clamped_iterate(b, *x, xl, xh, dxmax, -1);
        nt = add_trial(t, nt, dn);
        nt = add_trial(t, nt, up);
        /* second level, while the scan stays at four lengths (beyond that the extra
           arithmetic of a length shows in the scan time): brackets as they stand after a
           step in that direction */
        if (nt < width) nt = add_trial(t, nt, clamped_iterate(b, dn, xl, *x, dxmax, -1));
        if (nt < width) nt = add_trial(t, nt, clamped_iterate(b, up, *x, xh, dxmax, 1));
      }
      if (!derivatives(ev, e, t, nt, tf, tdf)) return PLL_FAILURE;
      k = 0;
    }
    f = tf[k];
    df = tdf[k];
    ev->n_newton++;
    if (!isfinite(f) || !isfinite(df))
    {
      pllhip_eval_error(PLLHIP_EVAL_ERROR_NEWTON_DERIV, "Wrong likelihood derivatives");
      return PLL_FAILURE;
    }
    if (df > 0.0)
    {
      if (fabs(f) < b->tolerance) return PLL_SUCCESS;
      if (f < 0.0) xl = *x; else xh = *x;
      dx = -f / df;
    }
    else
      dx = -f / fabs(df);
    dx = PLL_MAX(PLL_MIN(dx, dxmax), -dxmax);
    if (*x + dx < xl) dx = xl - *x;
    if (*x + dx > xh) dx = xh - *x;
    if (fabs(dx) < b->tolerance) return PLL_SUCCESS;
    *x += dx;
    *x = PLL_MAX(PLL_MIN(*x, b->bl_max), b->bl_min);
  }
}

/* UNLINKED: one function per partition, each with its own bracket and convergence flag,
   all evaluated by one scan per iteration (pllmod_opt_minimize_newton_multi,
   src/optimize/opt_algorithms.c:133-261).  ev->nr_x holds the iterates. */
static int newton_unlinked(const blo_t * b, const pll_unode_t * e)
{
  pllhip_eval_t * ev = b->ev;
  const unsigned int n = ev->nparts;
  const double dxmax = b->bl_max / b->max_newton;
  double * x = ev->nr_x, * xl = ev->nr_xl, * xh = ev->nr_xh, * f = ev->nr_f, * df = ev->nr_df;
  int * converged = ev->nr_converged;
  unsigned int i, iter = 0;
  int all_converged = 0;
  for (i = 0; i < n; ++i)
  {
    x[i] = PLL_MAX(PLL_MIN(x[i], b->bl_max), b->bl_min);
    xl[i] = b->bl_min;
    xh[i] = b->bl_max;
    converged[i] = 0;
  }
  while (!all_converged)
  {
    if (iter++ > b->max_newton)
    {
      pllhip_eval_error(PLLHIP_EVAL_ERROR_NEWTON_LIMIT, "Exceeded maximum number of iterations");
      return PLL_FAILURE;
    }
    if (!derivatives_unlinked(ev, e, x, f, df)) return PLL_FAILURE;
    ev->n_newton++;
    all_converged = 1;
    for (i = 0; i < n; ++i)
    {
      double dx;
      if (converged[i]) continue;
      if (!isfinite(f[i]) || !isfinite(df[i]))
      {
        pllhip_eval_error(PLLHIP_EVAL_ERROR_NEWTON_DERIV, "Wrong likelihood derivatives");
        return PLL_FAILURE;
      }
      if (df[i] > 0.0)
      {
        if (fabs(f[i]) < b->tolerance) { converged[i] = 1; continue; }
        if (f[i] < 0.0) xl[i] = x[i]; else xh[i] = x[i];
        dx = -f[i] / df[i];
      }
      else
        dx = -f[i] / fabs(df[i]);
      dx = PLL_MAX(PLL_MIN(dx, dxmax), -dxmax);
      if (x[i] + dx < xl[i]) dx = xl[i] - x[i];
      if (x[i] + dx > xh[i]) dx = xh[i] - x[i];
      if (fabs(dx) < b->tolerance) { converged[i] = 1; continue; }
      x[i] += dx;
      x[i] = PLL_MAX(PLL_MIN(x[i], b->bl_max), b->bl_min);
      all_converged = 0;
    }
  }
  return PLL_SUCCESS;
}

/* recompute the CLV at `parent` from the far ends of c1 and c2
   (update_partials_and_scalers, src/optimize/pll_optimize.c:748-775) */
static int reorient(pllhip_eval_t * ev, const pll_unode_t * parent, const pll_unode_t * c1,
                    const pll_unode_t * c2)
{
  pll_operation_t op;
  unsigned int p;
  op.parent_clv_index = parent->clv_index;
  op.parent_scaler_index = parent->scaler_index;
  op.child1_clv_index = c1->back->clv_index;
  op.child1_matrix_index = c1->back->pmatrix_index;
  op.child1_scaler_index = c1->back->scaler_index;
  op.child2_clv_index = c2->back->clv_index;
  op.child2_matrix_index = c2->back->pmatrix_index;
  op.child2_scaler_index = c2->back->scaler_index;
  (void)p;
  if (!pllhip_update_partials_batch(ev->parts, ev->nparts, &op, 1)) return PLL_FAILURE;
  ev->n_ops++;
  return pll_errno ? PLL_FAILURE : PLL_SUCCESS;
}

/* this branch's P-matrix in every local partition, at the lengths now in force */
static int refresh_pmatrix(pllhip_eval_t * ev, const pll_unode_t * edge)
{
  unsigned int p;
  for (p = 0; p < ev->nparts; ++p)
  {
    double t;
    if (!ev->parts[p]) continue;
    t = effective_length(ev, p, edge->pmatrix_index, edge->length);
    if (!pll_update_prob_matrices(ev->parts[p], ev->params[p], &edge->pmatrix_index, &t, 1))
      return PLL_FAILURE;
  }
  ev->n_pmat++;
  return PLL_SUCCESS;
}

static int optimise_around(const blo_t * b, pll_unode_t * p_edge, int radius)
{
  pllhip_eval_t * ev = b->ev;
  pll_unode_t * q = p_edge->next, * z = q ? q->next : NULL;
  const unsigned int m = p_edge->pmatrix_index;
  unsigned int p;
  int changed = 0;

  for (p = 0; p < ev->nparts; ++p)
    if (ev->parts[p] &&
        !pll_update_sumtable(ev->parts[p], p_edge->clv_index, p_edge->back->clv_index,
                             p_edge->scaler_index, p_edge->back->scaler_index, ev->params[p],
                             ev->sumtables[p]))
      return PLL_FAILURE;

  if (ev->linkage == PLLHIP_EVAL_BRLEN_UNLINKED)
  {
    double * x = ev->nr_x, * orig = ev->nr_orig;
    for (p = 0; p < ev->nparts; ++p) x[p] = ev->parts[p] ? ev->part_brlens[p][m] : 0.0;
    /* every worker needs all per-partition lengths (src/optimize/pll_optimize.c:1436-1442) */
    if (ev->nparts > 1 && ev->reduce_cb) ev->reduce_cb(ev->ctx, x, ev->nparts, 1 /* MAX */);
    memcpy(orig, x, sizeof(double) * ev->nparts);
    if (!newton_unlinked(b, p_edge))
    {
      if (pll_errno != PLLHIP_EVAL_ERROR_NEWTON_LIMIT) return PLL_FAILURE;
      for (p = 0; p < ev->nparts; ++p)
        if (!ev->nr_converged[p]) x[p] = orig[p];      /* no lnL check: keep the old length */
      pll_errno = 0;
    }
    for (p = 0; p < ev->nparts; ++p)
    {
      if (fabs(x[p] - orig[p]) < 1e-10) continue;
      ev->part_brlens[p][m] = x[p];
      changed = 1;
    }
  }
  else
  {
    const double xorig = p_edge->length;
    double x = xorig;
    if (!newton(b, p_edge, &x))
    {
      if (pll_errno != PLLHIP_EVAL_ERROR_NEWTON_LIMIT) return PLL_FAILURE;
      x = xorig;                    /* no convergence, no lnL check: keep the old length */
      pll_errno = 0;
    }
    if (fabs(x - xorig) >= 1e-10)
    {
      p_edge->length = p_edge->back->length = x;
      changed = 1;
    }
  }
  if (changed && !refresh_pmatrix(ev, p_edge)) return PLL_FAILURE;
  if (radius && q && z)
  {
    if (!reorient(ev, q, p_edge, z) || !optimise_around(b, q->back, radius - 1)) return PLL_FAILURE;
    if (!reorient(ev, z, q, p_edge) || !optimise_around(b, z->back, radius - 1)) return PLL_FAILURE;
    if (!reorient(ev, p_edge, z, q)) return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

/* ---------------------------------------------------------------------- */
/* Substitution mapping: expected endpoint pairs, substitution counts and  */
/* dwell times per branch (include/pllhip.h, "substitution mapping")       */
/* ---------------------------------------------------------------------- */

/* phi(x) = expm1(x) / x, phi(0) = 1 */
static double sm_phi(double x) { return x == 0.0 ? 1.0 : expm1(x) / x; }

int pllhip_substmap_counts(unsigned int states, unsigned int states_padded, const double * eigenvecs,
                           const double * inv_eigenvecs, const double * eigenvals, double tau, const double * F,
                           double * counts, double * dwell)
{
  const unsigned int S = states, Sp = states_padded;
  const double * V = inv_eigenvecs, * W = eigenvecs;         /* V[i][k] = V[i * Sp + k], V^-1[k][j] = W[k * Sp + j] */
  double * X, * G, * Y;
  unsigned int a, b, i, j, k, l;
  if (!S || Sp < S || !eigenvecs || !inv_eigenvecs || !eigenvals || !F || !counts || !dwell || !(tau >= 0.0) || isinf(tau))
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "pllhip_substmap_counts: NULL arguments, or a time that is negative or not finite");
    return PLL_FAILURE;
  }
  X = (double *)calloc((size_t)3 * S * S, sizeof(double));
  if (!X)
  {
    pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "pllhip_substmap_counts: cannot allocate the work space");
    return PLL_FAILURE;
  }
  G = X + (size_t)S * S;
  Y = G + (size_t)S * S;
  /* X[k][j] = sum_i V[i][k] F[i][j];  G[k][l] = sum_j X[k][j] V^-1[l][j], times K[k][l] */
  for (k = 0; k < S; ++k)
    for (j = 0; j < S; ++j)
    {
      double x = 0.0;
      for (i = 0; i < S; ++i) x += V[i * Sp + k] * F[i * S + j];
      X[k * S + j] = x;
    }
  for (k = 0; k < S; ++k)
    for (l = 0; l < S; ++l)
    {
      /* K = tau e^(hi tau) phi((lo - hi) tau) with hi >= lo: symmetric, the argument of phi never positive */
      const double hi = eigenvals[k] > eigenvals[l] ? eigenvals[k] : eigenvals[l];
      const double lo = eigenvals[k] > eigenvals[l] ? eigenvals[l] : eigenvals[k];
      const double K = tau * exp(hi * tau) * sm_phi((lo - hi) * tau);
      double g = 0.0;
      for (j = 0; j < S; ++j) g += X[k * S + j] * W[l * Sp + j];
      G[k * S + l] = g * K;
    }
  /* Y[a][l] = sum_k V^-1[k][a] (G o K)[k][l];  M[a][b] = sum_l Y[a][l] V[b][l] */
  for (a = 0; a < S; ++a)
    for (l = 0; l < S; ++l)
    {
      double y = 0.0;
      for (k = 0; k < S; ++k) y += W[k * Sp + a] * G[k * S + l];
      Y[a * S + l] = y;
    }
  for (a = 0; a < S; ++a)
    for (b = 0; b < S; ++b)
    {
      double M = 0.0, q = 0.0;
      for (l = 0; l < S; ++l) M += Y[a * S + l] * V[b * Sp + l];
      if (a == b)
      {
        dwell[a] = M;
        counts[a * S + b] = 0.0;
        continue;
      }
      for (k = 0; k < S; ++k) q += V[a * Sp + k] * eigenvals[k] * W[k * Sp + b];
      counts[a * S + b] = q * M;
    }
  free(X);
  return PLL_SUCCESS;
}

/* F [cats][S][S] and differ [sites] (or NULL) of an edge on the host, from the partition's own arrays: the definitions of
   include/pllhip.h in plain C, in the order of the device kernels (scale = m ((w D) / T), pi applied to the sum) */
static int sm_host_pairs(const pll_partition_t * p, unsigned int pc, int ps, unsigned int cc, int cs, unsigned int m,
                         const unsigned int * fi, double * F, double * differ, unsigned long long * dropped)
{
  const unsigned int S = p->states, Sp = p->states_padded, R = p->rate_cats;
  const size_t N = p->sites, cells = N * R;
  double * A = (double *)calloc(cells ? 3 * cells : 1, sizeof(double)), * B = A ? A + cells : NULL, * D = A ? B + cells : NULL;
  unsigned int * c = (unsigned int *)calloc(N ? N : 1, sizeof(unsigned int));
  size_t n;
  unsigned int r, i, j;
  if (!A || !c)
  {
    free(A); free(c);
    pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the site-category table");
    return 0;
  }
  sc_host_table_scaled(p, pc, ps, cc, cs, m, fi, A, B, c, D);
  memset(F, 0, sizeof(double) * R * S * S);
  *dropped = 0;
  for (n = 0; n < N; ++n)
  {
    double T = 0.0, df = 0.0;
    for (r = 0; r < R; ++r) T += p->rate_weights[r] * (A[n * R + r] + B[n * R + r]);
    if (!(T > 0.0))
    {
      if (p->pattern_weights[n]) ++*dropped;
      if (differ) differ[n] = 0.0;
      continue;
    }
    for (r = 0; r < R; ++r)
    {
      const double * pi = p->frequencies[fi[r]];
      const double * P = p->pmatrix[m] + (size_t)r * S * Sp;
      const double scale = (double)p->pattern_weights[n] * ((p->rate_weights[r] * D[n * R + r]) / T);
      double * Fr = F + (size_t)r * S * S, l0 = 0.0;
      for (i = 0; i < S; ++i)
      {
        const double pa = sc_elem(p, pc, n, r, i), a = scale * pa;
        double off = 0.0;
        if (pa == 0.0) continue;
        for (j = 0; j < S; ++j)
        {
          const double ch = sc_elem(p, cc, n, r, j);
          Fr[i * S + j] += a * ch;
          if (j != i) off += P[i * Sp + j] * ch;
        }
        l0 += pi[i] * pa * off;
      }
      df += (p->rate_weights[r] * (D[n * R + r] * l0)) / T;
    }
    if (differ) differ[n] = df;
  }
  for (r = 0; r < R; ++r)
    for (i = 0; i < S; ++i)
      for (j = 0; j < S; ++j) F[((size_t)r * S + i) * S + j] *= p->frequencies[fi[r]][i];
  free(A); free(c);
  return 1;
}

static void sm_destroy_branch(pllhip_branch_subst_t * b)
{
  free(b->pairs); free(b->counts); free(b->dwell); free(b->differ);
}

void pllhip_eval_destroy_substitution_map(pllhip_substitution_map_t * map)
{
  unsigned int k, m;
  if (!map) return;
  for (k = 0; map->branches && k < map->partition_count; ++k)
  {
    for (m = 0; map->branches[k] && m < map->branch_count; ++m) sm_destroy_branch(&map->branches[k][m]);
    free(map->branches[k]);
  }
  free(map->branches);
  free(map->partition_indices);
  free(map);
}

typedef struct
{
  pllhip_eval_t * ev;
  pllhip_substitution_map_t * map;
  unsigned int flags;
  int device;
} sm_walk_t;

/* the record of branch `edge` in every local partition; the vectors of both ends point at each other */
static int sm_edge(const sm_walk_t * w, pll_unode_t * edge)
{
  pllhip_eval_t * ev = w->ev;
  const unsigned int m = edge->pmatrix_index;
  unsigned int p, k = 0, r, x;
  for (p = 0; p < ev->nparts; ++p)
  {
    pll_partition_t * part = ev->parts[p];
    const unsigned int * fi = ev->params[p];
    pllhip_branch_subst_t * b;
    unsigned int S, R;
    size_t cells;
    double t, * F = NULL, * cr, * dr;
    if (!part) continue;
    S = part->states; R = part->rate_cats; cells = (size_t)R * S * S;
    b = &w->map->branches[k++][m];
    b->node = edge;
    b->states = S; b->cats = R; b->sites = part->sites;
    b->pairs = (double *)calloc(cells, sizeof(double));
    b->counts = (double *)calloc((size_t)S * S, sizeof(double));
    b->dwell = (double *)calloc(S, sizeof(double));
    if (w->flags & PLLHIP_SUBST_SITES) b->differ = (double *)calloc(part->sites ? part->sites : 1, sizeof(double));
    F = (double *)calloc(cells + (size_t)S * S + S, sizeof(double));
    if (!b->pairs || !b->counts || !b->dwell || ((w->flags & PLLHIP_SUBST_SITES) && !b->differ) || !F)
    {
      free(F);
      pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the substitution map");
      return 0;
    }
    cr = F + cells; dr = cr + (size_t)S * S;
    if (w->device)
    {
      pllhip_edge_pairs_t * ep = pllhip_substmap_edge(part, edge->clv_index, edge->scaler_index, edge->back->clv_index,
                                                      edge->back->scaler_index, m, fi, w->flags);
      if (!ep) { free(F); return 0; }
      memcpy(F, ep->F, sizeof(double) * cells);
      memcpy(b->pairs, ep->pairs, sizeof(double) * cells);
      if (b->differ && part->sites) memcpy(b->differ, ep->differ, sizeof(double) * part->sites);
      b->dropped = ep->dropped;
      pllhip_edge_pairs_destroy(ep);
    }
    else
    {
      if (!sm_host_pairs(part, edge->clv_index, edge->scaler_index, edge->back->clv_index, edge->back->scaler_index, m, fi,
                         F, b->differ, &b->dropped)) { free(F); return 0; }
      for (r = 0; r < R; ++r)
        for (x = 0; x < S * S; ++x)
          b->pairs[(size_t)r * S * S + x] = F[(size_t)r * S * S + x] * part->pmatrix[m][((size_t)r * S + x / S) * part->states_padded + x % S];
    }
    for (x = 0; x < cells; ++x) b->posterior_weight += b->pairs[x];
    /* the time of category r: what pll_update_prob_matrices exponentiates under */
    t = effective_length(ev, p, m, edge->length);
    for (r = 0; r < R; ++r)
    {
      const double q = part->prop_invar[fi[r]];
      const double tau = part->rates[r] * t / (1.0 - q);
      if (!part->eigen_decomp_valid[fi[r]] && !pll_update_eigen(part, fi[r])) { free(F); return 0; }
      if (!pllhip_substmap_counts(S, part->states_padded, part->eigenvecs[fi[r]], part->inv_eigenvecs[fi[r]],
                                  part->eigenvals[fi[r]], tau, F + (size_t)r * S * S, cr, dr)) { free(F); return 0; }
      for (x = 0; x < S * S; ++x) b->counts[x] += cr[x];
      for (x = 0; x < S; ++x) b->dwell[x] += dr[x];
    }
    for (x = 0; x < S * S; ++x) b->total += b->counts[x];
    free(F);
  }
  return 1;
}

/* every branch once, by the re-rooting walk of optimise_around: the vector of an inner node is turned towards each of
   its neighbours in turn and put back as it was */
static int sm_walk(const sm_walk_t * w, pll_unode_t * edge, int visit)
{
  pll_unode_t * q = edge->next, * z = q ? q->next : NULL;
  if (visit && !sm_edge(w, edge)) return 0;
  if (q && z)
  {
    if (!reorient(w->ev, q, edge, z) || !sm_walk(w, q->back, 1)) return 0;
    if (!reorient(w->ev, z, q, edge) || !sm_walk(w, z->back, 1)) return 0;
    if (!reorient(w->ev, edge, z, q)) return 0;
  }
  return 1;
}

pllhip_substitution_map_t * pllhip_eval_substitution_map(pllhip_eval_t * ev, unsigned int flags)
{
  sm_walk_t w;
  pllhip_substitution_map_t * map;
  unsigned int p, k = 0, local = 0;
  pll_errno = 0;
  if (flags & ~PLLHIP_SUBST_SITES)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "unknown flags for the substitution map");
    return NULL;
  }
  for (p = 0; p < ev->nparts; ++p) if (ev->parts[p]) ++local;
  if (!local)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "substitution map: no local partition");
    return NULL;
  }
  ev->last_was_full = 0;
  if (!update_vectors(ev, 0))
  {
    if (!pll_errno) pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "substitution map: the traversal failed");
    return NULL;
  }
  map = (pllhip_substitution_map_t *)calloc(1, sizeof(*map));
  if (map)
  {
    map->partition_count = local;
    map->branch_count = ev->edges;
    map->partition_indices = (unsigned int *)calloc(local, sizeof(unsigned int));
    map->branches = (pllhip_branch_subst_t **)calloc(local, sizeof(*map->branches));
    for (p = 0; map->partition_indices && map->branches && p < ev->nparts; ++p)
      if (ev->parts[p])
      {
        map->partition_indices[k] = p;
        map->branches[k] = (pllhip_branch_subst_t *)calloc(ev->edges, sizeof(pllhip_branch_subst_t));
        if (!map->branches[k++]) break;
      }
  }
  if (!map || k < local)
  {
    pllhip_eval_destroy_substitution_map(map);
    pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the substitution map");
    return NULL;
  }
  w.ev = ev; w.map = map; w.flags = flags;
  w.device = pllhip_substmap_edge && pllhip_edge_pairs_destroy;
  if (sm_walk(&w, ev->root, 1) && sm_walk(&w, ev->root->back, 0) && !pll_errno) return map;
  if (!pll_errno) pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "substitution map: the walk failed");
  pllhip_eval_destroy_substitution_map(map);
  /* the walk stopped with some vector turned away from the root: let the next evaluation rebuild them */
  memset(ev->clv_valid, 0, ev->records);
  return NULL;
}

/* ---------------------------------------------------------------------- */
/* Sampled ancestral states: one draw of all unobserved nodes from their    */
/* joint posterior (include/pllhip.h, "sampled ancestral states")           */
/* ---------------------------------------------------------------------- */

/* the draws of the simulation contract (rell_mix, sim_key, sim_u, the bisection of sim_pick) */
static unsigned long long as_mix(unsigned long long seed, unsigned long long c)
{
  unsigned long long z = seed + (c + 1ULL) * 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

static double as_u(unsigned long long seed, unsigned long long b, unsigned int stream, unsigned long long n)
{
  return (double)(as_mix(as_mix(seed, (b << 32) | stream), n) >> 11) * 0x1.0p-53;
}

/* cum[0 .. n): the masses cumulated left to right; the pick for the draw u */
static unsigned int as_pick(const double * cum, unsigned int n, double u)
{
  const double x = u * cum[n - 1];
  unsigned int lo = 0, hi = n - 1;
  while (lo < hi)
  {
    const unsigned int mid = (lo + hi) >> 1;
    if (cum[mid] > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

static int as_check(const pll_partition_t * part, unsigned int p, const pllhip_ancsample_params_t * params,
                    const unsigned int * fi)
{
  unsigned int r;
  double sum = 0.0;
  if (part->states > 256 || part->rate_cats > 128)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled ancestral states: partition %u has more than 256 states or more "
                      "than 128 categories", p);
    return 0;
  }
  if (params->alphabet && strnlen(params->alphabet, part->states) < part->states)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled ancestral states: the alphabet has fewer than %u characters "
                      "(partition %u)", part->states, p);
    return 0;
  }
  for (r = 0; r < part->rate_cats; ++r)
  {
    if (fi[r] >= part->rate_matrices)
    {
      pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled ancestral states: parameter index %u of category %u of "
                        "partition %u is out of range", fi[r], r, p);
      return 0;
    }
    if (!(part->rate_weights[r] >= 0.0) || !isfinite(part->rate_weights[r]))
    {
      pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled ancestral states: weight %u of partition %u is negative or "
                        "not finite", r, p);
      return 0;
    }
    sum += part->rate_weights[r];
  }
  if (sum > 0.0) return 1;
  pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled ancestral states: the weights of partition %u add up to 0", p);
  return 0;
}

/* The contract of INTEGRATION.md, "Sampled ancestral states", in plain C from the partition's host arrays: the second
   implementation of k_ancsample_walk, for libraries that keep host arrays.  The edges come parents first (as_edges);
   edge 0 is the root edge.  Every product and sum is one fp64 operation in the order written (the file is built
   without contraction).  0: out of memory. */
static int as_host(const pll_partition_t * part, const pllhip_ancsample_params_t * params, unsigned int edge_count,
                   const unsigned int * parent, const unsigned int * child, const unsigned int * matrix,
                   const double * A, const double * B, const unsigned int * fi, unsigned int node_count,
                   unsigned char * out, unsigned char * component, unsigned long long * dropped)
{
  const unsigned int S = part->states, Sp = part->states_padded, R = part->rate_cats, tips = part->tips;
  const size_t N = part->sites;
  const int with_tips = (params->flags & PLLHIP_ANCS_TIPS) != 0;
  const unsigned int root = parent[0], other = child[0], m0 = matrix[0];
  double * comp = (double *)malloc(sizeof(double) * (2 * R + S)), * cum = comp ? comp + 2 * R : NULL;   /* [2R], [S] */
  unsigned char * state = (unsigned char *)malloc(node_count ? node_count : 1);
  size_t n;
  unsigned int b, r, i, j, k;
  *dropped = 0;
  if (!comp || !state) { free(comp); free(state); return 0; }
  for (n = 0; n < N; ++n)
  {
    double acc = 0.0;
    for (r = 0; r < R; ++r)
    {
      acc = acc + part->rate_weights[r] * A[n * R + r];
      comp[2 * r] = acc;
      acc = acc + part->rate_weights[r] * B[n * R + r];
      comp[2 * r + 1] = acc;
    }
    if (!(acc > 0.0) || !isfinite(acc))
    {
      if (part->pattern_weights[n] > 0) ++*dropped;     /* (the caller filled everything with 0xFF) */
      continue;
    }
    for (b = 0; b < params->replicates; ++b)
    {
      const unsigned long long rep = (unsigned long long)params->first_replicate + b;
      unsigned char * rows = out + (size_t)b * node_count * N + n;
      int inv;
      k = as_pick(comp, 2 * R, as_u(params->seed, rep, 0, n));
      r = k >> 1;
      inv = (int)(k & 1u);
      if (component) component[(size_t)b * N + n] = (unsigned char)(r | (inv ? 0x80u : 0u));
      if (inv) state[root] = (unsigned char)((part->invariant ? part->invariant[n] : -1) & 255);
      else
      {
        const double * P = part->pmatrix[m0] + (size_t)r * S * Sp, * pi = part->frequencies[fi[r]];
        acc = 0.0;
        for (i = 0; i < S; ++i)
        {
          double t = 0.0;
          for (j = 0; j < S; ++j) t = t + P[i * Sp + j] * sc_elem(part, other, n, r, j);
          acc = acc + (pi[i] * sc_elem(part, root, n, r, i)) * t;
          cum[i] = acc;
        }
        state[root] = (unsigned char)as_pick(cum, S, as_u(params->seed, rep, 2, n));
      }
      for (k = 0; k <= edge_count; ++k)
      {
        const unsigned int node = k ? child[k - 1] : root;
        if (k && inv) state[node] = state[root];
        else if (k)
        {
          const double * row = part->pmatrix[matrix[k - 1]] + ((size_t)r * S + state[parent[k - 1]]) * Sp;
          acc = 0.0;
          for (j = 0; j < S; ++j)
          {
            acc = acc + row[j] * sc_elem(part, node, n, r, j);
            cum[j] = acc;
          }
          state[node] = (unsigned char)as_pick(cum, S, as_u(params->seed, rep, 3u + matrix[k - 1], n));
        }
        if (node >= tips || with_tips)
          rows[(size_t)node * N] = state[node] == 255 || !params->alphabet ? state[node]
                                                                            : (unsigned char)params->alphabet[state[node]];
      }
    }
  }
  free(comp);
  free(state);
  return 1;
}

/* the edges of the tree seen from the inner record `root`, parents first and root -> root->back first; 0: out of
   memory.  (The walk of pllhip_simulate_utree.) */
static int as_edges(const pllhip_eval_t * ev, const pll_unode_t * root, unsigned int ** parent, unsigned int ** child,
                    unsigned int ** matrix, unsigned int * count, double * length)
{
  const size_t cap = (size_t)ev->edges + 1;
  const pll_unode_t ** stack = (const pll_unode_t **)malloc((cap + 1) * sizeof(pll_unode_t *));
  size_t top = 0;
  *parent = (unsigned int *)malloc(cap * sizeof(unsigned int));
  *child = (unsigned int *)malloc(cap * sizeof(unsigned int));
  *matrix = (unsigned int *)malloc(cap * sizeof(unsigned int));
  *count = 0;
  if (!stack || !*parent || !*child || !*matrix)
  {
    free((void *)stack); free(*parent); free(*child); free(*matrix);
    *parent = *child = *matrix = NULL;
    return 0;
  }
  stack[top++] = root;
  while (top)
  {
    const pll_unode_t * entry = stack[--top];
    const pll_unode_t * n = entry == root ? entry : entry->next;
    if (!n) continue;
    do
    {
      if (*count == cap) break;
      (*parent)[*count] = n->clv_index;
      (*child)[*count] = n->back->clv_index;
      (*matrix)[*count] = n->pmatrix_index;
      if (length) length[*count] = n->length;           /* [edges + 1], the tree's own lengths */
      ++*count;
      stack[top++] = n->back;
      n = n->next;
    } while (n != entry);
  }
  free((void *)stack);
  return 1;
}

void pllhip_eval_destroy_sampled_ancestral(pllhip_sampled_ancestral_t * sa)
{
  unsigned int k;
  if (!sa) return;
  for (k = 0; k < sa->partition_count; ++k)
  {
    if (sa->out) free(sa->out[k]);
    if (sa->component) free(sa->component[k]);
  }
  free(sa->out); free(sa->component); free(sa->dropped); free(sa->sites); free(sa->partition_indices);
  free(sa->clv_index);
  free(sa);
}

/* what both sampling calls do first: the root edge from its inner end, the checks of every local partition, and a full
   evaluation at the current root that stores every vector.  0: refused or failed (pll_errno set) */
static int as_begin(pllhip_eval_t * ev, const pllhip_ancsample_params_t * params, const pll_unode_t ** root_out,
                    unsigned int * rows_out, unsigned int * local_out)
{
  const pll_unode_t * root;
  unsigned int p, rows = 0, local = 0;
  root = ev->root->next ? ev->root : ev->root->back;         /* the same edge from its inner end */
  if (!root->next)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled ancestral states: the root edge joins two tips");
    return 0;
  }
  for (p = 0; p < ev->nparts; ++p)
    if (ev->parts[p])
    {
      if (!as_check(ev->parts[p], p, params, ev->params[p])) return 0;
      if (ev->parts[p]->tips + ev->parts[p]->clv_buffers > rows) rows = ev->parts[p]->tips + ev->parts[p]->clv_buffers;
      ++local;
    }
  if (!local)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled ancestral states: no local partition");
    return 0;
  }
  /* a full evaluation at the current root that stores every vector: evaluate-only mode is off for it, and the next
     full evaluation decides anew */
  pllhip_eval_invalidate_all(ev);
  if (ev->transient != PLLHIP_EVAL_TRANSIENT_OFF) partitions_transient(ev, 0, 1);
  ev->last_was_full = 0;
  if (!update_vectors(ev, 0))
  {
    if (!pll_errno) pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled ancestral states: the traversal failed");
    return 0;
  }
  *root_out = root; *rows_out = rows; *local_out = local;
  return 1;
}

pllhip_sampled_ancestral_t * pllhip_eval_sample_ancestral(pllhip_eval_t * ev, const pllhip_ancsample_params_t * params)
{
  const int device = pllhip_sample_ancestral_edges != NULL;
  const pll_unode_t * root;
  pllhip_sampled_ancestral_t * sa = NULL;
  unsigned int * parent = NULL, * child = NULL, * matrix = NULL;
  unsigned int p, k = 0, local = 0, count = 0, rows = 0, i;
  pll_errno = 0;
  if (!params || !params->replicates || (params->flags & ~(unsigned int)(PLLHIP_ANCS_TIPS | PLLHIP_ANCS_COMPONENT)) ||
      (unsigned long long)params->first_replicate + params->replicates > (1ULL << 32))
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled ancestral states: NULL parameters, zero replicates, unknown "
                      "flags or a replicate number of 2^32 or more");
    return NULL;
  }
  if (!as_begin(ev, params, &root, &rows, &local)) return NULL;
  sa = (pllhip_sampled_ancestral_t *)calloc(1, sizeof(*sa));
  if (!sa || !as_edges(ev, root, &parent, &child, &matrix, &count, NULL)) goto nomem;
  sa->partition_count = local;
  sa->node_count = rows;
  sa->replicates = params->replicates;
  sa->partition_indices = (unsigned int *)calloc(local, sizeof(unsigned int));
  sa->sites = (unsigned int *)calloc(local, sizeof(unsigned int));
  sa->dropped = (unsigned long long *)calloc(local, sizeof(unsigned long long));
  sa->out = (unsigned char **)calloc(local, sizeof(unsigned char *));
  sa->component = (unsigned char **)calloc(local, sizeof(unsigned char *));
  sa->clv_index = (unsigned int *)calloc(rows ? rows : 1, sizeof(unsigned int));
  if (!sa->partition_indices || !sa->sites || !sa->dropped || !sa->out || !sa->component || !sa->clv_index) goto nomem;
  for (i = 0; i < rows; ++i) sa->clv_index[i] = i;
  for (p = 0; p < ev->nparts; ++p)
  {
    pll_partition_t * part = ev->parts[p];
    size_t cells;
    int ok;
    if (!part) continue;
    cells = (size_t)params->replicates * part->sites;
    sa->partition_indices[k] = p;
    sa->sites[k] = part->sites;
    sa->out[k] = (unsigned char *)malloc(cells && rows ? cells * rows : 1);
    sa->component[k] = (unsigned char *)malloc(cells ? cells : 1);
    if (!sa->out[k] || !sa->component[k]) goto nomem;
    memset(sa->out[k], 0xFF, cells * rows);
    memset(sa->component[k], 0xFF, cells);
    if (device)
    {
      pllhip_ancsample_params_t q = *params;
      q.flags |= PLLHIP_ANCS_COMPONENT;
      ok = pllhip_sample_ancestral_edges(part, &q, root->clv_index, root->scaler_index, root->back->clv_index,
                                         root->back->scaler_index, count, parent, child, matrix, ev->params[p], rows,
                                         sa->out[k], sa->component[k], &sa->dropped[k]);
    }
    else
    {
      double * A, * B;
      unsigned int * c;
      const pll_unode_t * saved = ev->root;
      ev->root = (pll_unode_t *)root;                      /* (sc_host_root_table reads the edge from ev->root) */
      ok = sc_host_root_table(ev, p, &A, &B, &c);
      ev->root = (pll_unode_t *)saved;
      if (ok)
      {
        ok = as_host(part, params, count, parent, child, matrix, A, B, ev->params[p], rows, sa->out[k],
                     sa->component[k], &sa->dropped[k]);
        free(A); free(B); free(c);
        if (!ok) goto nomem;
      }
    }
    if (!ok) goto fail;
    ++k;
  }
  free(parent); free(child); free(matrix);
  return sa;
nomem:
  pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the sampled ancestral states");
fail:
  if (!pll_errno) pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled ancestral states: the call failed");
  free(parent); free(child); free(matrix);
  pllhip_eval_destroy_sampled_ancestral(sa);
  return NULL;
}

/* ---------------------------------------------------------------------- */
/* Sampled substitution histories: stochastic mapping by uniformization,    */
/* conditioned on the sampled ends of every branch (include/pllhip.h,       */
/* "sampled substitution histories"; the process: INTEGRATION.md)           */
/* ---------------------------------------------------------------------- */

int pllhip_history_rate_table(unsigned int states, unsigned int states_padded, const double * eigenvecs,
                              const double * inv_eigenvecs, const double * eigenvals, unsigned int K, double * mu,
                              double * Rpow)
{
  const size_t S = states, Sp = states_padded, SS = S * S;
  const double * W = eigenvecs, * V = inv_eigenvecs;
  double * Q, * R, m = 0.0;
  size_t a, b, d, k;
  if (!states || !K || !eigenvecs || !inv_eigenvecs || !eigenvals || !mu || !Rpow)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "pllhip_history_rate_table: a NULL argument, no states or K = 0");
    return PLL_FAILURE;
  }
  Q = (double *)calloc(2 * SS, sizeof(double));
  if (!Q)
  {
    pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the rate table");
    return PLL_FAILURE;
  }
  R = Q + SS;
  for (a = 0; a < S; ++a)
  {
    double sum = 0.0;
    for (b = 0; b < S; ++b)
    {
      double q = 0.0;
      if (b == a) continue;
      for (k = 0; k < S; ++k) q += V[a * Sp + k] * eigenvals[k] * W[k * Sp + b];
      Q[a * S + b] = q > 0.0 ? q : 0.0;
      sum = sum + Q[a * S + b];
    }
    Q[a * S + a] = -sum;
    if (sum > m) m = sum;
  }
  *mu = m;
  for (a = 0; a < S; ++a)
  {
    double off = 0.0;
    if (!(m > 0.0)) { R[a * S + a] = 1.0; continue; }
    for (b = 0; b < S; ++b)
    {
      if (b == a) continue;
      R[a * S + b] = Q[a * S + b] / m;
      off = off + R[a * S + b];
    }
    R[a * S + a] = 1.0 - off > 0.0 ? 1.0 - off : 0.0;
  }
  memset(Rpow, 0, sizeof(double) * SS);
  for (a = 0; a < S; ++a) Rpow[a * S + a] = 1.0;
  for (k = 1; k < K; ++k)
  {
    const double * prev = Rpow + (k - 1) * SS;
    double * next = Rpow + k * SS;
    for (a = 0; a < S; ++a)
      for (b = 0; b < S; ++b)
      {
        double acc = 0.0;
        for (d = 0; d < S; ++d) acc = acc + prev[a * S + d] * R[d * S + b];
        next[a * S + b] = acc;
      }
  }
  free(Q);
  return PLL_SUCCESS;
}

int pllhip_history_poisson(double lambda, double * pois, unsigned int * K)
{
  double loglam, sum = 0.0;
  unsigned int k;
  if (!pois || !K || !(lambda >= 0.0) || !isfinite(lambda))
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "pllhip_history_poisson: a NULL argument, or lambda negative or not finite");
    return PLL_FAILURE;
  }
  if (lambda == 0.0)
  {
    pois[0] = 1.0;
    *K = 1;
    return PLL_SUCCESS;
  }
  loglam = log(lambda);
  for (k = 0; k <= PLLHIP_HIST_MAX_TABLE; ++k)
  {
    const double p = exp((double)k * loglam - lambda - lgamma((double)k + 1.0));
    if ((double)k > lambda && p < 0x1.0p-70 * sum)
    {
      *K = k;
      return PLL_SUCCESS;
    }
    if (k == PLLHIP_HIST_MAX_TABLE) break;
    pois[k] = p;
    sum = sum + p;
  }
  pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "pllhip_history_poisson: lambda = %g needs more than %u entries", lambda,
                    PLLHIP_HIST_MAX_TABLE);
  return PLL_FAILURE;
}

int pllhip_history_summary(unsigned int states, unsigned int cats, const double * tau,
                           const unsigned long long * counts_int, const unsigned long long * units, double * counts,
                           double * dwell, double * total)
{
  const size_t S = states;
  size_t x, r;
  double sum = 0.0;
  if (!tau || !counts_int || !units || !counts || !dwell || !total)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "pllhip_history_summary: a NULL argument");
    return PLL_FAILURE;
  }
  for (x = 0; x < S * S; ++x)
  {
    counts[x] = (double)counts_int[x];
    sum += counts[x];
  }
  for (x = 0; x < S; ++x)
  {
    double d = 0.0;
    for (r = 0; r < cats; ++r) d = d + (tau[r] * 0x1.0p-32) * (double)(long long)units[r * S + x];
    dwell[x] = d;
  }
  *total = sum;
  return PLL_SUCCESS;
}

void pllhip_history_tables_destroy(pllhip_history_tables_t * t)
{
  if (!t) return;
  free(t->slot); free(t->mu); free(t->rpow); free(t->tau); free(t->len); free(t->off); free(t->pois);
  free(t);
}

pllhip_history_tables_t * pllhip_history_tables_create(const pll_partition_t * part, unsigned int edge_count,
                                                       const unsigned int * matrix_indices,
                                                       const unsigned int * params_indices,
                                                       const double * branch_lengths, const char * who)
{
  pllhip_history_tables_t * t;
  unsigned int S, R, e, r, s, * rm = NULL;
  unsigned long long wsum = 0, cap = 0;
  double tmp[PLLHIP_HIST_MAX_TABLE], * one = NULL;
  size_t n;
  if (!part || !params_indices || (edge_count && (!matrix_indices || !branch_lengths)))
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "%s: the partition, params_indices, the edge list or the branch lengths "
                      "are NULL", who);
    return NULL;
  }
  S = part->states; R = part->rate_cats;
  for (n = 0; n < part->sites; ++n) wsum += part->pattern_weights[n];
  if (wsum >= (1ULL << 31))
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "%s: the pattern weights add up to %llu, 2^31 or more", who, wsum);
    return NULL;
  }
  for (r = 0; r < R; ++r)
  {
    if (params_indices[r] >= part->rate_matrices)
    {
      pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "%s: parameter index %u of category %u out of range (%u rate matrices)",
                        who, params_indices[r], r, part->rate_matrices);
      return NULL;
    }
    if (!part->eigen_decomp_valid[params_indices[r]])
    {
      pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "%s: the eigen system of rate matrix %u is not valid: no matrix can "
                        "have been made from it", who, params_indices[r]);
      return NULL;
    }
  }
  for (e = 0; e < edge_count; ++e)
  {
    if (matrix_indices[e] >= PLLHIP_HIST_MAX_MATRIX)
    {
      pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "%s: matrix index %u of edge %u is 2^19 or more", who,
                        matrix_indices[e], e);
      return NULL;
    }
    if (!(branch_lengths[e] >= 0.0) || !isfinite(branch_lengths[e]))
    {
      pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "%s: the length of edge %u is negative or not finite", who, e);
      return NULL;
    }
  }
  t = (pllhip_history_tables_t *)calloc(1, sizeof(*t));
  rm = (unsigned int *)calloc(R ? R : 1, sizeof(unsigned int));
  one = (double *)calloc((size_t)S * S + 1, sizeof(double));
  if (!t || !rm || !one) goto nomem;
  t->states = S; t->cats = R; t->edge_count = edge_count;
  t->kmax = 2;
  t->slot = (unsigned int *)calloc(R ? R : 1, sizeof(unsigned int));
  t->mu = (double *)calloc(R ? R : 1, sizeof(double));
  t->tau = (double *)calloc((size_t)edge_count * R + 1, sizeof(double));
  t->len = (unsigned int *)calloc((size_t)edge_count * R + 1, sizeof(unsigned int));
  t->off = (unsigned long long *)calloc((size_t)edge_count * R + 1, sizeof(unsigned long long));
  if (!t->slot || !t->mu || !t->tau || !t->len || !t->off) goto nomem;
  /* the distinct rate matrices and their mu */
  for (r = 0; r < R; ++r)
  {
    const unsigned int i = params_indices[r];
    for (s = 0; s < t->nmat && rm[s] != i; ++s) ;
    t->slot[r] = s;
    if (s < t->nmat) continue;
    rm[t->nmat++] = i;
    if (!pllhip_history_rate_table(S, part->states_padded, part->eigenvecs[i], part->inv_eigenvecs[i],
                                   part->eigenvals[i], 1, &t->mu[s], one)) goto fail;
  }
  /* the Poisson table of every (edge, category) */
  for (e = 0; e < edge_count; ++e)
    for (r = 0; r < R; ++r)
    {
      const double tau = part->rates[r] * branch_lengths[e] / (1.0 - part->prop_invar[params_indices[r]]);
      const double lambda = t->mu[t->slot[r]] * tau;
      unsigned int K = 0;
      if (!(lambda >= 0.0) || !isfinite(lambda) || !pllhip_history_poisson(lambda, tmp, &K))
      {
        pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "%s: edge %u (matrix %u), category %u: mu tau = %g needs a table of "
                          "more than %u entries", who, e, matrix_indices[e], r, lambda, PLLHIP_HIST_MAX_TABLE);
        goto fail;
      }
      if (t->pois_count + K > cap)
      {
        double * grown;
        cap = 2 * cap + K + 1024;
        grown = (double *)realloc(t->pois, (size_t)cap * sizeof(double));
        if (!grown) goto nomem;
        t->pois = grown;
      }
      memcpy(t->pois + t->pois_count, tmp, sizeof(double) * K);
      t->tau[(size_t)e * R + r] = tau;
      t->len[(size_t)e * R + r] = K;
      t->off[(size_t)e * R + r] = t->pois_count;
      t->pois_count += K;
      if (K > t->kmax) t->kmax = K;
    }
  t->rpow = (double *)calloc((size_t)(t->nmat ? t->nmat : 1) * t->kmax * S * S, sizeof(double));
  if (!t->rpow) goto nomem;
  for (s = 0; s < t->nmat; ++s)
    if (!pllhip_history_rate_table(S, part->states_padded, part->eigenvecs[rm[s]], part->inv_eigenvecs[rm[s]],
                                   part->eigenvals[rm[s]], t->kmax, &t->mu[s], t->rpow + (size_t)s * t->kmax * S * S))
      goto fail;
  free(rm); free(one);
  return t;
nomem:
  pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "%s: cannot allocate the history tables", who);
fail:
  free(rm); free(one);
  pllhip_history_tables_destroy(t);
  return NULL;
}

static int hs_cmp(const void * a, const void * b)
{
  const unsigned long long x = *(const unsigned long long *)a, y = *(const unsigned long long *)b;
  return x < y ? -1 : x > y;
}

/* One site of one edge in one replicate, in plain C: the second implementation of k_history_edges.  a, c: the sampled
   states at the parent and the child, r the sampled category.  cum holds max(kmax, states) doubles, key 1023 words.
   Returns the number of real jumps, or -1 for a dropped edge (nothing added). */
static int hs_site(const pllhip_history_tables_t * T, unsigned long long seed, unsigned long long rep, unsigned int m,
                   unsigned int e, unsigned long long n, unsigned int r, unsigned int a, unsigned int c,
                   unsigned long long w, unsigned long long * counts, unsigned long long * units, double * cum,
                   unsigned long long * key)
{
  const size_t S = T->states, SS = S * S;
  const unsigned int K = T->len[(size_t)e * T->cats + r], base = PLLHIP_HIST_STREAM + (m << 11);
  const double * pois = T->pois + T->off[(size_t)e * T->cats + r];
  const double * rp = T->rpow + (size_t)T->slot[r] * T->kmax * SS, * R1 = rp + SS;
  double acc = 0.0;
  unsigned int k, i, N, x = a;
  int real = 0;
  for (k = 0; k < K; ++k)
  {
    acc = acc + pois[k] * rp[k * SS + a * S + c];
    cum[k] = acc;
  }
  if (!(acc > 0.0) || !isfinite(acc)) return -1;
  N = as_pick(cum, K, as_u(seed, rep, base, n));
  /* the event times in order: (T_i, i) ascending */
  for (i = 1; i <= N; ++i) key[i - 1] = ((as_mix(as_mix(seed, (rep << 32) | (base + 1024u + i)), n) >> 32) << 10) | i;
  qsort(key, N, sizeof(unsigned long long), hs_cmp);
  for (i = 1; i <= N; ++i)
  {
    const double * to = rp + (size_t)(N - i) * SS;
    unsigned int d, y;
    acc = 0.0;
    for (d = 0; d < S; ++d)
    {
      acc = acc + R1[x * S + d] * to[d * S + c];
      cum[d] = acc;
    }
    y = as_pick(cum, (unsigned int)S, as_u(seed, rep, base + i, n));
    if (y != x)
    {
      const unsigned long long t = key[i - 1] >> 10;
      counts[x * S + y] += w;
      units[x] += w * t;
      units[y] -= w * t;
      ++real;
      x = y;
    }
  }
  units[c] += w << 32;
  return real;
}

/* every replicate, edge and site of a partition on the host, from the identity-coded rows of the ancestral draw
   (`states`: [replicate][node_count][sites] with the tip rows, `comp`: [replicate][sites]).  0: out of memory. */
static int hs_host(const pll_partition_t * part, const pllhip_ancsample_params_t * params,
                   const pllhip_history_tables_t * T, unsigned int edge_count, const unsigned int * parent,
                   const unsigned int * child, const unsigned int * matrix, unsigned int node_count,
                   const unsigned char * states, const unsigned char * comp, unsigned long long * counts,
                   unsigned long long * units, unsigned char * changes, unsigned long long * dropped_edges)
{
  const size_t S = part->states, R = part->rate_cats, N = part->sites;
  double * cum = (double *)malloc(sizeof(double) * (T->kmax > S ? T->kmax : S));
  unsigned long long * key = (unsigned long long *)malloc(sizeof(unsigned long long) * PLLHIP_HIST_MAX_TABLE);
  unsigned int b, e;
  size_t n;
  if (!cum || !key) { free(cum); free(key); return 0; }
  for (b = 0; b < params->replicates; ++b)
    for (e = 0; e < edge_count; ++e)
    {
      const size_t be = (size_t)b * edge_count + e;
      const unsigned char * pa = states + ((size_t)b * node_count + parent[e]) * N;
      const unsigned char * ch = states + ((size_t)b * node_count + child[e]) * N;
      for (n = 0; n < N; ++n)
      {
        const unsigned int k = comp[(size_t)b * N + n];
        int real = 0;
        if (k == 0xFF) continue;                        /* a dropped site: its changes byte stays 0xFF */
        if (!(k & 0x80u) && (pa[n] >= S || ch[n] >= S)) real = -1;      /* (no such state: no mass) */
        else if (!(k & 0x80u))
          real = hs_site(T, params->seed, (unsigned long long)params->first_replicate + b, matrix[e], e, n, k, pa[n], ch[n],
                         part->pattern_weights[n], counts + be * S * S, units + (be * R + k) * S, cum, key);
        if (real < 0 && part->pattern_weights[n] > 0) ++dropped_edges[be];
        if (changes && real >= 0) changes[be * N + n] = (unsigned char)(real > 254 ? 254 : real);
      }
    }
  free(cum); free(key);
  return 1;
}

void pllhip_eval_destroy_sampled_histories(pllhip_sampled_histories_t * sh)
{
  unsigned int k;
  if (!sh) return;
  for (k = 0; k < sh->partition_count; ++k)
  {
    if (sh->out) free(sh->out[k]);
    if (sh->component) free(sh->component[k]);
    if (sh->counts) free(sh->counts[k]);
    if (sh->units) free(sh->units[k]);
    if (sh->dwell) free(sh->dwell[k]);
    if (sh->total) free(sh->total[k]);
    if (sh->dropped_edges) free(sh->dropped_edges[k]);
    if (sh->changes) free(sh->changes[k]);
  }
  free(sh->out); free(sh->component); free(sh->counts); free(sh->units); free(sh->dwell); free(sh->total);
  free(sh->dropped_edges); free(sh->changes);
  free(sh->dropped); free(sh->sites); free(sh->states); free(sh->cats); free(sh->partition_indices); free(sh->clv_index);
  free(sh);
}

pllhip_sampled_histories_t * pllhip_eval_sample_histories(pllhip_eval_t * ev, const pllhip_ancsample_params_t * params)
{
  const int device = pllhip_sample_histories_edges != NULL;
  const unsigned int known = PLLHIP_ANCS_TIPS | PLLHIP_ANCS_COMPONENT | PLLHIP_HIST_SITES;
  const pll_unode_t * root;
  pllhip_sampled_histories_t * sh = NULL;
  pllhip_history_tables_t * T = NULL;
  unsigned int * parent = NULL, * child = NULL, * matrix = NULL, * sp = NULL, * sc = NULL, * smx = NULL;
  double * length = NULL, * slen = NULL, * cd = NULL;
  unsigned char * states = NULL;
  unsigned int p, k = 0, local = 0, count = 0, rows = 0, i, e, E;
  pllhip_ancsample_params_t anc;
  int with_sites;
  pll_errno = 0;
  if (!params || !params->replicates || (params->flags & ~known) ||
      (unsigned long long)params->first_replicate + params->replicates > (1ULL << 32))
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled histories: NULL parameters, zero replicates, unknown flags or a "
                      "replicate number of 2^32 or more");
    return NULL;
  }
  if (ev->edges >= PLLHIP_HIST_MAX_MATRIX)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled histories: 2^19 or more branches");
    return NULL;
  }
  with_sites = (params->flags & PLLHIP_HIST_SITES) != 0;
  anc = *params;
  anc.flags &= ~PLLHIP_HIST_SITES;
  if (!as_begin(ev, &anc, &root, &rows, &local)) return NULL;
  E = ev->edges;
  sh = (pllhip_sampled_histories_t *)calloc(1, sizeof(*sh));
  length = (double *)calloc((size_t)E + 1, sizeof(double));
  sp = (unsigned int *)calloc(3 * (size_t)E + 1, sizeof(unsigned int));
  slen = (double *)calloc((size_t)E + 1, sizeof(double));
  if (!sh || !length || !sp || !slen || !as_edges(ev, root, &parent, &child, &matrix, &count, length)) goto nomem;
  /* the same edges by pmatrix_index: the order of the result (the draw does not depend on the order of its list) */
  sc = sp + E; smx = sc + E;
  for (e = 0; e < count; ++e)
    if (count != E || matrix[e] >= E)
    {
      pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled histories: the tree's pmatrix indices do not number its branches");
      goto fail;
    }
  for (e = 0; e < count; ++e) { sp[matrix[e]] = parent[e]; sc[matrix[e]] = child[e]; smx[matrix[e]] = matrix[e]; }
  sh->partition_count = local;
  sh->node_count = rows;
  sh->replicates = params->replicates;
  sh->branch_count = E;
  sh->partition_indices = (unsigned int *)calloc(local, sizeof(unsigned int));
  sh->sites = (unsigned int *)calloc(local, sizeof(unsigned int));
  sh->states = (unsigned int *)calloc(local, sizeof(unsigned int));
  sh->cats = (unsigned int *)calloc(local, sizeof(unsigned int));
  sh->dropped = (unsigned long long *)calloc(local, sizeof(unsigned long long));
  sh->out = (unsigned char **)calloc(local, sizeof(unsigned char *));
  sh->component = (unsigned char **)calloc(local, sizeof(unsigned char *));
  sh->counts = (unsigned long long **)calloc(local, sizeof(unsigned long long *));
  sh->units = (unsigned long long **)calloc(local, sizeof(unsigned long long *));
  sh->dwell = (double **)calloc(local, sizeof(double *));
  sh->total = (double **)calloc(local, sizeof(double *));
  sh->dropped_edges = (unsigned long long **)calloc(local, sizeof(unsigned long long *));
  if (with_sites) sh->changes = (unsigned char **)calloc(local, sizeof(unsigned char *));
  sh->clv_index = (unsigned int *)calloc(rows ? rows : 1, sizeof(unsigned int));
  if (!sh->partition_indices || !sh->sites || !sh->states || !sh->cats || !sh->dropped || !sh->out || !sh->component ||
      !sh->counts || !sh->units || !sh->dwell || !sh->total || !sh->dropped_edges || (with_sites && !sh->changes) ||
      !sh->clv_index) goto nomem;
  for (i = 0; i < rows; ++i) sh->clv_index[i] = i;
  for (p = 0; p < ev->nparts; ++p)
  {
    pll_partition_t * part = ev->parts[p];
    size_t cells, S, R, be;
    int ok;
    if (!part) continue;
    S = part->states; R = part->rate_cats;
    cells = (size_t)params->replicates * part->sites;
    be = (size_t)params->replicates * E;
    sh->partition_indices[k] = p;
    sh->sites[k] = part->sites; sh->states[k] = part->states; sh->cats[k] = part->rate_cats;
    sh->out[k] = (unsigned char *)malloc(cells && rows ? cells * rows : 1);
    sh->component[k] = (unsigned char *)malloc(cells ? cells : 1);
    sh->counts[k] = (unsigned long long *)calloc(be * S * S + 1, sizeof(unsigned long long));
    sh->units[k] = (unsigned long long *)calloc(be * R * S + 1, sizeof(unsigned long long));
    sh->dwell[k] = (double *)calloc(be * S + 1, sizeof(double));
    sh->total[k] = (double *)calloc(be ? be : 1, sizeof(double));
    sh->dropped_edges[k] = (unsigned long long *)calloc(be ? be : 1, sizeof(unsigned long long));
    if (with_sites) sh->changes[k] = (unsigned char *)malloc(cells * E + 1);
    if (!sh->out[k] || !sh->component[k] || !sh->counts[k] || !sh->units[k] || !sh->dwell[k] || !sh->total[k] ||
        !sh->dropped_edges[k] || (with_sites && !sh->changes[k])) { ++k; goto nomem; }
    ++k;
    memset(sh->out[k - 1], 0xFF, cells * rows);
    memset(sh->component[k - 1], 0xFF, cells);
    if (with_sites) memset(sh->changes[k - 1], 0xFF, cells * E);
    /* the lengths the matrices of this partition were made from */
    for (e = 0; e < count; ++e) slen[matrix[e]] = effective_length(ev, p, matrix[e], length[e]);
    if (device)
    {
      pllhip_ancsample_params_t q = *params;
      q.flags |= PLLHIP_ANCS_COMPONENT;
      ok = pllhip_sample_histories_edges(part, &q, root->clv_index, root->scaler_index, root->back->clv_index,
                                         root->back->scaler_index, E, sp, sc, smx, ev->params[p], rows, ev->params[p],
                                         slen, sh->out[k - 1], sh->component[k - 1], &sh->dropped[k - 1], sh->counts[k - 1],
                                         sh->units[k - 1], with_sites ? sh->changes[k - 1] : NULL, sh->dropped_edges[k - 1]);
      if (ok) T = pllhip_history_tables_create(part, E, smx, ev->params[p], slen, "sampled histories");
      if (!ok || !T) goto fail;
    }
    else
    {
      double * A, * B;
      unsigned int * c;
      const pll_unode_t * saved = ev->root;
      pllhip_ancsample_params_t q = *params;
      size_t x;
      q.flags = PLLHIP_ANCS_TIPS;
      q.alphabet = NULL;
      T = pllhip_history_tables_create(part, E, smx, ev->params[p], slen, "sampled histories");
      if (!T) goto fail;
      states = (unsigned char *)malloc(cells && rows ? cells * rows : 1);
      if (!states) goto nomem;
      memset(states, 0xFF, cells * rows);
      ev->root = (pll_unode_t *)root;                      /* (sc_host_root_table reads the edge from ev->root) */
      ok = sc_host_root_table(ev, p, &A, &B, &c);
      ev->root = (pll_unode_t *)saved;
      if (!ok) goto fail;
      ok = as_host(part, &q, count, parent, child, matrix, A, B, ev->params[p], rows, states, sh->component[k - 1],
                   &sh->dropped[k - 1]);
      free(A); free(B); free(c);
      if (!ok || !hs_host(part, params, T, E, sp, sc, smx, rows, states, sh->component[k - 1], sh->counts[k - 1],
                          sh->units[k - 1], with_sites ? sh->changes[k - 1] : NULL, sh->dropped_edges[k - 1])) goto nomem;
      /* the rows the caller asked for, in the caller's alphabet */
      for (x = 0; x < cells * rows; ++x)
      {
        const size_t row = x / part->sites % rows;
        if (states[x] == 0xFF || (row < part->tips && !(params->flags & PLLHIP_ANCS_TIPS))) continue;
        sh->out[k - 1][x] = params->alphabet ? (unsigned char)params->alphabet[states[x]] : states[x];
      }
      free(states); states = NULL;
    }
    cd = (double *)malloc(sizeof(double) * (S * S + 1));
    if (!cd) goto nomem;
    for (i = 0; i < params->replicates; ++i)
      for (e = 0; e < E; ++e)
      {
        const size_t x = (size_t)i * E + e;
        if (!pllhip_history_summary(part->states, part->rate_cats, T->tau + (size_t)e * R, sh->counts[k - 1] + x * S * S,
                                    sh->units[k - 1] + x * R * S, cd, sh->dwell[k - 1] + x * S, &sh->total[k - 1][x]))
          goto fail;
      }
    free(cd); cd = NULL;
    pllhip_history_tables_destroy(T); T = NULL;
  }
  free(parent); free(child); free(matrix); free(length); free(sp); free(slen);
  return sh;
nomem:
  pllhip_eval_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the sampled histories");
fail:
  if (!pll_errno) pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "sampled histories: the call failed");
  free(parent); free(child); free(matrix); free(length); free(sp); free(slen); free(states); free(cd);
  pllhip_history_tables_destroy(T);
  pllhip_eval_destroy_sampled_histories(sh);
  return NULL;
}

double pllhip_eval_optimize_branches(pllhip_eval_t * ev, double min_brlen, double max_brlen,
                                     double lh_epsilon, int max_iters, int radius)
{
  return pllhip_eval_optimize_impl(ev, min_brlen, max_brlen, lh_epsilon, max_iters, radius, 0);
}

/* keep_flags: the caller tracks validity itself (the SPR scan optimises the three
   branches around an insertion point and restores them afterwards) */
double pllhip_eval_optimize_impl(pllhip_eval_t * ev, double min_brlen, double max_brlen,
                                 double lh_epsilon, int max_iters, int radius, int keep_flags)
{
  blo_t b;
  double lnl, new_lnl;
  int iters = max_iters;
  pll_unode_t * root = ev->root;
  if (radius < PLLHIP_EVAL_RADIUS_ALL)
  {
    pllhip_eval_error(PLL_ERROR_PARAM_INVALID, "Invalid radius for branch length optimization");
    return 0.0;
  }
  b.ev = ev;
  b.bl_min = (min_brlen > 0) ? min_brlen : 1e-6;
  b.bl_max = (max_brlen > 0) ? max_brlen : 100.0;
  b.tolerance = (min_brlen > 0) ? min_brlen / 10.0 : 1e-4;
  b.max_newton = 30;
  if (!ensure_sumtables(ev)) return 0.0;

  /* precondition of the reference: CLVs valid towards the root, P-matrices current */
  lnl = pllhip_eval_loglh(ev, 1);
  if (isnan(lnl)) return 0.0;

  while (iters)
  {
    if (!optimise_around(&b, root, radius)) return 0.0;
    if (radius && !optimise_around(&b, root->back, radius - 1)) return 0.0;
    new_lnl = edge_loglh(ev, root->back, 0);
    if (new_lnl - lnl > new_lnl * 1e-13)
    {
      iters--;
      if (fabs(new_lnl - lnl) < lh_epsilon) iters = 0;
      lnl = new_lnl;
    }
    else
    {
      pllhip_eval_error(PLLHIP_EVAL_ERROR_NEWTON_WORSE,
                 "BL opt converged to a worse likelihood score by %.15f units", new_lnl - lnl);
      lnl = new_lnl;
      break;
    }
  }
  /* P-matrices are current for every branch; CLVs were last refreshed at
     different moments of the sweep: let the next evaluation rebuild them */
  if (!keep_flags) memset(ev->clv_valid, 0, ev->records);
  return -lnl;
}

unsigned long pllhip_eval_ops(const pllhip_eval_t * ev) { return ev->n_ops; }
unsigned long pllhip_eval_pmatrix_updates(const pllhip_eval_t * ev) { return ev->n_pmat; }
unsigned long pllhip_eval_derivative_calls(const pllhip_eval_t * ev) { return ev->n_deriv; }
unsigned long pllhip_eval_newton_iterations(const pllhip_eval_t * ev) { return ev->n_newton; }
