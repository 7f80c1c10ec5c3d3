/* pllhip_ancsample.c -- pllhip_sample_ancestral_utree and pllhip_sample_histories_utree: the edge list of a pll_utree_t
 * seen from an inner node, handed to pllhip_sample_ancestral_edges (pll_ancsample_dev.hip; contract: INTEGRATION.md,
 * "Sampled ancestral states") or, with the lengths of its edges, to pllhip_sample_histories_edges (pll_history_dev.hip;
 * "Sampled substitution histories").
 *
 * Rows are clv_index, matrices pmatrix_index, the root edge is root -- root->back; the walk is that of
 * pllhip_simulate_utree.  Neither matrices nor vectors are touched. */
#include "pll.h"
#include "pllhip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int ancs_error(int code, const char * msg)
{
  pll_errno = code;
  snprintf(pll_errmsg, 200, "%s", msg);
  return PLL_FAILURE;
}

/* the edge list of the tree seen from `root`, with the lengths of its edges; a tree over the partition's vectors has
   fewer edges than vectors: a list that comes out longer cannot be valid and goes to the edges form as far as it got,
   which names the offender.  0: out of memory (the error is set) */
typedef struct
{
  unsigned int * parent, * child, * matrix;
  double * length;
  size_t count;
} ancs_list_t;

static void ancs_list_free(ancs_list_t * l)
{
  free(l->parent); free(l->child); free(l->matrix); free(l->length);
}

static int ancs_list(const pll_partition_t * partition, const pll_unode_t * root, ancs_list_t * l, const char * who)
{
  const size_t cap = (size_t)partition->tips + partition->clv_buffers + 1;
  const pll_unode_t ** stack = (const pll_unode_t **)malloc((cap + 1) * sizeof(pll_unode_t *));
  size_t top = 0;
  l->count = 0;
  l->parent = (unsigned int *)malloc(cap * sizeof(unsigned int));
  l->child = (unsigned int *)malloc(cap * sizeof(unsigned int));
  l->matrix = (unsigned int *)malloc(cap * sizeof(unsigned int));
  l->length = (double *)malloc(cap * sizeof(double));
  if (!l->parent || !l->child || !l->matrix || !l->length || !stack)
  {
    free((void *)stack);
    ancs_list_free(l);
    pll_errno = PLL_ERROR_MEM_ALLOC;
    snprintf(pll_errmsg, 200, "%s: cannot allocate the edge list", who);
    return 0;
  }
  /* stack entry: the record a node was entered by (the root: all of its records lead out) */
  stack[top++] = root;
  while (top && l->count < cap)
  {
    const pll_unode_t * entry = stack[--top];
    const pll_unode_t * n = entry == root ? entry : entry->next;
    if (!n) continue;                                 /* a tip */
    do
    {
      if (l->count == cap) break;
      l->parent[l->count] = n->clv_index;
      l->child[l->count] = n->back->clv_index;
      l->matrix[l->count] = n->pmatrix_index;
      l->length[l->count] = n->length;
      ++l->count;
      stack[top++] = n->back;
      n = n->next;
    } while (n != entry);
  }
  free((void *)stack);
  return 1;
}

int pllhip_sample_ancestral_utree(pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                                  const pll_unode_t * root, const unsigned int * freqs_indices, unsigned char * out,
                                  unsigned char * component, unsigned long long * dropped)
{
  ancs_list_t l;
  int ok;
  if (!partition || !params || !freqs_indices || !out)
    return ancs_error(PLL_ERROR_PARAM_INVALID,
                      "pllhip_sample_ancestral_utree: the partition, the parameters, freqs_indices or the output is NULL");
  if (!root || !root->next || !root->back)
    return ancs_error(PLL_ERROR_PARAM_INVALID, "pllhip_sample_ancestral_utree: the root must be an inner node");
  if (!ancs_list(partition, root, &l, "pllhip_sample_ancestral_utree")) return PLL_FAILURE;
  ok = pllhip_sample_ancestral_edges(partition, params, root->clv_index, root->scaler_index, root->back->clv_index,
                                     root->back->scaler_index, (unsigned int)l.count, l.parent, l.child, l.matrix,
                                     freqs_indices, partition->tips + partition->clv_buffers, out, component, dropped);
  ancs_list_free(&l);
  return ok;
}

int pllhip_sample_histories_utree(pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                                  const pll_unode_t * root, const unsigned int * freqs_indices,
                                  const unsigned int * params_indices, unsigned char * out, unsigned char * component,
                                  unsigned long long * dropped, unsigned long long * counts, unsigned long long * units,
                                  unsigned char * changes, unsigned long long * dropped_edges, unsigned int * edge_count,
                                  unsigned int * edge_matrix)
{
  ancs_list_t l;
  int ok;
  if (!partition || !params || !freqs_indices || !params_indices)
    return ancs_error(PLL_ERROR_PARAM_INVALID,
                      "pllhip_sample_histories_utree: the partition, the parameters, freqs_indices or params_indices is NULL");
  if (!root || !root->next || !root->back)
    return ancs_error(PLL_ERROR_PARAM_INVALID, "pllhip_sample_histories_utree: the root must be an inner node");
  if (!ancs_list(partition, root, &l, "pllhip_sample_histories_utree")) return PLL_FAILURE;
  ok = pllhip_sample_histories_edges(partition, params, root->clv_index, root->scaler_index, root->back->clv_index,
                                     root->back->scaler_index, (unsigned int)l.count, l.parent, l.child, l.matrix,
                                     freqs_indices, partition->tips + partition->clv_buffers, params_indices, l.length,
                                     out, component, dropped, counts, units, changes, dropped_edges);
  if (ok && edge_count) *edge_count = (unsigned int)l.count;
  if (ok && edge_matrix) memcpy(edge_matrix, l.matrix, l.count * sizeof(unsigned int));
  ancs_list_free(&l);
  return ok;
}
