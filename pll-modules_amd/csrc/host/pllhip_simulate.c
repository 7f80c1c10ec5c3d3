/* pllhip_simulate.c -- pllhip_simulate_utree: the edge list of a pll_utree_t seen from an inner node, handed to
 * pllhip_simulate_edges (pll_simulate_dev.hip; contract: INTEGRATION.md, "Simulated alignments").
 *
 * Rows are clv_index, matrices pmatrix_index; the walk follows `back` out of every record of a node's ring except the
 * one it came in by, so multifurcating nodes need nothing special. */
#include "pll.h"
#include "pllhip.h"

#include <stdio.h>
#include <stdlib.h>

static int sim_error(int code, const char * msg)
{
  pll_errno = code;
  snprintf(pll_errmsg, 200, "%s", msg);
  return PLL_FAILURE;
}

typedef struct { unsigned int * parent, * child, * matrix; double * length; const pll_unode_t ** stack; } sim_lists_t;

static void sim_free(sim_lists_t * l)
{
  free(l->parent);
  free(l->child);
  free(l->matrix);
  free(l->length);
  free((void *)l->stack);
}

int pllhip_simulate_utree(pll_partition_t * partition, const pllhip_sim_params_t * params, const pll_unode_t * root,
                          const unsigned int * params_indices, int update_matrices, unsigned char * out)
{
  sim_lists_t l = {NULL, NULL, NULL, NULL, NULL};
  size_t cap, count = 0, top = 0;
  int ok;
  if (!partition || !params || !params_indices || !out)
    return sim_error(PLL_ERROR_PARAM_INVALID,
                     "pllhip_simulate_utree: the partition, the parameters, params_indices or the output is NULL");
  if (!root || !root->next)
    return sim_error(PLL_ERROR_PARAM_INVALID, "pllhip_simulate_utree: the root must be an inner node");
  /* a tree over the partition's vectors has fewer edges than vectors; a list that comes out longer cannot be valid and
     goes to the edges form as far as it got, which names the offender */
  cap = (size_t)partition->tips + partition->clv_buffers + 1;
  l.parent = (unsigned int *)malloc(cap * sizeof(unsigned int));
  l.child = (unsigned int *)malloc(cap * sizeof(unsigned int));
  l.matrix = (unsigned int *)malloc(cap * sizeof(unsigned int));
  l.length = (double *)malloc(cap * sizeof(double));
  l.stack = (const pll_unode_t **)malloc((cap + 1) * sizeof(pll_unode_t *));
  if (!l.parent || !l.child || !l.matrix || !l.length || !l.stack)
  {
    sim_free(&l);
    return sim_error(PLL_ERROR_MEM_ALLOC, "pllhip_simulate_utree: cannot allocate the edge list");
  }
  /* stack entry: the record a node was entered by (the root: all of its records lead out) */
  l.stack[top++] = root;
  while (top && count < cap)
  {
    const pll_unode_t * entry = l.stack[--top];
    const pll_unode_t * n = entry == root ? entry : entry->next;
    if (!n) continue;                                 /* a tip */
    do
    {
      if (count == cap) break;
      l.parent[count] = n->clv_index;
      l.child[count] = n->back->clv_index;
      l.matrix[count] = n->pmatrix_index;
      l.length[count] = n->length;
      ++count;
      l.stack[top++] = n->back;
      n = n->next;
    } while (n != entry);
  }
  ok = PLL_SUCCESS;
  if (update_matrices)
    ok = pll_update_prob_matrices(partition, params_indices, l.matrix, l.length, (unsigned int)count);
  if (ok)
    ok = pllhip_simulate_edges(partition, params, root->clv_index, (unsigned int)count, l.parent, l.child, l.matrix,
                               params_indices, partition->tips + partition->clv_buffers, out);
  sim_free(&l);
  return ok;
}
