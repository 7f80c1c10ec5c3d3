/* pllhip_ancsample.c -- pllhip_sample_ancestral_utree: the edge list of a pll_utree_t seen from an inner node, handed to
 * pllhip_sample_ancestral_edges (pll_ancsample_dev.hip; contract: INTEGRATION.md, "Sampled ancestral states").
 *
 * Rows are clv_index, matrices pmatrix_index, the root edge is root -- root->back; the walk is that of
 * pllhip_simulate_utree.  Neither matrices nor vectors are touched. */
#include "pll.h"
#include "pllhip.h"

#include <stdio.h>
#include <stdlib.h>

static int ancs_error(int code, const char * msg)
{
  pll_errno = code;
  snprintf(pll_errmsg, 200, "%s", msg);
  return PLL_FAILURE;
}

int pllhip_sample_ancestral_utree(pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                                  const pll_unode_t * root, const unsigned int * freqs_indices, unsigned char * out,
                                  unsigned char * component, unsigned long long * dropped)
{
  unsigned int * parent, * child, * matrix;
  const pll_unode_t ** stack;
  size_t cap, count = 0, top = 0;
  int ok;
  if (!partition || !params || !freqs_indices || !out)
    return ancs_error(PLL_ERROR_PARAM_INVALID,
                      "pllhip_sample_ancestral_utree: the partition, the parameters, freqs_indices or the output is NULL");
  if (!root || !root->next || !root->back)
    return ancs_error(PLL_ERROR_PARAM_INVALID, "pllhip_sample_ancestral_utree: the root must be an inner node");
  /* a tree over the partition's vectors has fewer edges than vectors; a list that comes out longer cannot be valid and
     goes to the edges form as far as it got, which names the offender */
  cap = (size_t)partition->tips + partition->clv_buffers + 1;
  parent = (unsigned int *)malloc(cap * sizeof(unsigned int));
  child = (unsigned int *)malloc(cap * sizeof(unsigned int));
  matrix = (unsigned int *)malloc(cap * sizeof(unsigned int));
  stack = (const pll_unode_t **)malloc((cap + 1) * sizeof(pll_unode_t *));
  ok = parent && child && matrix && stack;
  if (!ok) (void)ancs_error(PLL_ERROR_MEM_ALLOC, "pllhip_sample_ancestral_utree: cannot allocate the edge list");
  /* stack entry: the record a node was entered by (the root: all of its records lead out) */
  if (ok) stack[top++] = root;
  while (ok && top && count < cap)
  {
    const pll_unode_t * entry = stack[--top];
    const pll_unode_t * n = entry == root ? entry : entry->next;
    if (!n) continue;                                 /* a tip */
    do
    {
      if (count == cap) break;
      parent[count] = n->clv_index;
      child[count] = n->back->clv_index;
      matrix[count] = n->pmatrix_index;
      ++count;
      stack[top++] = n->back;
      n = n->next;
    } while (n != entry);
  }
  if (ok)
    ok = pllhip_sample_ancestral_edges(partition, params, root->clv_index, root->scaler_index, root->back->clv_index,
                                       root->back->scaler_index, (unsigned int)count, parent, child, matrix,
                                       freqs_indices, partition->tips + partition->clv_buffers, out, component, dropped);
  free(parent);
  free(child);
  free(matrix);
  free((void *)stack);
  return ok;
}
