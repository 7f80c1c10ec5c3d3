/* pllhip_nj.c -- the join list of a neighbour-joining run (pll_distance_dev.hip) -> pll_utree_t.
 *
 * Nodes 0 .. T-1 are the tips (clv_index = taxon index, pmatrix_index = taxon index, no scaler), node T + q is the
 * inner node round q made, node 2T - 3 the one the last three slots meet in.  Record 0 of an inner node looks at its
 * parent (the node that joined it later), records 1 and 2 at its children; all three records of the last node look
 * at children.  Inner edges get the matrix indices T .. 2T - 4.  Negative lengths become 0. */
#include "nj_tree.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static void nj_error(int code, const char * msg)
{
  pll_errno = code;
  snprintf(pll_errmsg, 200, "%s", msg);
}

static void nj_link(pll_unode_t * up, pll_unode_t * down, double length, unsigned int * edge, unsigned int tips)
{
  up->back = down;
  down->back = up;
  up->length = down->length = length > 0.0 ? length : 0.0;
  up->pmatrix_index = down->pmatrix_index = up->clv_index < tips ? up->clv_index : (*edge)++;
}

pll_utree_t * pllhip_nj_build_tree(unsigned int tips, const unsigned int * slots, const double * lengths,
                                   const char * const * labels)
{
  const unsigned int inner = tips - 2, nodes = tips + inner, rounds = tips - 3;
  pll_unode_t ** rec = (pll_unode_t **)calloc((size_t)nodes * 3, sizeof(*rec));    /* [node][record] */
  unsigned int * node_of = (unsigned int *)malloc(sizeof(unsigned int) * tips);  /* slot -> node */
  unsigned int i, j, q, edge = tips;
  pll_utree_t * tree = NULL;
  int ok = rec && node_of;
  for (i = 0; ok && i < nodes; ++i)
  {
    const unsigned int nrec = i < tips ? 1 : 3;
    for (j = 0; ok && j < nrec; ++j)
    {
      pll_unode_t * r = (pll_unode_t *)calloc(1, sizeof(*r));
      ok = r != NULL;
      if (!ok) break;
      rec[3 * i + j] = r;
      r->clv_index = i;
      if (i < tips)
      {
        r->node_index = i;
        r->scaler_index = PLL_SCALE_BUFFER_NONE;
        if (labels && labels[i]) ok = (r->label = strdup(labels[i])) != NULL;
      }
      else
      {
        r->node_index = tips + 3 * (i - tips) + j;
        r->scaler_index = (int)(i - tips);
      }
    }
    if (ok && i >= tips)
      for (j = 0; j < 3; ++j) rec[3 * i + j]->next = rec[3 * i + (j + 1) % 3];
  }
  if (ok)
  {
    const unsigned int last = nodes - 1;
    for (i = 0; i < tips; ++i) node_of[i] = i;
    for (q = 0; q < rounds; ++q)
    {
      const unsigned int u = tips + q, si = slots[2 * q], sj = slots[2 * q + 1];
      nj_link(rec[3 * node_of[si]], rec[3 * u + 1], lengths[2 * q], &edge, tips);
      nj_link(rec[3 * node_of[sj]], rec[3 * u + 2], lengths[2 * q + 1], &edge, tips);
      node_of[si] = u;
    }
    for (j = 0; j < 3; ++j)
      nj_link(rec[3 * node_of[slots[2 * rounds + j]]], rec[3 * last + j], lengths[2 * rounds + j], &edge, tips);
    tree = pll_utree_wraptree(rec[3 * last], tips);
  }
  if (!tree)
  {
    for (i = 0; rec && i < nodes * 3; ++i)
      if (rec[i]) { free(rec[i]->label); free(rec[i]); }
    if (!ok) nj_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the neighbour-joining tree");
  }
  free(rec);
  free(node_of);
  return tree;
}
