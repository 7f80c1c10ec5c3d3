/* consensus_host_check.c -- the consensus' host side (csrc/host/pllhip_consensus.c: the integer thresholds and the
 * tree of a split system) under the host sanitizers, as a program of its own: no device, no Python.
 *
 * Build and run from the repository root:
 *
 *   gcc -std=gnu99 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined \
 *       -Iinclude -Ipll-modules_amd/csrc -o /tmp/consensus_host_check tools/consensus_host_check.c \
 *       pll-modules_amd/csrc/host/pllhip_consensus.c pll-modules_amd/csrc/host/pllhip_treeset.c \
 *       pll-modules_amd/csrc/host/pll_utree.c -lm
 *   /tmp/consensus_host_check
 *
 * Caterpillars and comb-of-cherries trees of 4 .. 3000 tips are flattened into their splits; the builder gets all of
 * them, every second one, one, and none, with and without labels and supports.  Every tree it returns is exported,
 * parsed back, flattened again where it is binary, cloned and destroyed; its inner nodes are counted and the support
 * labels read back.  Then systems that must be rejected, and the thresholds.  Leaks count (detect_leaks is on by
 * default).  Exit status 0 and "ok" when all of it held.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pll.h"
#include "treeset_plan.h"

__thread int pll_errno;
__thread char pll_errmsg[200];

static unsigned int built = 0, rejected = 0;

static void die(const char * what)
{
  fprintf(stderr, "consensus_host_check: %s (pll_errno %d: %s)\n", what, pll_errno, pll_errmsg);
  exit(1);
}

static char ** make_names(unsigned int T)
{
  char ** names = (char **)malloc(T * sizeof(char *));
  unsigned int i;
  for (i = 0; i < T; ++i)
  {
    names[i] = (char *)malloc(12);
    snprintf(names[i], 12, "c%u", i);
  }
  return names;
}

/* shape 0: a caterpillar with c0 in the middle of the spine (from 6 tips on); shape 1: cherries along a spine */
static char * make_newick(unsigned int T, int shape)
{
  char * text = (char *)malloc((size_t)T * 14u + 16u), * at = text;
  unsigned int i;
  if (shape == 0 || T < 8u)
  {
    const unsigned int mid = T / 2u >= 3u ? T / 2u : 0u;      /* c0 changes places with c(mid) */
    at += sprintf(at, "(c%u,c1,", mid);
    for (i = 2; i + 1u < T; ++i) at += sprintf(at, "(c%u,", i == mid ? 0u : i);
    at += sprintf(at, "c%u", T - 1u == mid ? 0u : T - 1u);
    for (i = 2; i + 1u < T; ++i) *at++ = ')';
  }
  else
  {
    const unsigned int pairs = (T - 2u) / 2u, wrapped = T % 2u ? pairs : pairs - 1u;
    at += sprintf(at, "(c0,c1,");
    for (i = 0; i < wrapped; ++i) at += sprintf(at, "((c%u,c%u),", 2u + 2u * i, 3u + 2u * i);
    if (T % 2u) at += sprintf(at, "c%u", T - 1u);
    else at += sprintf(at, "(c%u,c%u)", T - 2u, T - 1u);
    for (i = 0; i < wrapped; ++i) *at++ = ')';
  }
  sprintf(at, ");");
  return text;
}

static unsigned int inner_labels(const pll_utree_t * tree, const double * support, unsigned int K)
{
  unsigned int i, found = 0;
  for (i = tree->tip_count; i < tree->tip_count + tree->inner_count; ++i)
  {
    const pll_unode_t * n = tree->nodes[i], * s = n;
    unsigned int k;
    do { if (s->label != n->label) die("the records of a node do not share its label"); s = s->next; } while (s != n);
    if (!n->label) continue;
    for (k = 0; k < K; ++k)
      if (strtod(n->label, NULL) == support[k]) break;
    if (k == K) die("an inner label is no support value");
    ++found;
  }
  return found;
}

static void check_system(unsigned int T, const pllhip_ts_labels_t * labels, unsigned int K, const uint32_t * words,
                         const double * support)
{
  pll_utree_t * tree = pllhip_ts_tree_from_splits(T, labels, K, words, support), * back, * copy;
  char * newick;
  unsigned int i;
  if (!tree) die("a good split system is rejected");
  if (tree->tip_count != T || tree->inner_count != K + 1u || tree->edge_count != T + K) die("counts");
  if ((tree->binary != 0) != (K == T - 3u)) die("binary flag");
  for (i = 0; i < T; ++i)
  {
    const pll_unode_t * n = tree->nodes[i];
    if (n->next || n->node_index != i || n->clv_index != i || !n->back || n->back->back != n) die("tip record");
    if (labels ? (!n->label || strcmp(n->label, pllhip_ts_labels_get(labels, i))) : n->label != NULL) die("tip label");
  }
  if (tree->nodes[0]->back != tree->vroot && tree->nodes[0]->back->next == NULL) die("vroot");
  if (inner_labels(tree, support, K) != (support ? K : 0u)) die("support labels");
  newick = pll_utree_export_newick(tree->vroot, NULL);
  if (!newick) die("export");
  if (labels)
  {
    back = pll_utree_parse_newick_string(newick);
    if (!back || back->tip_count != T || back->inner_count != K + 1u) die("the exported tree does not parse back");
    if (K == T - 3u)
    {
      uint32_t * order = (uint32_t *)malloc((T - 1u) * 4u), * lo = (uint32_t *)malloc(K * 4u), * hi = (uint32_t *)malloc(K * 4u);
      uint32_t * again = (uint32_t *)malloc((size_t)K * pllhip_ts_words(T) * 4u), * p1 = (uint32_t *)malloc(K * 4u);
      uint32_t * p2 = (uint32_t *)malloc(K * 4u);
      pllhip_ts_step_t * program = (pllhip_ts_step_t *)malloc((2u * T - 3u) * sizeof(pllhip_ts_step_t));
      const unsigned int len = pllhip_ts_words(T);
      if (!pllhip_ts_flatten(back, T, labels, order, lo, hi, NULL, program, NULL)) die("the binary tree does not flatten");
      pllhip_ts_plan_splits(T, order, lo, hi, again, NULL);
      pllhip_ts_sort_splits(T, K, again, p1);
      pllhip_ts_sort_splits(T, K, words, p2);
      for (i = 0; i < K; ++i)
        if (memcmp(again + (size_t)p1[i] * len, words + (size_t)p2[i] * len, len * 4u)) die("the tree has other splits");
      free(order); free(lo); free(hi); free(again); free(p1); free(p2); free(program);
    }
    pll_utree_destroy(back, NULL);
  }
  copy = pll_utree_clone(tree);
  if (!copy || copy->inner_count != K + 1u) die("clone");
  pll_utree_destroy(copy, NULL);
  free(newick);
  pll_utree_destroy(tree, NULL);
  ++built;
}

static void check_shape(unsigned int T, int shape)
{
  const unsigned int R = T - 3u, len = pllhip_ts_words(T);
  char ** names = make_names(T);
  char * newick = make_newick(T, shape);
  pllhip_ts_labels_t * labels = pllhip_ts_labels_create(T, (const char * const *)names);
  pll_utree_t * tree = pll_utree_parse_newick_string(newick);
  uint32_t * order = (uint32_t *)malloc((T - 1u) * 4u), * lo = (uint32_t *)malloc(R * 4u), * hi = (uint32_t *)malloc(R * 4u);
  uint32_t * words = (uint32_t *)malloc((size_t)R * len * 4u), * some = (uint32_t *)malloc((size_t)R * len * 4u);
  double * support = (double *)malloc(R * sizeof(double));
  pllhip_ts_step_t * program = (pllhip_ts_step_t *)malloc((2u * T - 3u) * sizeof(pllhip_ts_step_t));
  unsigned int i, K = 0;
  if (!labels || !tree) die("setting up a shape");
  if (!pllhip_ts_flatten(tree, T, labels, order, lo, hi, NULL, program, NULL)) die("flatten");
  pllhip_ts_plan_splits(T, order, lo, hi, words, NULL);
  for (i = 0; i < R; ++i) support[i] = (double)(i % 7u + 1u) / 7.0;
  check_system(T, labels, R, words, support);
  check_system(T, NULL, R, words, NULL);
  for (i = 0; i < R; i += 2u) memcpy(some + (size_t)K++ * len, words + (size_t)i * len, len * 4u);
  check_system(T, labels, K, some, support);
  check_system(T, labels, 1, words + (size_t)(R / 2u) * len, support);
  check_system(T, labels, 0, NULL, NULL);
  check_system(T, NULL, 0, words, support);

  if (R >= 2u)
  {
    /* the same split twice */
    memcpy(some, words, len * 4u);
    memcpy(some + len, words, len * 4u);
    pll_errno = 0;
    if (pllhip_ts_tree_from_splits(T, labels, 2, some, NULL) || pll_errno != PLL_ERROR_PARAM_INVALID) die("a split given twice");
    ++rejected;
  }
  /* not in normal form; trivial */
  memcpy(some, words, len * 4u);
  some[0] &= ~1u;
  pll_errno = 0;
  if (pllhip_ts_tree_from_splits(T, labels, 1, some, NULL) || pll_errno != PLL_ERROR_PARAM_INVALID) die("tip 0's bit clear");
  memset(some, 0, len * 4u);
  some[0] = 1u;
  pll_errno = 0;
  if (pllhip_ts_tree_from_splits(T, labels, 1, some, NULL) || pll_errno != PLL_ERROR_PARAM_INVALID) die("a trivial split");
  pll_errno = 0;
  if (pllhip_ts_tree_from_splits(T, labels, R + 1u, words, NULL) || pll_errno != PLL_ERROR_PARAM_INVALID) die("too many splits");
  rejected += 3u;

  pll_utree_destroy(tree, NULL);
  pllhip_ts_labels_destroy(labels);
  for (i = 0; i < T; ++i) free(names[i]);
  free(names); free(newick); free(order); free(lo); free(hi); free(words); free(some); free(support); free(program);
}

int main(void)
{
  static const unsigned int TIPS[] = {4, 5, 8, 9, 31, 32, 33, 64, 65, 130, 3000};
  unsigned int k, major, minor;
  for (k = 0; k < sizeof(TIPS) / sizeof(TIPS[0]); ++k)
  {
    check_shape(TIPS[k], 0);
    check_shape(TIPS[k], 1);
  }

  {
    /* two splits that overlap: {1,2} and {2,3} of six tips */
    uint32_t bad[2] = {0x3fu & ~0x06u, 0x3fu & ~0x0cu};
    pll_errno = 0;
    if (pllhip_ts_tree_from_splits(6, NULL, 2, bad, NULL) || pll_errno != PLL_ERROR_PARAM_INVALID) die("incompatible splits");
    bad[1] = 0x7fu;                                    /* a bit beyond the tips */
    pll_errno = 0;
    if (pllhip_ts_tree_from_splits(6, NULL, 2, bad, NULL) || pll_errno != PLL_ERROR_PARAM_INVALID) die("a bit beyond the tips");
    rejected += 2u;
  }

  if (!pllhip_ts_consensus_needs(8, 0.75, &major, &minor) || major != 7u || minor != 7u) die("needs 8, 0.75");
  if (!pllhip_ts_consensus_needs(8, 0.25, &major, &minor) || major != 5u || minor != 3u) die("needs 8, 0.25");
  if (!pllhip_ts_consensus_needs(2, 0.5, &major, &minor) || major != 2u || minor != 2u) die("needs 2, 0.5");
  if (!pllhip_ts_consensus_needs(4294967295u, 0.0, &major, &minor) || major != 2147483648u || minor != 1u) die("needs 2^32 - 1");
  if (!pllhip_ts_consensus_needs(4294967295u, 1.0, &major, NULL) || major != 4294967295u) die("needs strict");
  if (pllhip_ts_consensus_needs(0, 0.5, &major, &minor) || pllhip_ts_consensus_needs(3, 1.5, &major, &minor) ||
      pllhip_ts_consensus_needs(3, -0.5, NULL, NULL))
    die("bad arguments accepted");
  printf("ok: %u trees built, %u systems rejected\n", built, rejected);
  return 0;
}
