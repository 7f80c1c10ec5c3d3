/*
 * client.c -- a pll-modules-shaped client of the engine's parsimony trees (tests/test_parsimony.py).
 *
 * Follows pllmod_utree_create_parsimony: a partition with 0 CLV buffers, 1 rate category, 1 P-matrix and no
 * scale buffers, pll_fastparsimony_init, pll_fastparsimony_stepwise, the partition destroyed, then the parsimony
 * object; then pll_utree_reset_template_indices and pll_utree_check_integrity on the tree.  It then runs one full
 * likelihood traversal over the tree (JC, every branch 0.1) and prints "score", "newick" and "lnl" lines.
 *
 * usage: client TIPS SITES SEED.  Alignment: state (site * 7 + tip * 3 + site * tip) % 4, every 11th entry a gap.
 */
#include "pll.h"

static char ** make_alignment(unsigned int tips, unsigned int sites)
{
  char ** seq = (char **)calloc(tips, sizeof(char *));
  for (unsigned int t = 0; t < tips; ++t)
  {
    seq[t] = (char *)calloc(sites + 1, 1);
    for (unsigned int n = 0; n < sites; ++n)
      seq[t][n] = ((n + t) % 11 == 0) ? '-' : "ACGT"[(n * 7 + t * 3 + n * t) % 4];
  }
  return seq;
}

static int set_length(pll_unode_t * node)
{
  node->length = 0.1;
  return 1;
}

int main(int argc, char ** argv)
{
  if (argc < 4) { fprintf(stderr, "usage: client TIPS SITES SEED\n"); return 2; }
  const unsigned int tips = (unsigned int)atoi(argv[1]), sites = (unsigned int)atoi(argv[2]);
  const unsigned int seed = (unsigned int)atoi(argv[3]);
  char ** seq = make_alignment(tips, sites);
  char ** labels = (char **)calloc(tips, sizeof(char *));
  for (unsigned int t = 0; t < tips; ++t)
  {
    labels[t] = (char *)malloc(16);
    snprintf(labels[t], 16, "t%u", t);
  }

  /* pllmod_utree_create_parsimony */
  pll_partition_t * pp = pll_partition_create(tips, 0, 4, sites, 1, 1, 1, 0, PLL_ATTRIB_ARCH_CPU);
  if (!pp) { fprintf(stderr, "partition: %s\n", pll_errmsg); return 1; }
  for (unsigned int t = 0; t < tips; ++t)
    if (!pll_set_tip_states(pp, t, pll_map_nt, seq[t])) { fprintf(stderr, "tip: %s\n", pll_errmsg); return 1; }
  pll_parsimony_t * pars = pll_fastparsimony_init(pp);
  if (!pars) { fprintf(stderr, "init: %s\n", pll_errmsg); return 1; }
  unsigned int score = 0;
  pll_utree_t * tree = pll_fastparsimony_stepwise(&pars, labels, &score, 1, seed);
  pll_partition_destroy(pp);
  pll_parsimony_destroy(pars);
  if (!tree) { fprintf(stderr, "stepwise: %s\n", pll_errmsg); return 1; }
  pll_utree_reset_template_indices(tree->nodes[tree->tip_count + tree->inner_count - 1], tree->tip_count);
  pll_utree_every(tree, set_length);
  if (!pll_utree_check_integrity(tree)) { fprintf(stderr, "integrity: %s\n", pll_errmsg); return 1; }

  /* one likelihood traversal over the tree */
  pll_partition_t * lp = pll_partition_create(tips, tips - 2, 4, sites, 1, 2 * tips - 3, 1, tips - 2,
                                              PLL_ATTRIB_ARCH_CPU);
  if (!lp) { fprintf(stderr, "partition: %s\n", pll_errmsg); return 1; }
  const double subst[6] = {1, 1, 1, 1, 1, 1}, freqs[4] = {0.25, 0.25, 0.25, 0.25}, rate = 1.0;
  pll_set_subst_params(lp, 0, subst);
  pll_set_frequencies(lp, 0, freqs);
  pll_set_category_rates(lp, &rate);
  for (unsigned int t = 0; t < tips; ++t) pll_set_tip_states(lp, t, pll_map_nt, seq[t]);
  pll_unode_t * root = tree->vroot->next ? tree->vroot : tree->vroot->back;
  pll_unode_t ** trav = (pll_unode_t **)calloc(2 * tips, sizeof(*trav));
  unsigned int trav_size = 0, matrix_count = 0, ops_count = 0;
  if (!pll_utree_traverse(root, PLL_TREE_TRAVERSE_POSTORDER, set_length, trav, &trav_size))
  { fprintf(stderr, "traverse: %s\n", pll_errmsg); return 1; }
  pll_operation_t * ops = (pll_operation_t *)calloc(tips, sizeof(*ops));
  unsigned int * mats = (unsigned int *)calloc(2 * tips, sizeof(unsigned int));
  double * lens = (double *)calloc(2 * tips, sizeof(double));
  pll_utree_create_operations(trav, trav_size, lens, mats, ops, &matrix_count, &ops_count);
  const unsigned int params[1] = {0};
  pll_update_prob_matrices(lp, params, mats, lens, matrix_count);
  pll_update_prob_matrices(lp, params, &root->pmatrix_index, &root->length, 1);
  pll_update_partials(lp, ops, ops_count);
  const double lnl = pll_compute_edge_loglikelihood(lp, root->clv_index, root->scaler_index, root->back->clv_index,
                                                    root->back->scaler_index, root->pmatrix_index, params, NULL);
  char * nwk = pll_utree_export_newick(root, NULL);
  printf("score %u\nnewick %s\nlnl %.17g\n", score, nwk, lnl);
  free(nwk);
  free(ops); free(mats); free(lens); free(trav);
  pll_partition_destroy(lp);
  pll_utree_destroy(tree, NULL);
  for (unsigned int t = 0; t < tips; ++t) { free(seq[t]); free(labels[t]); }
  free(seq); free(labels);
  return 0;
}
