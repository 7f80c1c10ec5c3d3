/*
 * client.c -- a pll-modules-shaped client of the engine's parsimony SPR rounds and taxon extension
 * (tests/test_parsimony_spr.py).
 *
 * Resolve (pllmod_utree_resolve_parsimony_multipart): the constraint is a star of blocks of 4 taxa, each block a
 * multifurcating clade.  The client builds a binary resolution of it (a caterpillar per multifurcation) and the map
 * of every clv index to the multifurcating node it resolves (tips to themselves), as pllmod_utree_resolve_multi
 * does, then runs pll_fastparsimony_stepwise_spr_round until the score stops improving (at most 10 rounds).
 * Extend (pllmod_utree_extend_parsimony_multipart): a caterpillar of the first TIPS/2 taxa is extended by the
 * others, then pll_utree_reset_template_indices and pll_utree_check_integrity.
 * Prints "resolve_score", "resolve_rounds", "resolve_newick", "extend_score" and "extend_newick" lines.
 *
 * usage: client TIPS SITES SEED (TIPS a multiple of 4, at least 12).  Alignment: state (site * 5 + tip * 3 +
 * site * tip) % 4, an entry a gap where (site + 2 tip) % 13 == 0.
 */
#include "pll.h"

static unsigned int next_clv, next_pmatrix;

static pll_unode_t * new_tip(unsigned int i, char * const * labels)
{
  pll_unode_t * r = (pll_unode_t *)calloc(1, sizeof(*r));
  r->clv_index = r->node_index = i;
  r->scaler_index = PLL_SCALE_BUFFER_NONE;
  r->label = strdup(labels[i]);
  return r;
}

static void link(pll_unode_t * a, pll_unode_t * b)
{
  a->back = b;
  b->back = a;
  a->length = b->length = 0.1;
  a->pmatrix_index = b->pmatrix_index = next_pmatrix++;
}

/* resolves a multifurcation over `n` subtrees (records facing up) into a caterpillar; returns the record facing
   up; every new inner node maps to group `group` */
static pll_unode_t * caterpillar(pll_unode_t ** sub, unsigned int n, int group, int * map)
{
  pll_unode_t * cur = sub[0];
  for (unsigned int i = 1; i < n; ++i)
  {
    pll_unode_t * r[3];
    for (int j = 0; j < 3; ++j)
    {
      r[j] = (pll_unode_t *)calloc(1, sizeof(pll_unode_t));
      r[j]->clv_index = next_clv;
      r[j]->scaler_index = -1;
    }
    r[0]->next = r[1]; r[1]->next = r[2]; r[2]->next = r[0];
    map[next_clv++] = group;
    link(r[0], cur);
    link(r[1], sub[i]);
    cur = r[2];
  }
  return cur;
}

static pll_partition_t * make_partition(unsigned int tips, unsigned int sites, char ** seq)
{
  pll_partition_t * p = pll_partition_create(tips, 0, 4, sites, 1, 1, 1, 0, PLL_ATTRIB_ARCH_CPU);
  if (!p) return NULL;
  for (unsigned int t = 0; t < tips; ++t)
    if (!pll_set_tip_states(p, t, pll_map_nt, seq[t])) return NULL;
  return p;
}

int main(int argc, char ** argv)
{
  if (argc < 4) { fprintf(stderr, "usage: client TIPS SITES SEED\n"); return 2; }
  const unsigned int tips = (unsigned int)atoi(argv[1]), sites = (unsigned int)atoi(argv[2]);
  const unsigned int seed = (unsigned int)atoi(argv[3]);
  if (tips < 12 || tips % 4) { fprintf(stderr, "TIPS: a multiple of 4, at least 12\n"); return 2; }
  char ** seq = (char **)calloc(tips, sizeof(char *));
  char ** labels = (char **)calloc(tips, sizeof(char *));
  for (unsigned int t = 0; t < tips; ++t)
  {
    seq[t] = (char *)calloc(sites + 1, 1);
    for (unsigned int n = 0; n < sites; ++n)
      seq[t][n] = ((n + 2 * t) % 13 == 0) ? '-' : "ACGT"[(n * 5 + t * 3 + n * t) % 4];
    labels[t] = (char *)malloc(16);
    snprintf(labels[t], 16, "t%u", t);
  }

  /* resolve: the binary resolution and its clv-index map */
  const unsigned int blocks = tips / 4;
  int * map = (int *)calloc(2 * tips, sizeof(int));
  pll_unode_t ** up = (pll_unode_t **)calloc(blocks, sizeof(*up));
  next_clv = tips;
  next_pmatrix = 0;
  for (unsigned int t = 0; t < tips; ++t) map[t] = (int)t;
  const int root_group = (int)(2 * tips);        /* the star's centre: a node of the constraint of its own */
  for (unsigned int b = 0; b < blocks; ++b)
  {
    pll_unode_t * sub[4];
    for (unsigned int i = 0; i < 4; ++i) sub[i] = new_tip(4 * b + i, labels);
    up[b] = caterpillar(sub, 4, (int)(tips + 3 * b), map);
  }
  pll_unode_t * top = caterpillar(up, blocks - 1, root_group, map);
  link(top, up[blocks - 1]);
  pll_utree_t * tree = pll_utree_wraptree(top, tips);
  if (!tree || !pll_utree_check_integrity(tree)) { fprintf(stderr, "resolution: %s\n", pll_errmsg); return 1; }

  pll_partition_t * part = make_partition(tips, sites, seq);
  if (!part) { fprintf(stderr, "partition: %s\n", pll_errmsg); return 1; }
  pll_parsimony_t * pars = pll_fastparsimony_init(part);
  if (!pars) { fprintf(stderr, "init: %s\n", pll_errmsg); return 1; }
  unsigned int score = ~0u, best, rounds = 0;
  int rc;
  do
  {
    best = score;
    rc = pll_fastparsimony_stepwise_spr_round(tree, &pars, 1, NULL, seed, map, &score);
    ++rounds;
  } while (rc && rounds < 10 && score < best);
  if (!rc) { fprintf(stderr, "spr round: %s\n", pll_errmsg); return 1; }
  if (!pll_utree_check_integrity(tree)) { fprintf(stderr, "integrity: %s\n", pll_errmsg); return 1; }
  char * nwk = pll_utree_export_newick(tree->vroot, NULL);
  printf("resolve_score %u\nresolve_rounds %u\nresolve_newick %s\n", score, rounds, nwk);
  free(nwk);
  pll_utree_destroy(tree, NULL);

  /* extend: a caterpillar of the first tips / 2 taxa */
  const unsigned int half = tips / 2;
  size_t len = 16 * tips + 16;
  char * text = (char *)calloc(len, 1);
  strcpy(text, "(t0,t1,");
  for (unsigned int t = 2; t + 1 < half; ++t) snprintf(text + strlen(text), len - strlen(text), "(t%u,", t);
  snprintf(text + strlen(text), len - strlen(text), "t%u", half - 1);
  for (unsigned int t = 2; t + 1 < half; ++t) strcat(text, ")");
  strcat(text, ");");
  tree = pll_utree_parse_newick_string(text);
  free(text);
  if (!tree) { fprintf(stderr, "newick: %s\n", pll_errmsg); return 1; }
  if (!pll_fastparsimony_stepwise_extend(tree, &pars, 1, labels + half, NULL, seed, &score))
  { fprintf(stderr, "extend: %s\n", pll_errmsg); return 1; }
  pll_utree_reset_template_indices(tree->nodes[tree->tip_count + tree->inner_count - 1], tree->tip_count);
  if (tree->tip_count != tips || !pll_utree_check_integrity(tree))
  { fprintf(stderr, "extended tree: %s\n", pll_errmsg); return 1; }
  nwk = pll_utree_export_newick(tree->vroot, NULL);
  printf("extend_score %u\nextend_newick %s\n", score, nwk);
  free(nwk);
  pll_utree_destroy(tree, NULL);
  pll_parsimony_destroy(pars);
  pll_partition_destroy(part);
  for (unsigned int t = 0; t < tips; ++t) { free(seq[t]); free(labels[t]); }
  free(seq); free(labels); free(map); free(up);
  return 0;
}
