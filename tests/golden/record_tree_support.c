/* record_tree_support.c -- records tests/golden/tree_support_fixtures.json: small trees and what pll-modules'
 * pllmod_utree_split_create, pllmod_utree_split_rf_distance and pllmod_utree_tbe_naive make of them
 * (tests/test_tree_support_restatement.py pins its restatement to this file).
 *
 * pllmod_utree_tbe_nature is left out on purpose: it takes its leaf counts from a contiguous range of clv_index below
 * every node, which parsed and random trees do not have ("Split support and tree distances"), so it
 * is no yardstick.
 *
 * Built outside the tree against a pll-modules checkout at $REF, the way record_msa_stats.c is (run from the
 * repository root, after `make -C oracle`):
 *
 *   cc -std=gnu99 -D_GNU_SOURCE -O2 -w -ffunction-sections -Iinclude -I$REF/src -I$REF/src/tree \
 *      -o /tmp/record_tree_support tests/golden/record_tree_support.c $REF/src/pllmod_common.c \
 *      $REF/src/tree/utree_distances.c $REF/src/tree/tbe_functions.c $REF/src/tree/tree_hashtable.c \
 *      $REF/src/tree/pll_tree.c $REF/src/tree/utree_operations.c \
 *      -Loracle/_build -lpll_oracle -lm -Wl,-rpath,$PWD/oracle/_build -Wl,--gc-sections
 *   /tmp/record_tree_support > tests/golden/tree_support_fixtures.json
 *
 * /tmp/record_tree_support time T B prints the single-thread seconds of pllmod_utree_tbe_naive for one reference
 * tree of T tips against B trees (the context figure of DESIGN.md section 16), and nothing else.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "pll.h"
#include "pll_tree.h"

#define NTREES 5

static unsigned long long rng_state = 0x9E3779B97F4A7C15ULL;
static unsigned int rnd(unsigned int n)
{
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (unsigned int)((rng_state >> 33) % n);
}

static char ** make_names(unsigned int T)
{
  char ** names = (char **)malloc(T * sizeof(char *));
  unsigned int i;
  for (i = 0; i < T; ++i)
  {
    names[i] = (char *)malloc(16);
    snprintf(names[i], 16, "t%u", i);
  }
  return names;
}

/* `moves` nearest-neighbour interchanges on inner edges drawn at random */
static void scramble(pll_utree_t * tree, unsigned int moves)
{
  const unsigned int T = tree->tip_count;
  while (moves)
  {
    pll_unode_t * r = tree->nodes[T + rnd(tree->inner_count)];
    unsigned int k = rnd(3);
    while (k--) r = r->next;
    if (!r->back->next) continue;
    if (pllmod_utree_nni(r, rnd(2) ? PLL_UTREE_MOVE_NNI_LEFT : PLL_UTREE_MOVE_NNI_RIGHT, NULL)) --moves;
  }
}

static void print_splits(const char * indent, pll_split_t * s, unsigned int T, const char * tail)
{
  const unsigned int len = (T + 31) / 32;
  unsigned int i, w;
  printf("%s[", indent);
  for (i = 0; i + 3 < T; ++i)
  {
    printf("%s[", i ? ", " : "");
    for (w = 0; w < len; ++w) printf("%s%u", w ? ", " : "", s[i][w]);
    printf("]");
  }
  printf("]%s\n", tail);
}

static void print_newick(const char * indent, pll_utree_t * tree, const char * tail)
{
  char * s = pll_utree_export_newick(tree->vroot, NULL);
  printf("%s\"%s\"%s\n", indent, s, tail);
  free(s);
}

static void make_trees(unsigned int T, char ** names, unsigned int seed, pll_utree_t ** ref, pll_utree_t ** trees)
{
  unsigned int b;
  *ref = pllmod_utree_create_random(T, (const char * const *)names, seed);
  for (b = 0; b < NTREES; ++b)
  {
    if (b == NTREES - 1) trees[b] = pllmod_utree_create_random(T, (const char * const *)names, seed + 1000);
    else
    {
      trees[b] = pll_utree_clone(*ref);
      scramble(trees[b], T > 4 ? b : (b ? 1 : 0));
    }
    if (!pllmod_utree_consistency_set(*ref, trees[b])) { fprintf(stderr, "consistency_set failed\n"); exit(1); }
  }
}

static void record(unsigned int T, int last)
{
  char ** names = make_names(T);
  pll_utree_t * ref, * trees[NTREES];
  pll_split_t * rs, * bs[NTREES];
  double * tbe = (double *)malloc((T - 3) * sizeof(double));
  unsigned int i, b;

  make_trees(T, names, 100 + T, &ref, trees);
  rs = pllmod_utree_split_create(ref->vroot, T, NULL);
  printf("    {\n      \"tips\": %u,\n      \"labels\": [", T);
  /* labels[id]: the label of the tip whose node_index is id */
  {
    char ** by_id = (char **)malloc(T * sizeof(char *));
    for (i = 0; i < T; ++i) by_id[ref->nodes[i]->node_index] = ref->nodes[i]->label;
    for (i = 0; i < T; ++i) printf("%s\"%s\"", i ? ", " : "", by_id[i]);
    free(by_id);
  }
  printf("],\n");
  print_newick("      \"ref\": ", ref, ",");
  print_splits("      \"ref_splits\": ", rs, T, ",");
  printf("      \"trees\": [\n");
  for (b = 0; b < NTREES; ++b) print_newick("        ", trees[b], b + 1 < NTREES ? "," : "");
  printf("      ],\n      \"splits\": [\n");
  for (b = 0; b < NTREES; ++b)
  {
    bs[b] = pllmod_utree_split_create(trees[b]->vroot, T, NULL);
    print_splits("        ", bs[b], T, b + 1 < NTREES ? "," : "");
  }
  printf("      ],\n      \"rf_to_first\": [");
  for (b = 0; b < NTREES; ++b) printf("%s%u", b ? ", " : "", pllmod_utree_split_rf_distance(bs[0], bs[b], T));
  printf("],\n      \"rf_to_ref\": [");
  for (b = 0; b < NTREES; ++b) printf("%s%u", b ? ", " : "", pllmod_utree_split_rf_distance(rs, bs[b], T));
  printf("],\n      \"tbe\": [\n");
  for (b = 0; b < NTREES; ++b)
  {
    if (!pllmod_utree_tbe_naive(rs, bs[b], T, tbe)) { fprintf(stderr, "tbe_naive failed\n"); exit(1); }
    printf("        [");
    for (i = 0; i + 3 < T; ++i) printf("%s%.17g", i ? ", " : "", tbe[i]);
    printf("]%s\n", b + 1 < NTREES ? "," : "");
  }
  printf("      ]\n    }%s\n", last ? "" : ",");

  for (b = 0; b < NTREES; ++b) { pllmod_utree_split_destroy(bs[b]); pll_utree_destroy(trees[b], NULL); }
  pllmod_utree_split_destroy(rs);
  pll_utree_destroy(ref, NULL);
  for (i = 0; i < T; ++i) free(names[i]);
  free(names);
  free(tbe);
}

static int time_naive(unsigned int T, unsigned int B)
{
  char ** names = make_names(T);
  pll_utree_t * ref = pllmod_utree_create_random(T, (const char * const *)names, 7);
  pll_split_t * rs = pllmod_utree_split_create(ref->vroot, T, NULL);
  double * tbe = (double *)malloc((T - 3) * sizeof(double)), seconds = 0.0, sum = 0.0;
  unsigned int b, i;
  for (b = 0; b < B; ++b)
  {
    pll_utree_t * t = pll_utree_clone(ref);
    pll_split_t * s;
    struct timespec t0, t1;
    scramble(t, T / 10 + 1);
    pllmod_utree_consistency_set(ref, t);
    s = pllmod_utree_split_create(t->vroot, T, NULL);
    clock_gettime(CLOCK_MONOTONIC, &t0);
    pllmod_utree_tbe_naive(rs, s, T, tbe);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    seconds += (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    for (i = 0; i + 3 < T; ++i) sum += tbe[i];
    pllmod_utree_split_destroy(s);
    pll_utree_destroy(t, NULL);
  }
  printf("{\"tips\": %u, \"trees\": %u, \"tbe_naive_seconds\": %.6f, \"mean_support\": %.6f}\n", T, B, seconds,
         sum / ((double)B * (T - 3)));
  return 0;
}

/* the two tree pairs of the reference's test/src/tree/split-tbe.c and the values of test/out/tree/split-tbe.out */
static const char * REF_TREE =
  "(Woolly:0.02000173,Spider:0.01195957,(Howler:0.03921588,"
  "(((Squirrel:0.04951841,(Tamarin:0.01882103,PMarmoset:0.01872779)1000:0.01620522)432:0.00209062,"
  "(Titi:0.01974091,Saki:0.02183432)999:0.01197670)385:0.00073575,(((Gorilla:0.00549912,"
  "(Human:0.00667950,Chimp:0.00208720)792:0.00128616)986:0.00708195,"
  "(Gibbon:0.02407730,Orangutan:0.01258485)738:0.00147021)937:0.01302782,"
  "(Colobus:0.00276602,(DLangur:0.00477650,(Patas:0.01102645,"
  "((Tant_cDNA:0.00133132,AGM_cDNA:0.00133913)998:0.00516221,"
  "(Rhes_cDNA:0.00595363,Baboon:0.00312241)969:0.00413146)657:0.00250131)1000:0.01235639"
  ")505:0.00123650)1000:0.03064698)1000:0.13115789)998:0.01474962)1000:0.00860350);";
static const char * BOOT_TREE[2] = {
  "((Squirrel:0.04749782,((Saki:0.02577556,Titi:0.02534069):0.01417705,"
  "(Tamarin:0.01830913,PMarmoset:0.01752493):0.01595714):0.00164378):0.00319885,"
  "(Howler:0.03662786,(Spider:0.01128245,Woolly:0.02588956):0.00481877):0.01827684,"
  "(((Gorilla:0.00609643,(Chimp:0.00068926,Human:0.01011787):0.00064788):0.00456013,"
  "(Gibbon:0.02515313,Orangutan:0.00762452):0.00213596):0.01362313,"
  "((DLangur:0.00941860,Colobus:0.00415358):0.00389312,(Patas:0.01861160,"
  "((Baboon:0.00583652,Rhes_cDNA:0.00860553):0.00375633,(Tant_cDNA:0.00133482,"
  "AGM_cDNA:0.00001389):0.00461931):0.00341803):0.01152701):0.03383894):0.15261034);",
  "((Baboon:0.100000,(Colobus:0.100000,(Gibbon:0.100000,"
  "(Tamarin:0.100000,Human:0.100000):0.100000):0.100000):0.100000):0.100000,"
  "(DLangur:0.100000,(AGM_cDNA:0.100000,(Saki:0.100000,((Woolly:0.100000,"
  "Rhes_cDNA:0.100000):0.100000,Chimp:0.100000):0.100000):0.100000):0.100000):0.100000,"
  "(Squirrel:0.100000,((PMarmoset:0.100000,((Patas:0.100000,Tant_cDNA:0.100000):0.100000,"
  "(Spider:0.100000,(Titi:0.100000,"
  "(Howler:0.100000,Orangutan:0.100000):0.100000):0.100000):0.100000):0.100000):0.100000,"
  "Gorilla:0.100000):0.100000):0.100000):0.0;" };
static const char * PRINTED[2] = {
  "1.000000 1.000000 1.000000 1.000000 0.800000 1.000000 1.000000 1.000000 1.000000 1.000000 1.000000 1.000000 "
  "1.000000 1.000000 1.000000 0.500000 1.000000",
  "0.000000 0.000000 0.142857 0.166667 0.200000 0.250000 0.000000 0.000000 0.000000 0.000000 0.000000 0.000000 "
  "0.000000 0.000000 0.000000 0.000000 0.000000" };

static void record_own_test(void)
{
  int k;
  unsigned int i;
  printf("  \"split_tbe_out\": {\n    \"ref\": \"%s\",\n    \"pairs\": [\n", REF_TREE);
  for (k = 0; k < 2; ++k)
  {
    /* what this build computes must be what the reference's expected output prints */
    pll_utree_t * a = pll_utree_parse_newick_string(REF_TREE), * b = pll_utree_parse_newick_string(BOOT_TREE[k]);
    pll_split_t * sa, * sb;
    double tbe[17];
    char line[400] = "";
    pllmod_utree_consistency_set(a, b);
    sa = pllmod_utree_split_create(a->vroot, a->tip_count, NULL);
    sb = pllmod_utree_split_create(b->vroot, b->tip_count, NULL);
    pllmod_utree_tbe_naive(sa, sb, a->tip_count, tbe);
    for (i = 0; i < 17; ++i) snprintf(line + strlen(line), 16, "%s%.6lf", i ? " " : "", tbe[i]);
    if (strcmp(line, PRINTED[k])) { fprintf(stderr, "pair %d: computed '%s'\n", k, line); exit(1); }
    printf("      {\"tree\": \"%s\",\n       \"printed\": \"%s\"}%s\n", BOOT_TREE[k], PRINTED[k], k ? "" : ",");
    pllmod_utree_split_destroy(sa);
    pllmod_utree_split_destroy(sb);
    pll_utree_destroy(a, NULL);
    pll_utree_destroy(b, NULL);
  }
  printf("    ]\n  }\n");
}

int main(int argc, char ** argv)
{
  static const unsigned int TIPS[] = {4, 5, 8, 31, 32, 33, 64, 65};
  const unsigned int n = sizeof(TIPS) / sizeof(TIPS[0]);
  unsigned int k;
  if (argc == 4 && !strcmp(argv[1], "time")) return time_naive((unsigned int)atoi(argv[2]), (unsigned int)atoi(argv[3]));
  printf("{\n  \"cases\": [\n");
  for (k = 0; k < n; ++k) record(TIPS[k], k + 1 == n);
  printf("  ],\n");
  record_own_test();
  printf("}\n");
  return 0;
}
