/* record_msa_stats.c -- records tests/golden/msa_stats_fixtures.json: small alignments and what pll-modules'
 * pllmod_msa_empirical_frequencies, pllmod_msa_empirical_invariant_sites and pllmod_msa_compute_stats make of them
 * against the CPU oracle (tests/test_msa_stats_restatement.py pins its restatement to this file).
 *
 * The exchangeabilities are left out on purpose: the reference resets only half of its per-column counter
 * ("Empirical parameters and alignment statistics"), so they are no yardstick.
 *
 * Built outside the tree against a pll-modules checkout at $REF, the way oracle/Makefile.ref links binary_driver
 * (run from the repository root, after `make -C oracle`):
 *
 *   cc -std=gnu99 -D_GNU_SOURCE -O2 -w -ffunction-sections -Iinclude -I$REF/src -I$REF/src/msa \
 *      -o /tmp/record_msa_stats tests/golden/record_msa_stats.c $REF/src/pllmod_common.c $REF/src/msa/pll_msa.c \
 *      -Loracle/_build -lpll_oracle -lm -Wl,-rpath,$PWD/oracle/_build -Wl,--gc-sections
 *   /tmp/record_msa_stats > tests/golden/msa_stats_fixtures.json
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pll.h"
#include "pll_msa.h"

/* src/util is not linked: the one function of it that the statistics call */
size_t pllmod_util_subst_rate_count(unsigned int states) { return (size_t)states * (states - 1) / 2; }

static unsigned long long rng_state = 0x9E3779B97F4A7C15ULL;
static unsigned int rnd(unsigned int n)
{
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (unsigned int)((rng_state >> 33) % n);
}

typedef struct
{
  const char * name, * map_name;
  const pll_state_t * map;
  unsigned int states, count, length;
  const char * alphabet;           /* characters are drawn from it uniformly */
  int gap_col, gap_seq, dup_from, dup_to, dup_label;   /* -1: none */
  unsigned int max_weight;
  int attributes[2];               /* partitions to record (-1: none) */
} case_t;

static void print_ulongs(const char * key, const unsigned long * v, unsigned long n, const char * tail)
{
  unsigned long i;
  printf("      \"%s\": [", key);
  for (i = 0; i < n; ++i) printf("%s%lu", i ? ", " : "", v[i]);
  printf("]%s\n", tail);
}

static void print_doubles(const char * key, const double * v, unsigned long n, const char * tail, const char * indent)
{
  unsigned long i;
  printf("%s\"%s\": [", indent, key);
  for (i = 0; i < n; ++i) printf("%s%.17g", i ? ", " : "", v[i]);
  printf("]%s\n", tail);
}

static void record(const case_t * c, int last)
{
  unsigned int i, j, a;
  const size_t nalpha = strlen(c->alphabet);
  char ** rows = (char **)calloc(c->count, sizeof(char *));
  char ** labels = (char **)calloc(c->count, sizeof(char *));
  unsigned int * w = (unsigned int *)calloc(c->length, sizeof(unsigned int));
  for (i = 0; i < c->count; ++i)
  {
    rows[i] = (char *)calloc(c->length + 1, 1);
    labels[i] = (char *)calloc(16, 1);
    snprintf(labels[i], 16, "taxon%u", i);
    for (j = 0; j < c->length; ++j) rows[i][j] = c->alphabet[rnd((unsigned int)nalpha)];
  }
  /* a few columns where every sequence shows the same unambiguous character, so that some are invariant */
  for (j = 3; j < c->length; j += 7)
    for (i = 0; i < c->count; ++i) rows[i][j] = c->alphabet[j % 2];
  if (c->gap_col >= 0) for (i = 0; i < c->count; ++i) rows[i][c->gap_col] = '-';
  if (c->gap_seq >= 0) memset(rows[c->gap_seq], '-', c->length);
  if (c->dup_from >= 0) memcpy(rows[c->dup_to], rows[c->dup_from], c->length);
  if (c->dup_label >= 0) snprintf(labels[c->dup_label], 16, "taxon0");
  for (j = 0; j < c->length; ++j) w[j] = c->max_weight > 1 ? 1 + rnd(c->max_weight) : 1;

  printf("  {\n    \"name\": \"%s\", \"map\": \"%s\", \"states\": %u,\n", c->name, c->map_name, c->states);
  printf("    \"rows\": [");
  for (i = 0; i < c->count; ++i) printf("%s\"%s\"", i ? ", " : "", rows[i]);
  printf("],\n    \"labels\": [");
  for (i = 0; i < c->count; ++i) printf("%s\"%s\"", i ? ", " : "", labels[i]);
  printf("],\n    \"weights\": [");
  for (j = 0; j < c->length; ++j) printf("%s%u", j ? ", " : "", w[j]);
  printf("],\n");

  {
    pll_msa_t msa;
    pllmod_msa_stats_t * st;
    msa.count = (int)c->count;
    msa.length = (int)c->length;
    msa.sequence = rows;
    msa.label = labels;
    st = pllmod_msa_compute_stats(&msa, c->states, c->map, w, PLLMOD_MSA_STATS_ALL);
    if (!st) { fprintf(stderr, "%s: pllmod_msa_compute_stats failed: %s\n", c->name, pll_errmsg); exit(1); }
    printf("    \"stats\": {\n");
    print_ulongs("dup_taxa_pairs", st->dup_taxa_pairs, 2 * st->dup_taxa_pairs_count, ",");
    print_ulongs("dup_seqs_pairs", st->dup_seqs_pairs, 2 * st->dup_seqs_pairs_count, ",");
    printf("      \"gap_prop\": %.17g,\n", st->gap_prop);
    print_ulongs("gap_seqs", st->gap_seqs, st->gap_seqs_count, ",");
    print_ulongs("gap_cols", st->gap_cols, st->gap_cols_count, ",");
    printf("      \"inv_prop\": %.17g,\n", st->inv_prop);
    print_ulongs("inv_cols", st->inv_cols, st->inv_cols_count, ",");
    print_doubles("freqs", st->freqs, c->states, "", "      ");
    printf("    },\n");
    pllmod_msa_destroy_stats(st);
  }

  printf("    \"partitions\": [\n");
  for (a = 0; a < 2 && c->attributes[a] >= 0; ++a)
  {
    double * freqs, pinv;
    pll_partition_t * p = pll_partition_create(c->count, c->count - 2, c->states, c->length, 1, 2 * c->count - 3, 1,
                                               c->count - 2, (unsigned int)c->attributes[a]);
    if (!p) { fprintf(stderr, "%s: pll_partition_create failed: %s\n", c->name, pll_errmsg); exit(1); }
    for (i = 0; i < c->count; ++i)
      if (!pll_set_tip_states(p, i, c->map, rows[i])) { fprintf(stderr, "%s: pll_set_tip_states failed\n", c->name); exit(1); }
    pll_set_pattern_weights(p, w);
    freqs = pllmod_msa_empirical_frequencies(p);
    pinv = pllmod_msa_empirical_invariant_sites(p);
    if (!freqs) { fprintf(stderr, "%s: pllmod_msa_empirical_frequencies failed\n", c->name); exit(1); }
    printf("      {\"attributes\": %d, \"pinv\": %.17g,\n", c->attributes[a], pinv);
    print_doubles("freqs", freqs, c->states, "}", "       ");
    if (a + 1 < 2 && c->attributes[a + 1] >= 0) printf("      ,\n");
    free(freqs);
    pll_partition_destroy(p);
  }
  printf("    ]\n  }%s\n", last ? "" : ",");
  for (i = 0; i < c->count; ++i) { free(rows[i]); free(labels[i]); }
  free(rows); free(labels); free(w);
}

int main(void)
{
  /* ambiguity codes of 2 (R Y M K S W), 3 (B D H V) and 4 (N -) states among the plain ones */
  static const char * dna = "ACGTACGTACGTACGTACGTacgtRYMKSWBDHVN-";
  static const char * aa = "ARNDCQEGHILKMFPSTWYVARNDCQEGHILKMFPSTWYVBZX-";
  static const char * bin = "0101010101-";
  const case_t cases[] = {
    {"dna_6x65", "pll_map_nt", pll_map_nt, 4, 6, 65, dna, -1, -1, -1, -1, -1, 9, {PLL_ATTRIB_PATTERN_TIP, -1}},
    {"aa_5x40", "pll_map_aa", pll_map_aa, 20, 5, 40, aa, -1, -1, -1, -1, -1, 5, {PLL_ATTRIB_PATTERN_TIP, -1}},
    {"bin_4x33", "pll_map_bin", pll_map_bin, 2, 4, 33, bin, -1, -1, -1, -1, -1, 3, {PLL_ATTRIB_PATTERN_TIP, -1}},
    {"dna_gaps_dups_7x24", "pll_map_nt", pll_map_nt, 4, 7, 24, dna, 5, 3, 1, 6, 4, 4, {PLL_ATTRIB_PATTERN_TIP, -1}},
    {"dna_vector_tips_6x65", "pll_map_nt", pll_map_nt, 4, 6, 65, dna, 11, -1, -1, -1, -1, 9, {0, PLL_ATTRIB_PATTERN_TIP}},
    {"aa_vector_tips_5x40", "pll_map_aa", pll_map_aa, 20, 5, 40, aa, 2, -1, -1, -1, -1, 1, {0, -1}},
  };
  const unsigned int n = sizeof(cases) / sizeof(cases[0]);
  unsigned int k;
  printf("{\"cases\": [\n");
  for (k = 0; k < n; ++k) record(&cases[k], k + 1 == n);
  printf("]}\n");
  return 0;
}
