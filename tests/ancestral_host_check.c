/* ancestral_host_check.c -- pllhip_eval_compute_ancestral (csrc/host/pllhip_eval.c) on the CPU oracle's sources, as a
 * program of its own for -fsanitize=address,undefined: no device, no Python.  tests/test_ancestral.py builds it together
 * with the oracle's sources and the driver's two C files, and runs it.
 *
 * A 6-tip tree, a 4-state partition with two rate categories over 23 coded sites (one column of gaps):
 *   - both flag settings: rows sum to 1, states / state_probs follow the first-maximum rule, the summary is the same
 *     with and without the table, the root is where it was and the log-likelihood is unchanged;
 *   - the error path: a partition whose rate matrix is all zeros (no eigen-decomposition: the P-matrix update of the
 *     first re-rooting fails, after everything has been allocated) -- the call returns NULL with pll_errno set and the
 *     root restored, and nothing leaks.
 * Prints "ok" and exits 0; any finding exits 1 (the sanitizers add their own reports and status).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pll.h"
#include "pllhip.h"
#include "pllhip_eval.h"

#define TIPS 6u
#define SITES 23u

static const char * NEWICK = "((t0:0.11,t1:0.07):0.05,(t2:0.13,t3:0.04):0.06,(t4:0.12,t5:0.02):0.08);";

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED: " __VA_ARGS__); printf("\n"); ++bad; } } while (0)

static pll_partition_t * make_partition(const pll_utree_t * tree, int degenerate)
{
  static const double gtr[6] = {1.452176, 0.937951, 0.462880, 0.617729, 1.745312, 1.0};
  static const double zeros[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double * subst = degenerate ? zeros : gtr;
  static const double freqs[4] = {0.17, 0.19, 0.25, 0.39};
  double rates[2];
  char seq[SITES + 1];
  unsigned int t, i;
  unsigned long long s = 0x9e3779b97f4a7c15ULL;
  pll_partition_t * part = pll_partition_create(TIPS, TIPS - 2u, 4, SITES, 1, 2u * TIPS - 3u, 2, TIPS - 2u,
                                                PLL_ATTRIB_ARCH_CPU | PLL_ATTRIB_PATTERN_TIP);
  if (!part) return NULL;
  if (!pll_compute_gamma_cats(0.7, 2, rates, PLL_GAMMA_RATES_MEAN)) abort();
  pll_set_subst_params(part, 0, subst);
  pll_set_frequencies(part, 0, freqs);
  pll_set_category_rates(part, rates);
  for (t = 0; t < TIPS; ++t)
  {
    const pll_unode_t * tip = tree->nodes[t];
    for (i = 0; i < SITES; ++i)
    {
      s = s * 6364136223846793005ULL + 1442695040888963407ULL;
      seq[i] = (i == 5) ? '-' : "ACGT"[(s >> 40) & 3u];
    }
    seq[SITES] = 0;
    if (!pll_set_tip_states(part, tip->clv_index, pll_map_nt, seq)) abort();
  }
  return part;
}

static void check_result(const pllhip_ancestral_t * anc, int with_probs)
{
  unsigned int i, n, k;
  CHECK(anc->node_count == TIPS - 2u && anc->partition_count == 1u, "counts %u %u", anc->node_count, anc->partition_count);
  CHECK(anc->partition_indices[0] == 0u, "partition index");
  CHECK(anc->site_offset[0] == 0 && anc->site_offset[1] == SITES, "site offsets");
  CHECK(anc->prob_offset[0] == 0 && anc->prob_offset[1] == (size_t)SITES * 4, "prob offsets");
  CHECK((anc->probs != NULL) == (with_probs != 0), "probs present: %d", anc->probs != NULL);
  for (i = 0; i < anc->node_count; ++i)
  {
    CHECK(anc->nodes[i] && anc->nodes[i]->next, "node %u is not an inner record", i);
    for (n = 0; n < SITES; ++n)
    {
      CHECK(anc->states[i][n] < 4, "state %u", anc->states[i][n]);
      CHECK(anc->state_probs[i][n] >= 0.25 - 1e-12 && anc->state_probs[i][n] <= 1.0 + 1e-12, "state_probs %g",
            anc->state_probs[i][n]);
      if (with_probs)
      {
        const double * row = anc->probs[i] + (size_t)n * 4;
        double sum = 0.0, best = row[0];
        unsigned int idx = 0;
        for (k = 0; k < 4; ++k) sum += row[k];
        for (k = 1; k < 4; ++k) if (row[k] > best) { best = row[k]; idx = k; }
        CHECK(fabs(sum - 1.0) <= 1e-12, "row sum %.17g", sum);
        CHECK(anc->states[i][n] == idx && anc->state_probs[i][n] == best, "summary of node %u site %u", i, n);
      }
    }
  }
}

int main(void)
{
  static const unsigned int params[2] = {0, 0};
  pll_utree_t * tree = pll_utree_parse_newick_string(NEWICK);
  pll_partition_t * part = tree ? make_partition(tree, 0) : NULL;
  pll_partition_t * broken = tree ? make_partition(tree, 1) : NULL;
  pllhip_eval_t * ev = tree ? pllhip_eval_create(tree, 1, 0) : NULL;
  pllhip_ancestral_t * full, * brief, * none;
  pll_unode_t * root;
  double before, after;
  unsigned int i;
  if (!tree || !part || !broken || !ev) { fprintf(stderr, "setting up: %s\n", pll_errmsg); return 2; }
  if (!pllhip_eval_set_partition(ev, 0, part, params)) return 2;

  before = pllhip_eval_loglh(ev, 0);
  root = pllhip_eval_root(ev);
  CHECK(isfinite(before) && before < 0.0, "lnL %g", before);

  full = pllhip_eval_compute_ancestral(ev, PLLHIP_ANC_PROBS);
  CHECK(full != NULL, "with the table: %s", pll_errmsg);
  CHECK(pllhip_eval_root(ev) == root, "root after the call");
  brief = pllhip_eval_compute_ancestral(ev, 0);
  CHECK(brief != NULL, "without the table: %s", pll_errmsg);
  CHECK(pllhip_eval_root(ev) == root, "root after the second call");
  if (full) check_result(full, 1);
  if (brief) check_result(brief, 0);
  for (i = 0; full && brief && i < full->node_count; ++i)
  {
    CHECK(full->nodes[i] == brief->nodes[i], "node order");
    CHECK(!memcmp(full->states[i], brief->states[i], SITES), "states of node %u with and without the table", i);
    CHECK(!memcmp(full->state_probs[i], brief->state_probs[i], SITES * sizeof(double)), "state_probs of node %u", i);
  }
  after = pllhip_eval_loglh(ev, 1);
  CHECK(fabs(after - before) <= 1e-8 * fabs(before), "lnL %.17g before, %.17g after", before, after);
  pllhip_eval_destroy_ancestral(full);
  pllhip_eval_destroy_ancestral(brief);
  pllhip_eval_destroy_ancestral(NULL);

  /* unknown flags: refused before anything is allocated */
  pll_errno = 0;
  none = pllhip_eval_compute_ancestral(ev, 1u << 7);
  CHECK(none == NULL && pll_errno == PLL_ERROR_PARAM_INVALID, "unknown flags: errno %d", pll_errno);

  /* a partition without a usable rate matrix: the first re-rooting fails */
  if (!pllhip_eval_set_partition(ev, 0, broken, params)) return 2;
  pllhip_eval_invalidate_all(ev);
  pll_errno = 0;
  none = pllhip_eval_compute_ancestral(ev, PLLHIP_ANC_PROBS);
  CHECK(none == NULL, "the broken partition gave a result");
  CHECK(pll_errno != 0, "no error code for the broken partition");
  CHECK(pllhip_eval_root(ev) == root, "root after the failed call");
  pllhip_eval_destroy_ancestral(none);

  /* and the evaluator still works with the good one */
  if (!pllhip_eval_set_partition(ev, 0, part, params)) return 2;
  after = pllhip_eval_loglh(ev, 0);
  CHECK(fabs(after - before) <= 1e-8 * fabs(before), "lnL %.17g before, %.17g at the end", before, after);

  pllhip_eval_destroy(ev);
  pll_partition_destroy(part);
  pll_partition_destroy(broken);
  pll_utree_destroy(tree, NULL);
  if (bad) { printf("FAILED: %d findings\n", bad); return 1; }
  printf("ok\n");
  return 0;
}
