/* eval_threads_host_check.c -- the evaluation driver (csrc/host/pllhip_eval.c, pllhip_search.c) run by several host
 * threads of one process, the way pll-modules' worker threads run treeinfo: every thread owns a partition over its
 * slice of the sites and an evaluator of its own, and the threads meet only in the reduce callback.  A program of
 * its own for -fsanitize=thread: no device, no Python (the C++ / HIP host code cannot be built for the CPU and is
 * not covered).
 *
 * Build and run from the repository root (no -fopenmp: libgomp is not instrumented and drowns the report):
 *
 *   make -C oracle OUT=/tmp/oracle_tsan CFLAGS="-O1 -g -fno-omit-frame-pointer -fsanitize=thread -march=x86-64-v3 \
 *       -fno-fast-math -ffp-contract=off -std=gnu99 -fPIC -Wall -Wextra -Wno-unused-parameter -Wno-unknown-pragmas \
 *       -fvisibility=default"
 *   gcc -std=gnu99 -O1 -g -fno-omit-frame-pointer -fsanitize=thread -Iinclude -o /tmp/eval_threads_host_check \
 *       tools/eval_threads_host_check.c -L/tmp/oracle_tsan -Wl,-rpath,/tmp/oracle_tsan -lpll_oracle -lpthread -lm
 *   /tmp/eval_threads_host_check
 *
 * W = 2 and W = 3 threads.  Each parses the same newick string, builds a 4-state, 4-category partition over its
 * slice of 401 seeded sites, and calls pllhip_eval_loglh, pllhip_eval_optimize_branches (4 iterations) and one
 * pllhip_eval_spr_round.  The reduce callback combines the threads' payloads in rank order behind a pthread
 * barrier, so every thread holds bit-identical values.  Exit status 0 and "ok" when the threads agree bit for bit
 * and every value is finite; ThreadSanitizer adds its own non-zero status (66) when it has reported a race.
 */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pll.h"
#include "pllhip_eval.h"

#define TIPS 8u
#define SITES 401u
#define MAX_WORKERS 3u
#define MAX_PAYLOAD 1024u

static const char * NEWICK =
  "((t0:0.11,t1:0.07):0.05,(t2:0.13,(t3:0.04,t4:0.09):0.06):0.03,((t5:0.12,t6:0.02):0.08,t7:0.15):0.10);";

typedef struct
{
  unsigned int workers;
  pthread_barrier_t barrier;
  double slots[MAX_WORKERS][MAX_PAYLOAD];
} group_t;

typedef struct
{
  group_t * group;
  unsigned int rank;
  int failed;
  double lnl, lnl_opt, lnl_spr;
  unsigned long moves;
  char * newick;
} worker_t;

/* the alignment every worker cuts its slice from: a seeded walk down the tips, so that columns are not pure noise */
static void make_alignment(char rows[TIPS][SITES + 1])
{
  unsigned long long s = 0x9e3779b97f4a7c15ULL;
  unsigned int t, i;
  for (i = 0; i < SITES; ++i)
  {
    char c = 0;
    for (t = 0; t < TIPS; ++t)
    {
      s = s * 6364136223846793005ULL + 1442695040888963407ULL;
      if (t == 0 || ((s >> 33) & 7u) < 3u) c = "ACGT"[(s >> 40) & 3u];
      rows[t][i] = c;
    }
  }
  for (t = 0; t < TIPS; ++t) rows[t][SITES] = 0;
}

static void reduce_cb(void * ctx, double * data, size_t n, int op)
{
  worker_t * w = (worker_t *)ctx;
  group_t * g = w->group;
  unsigned int r;
  size_t i;
  if (n > MAX_PAYLOAD) { fprintf(stderr, "eval_threads_host_check: a payload of %zu values\n", n); abort(); }
  memcpy(g->slots[w->rank], data, n * sizeof(double));
  pthread_barrier_wait(&g->barrier);
  for (i = 0; i < n; ++i)
  {
    double a = g->slots[0][i];
    for (r = 1; r < g->workers; ++r)
    {
      const double b = g->slots[r][i];
      a = op == 0 ? a + b : op == 1 ? (b > a ? b : a) : (b < a ? b : a);
    }
    data[i] = a;
  }
  pthread_barrier_wait(&g->barrier);       /* nobody overwrites a slot that somebody still reads */
}

static char rows[TIPS][SITES + 1];

static void * work(void * arg)
{
  worker_t * w = (worker_t *)arg;
  const unsigned int W = w->group->workers;
  const unsigned int lo = SITES * w->rank / W, hi = SITES * (w->rank + 1u) / W, n = hi - lo;
  static const double subst[6] = {1.452176, 0.937951, 0.462880, 0.617729, 1.745312, 1.0};
  static const double freqs[4] = {0.17, 0.19, 0.25, 0.39};
  static const unsigned int params[4] = {0, 0, 0, 0};
  double rates[4];
  char slice[SITES + 1];
  pll_utree_t * tree = pll_utree_parse_newick_string(NEWICK);
  pll_partition_t * part = pll_partition_create(TIPS, TIPS - 2u, 4, n, 1, 2u * TIPS - 3u, 4, TIPS - 2u,
                                                PLL_ATTRIB_ARCH_CPU | PLL_ATTRIB_PATTERN_TIP);
  pllhip_eval_t * ev = tree ? pllhip_eval_create(tree, 1, 0) : NULL;
  pllhip_spr_params_t prm = {1, 5, 5, 0, 1e-4, 10.0, 8, 0.1, 1.0, 0.1};
  pllhip_spr_stats_t stats;
  unsigned int i;
  /* a worker that cannot set itself up would leave its peers in the barrier: end the program */
  if (!tree || !part || !ev) { fprintf(stderr, "worker %u: setting up: %s\n", w->rank, pll_errmsg); abort(); }
  if (!pll_compute_gamma_cats(0.841, 4, rates, PLL_GAMMA_RATES_MEAN)) abort();
  pll_set_subst_params(part, 0, subst);
  pll_set_frequencies(part, 0, freqs);
  pll_set_category_rates(part, rates);
  for (i = 0; i < TIPS; ++i)
  {
    const pll_unode_t * tip = tree->nodes[i];
    const unsigned int row = (unsigned int)atoi(tip->label + 1);
    memcpy(slice, rows[row] + lo, n);
    slice[n] = 0;
    if (!pll_set_tip_states(part, tip->clv_index, pll_map_nt, slice)) abort();
  }
  if (!pllhip_eval_set_partition(ev, 0, part, params)) abort();
  pllhip_eval_set_parallel_context(ev, w, reduce_cb);

  w->lnl = pllhip_eval_loglh(ev, 0);
  w->lnl_opt = -pllhip_eval_optimize_branches(ev, 1e-4, 10.0, 0.01, 4, PLLHIP_EVAL_RADIUS_ALL);
  w->lnl_spr = pllhip_eval_spr_round(ev, &prm, NULL, &stats);
  w->moves = stats.moves_applied;
  w->newick = pll_utree_export_newick(pllhip_eval_root(ev), NULL);
  w->failed = !(isfinite(w->lnl) && isfinite(w->lnl_opt) && isfinite(w->lnl_spr) && w->lnl < 0.0 &&
                w->lnl_opt < 0.0 && w->lnl_spr < 0.0 && w->newick);

  pllhip_eval_destroy(ev);
  pll_partition_destroy(part);
  pll_utree_destroy(tree, NULL);
  return NULL;
}

int main(void)
{
  unsigned int W, r, bad = 0;
  make_alignment(rows);
  for (W = 2; W <= MAX_WORKERS; ++W)
  {
    static group_t group;
    worker_t workers[MAX_WORKERS];
    pthread_t threads[MAX_WORKERS];
    memset(workers, 0, sizeof(workers));
    group.workers = W;
    pthread_barrier_init(&group.barrier, NULL, W);
    for (r = 0; r < W; ++r)
    {
      workers[r].group = &group;
      workers[r].rank = r;
      workers[r].failed = 1;
      if (pthread_create(&threads[r], NULL, work, &workers[r])) { perror("pthread_create"); return 2; }
    }
    for (r = 0; r < W; ++r) pthread_join(threads[r], NULL);
    pthread_barrier_destroy(&group.barrier);
    for (r = 0; r < W; ++r)
    {
      const worker_t * w = &workers[r], * w0 = &workers[0];
      printf("W=%u rank %u: lnL %.17g  after 4 branch-length iterations %.17g  after one SPR round %.17g  (%lu moves)\n",
             W, r, w->lnl, w->lnl_opt, w->lnl_spr, w->moves);
      if (w->failed) { printf("W=%u rank %u: a value is not finite or not a log-likelihood\n", W, r); ++bad; continue; }
      if (w0->failed) continue;
      if (memcmp(&w->lnl, &w0->lnl, sizeof(double)) || memcmp(&w->lnl_opt, &w0->lnl_opt, sizeof(double)) ||
          memcmp(&w->lnl_spr, &w0->lnl_spr, sizeof(double)) || w->moves != w0->moves || strcmp(w->newick, w0->newick))
      {
        printf("W=%u rank %u disagrees with rank 0\n", W, r);
        ++bad;
      }
    }
    if (!workers[0].failed) printf("W=%u tree: %s\n", W, workers[0].newick);
    for (r = 0; r < W; ++r) free(workers[r].newick);
  }
  if (bad) { printf("FAILED: %u findings\n", bad); return 1; }
  printf("ok\n");
  return 0;
}
