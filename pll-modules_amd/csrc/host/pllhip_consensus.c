/* pllhip_consensus.c -- the host side of the tree set's consensus (treeset_plan.h): the integer thresholds, and the
 * multifurcating tree of a system of compatible splits.  Plain C, no device call. */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "treeset_plan.h"

static void * fail(int code, const char * msg)
{
  pll_errno = code;
  snprintf(pll_errmsg, 200, "%s", msg);
  return NULL;
}

/* the smallest c in 0 .. B with (double)c / (double)B > cut, for a cut below 1 */
static unsigned int first_above(unsigned int B, double cut)
{
  unsigned int lo = 0, hi = B;                     /* the quotient does not decrease with c, and B / B = 1 > cut */
  while (lo < hi)
  {
    const unsigned int mid = lo + (hi - lo) / 2u;
    if ((double)mid / (double)B > cut) hi = mid; else lo = mid + 1u;
  }
  return lo;
}

int pllhip_ts_consensus_needs(unsigned int B, double threshold, unsigned int * need_major, unsigned int * need_minor)
{
  unsigned int major, minor;
  if (!B || !(threshold >= 0.0 && threshold <= 1.0))
  {
    fail(PLL_ERROR_PARAM_INVALID, "consensus: the threshold must lie in [0, 1] and the set must hold a tree");
    return PLL_FAILURE;
  }
  if (threshold == 1.0) major = B;
  else if (threshold <= 0.5) major = B / 2u + 1u;
  else major = first_above(B, threshold);
  if (threshold >= 0.5) minor = major;
  else if (threshold == 0.0) minor = 1u;
  else minor = first_above(B, threshold);
  if (minor < 1u) minor = 1u;
  if (need_major) *need_major = major;
  if (need_minor) *need_minor = minor;
  return PLL_SUCCESS;
}

/* ---- the tree of a split system ---- */

typedef struct
{
  unsigned int size;         /* tips on the side away from tip 0 */
  unsigned int kids;
  long parent;               /* a cluster, ROOT, or UNSET */
  pll_unode_t * head;        /* the record that looks towards tip 0 */
  pll_unode_t * cursor;      /* the next free record of the ring */
} cs_cluster_t;

#define CS_UNSET (-2L)
#define CS_ROOT  (-1L)

typedef struct
{
  pll_unode_t ** rec;
  char ** text;
  size_t nrec, ntext;
} cs_pool_t;

static pll_unode_t * new_record(cs_pool_t * pool)
{
  pll_unode_t * r = (pll_unode_t *)calloc(1, sizeof(pll_unode_t));
  if (!r) return NULL;
  r->scaler_index = PLL_SCALE_BUFFER_NONE;
  pool->rec[pool->nrec++] = r;
  return r;
}

/* a ring of `count` records that share `label`; NULL: out of memory */
static pll_unode_t * new_ring(cs_pool_t * pool, unsigned int count, char * label)
{
  pll_unode_t * head = NULL, * prev = NULL;
  unsigned int k;
  for (k = 0; k < count; ++k)
  {
    pll_unode_t * r = new_record(pool);
    if (!r) return NULL;
    r->label = label;
    if (prev) prev->next = r; else head = r;
    prev = r;
  }
  prev->next = head;
  return head;
}

static void join(pll_unode_t * a, pll_unode_t * b)
{
  a->back = b;
  b->back = a;
}

static char * support_text(double v)
{
  char buf[40];
  int digits;
  for (digits = 1; digits <= 17; ++digits)
  {
    snprintf(buf, sizeof(buf), "%.*g", digits, v);
    if (strtod(buf, NULL) == v) break;
  }
  return strdup(buf);
}

static int by_size(const void * a, const void * b, void * ctx)
{
  const cs_cluster_t * c = (const cs_cluster_t *)ctx;
  const unsigned int x = *(const unsigned int *)a, y = *(const unsigned int *)b;
  if (c[x].size != c[y].size) return c[x].size < c[y].size ? -1 : 1;
  return x < y ? -1 : (x > y ? 1 : 0);
}

pll_utree_t * pllhip_ts_tree_from_splits(unsigned int T, const pllhip_ts_labels_t * labels, unsigned int K,
                                         const uint32_t * words, const double * support)
{
  const unsigned int len = pllhip_ts_words(T);
  const uint32_t last = (T % 32u) ? ((1u << (T % 32u)) - 1u) : 0xffffffffu;
  cs_cluster_t * cl = NULL;
  unsigned int * sorted = NULL, i, w, t, root_kids = 1;
  long * owner = NULL, * below = NULL;             /* per tip: the largest cluster so far that holds it; the smallest */
  pll_unode_t ** tip = NULL, * root = NULL, * root_cursor = NULL;
  cs_pool_t pool = {NULL, NULL, 0, 0};
  pll_utree_t * tree = NULL;

  if (T < 4u || T > PLLHIP_TS_MAX_TIPS || K > T - 3u || (K && !words))
    return (pll_utree_t *)fail(PLL_ERROR_PARAM_INVALID, "consensus tree: 4 .. 65535 tips and at most T - 3 splits");

  cl = (cs_cluster_t *)calloc(K ? K : 1u, sizeof(cs_cluster_t));
  sorted = (unsigned int *)malloc((K ? K : 1u) * sizeof(unsigned int));
  owner = (long *)malloc((size_t)T * sizeof(long));
  below = (long *)malloc((size_t)T * sizeof(long));
  tip = (pll_unode_t **)calloc(T, sizeof(pll_unode_t *));
  pool.rec = (pll_unode_t **)calloc(2u * ((size_t)T + K), sizeof(pll_unode_t *));
  pool.text = (char **)calloc((size_t)T + K, sizeof(char *));
  if (!cl || !sorted || !owner || !below || !tip || !pool.rec || !pool.text)
  { fail(PLL_ERROR_MEM_ALLOC, "consensus tree: cannot allocate the builder's arrays"); goto done; }

  for (i = 0; i < K; ++i)
  {
    const uint32_t * v = words + (size_t)i * len;
    unsigned int ones = 0;
    for (w = 0; w < len; ++w) ones += (unsigned int)__builtin_popcount(v[w]);
    if (!(v[0] & 1u) || (v[len - 1u] & ~last) || ones < 2u || ones > T - 2u)
    { fail(PLL_ERROR_PARAM_INVALID, "consensus tree: a split is trivial or not in normal form"); goto done; }
    cl[i].size = T - ones;
    cl[i].parent = CS_UNSET;
    sorted[i] = i;
  }
  if (K) qsort_r(sorted, K, sizeof(unsigned int), by_size, cl);
  for (t = 0; t < T; ++t) owner[t] = below[t] = CS_ROOT;

  /* smaller clusters first: what a tip belonged to so far lies inside the cluster at hand, or the two overlap */
  for (i = 0; i < K; ++i)
  {
    const unsigned int c = sorted[i];
    const uint32_t * v = words + (size_t)c * len;
    for (w = 0; w < len; ++w)
    {
      uint32_t m = ~v[w] & (w + 1u == len ? last : 0xffffffffu);
      for (; m; m &= m - 1u)
      {
        const long o = owner[t = 32u * w + (unsigned int)__builtin_ctz(m)];
        if (o == CS_ROOT) { below[t] = (long)c; cl[c].kids += 1u; }
        else if (cl[o].parent == CS_UNSET)
        {
          const uint32_t * inner = words + (size_t)o * len;
          unsigned int x;
          int inside = cl[o].size < cl[c].size;
          for (x = 0; x < len && inside; ++x)
            if (~inner[x] & v[x] & (x + 1u == len ? last : 0xffffffffu)) inside = 0;
          if (!inside)
          { fail(PLL_ERROR_PARAM_INVALID, "consensus tree: two splits are equal or incompatible"); goto done; }
          cl[o].parent = (long)c;
          cl[c].kids += 1u;
        }
        else if (cl[o].parent != (long)c)
        { fail(PLL_ERROR_PARAM_INVALID, "consensus tree: two splits are incompatible"); goto done; }
        owner[t] = (long)c;
      }
    }
  }
  for (t = 1; t < T; ++t) root_kids += below[t] == CS_ROOT ? 1u : 0u;
  for (i = 0; i < K; ++i) root_kids += cl[i].parent == CS_UNSET ? 1u : 0u;

  /* records: a tip is one, an inner node a ring of one per neighbour */
  for (t = 0; t < T; ++t)
  {
    const char * label = pllhip_ts_labels_get(labels, t);
    if (!(tip[t] = new_record(&pool))) { fail(PLL_ERROR_MEM_ALLOC, "consensus tree: out of memory"); goto done; }
    if (label)
    {
      if (!(tip[t]->label = strdup(label))) { fail(PLL_ERROR_MEM_ALLOC, "consensus tree: out of memory"); goto done; }
      pool.text[pool.ntext++] = tip[t]->label;
    }
    tip[t]->node_index = tip[t]->clv_index = tip[t]->pmatrix_index = t;
  }
  for (i = 0; i < K; ++i)
  {
    char * text = support ? support_text(support[i]) : NULL;
    if (support)
    {
      if (!text) { fail(PLL_ERROR_MEM_ALLOC, "consensus tree: out of memory"); goto done; }
      pool.text[pool.ntext++] = text;
    }
    if (!(cl[i].head = new_ring(&pool, cl[i].kids + 1u, text)))
    { fail(PLL_ERROR_MEM_ALLOC, "consensus tree: out of memory"); goto done; }
    cl[i].cursor = cl[i].head->next;
  }
  if (!(root = new_ring(&pool, root_kids, NULL))) { fail(PLL_ERROR_MEM_ALLOC, "consensus tree: out of memory"); goto done; }
  join(root, tip[0]);
  root_cursor = root->next;

  for (i = 0; i < K; ++i)
  {
    pll_unode_t ** at = cl[i].parent == CS_UNSET ? &root_cursor : &cl[cl[i].parent].cursor;
    join(*at, cl[i].head);
    *at = (*at)->next;
  }
  for (t = 1; t < T; ++t)
  {
    pll_unode_t ** at = below[t] == CS_ROOT ? &root_cursor : &cl[below[t]].cursor;
    join(*at, tip[t]);
    *at = (*at)->next;
  }

  pll_utree_reset_template_indices(root, T);
  tree = pll_utree_wraptree_multi(root, T, K + 1u);

done:
  if (!tree)
  {
    size_t k;
    for (k = 0; k < pool.nrec; ++k) free(pool.rec[k]);
    for (k = 0; k < pool.ntext; ++k) free(pool.text[k]);
  }
  free(cl); free(sorted); free(owner); free(below); free(tip); free(pool.rec); free(pool.text);
  return tree;
}
