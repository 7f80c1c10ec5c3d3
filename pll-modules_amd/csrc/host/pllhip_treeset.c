/* pllhip_treeset.c -- the host side of the tree set (treeset_plan.h): label table, validation, and the flattening of
 * one tree into a split plan and a transfer program.  Plain C, no device call; the tree is only read. */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "treeset_plan.h"

static int fail(int code, const char * msg)
{
  pll_errno = code;
  snprintf(pll_errmsg, 200, "%s", msg);
  return PLL_FAILURE;
}

/* ---- label table: (label, id) sorted by label ---- */

typedef struct { const char * label; unsigned int id; } ts_label_t;

struct pllhip_ts_labels
{
  unsigned int count;
  ts_label_t * entry;
  char * text;
  const char ** by_id;
};

static int label_cmp(const void * a, const void * b)
{
  return strcmp(((const ts_label_t *)a)->label, ((const ts_label_t *)b)->label);
}

pllhip_ts_labels_t * pllhip_ts_labels_create(unsigned int tip_count, const char * const * labels)
{
  unsigned int i;
  size_t bytes = 0, at = 0;
  pllhip_ts_labels_t * t;
  if (!labels || !tip_count) { fail(PLL_ERROR_PARAM_INVALID, "tree set: no labels"); return NULL; }
  for (i = 0; i < tip_count; ++i)
  {
    if (!labels[i]) { fail(PLL_ERROR_PARAM_INVALID, "tree set: a NULL label"); return NULL; }
    bytes += strlen(labels[i]) + 1;
  }
  t = (pllhip_ts_labels_t *)calloc(1, sizeof(*t));
  if (t)
  {
    t->entry = (ts_label_t *)malloc(tip_count * sizeof(ts_label_t));
    t->text = (char *)malloc(bytes);
    t->by_id = (const char **)malloc(tip_count * sizeof(char *));
  }
  if (!t || !t->entry || !t->text || !t->by_id)
  {
    pllhip_ts_labels_destroy(t);
    fail(PLL_ERROR_MEM_ALLOC, "tree set: cannot allocate the label table");
    return NULL;
  }
  t->count = tip_count;
  for (i = 0; i < tip_count; ++i)
  {
    const size_t n = strlen(labels[i]) + 1;
    memcpy(t->text + at, labels[i], n);
    t->entry[i].label = t->text + at;
    t->entry[i].id = i;
    t->by_id[i] = t->text + at;
    at += n;
  }
  qsort(t->entry, tip_count, sizeof(ts_label_t), label_cmp);
  for (i = 1; i < tip_count; ++i)
    if (!strcmp(t->entry[i - 1].label, t->entry[i].label))
    {
      char msg[200];
      snprintf(msg, sizeof(msg), "tree set: label '%.100s' is given twice", t->entry[i].label);
      pllhip_ts_labels_destroy(t);
      fail(PLL_ERROR_PARAM_INVALID, msg);
      return NULL;
    }
  return t;
}

void pllhip_ts_labels_destroy(pllhip_ts_labels_t * t)
{
  if (!t) return;
  free(t->entry);
  free(t->text);
  free((void *)t->by_id);
  free(t);
}

const char * pllhip_ts_labels_get(const pllhip_ts_labels_t * t, unsigned int id)
{
  return t && id < t->count ? t->by_id[id] : NULL;
}

long pllhip_ts_labels_find(const pllhip_ts_labels_t * t, const char * label)
{
  ts_label_t key, * hit;
  if (!t || !label) return -1;
  key.label = label;
  key.id = 0;
  hit = (ts_label_t *)bsearch(&key, t->entry, t->count, sizeof(ts_label_t), label_cmp);
  return hit ? (long)hit->id : -1;
}

/* ---- flattening ---- */

static unsigned int floor_log2(unsigned int v)
{
  unsigned int r = 0;
  while (v >>= 1) ++r;
  return r;
}

/* the id of a tip record, or -1 with the error set */
static long tip_id(const pll_unode_t * tip, unsigned int T, const pllhip_ts_labels_t * labels)
{
  char msg[200];
  if (labels)
  {
    const long id = tip->label ? pllhip_ts_labels_find(labels, tip->label) : -1;
    if (id >= 0) return id;
    snprintf(msg, sizeof(msg), "tree set: tip label '%.100s' is not one of the set's labels",
             tip->label ? tip->label : "(none)");
    fail(PLL_ERROR_PARAM_INVALID, msg);
    return -1;
  }
  if (tip->node_index < T) return (long)tip->node_index;
  snprintf(msg, sizeof(msg), "tree set: tip node_index %u is not below the tip count %u", tip->node_index, T);
  fail(PLL_ERROR_PARAM_INVALID, msg);
  return -1;
}

typedef struct
{
  const pll_unode_t * rec;   /* the record that looks towards tip 0 */
  uint32_t kid[2];           /* positions of the children in `node` (inner nodes) */
  uint32_t size;             /* tips below */
  uint32_t need;             /* stack entries its subprogram needs */
  uint32_t start;            /* first position of its tips in order */
  uint32_t tip;              /* id (tips) */
} ts_node_t;

int pllhip_ts_flatten(const pll_utree_t * tree, unsigned int T, const pllhip_ts_labels_t * labels,
                      uint32_t * order, uint32_t * lo, uint32_t * hi, pll_unode_t ** edge,
                      pllhip_ts_step_t * program, unsigned int * max_stack)
{
  const unsigned int total = 2u * T - 3u;          /* nodes below tip 0's neighbour, that neighbour included */
  const pll_unode_t * root = NULL;
  ts_node_t * node = NULL;
  uint32_t * stack = NULL;                         /* DFS: positions; emission: position * 2 + state */
  unsigned char * seen = NULL;
  unsigned int n = 0, sp = 0, i, ntips = 0, nedges = 0, nsteps = 0, depth = 0, deepest = 0;
  int rc = PLL_FAILURE;

  if (!tree || !order || !lo || !hi || !program)
    return fail(PLL_ERROR_PARAM_INVALID, "tree set: NULL argument");
  if (T < 4u || T > PLLHIP_TS_MAX_TIPS) return fail(PLL_ERROR_PARAM_INVALID, "tree set: 4 .. 65535 tips");
  if (!tree->nodes || tree->tip_count != T)
    return fail(PLL_ERROR_TREE_INVALID, "tree set: the tree has another number of tips than the set");
  if (tree->inner_count != T - 2u)
    return fail(PLL_ERROR_TREE_INVALID, "tree set: the tree is not binary");

  node = (ts_node_t *)malloc((size_t)total * sizeof(ts_node_t));
  stack = (uint32_t *)malloc((size_t)(total + 1u) * sizeof(uint32_t));
  seen = (unsigned char *)calloc(T, 1);
  if (!node || !stack || !seen) { fail(PLL_ERROR_MEM_ALLOC, "tree set: cannot allocate the flattener's arrays"); goto done; }

  /* the tip of id 0 */
  for (i = 0; i < T; ++i)
  {
    const pll_unode_t * tip = tree->nodes[i];
    long id;
    if (!tip || tip->next || !tip->back || tip->back->back != tip)
    { fail(PLL_ERROR_TREE_INVALID, "tree set: the first tip_count nodes of the tree are not linked tips"); goto done; }
    id = tip_id(tip, T, labels);
    if (id < 0) goto done;
    if (seen[id])
    { fail(PLL_ERROR_PARAM_INVALID, "tree set: two tips of the tree have the same id or label"); goto done; }
    seen[id] = 1;
    if (id == 0) root = tip;
  }
  /* T distinct ids below T: every id is present, id 0 among them */
  memset(seen, 0, T);
  seen[0] = 1;
  if (root->back->next == NULL) { fail(PLL_ERROR_TREE_INVALID, "tree set: two tips joined by one edge"); goto done; }

  /* preorder: parents before children */
  node[0].rec = root->back;
  n = 1;
  stack[sp++] = 0;
  while (sp)
  {
    const uint32_t pos = stack[--sp];
    const pll_unode_t * rec = node[pos].rec;
    if (!rec->next)
    {
      const long id = tip_id(rec, T, labels);
      if (id < 0) goto done;
      if (seen[id]) { fail(PLL_ERROR_TREE_INVALID, "tree set: a tip is reached twice"); goto done; }
      seen[id] = 1;
      node[pos].tip = (uint32_t)id;
      node[pos].kid[0] = node[pos].kid[1] = 0;
      ++ntips;
      continue;
    }
    if (!rec->next->next || rec->next->next->next != rec)
    { fail(PLL_ERROR_TREE_INVALID, "tree set: an inner node without exactly three neighbours (not binary)"); goto done; }
    for (i = 0; i < 2u; ++i)
    {
      const pll_unode_t * r = i ? rec->next->next : rec->next;
      if (!r->back || r->back->back != r) { fail(PLL_ERROR_TREE_INVALID, "tree set: broken back links"); goto done; }
      if (n >= total) { fail(PLL_ERROR_TREE_INVALID, "tree set: more nodes than a binary tree of the set's tips has"); goto done; }
      node[n].rec = r->back;
      node[pos].kid[i] = n;
      stack[sp++] = n++;
    }
  }
  if (n != total || ntips != T - 1u) { fail(PLL_ERROR_TREE_INVALID, "tree set: not a binary tree of the set's tips"); goto done; }

  /* sizes and stack needs: children have larger positions than their parent */
  for (i = total; i-- > 0;)
  {
    ts_node_t * v = node + i;
    if (!v->rec->next) { v->size = 1; v->need = 1; continue; }
    {
      const ts_node_t * a = node + v->kid[0], * b = node + v->kid[1];
      v->size = a->size + b->size;
      v->need = a->need == b->need ? a->need + 1u : (a->need > b->need ? a->need : b->need);
    }
  }

  /* postorder, the needier child first */
  ntips = 0;
  sp = 0;
  stack[sp++] = 0;
  while (sp)
  {
    const uint32_t item = stack[--sp], pos = item >> 1;
    ts_node_t * v = node + pos;
    if (!v->rec->next)
    {
      order[ntips++] = v->tip;
      program[nsteps].kind = PLLHIP_TS_PUSH;
      program[nsteps++].arg = v->tip;
      if (++depth > deepest) deepest = depth;
    }
    else if (!(item & 1u))
    {
      const int swap = node[v->kid[1]].need > node[v->kid[0]].need;
      v->start = ntips;
      stack[sp++] = item | 1u;
      stack[sp++] = v->kid[swap ? 0 : 1] << 1;
      stack[sp++] = v->kid[swap ? 1 : 0] << 1;
    }
    else
    {
      program[nsteps].kind = PLLHIP_TS_COMBINE;
      program[nsteps++].arg = v->size;
      --depth;
      if (pos)
      {
        lo[nedges] = v->start;
        hi[nedges] = ntips;
        if (edge) edge[nedges] = (pll_unode_t *)v->rec;
        ++nedges;
      }
    }
  }
  if (deepest > 1u + floor_log2(T) || deepest > PLLHIP_TS_MAX_STACK)
  { fail(PLL_ERROR_TREE_INVALID, "tree set: the transfer program exceeds its stack bound"); goto done; }
  if (max_stack) *max_stack = deepest;
  rc = PLL_SUCCESS;

done:
  free(node);
  free(stack);
  free(seen);
  return rc;
}

void pllhip_ts_plan_splits(unsigned int T, const uint32_t * order, const uint32_t * lo, const uint32_t * hi,
                           uint32_t * words, uint64_t * hash)
{
  const unsigned int len = pllhip_ts_words(T), tail = T % 32u;
  uint64_t all = 0;
  unsigned int e, w, k;
  for (k = 0; k < T; ++k) all += pllhip_ts_key(k);
  for (e = 0; e + 3u < T; ++e)
  {
    uint32_t * v = words + (size_t)e * len;
    uint64_t h = all;
    for (w = 0; w < len; ++w) v[w] = 0xffffffffu;
    if (tail) v[len - 1u] = (1u << tail) - 1u;
    for (k = lo[e]; k < hi[e]; ++k)
    {
      v[order[k] / 32u] &= ~(1u << (order[k] % 32u));
      h -= pllhip_ts_key(order[k]);
    }
    if (hash) hash[e] = h;
  }
}

static int split_cmp(const void * a, const void * b, void * ctx)
{
  const uint32_t * words = ((const uint32_t **)ctx)[0];
  const unsigned int len = (unsigned int)(size_t)((void **)ctx)[1];
  const uint32_t * x = words + (size_t)*(const uint32_t *)a * len, * y = words + (size_t)*(const uint32_t *)b * len;
  unsigned int w;
  for (w = 0; w < len; ++w)
    if (x[w] != y[w]) return x[w] < y[w] ? -1 : 1;
  return 0;
}

void pllhip_ts_sort_splits(unsigned int T, unsigned int count, const uint32_t * words, uint32_t * perm)
{
  const void * ctx[2];
  unsigned int i;
  ctx[0] = words;
  ctx[1] = (void *)(size_t)pllhip_ts_words(T);
  for (i = 0; i < count; ++i) perm[i] = i;
  qsort_r(perm, count, sizeof(uint32_t), split_cmp, (void *)ctx);
}
