/*
 * pll_parsimony.c -- randomized stepwise-addition parsimony trees (pll_fastparsimony_init / _stepwise,
 * pll_parsimony_destroy) and the Fitch cost of a given tree (pllhip_parsimony_tree_score).  Host side only: taxon
 * order, tree surgery, the choice of the insertion edge and error mapping; the state sets and every count live on
 * the device (parsimony_dev.h, kernels_parsimony.hpp).  The contract is the engine's own (INTEGRATION.md,
 * "Parsimony"): the same algorithm as libpll-2, not the same tree for a given seed.
 *
 * The tree under construction is kept rooted at the tip order[0]: c0 is its one neighbour, every other node has a
 * parent and inner nodes two children.  An edge is named by its lower node v; the side of the edge away from
 * order[0] is the subtree of v, which gives the tie rule's split key directly.
 */
#include "pll.h"
#include "pllhip.h"
#include "parsimony_dev.h"

typedef struct
{
  pll_parsimony_t pub;            /* first member: a pll_parsimony_t * of the object is the object */
  pllhip_pars_dev_t * dev;
} pars_obj_t;

static void pars_error(int code, const char * msg)
{
  pll_errno = code;
  snprintf(pll_errmsg, 200, "%s", msg);
}

pll_parsimony_t * pll_fastparsimony_init(const pll_partition_t * partition)
{
  if (!partition)
  {
    pars_error(PLL_ERROR_PARAM_INVALID, "No partition given");
    return NULL;
  }
  pars_obj_t * o = (pars_obj_t *)calloc(1, sizeof(*o));
  if (!o)
  {
    pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate parsimony object");
    return NULL;
  }
  o->dev = pllhip_pars_dev_create(partition);
  if (!o->dev)
  {
    free(o);
    return NULL;
  }
  o->pub.tips = partition->tips;
  o->pub.inner_nodes = partition->tips > 2 ? partition->tips - 2 : 0;
  o->pub.sites = partition->sites;
  o->pub.states = partition->states;
  o->pub.attributes = partition->attributes;
  o->pub.alignment = PLL_ALIGNMENT_CPU;
  o->pub.informative_count = partition->sites;
  return &o->pub;
}

void pll_parsimony_destroy(pll_parsimony_t * pars)
{
  if (!pars) return;
  pars_obj_t * o = (pars_obj_t *)pars;
  pllhip_pars_dev_destroy(o->dev);
  free(o);
}

/* one walk on every partition, counts summed */
static int walk_all(pll_parsimony_t * const * list, unsigned int count, const int * ops, unsigned int ndown,
                    unsigned int npre, int cand, unsigned long long * edge_acc, unsigned long long * score_acc)
{
  unsigned int i;
  for (i = 0; i < count; ++i)
    if (!pllhip_pars_dev_launch(((pars_obj_t *)list[i])->dev, ops, ndown, npre, cand, score_acc != NULL))
      return PLL_FAILURE;
  if (edge_acc) memset(edge_acc, 0, sizeof(*edge_acc) * npre);
  if (score_acc) *score_acc = 0;
  for (i = 0; i < count; ++i)
    if (!pllhip_pars_dev_collect(((pars_obj_t *)list[i])->dev, edge_acc, score_acc)) return PLL_FAILURE;
  return PLL_SUCCESS;
}

static int check_list(pll_parsimony_t * const * list, unsigned int count)
{
  unsigned int i;
  if (!list || !count)
  {
    pars_error(PLL_ERROR_PARAM_INVALID, "No parsimony objects given");
    return PLL_FAILURE;
  }
  for (i = 0; i < count; ++i)
  {
    if (!list[i])
    {
      pars_error(PLL_ERROR_PARAM_INVALID, "NULL parsimony object in the list");
      return PLL_FAILURE;
    }
    if (list[i]->tips != list[0]->tips)
    {
      pars_error(PLL_ERROR_STEPWISE_TIPS, "Parsimony objects with different tip counts");
      return PLL_FAILURE;
    }
  }
  return PLL_SUCCESS;
}

/* ------------------------------------------------------------------ */
/* stepwise addition                                                  */
/* ------------------------------------------------------------------ */

typedef struct
{
  unsigned int tips, nodes;       /* node ids: tips 0..tips-1, inner tips.. */
  int * parent;                   /* [nodes]; the root tip r0 has -1 */
  int * child;                    /* [nodes][2]; -1 for tips */
  int r0, c0;
} ptree_t;

/* tips of the subtree of v, sorted, into out; returns the count.  The subtree of `excl` (< 0: none) is left out. */
static unsigned int subtree_tips(const ptree_t * t, int v, int excl, int * out, int * stack)
{
  unsigned int n = 0, sp = 0, i, j;
  stack[sp++] = v;
  while (sp)
  {
    const int x = stack[--sp];
    if (x == excl) continue;
    if (x < (int)t->tips) out[n++] = x;
    else { stack[sp++] = t->child[2 * x]; stack[sp++] = t->child[2 * x + 1]; }
  }
  for (i = 1; i < n; ++i)              /* insertion sort: the tie rule is rare and its keys short */
  {
    const int k = out[i];
    for (j = i; j > 0 && out[j - 1] > k; --j) out[j] = out[j - 1];
    out[j] = k;
  }
  return n;
}

/* preorder ops of every edge of the tree (parents before children); edge_node[e] = lower node of edge e */
static unsigned int preorder_ops(const ptree_t * t, int * ops, int * edge_node, int * stack)
{
  unsigned int n = 0, sp = 0;
  /* c0: the set above it is the tip r0 */
  ops[0] = t->c0; ops[1] = t->r0; ops[2] = 0; ops[3] = -1;
  edge_node[n++] = t->c0;
  stack[sp++] = t->c0;
  while (sp)
  {
    const int u = stack[--sp];
    int k;
    for (k = 0; k < 2; ++k)
    {
      const int v = t->child[2 * u + k], sib = t->child[2 * u + 1 - k];
      int * op = ops + 4 * n;
      op[0] = v;
      if (u == t->c0) { op[1] = t->r0; op[2] = 0; }
      else { op[1] = u; op[2] = PLL_TRUE; }              /* bit 0: the set above u, U[u] */
      if (v >= (int)t->tips) { op[2] |= 2; stack[sp++] = v; }   /* bit 1: store U[v] for v's children */
      op[3] = sib;
      edge_node[n++] = v;
    }
  }
  return n;
}

/* Stepwise insertion of the taxa `taxa[0 .. k-1]` (node ids) into t, new inner nodes from *next_inner on.  ops
   holds `ndown` down ops the first walk must do before scoring (the sets the tree's last change left stale).
   ins_v (may be NULL): the lower node of the edge each taxon went to, in insertion order. */
static int insert_taxa(pll_parsimony_t * const * list, unsigned int count, ptree_t * t, const int * taxa,
                       unsigned int k, int * ops, unsigned int ndown, int * next_inner, int * edge_node, int * stack,
                       int * key_a, int * key_b, unsigned long long * cost, int * ins_v)
{
  unsigned int i, j;
  for (j = 0; j < k; ++j)
  {
    const int taxon = taxa[j];
    const unsigned int npre = preorder_ops(t, ops + 3 * ndown, edge_node, stack);
    if (!walk_all(list, count, ops, ndown, npre, taxon, cost, NULL)) return PLL_FAILURE;
    unsigned int best = 0;
    for (i = 1; i < npre; ++i)
      if (cost[i] < cost[best]) best = i;
    for (i = 0; i < npre; ++i)
    {
      if (cost[i] != cost[best] || i == best) continue;
      /* tie: the smaller split key (tips below the edge, sorted; a prefix is smaller) */
      const unsigned int na = subtree_tips(t, edge_node[best], -1, key_a, stack);
      const unsigned int nb = subtree_tips(t, edge_node[i], -1, key_b, stack);
      unsigned int m = 0;
      while (m < na && m < nb && key_a[m] == key_b[m]) ++m;
      if ((m < na && m < nb) ? key_b[m] < key_a[m] : nb < na) best = i;
    }
    /* insert the taxon on edge (v, parent of v) through the new inner node x */
    const int v = edge_node[best], u = t->parent[v], x = (*next_inner)++;
    if (ins_v) ins_v[j] = v;
    t->parent[x] = u;
    t->child[2 * x] = v;
    t->child[2 * x + 1] = taxon;
    t->parent[v] = x;
    t->parent[taxon] = x;
    if (v == t->c0) t->c0 = x;
    else t->child[2 * u + (t->child[2 * u] == v ? 0 : 1)] = x;
    ndown = 0;
    for (int y = x; y != t->r0; y = t->parent[y])
    {
      ops[3 * ndown] = y;
      ops[3 * ndown + 1] = t->child[2 * y];
      ops[3 * ndown + 2] = t->child[2 * y + 1];
      ++ndown;
    }
  }
  return PLL_SUCCESS;
}

/* inner nodes of t in postorder (children first) into post; returns the count */
static unsigned int postorder_inner(const ptree_t * t, int * post, int * stack)
{
  unsigned int sp = 0, n = 0, i;
  stack[sp++] = t->c0;
  while (sp)                         /* reverse of a (node, right, left) preorder is a postorder */
  {
    const int y = stack[--sp];
    post[n++] = y;
    for (i = 0; i < 2; ++i)
      if (t->child[2 * y + i] >= (int)t->tips) stack[sp++] = t->child[2 * y + i];
  }
  for (i = 0; i < n / 2; ++i)
  {
    const int y = post[i];
    post[i] = post[n - 1 - i];
    post[n - 1 - i] = y;
  }
  return n;
}

/* down ops of every inner node plus the join with r0 into ops; returns their count */
static unsigned int full_down_ops(const ptree_t * t, int * ops, int * post, int * stack)
{
  const unsigned int n = postorder_inner(t, post, stack);
  unsigned int i;
  for (i = 0; i < n; ++i)
  {
    const int y = post[i];
    ops[3 * i] = y;
    ops[3 * i + 1] = t->child[2 * y];
    ops[3 * i + 2] = t->child[2 * y + 1];
  }
  ops[3 * n] = -1; ops[3 * n + 1] = t->c0; ops[3 * n + 2] = t->r0;
  return n + 1;
}

/* the cost of t: a whole postorder pass plus the join with r0 */
static int tree_cost(pll_parsimony_t * const * list, unsigned int count, const ptree_t * t, int * ops, int * post,
                     int * stack, unsigned long long * total)
{
  const unsigned int ndown = full_down_ops(t, ops, post, stack);
  if (!walk_all(list, count, ops, ndown, 0, -1, NULL, total)) return PLL_FAILURE;
  if (*total > 0xFFFFFFFFULL)
  {
    pars_error(PLL_ERROR_PARAM_INVALID, "The parsimony score does not fit an unsigned int");
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

static pll_utree_t * build_utree(const ptree_t * t, char * const * labels)
{
  const unsigned int tips = t->tips;
  pll_unode_t ** rec = (pll_unode_t **)calloc(t->nodes * 3, sizeof(*rec));   /* [node][slot]: slot = neighbour */
  int * nb = (int *)malloc(sizeof(int) * t->nodes * 3);
  unsigned int i, j, edge = tips;
  pll_utree_t * tree = NULL;
  int ok = rec && nb;
  for (i = 0; ok && i < t->nodes; ++i)
  {
    const unsigned int nrec = i < tips ? 1 : 3;
    nb[3 * i] = (int)i == t->r0 ? t->c0 : t->parent[i];      /* (the parent of c0 is r0) */
    if (i >= tips) { nb[3 * i + 1] = t->child[2 * i]; nb[3 * i + 2] = t->child[2 * i + 1]; }
    for (j = 0; ok && j < nrec; ++j)
    {
      pll_unode_t * r = (pll_unode_t *)calloc(1, sizeof(*r));
      ok = r != NULL;
      if (!ok) break;
      rec[3 * i + j] = r;
      r->clv_index = i;
      r->length = 0.1;
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
  /* back pointers and branch matrices: tip edges get the tip's index, inner edges tips.. */
  for (i = 0; ok && i < t->nodes; ++i)
  {
    const unsigned int nrec = i < tips ? 1 : 3;
    for (j = 0; j < nrec; ++j)
    {
      pll_unode_t * r = rec[3 * i + j];
      const int z = nb[3 * i + j];
      unsigned int k = 0;
      if (z >= (int)tips)
        while (nb[3 * z + k] != (int)i) ++k;
      r->back = rec[3 * z + k];
      if (r->back->back == r) continue;           /* the other side named the edge already */
      r->pmatrix_index = (i < tips) ? i : ((unsigned)z < tips ? (unsigned)z : edge++);
      r->back->pmatrix_index = r->pmatrix_index;
      r->back->back = r;
    }
  }
  if (ok) tree = pll_utree_wraptree(rec[3 * t->c0], tips);
  if (!tree)
  {
    for (i = 0; rec && i < t->nodes * 3; ++i)
      if (rec[i]) { free(rec[i]->label); free(rec[i]); }
    if (!ok) pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the tree");
  }
  free(rec);
  free(nb);
  return tree;
}

pll_utree_t * pll_fastparsimony_stepwise(pll_parsimony_t ** list, char * const * labels, unsigned int * score,
                                         unsigned int count, unsigned int seed)
{
  if (!check_list(list, count)) return NULL;
  const unsigned int tips = list[0]->tips;
  if (tips < 3)
  {
    pars_error(PLL_ERROR_STEPWISE_TIPS, "Stepwise addition needs at least 3 tips");
    return NULL;
  }
  const unsigned int nodes = 2 * tips - 2;
  ptree_t t;
  t.tips = tips;
  t.nodes = nodes;
  t.parent = (int *)malloc(sizeof(int) * nodes);
  t.child = (int *)malloc(sizeof(int) * 2 * nodes);
  unsigned int * order = (unsigned int *)malloc(sizeof(unsigned int) * tips);
  int * ops = (int *)malloc(sizeof(int) * (3 * nodes + 4 * nodes + 8));
  int * edge_node = (int *)malloc(sizeof(int) * nodes);
  int * stack = (int *)malloc(sizeof(int) * 2 * nodes);
  int * key_a = (int *)malloc(sizeof(int) * tips);
  int * key_b = (int *)malloc(sizeof(int) * tips);
  unsigned long long * cost = (unsigned long long *)malloc(sizeof(unsigned long long) * nodes);
  pll_random_state * rng = pll_random_create(seed);
  pll_utree_t * tree = NULL;
  unsigned int i;
  if (!t.parent || !t.child || !order || !ops || !edge_node || !stack || !key_a || !key_b || !cost || !rng)
  {
    pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate stepwise addition state");
    goto done;
  }
  for (i = 0; i < tips; ++i) order[i] = i;
  for (i = tips - 1; i >= 1; --i)
  {
    const unsigned int j = (unsigned int)pll_random_getint(rng, (int)i + 1);
    const unsigned int x = order[i];
    order[i] = order[j];
    order[j] = x;
  }
  for (i = 0; i < nodes; ++i) { t.parent[i] = -1; t.child[2 * i] = t.child[2 * i + 1] = -1; }
  t.r0 = (int)order[0];
  t.c0 = (int)tips;
  t.parent[t.c0] = t.r0;
  t.child[2 * t.c0] = (int)order[1];
  t.child[2 * t.c0 + 1] = (int)order[2];
  t.parent[order[1]] = t.parent[order[2]] = t.c0;
  /* the sets the next walk has to recompute first: the path from the last new node up to c0 */
  unsigned int ndown = 1;
  ops[0] = t.c0; ops[1] = (int)order[1]; ops[2] = (int)order[2];
  int next_inner = (int)tips + 1;
  if (!insert_taxa(list, count, &t, (const int *)order + 3, tips - 3, ops, ndown, &next_inner, edge_node, stack,
                   key_a, key_b, cost, NULL))
    goto done;
  {
    unsigned long long total = 0;
    if (!tree_cost(list, count, &t, ops, edge_node, stack, &total)) goto done;
    tree = build_utree(&t, labels);
    if (tree && score) *score = (unsigned int)total;
  }
done:
  free(t.parent); free(t.child); free(order); free(ops); free(edge_node); free(stack);
  free(key_a); free(key_b); free(cost);
  if (rng) pll_random_destroy(rng);
  return tree;
}

/* ------------------------------------------------------------------ */
/* the cost of a given tree                                           */
/* ------------------------------------------------------------------ */

typedef struct
{
  int * ops;
  unsigned int n, tips, next_inner, limit;
  int bad;
} score_walk_t;

static int score_down(score_walk_t * w, const pll_unode_t * r)
{
  if (!r || w->bad) { w->bad = 1; return 0; }
  if (!r->next)
  {
    if (r->clv_index >= w->tips) w->bad = 1;
    return (int)r->clv_index;
  }
  if (!r->next->next || r->next->next->next != r || w->next_inner >= w->limit) { w->bad = 1; return 0; }
  const int a = score_down(w, r->next->back);
  const int b = score_down(w, r->next->next->back);
  if (w->bad) return 0;
  const int id = (int)w->next_inner++;
  w->ops[3 * w->n] = id; w->ops[3 * w->n + 1] = a; w->ops[3 * w->n + 2] = b;
  w->n++;
  return id;
}

int pllhip_parsimony_tree_score(pll_parsimony_t * const * list, unsigned int count, const pll_utree_t * tree,
                                unsigned int * score)
{
  if (!check_list(list, count)) return PLL_FAILURE;
  if (!tree || !tree->vroot || !score)
  {
    pars_error(PLL_ERROR_PARAM_INVALID, "No tree or no score target given");
    return PLL_FAILURE;
  }
  const unsigned int tips = list[0]->tips;
  if (tips < 3)
  {
    pars_error(PLL_ERROR_STEPWISE_TIPS, "A tree of fewer than 3 tips has no inner node");
    return PLL_FAILURE;
  }
  const pll_unode_t * root = tree->vroot->next ? tree->vroot : tree->vroot->back;
  score_walk_t w;
  w.tips = tips;
  w.next_inner = tips;
  w.limit = 2 * tips - 2;
  w.n = 0;
  w.bad = !root || !root->next;
  w.ops = (int *)malloc(sizeof(int) * 3 * (2 * tips));
  if (!w.ops)
  {
    pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the schedule");
    return PLL_FAILURE;
  }
  const int a = w.bad ? 0 : score_down(&w, root);
  const int b = w.bad ? 0 : score_down(&w, root->back);
  if (w.bad)
  {
    free(w.ops);
    pars_error(PLL_ERROR_TREE_INVALID, "The tree is not binary or names a tip the partitions do not have");
    return PLL_FAILURE;
  }
  w.ops[3 * w.n] = -1; w.ops[3 * w.n + 1] = a; w.ops[3 * w.n + 2] = b;
  unsigned long long total = 0;
  const int rc = walk_all(list, count, w.ops, w.n + 1, 0, -1, NULL, &total);
  free(w.ops);
  if (!rc) return PLL_FAILURE;
  if (total > 0xFFFFFFFFULL)
  {
    pars_error(PLL_ERROR_PARAM_INVALID, "The parsimony score does not fit an unsigned int");
    return PLL_FAILURE;
  }
  *score = (unsigned int)total;
  return PLL_SUCCESS;
}

/* ------------------------------------------------------------------ */
/* a caller's tree in ptree_t form                                    */
/* ------------------------------------------------------------------ */

/* The caller's records as a ptree_t rooted at r0: node ids are given per clv index by the caller (clv_id, a sorted
   (clv, id) table), up[id] is the record of node id that points to its parent (r0: to c0). */
typedef struct
{
  ptree_t t;
  pll_unode_t ** up;
} rtree_t;

typedef struct { unsigned int clv; int id; } clv_id_t;

static int cmp_clv_id(const void * a, const void * b)
{
  const unsigned int x = ((const clv_id_t *)a)->clv, y = ((const clv_id_t *)b)->clv;
  return x < y ? -1 : x > y;
}

static int id_of(const clv_id_t * tab, unsigned int n, unsigned int clv)
{
  clv_id_t key;
  key.clv = clv;
  const clv_id_t * f = (const clv_id_t *)bsearch(&key, tab, n, sizeof(*tab), cmp_clv_id);
  return f ? f->id : -1;
}

static void rtree_free(rtree_t * r)
{
  free(r->t.parent);
  free(r->t.child);
  free(r->up);
  memset(r, 0, sizeof(*r));
}

/* Walks the caller's tree from the record of tip r0 (a record of tree->nodes).  ids: `tab` (n entries, sorted by
   clv).  `nodes` is the capacity of the id space, `tips` the first inner id.  PLL_ERROR_TREE_INVALID: not binary or
   not connected as tree->nodes says. */
static int rtree_build(rtree_t * r, const pll_utree_t * tree, pll_unode_t * r0rec, const clv_id_t * tab,
                       unsigned int n, unsigned int tips, unsigned int nodes)
{
  unsigned int i, sp = 0, seen = 0;
  memset(r, 0, sizeof(*r));
  r->t.tips = tips;
  r->t.nodes = nodes;
  r->t.parent = (int *)malloc(sizeof(int) * nodes);
  r->t.child = (int *)malloc(sizeof(int) * 2 * nodes);
  r->up = (pll_unode_t **)calloc(nodes, sizeof(*r->up));
  pll_unode_t ** stack = (pll_unode_t **)malloc(sizeof(*stack) * (nodes + 1));
  if (!r->t.parent || !r->t.child || !r->up || !stack)
  {
    free(stack);
    rtree_free(r);
    pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the tree map");
    return PLL_FAILURE;
  }
  for (i = 0; i < nodes; ++i) { r->t.parent[i] = -1; r->t.child[2 * i] = r->t.child[2 * i + 1] = -1; }
  r->t.r0 = id_of(tab, n, r0rec->clv_index);
  r->up[r->t.r0] = r0rec;
  int bad = !r0rec->back;
  if (!bad) stack[sp++] = r0rec->back;
  ++seen;
  while (sp && !bad)
  {
    pll_unode_t * x = stack[--sp];
    const int id = id_of(tab, n, x->clv_index);
    const int pid = id_of(tab, n, x->back->clv_index);
    if (id < 0 || r->up[id] || ++seen > tree->tip_count + tree->inner_count) { bad = 1; break; }
    r->up[id] = x;
    r->t.parent[id] = pid;
    if (pid == r->t.r0) r->t.c0 = id;
    if (!x->next) { if (id >= (int)tips) bad = 1; continue; }
    if (id < (int)tips || !x->next->next || x->next->next->next != x) { bad = 1; break; }
    for (i = 0; i < 2; ++i)
    {
      pll_unode_t * c = i ? x->next->next->back : x->next->back;
      if (!c || c->back == NULL) { bad = 1; break; }
      r->t.child[2 * id + i] = id_of(tab, n, c->clv_index);
      stack[sp++] = c;
    }
  }
  free(stack);
  if (bad || seen != tree->tip_count + tree->inner_count || r->t.parent[r->t.r0] != -1)
  {
    rtree_free(r);
    pars_error(PLL_ERROR_TREE_INVALID, "The tree is not a binary unrooted tree");
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

/* common argument checks: the records of tree->nodes, tips first (next == NULL) and inner rings of three */
static int check_tree_shape(const pll_utree_t * tree)
{
  unsigned int i;
  if (!tree->nodes || !tree->vroot)
  {
    pars_error(PLL_ERROR_PARAM_INVALID, "The tree has no nodes");
    return PLL_FAILURE;
  }
  for (i = 0; i < tree->tip_count + tree->inner_count; ++i)
  {
    const pll_unode_t * x = tree->nodes[i];
    if (!x || (i < tree->tip_count) != (x->next == NULL) ||
        (x->next && (!x->next->next || x->next->next->next != x)))
    {
      pars_error(PLL_ERROR_TREE_INVALID, "The tree is not binary");
      return PLL_FAILURE;
    }
  }
  if (tree->inner_count != tree->tip_count - 2)
  {
    pars_error(PLL_ERROR_TREE_INVALID, "The tree is not binary");
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

/* the row of every tip record of the tree (tip_msa_idmap[clv], or clv); with `want` the rows must be a
   permutation of 0 .. map_size-1 restricted to the tips, map NULL or a permutation of 0 .. map_size-1 */
static int check_map(const unsigned int * map, unsigned int map_size)
{
  unsigned int i;
  if (!map) return PLL_SUCCESS;
  unsigned char * seen = (unsigned char *)calloc(map_size, 1);
  if (!seen)
  {
    pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the map check");
    return PLL_FAILURE;
  }
  int ok = 1;
  for (i = 0; i < map_size && ok; ++i)
  {
    ok = map[i] < map_size && !seen[map[i]];
    if (ok) seen[map[i]] = 1;
  }
  free(seen);
  if (!ok) pars_error(PLL_ERROR_PARAM_INVALID, "tip_msa_idmap is not a permutation of the partitions' tips");
  return ok ? PLL_SUCCESS : PLL_FAILURE;
}

/* ------------------------------------------------------------------ */
/* extension of a given tree                                          */
/* ------------------------------------------------------------------ */

int pll_fastparsimony_stepwise_extend(pll_utree_t * tree, pll_parsimony_t ** list, unsigned int count,
                                      char * const * labels, unsigned int * tip_msa_idmap, unsigned int seed,
                                      unsigned int * score)
{
  if (!tree)
  {
    pars_error(PLL_ERROR_PARAM_INVALID, "No tree given");
    return PLL_FAILURE;
  }
  if (!check_list(list, count)) return PLL_FAILURE;
  const unsigned int N = list[0]->tips, T = tree->tip_count;
  if (T < 3 || T > N)
  {
    pars_error(PLL_ERROR_STEPWISE_TIPS, "The tree has fewer than 3 tips or more tips than the partitions");
    return PLL_FAILURE;
  }
  if (!check_map(tip_msa_idmap, N) || !check_tree_shape(tree)) return PLL_FAILURE;
  const unsigned int k = N - T, nodes = 2 * N - 2, nold = 2 * T - 2;
  unsigned int i, j;
  int rc = PLL_FAILURE;
  rtree_t r;
  memset(&r, 0, sizeof(r));
  clv_id_t * tab = (clv_id_t *)malloc(sizeof(*tab) * nold);
  int * taxa = (int *)malloc(sizeof(int) * (k + 1));
  int * ord = (int *)malloc(sizeof(int) * (k + 1));
  int * ins_v = (int *)malloc(sizeof(int) * (k + 1));
  int * ops = (int *)malloc(sizeof(int) * (3 * nodes + 4 * nodes + 8));
  int * edge_node = (int *)malloc(sizeof(int) * nodes);
  int * stack = (int *)malloc(sizeof(int) * 2 * nodes);
  int * key_a = (int *)malloc(sizeof(int) * N);
  int * key_b = (int *)malloc(sizeof(int) * N);
  unsigned long long * cost = (unsigned long long *)malloc(sizeof(unsigned long long) * nodes);
  pll_unode_t ** fresh = (pll_unode_t **)calloc(4 * (size_t)k + 1, sizeof(*fresh));   /* per taxon: tip + ring */
  pll_unode_t ** newnodes = NULL;
  pll_random_state * rng = pll_random_create(seed);
  if (!tab || !taxa || !ord || !ins_v || !ops || !edge_node || !stack || !key_a || !key_b || !cost || !fresh || !rng)
  {
    pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate extension state");
    goto done;
  }
  /* ids: tip clv c -> its row, inner clv c (T .. 2T-3) -> N + c - T */
  pll_unode_t * r0rec = NULL;
  for (i = 0; i < nold; ++i)
  {
    const pll_unode_t * x = tree->nodes[i];
    const unsigned int c = x->clv_index;
    if (i < T ? c >= T : (c < T || c >= nold))
    {
      pars_error(PLL_ERROR_PARAM_INVALID, "The tree's clv indices are not 0 .. T-1 (tips), T .. 2T-3 (inner)");
      goto done;
    }
    tab[i].clv = c;
    tab[i].id = i < T ? (int)(tip_msa_idmap ? tip_msa_idmap[c] : c) : (int)(N + c - T);
  }
  qsort(tab, nold, sizeof(*tab), cmp_clv_id);
  for (i = 1; i < nold; ++i)
    if (tab[i].clv == tab[i - 1].clv)
    {
      pars_error(PLL_ERROR_PARAM_INVALID, "The tree names a clv index twice");
      goto done;
    }
  for (i = 0; i < T; ++i)           /* r0: the tip of the smallest row */
  {
    const int row = id_of(tab, nold, tree->nodes[i]->clv_index);
    if (!r0rec || row < id_of(tab, nold, r0rec->clv_index)) r0rec = tree->nodes[i];
  }
  if (!rtree_build(&r, tree, r0rec, tab, nold, N, nodes)) goto done;
  /* insertion order: the stepwise shuffle over the new taxa */
  for (j = 0; j < k; ++j) ord[j] = (int)j;
  for (j = k ? k - 1 : 0; j >= 1; --j)
  {
    const unsigned int q = (unsigned int)pll_random_getint(rng, (int)j + 1);
    const int x = ord[j];
    ord[j] = ord[q];
    ord[q] = x;
  }
  for (j = 0; j < k; ++j) taxa[j] = (int)(tip_msa_idmap ? tip_msa_idmap[T + ord[j]] : T + ord[j]);
  /* every record and label first, so that a failure leaves the tree as it was */
  for (j = 0; j < 4 * k; ++j)
    if (!(fresh[j] = (pll_unode_t *)calloc(1, sizeof(pll_unode_t))))
    {
      pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the new nodes");
      goto done;
    }
  newnodes = (pll_unode_t **)calloc(nodes, sizeof(*newnodes));
  if (!newnodes)
  {
    pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate the node table");
    goto done;
  }
  /* the device work: a full postorder, then the insertions, then the final cost */
  {
    int next_inner = (int)(N + T - 2);
    const unsigned int nd = full_down_ops(&r.t, ops, edge_node, stack) - 1;   /* without the join */
    unsigned long long total = 0;
    if (!insert_taxa(list, count, &r.t, taxa, k, ops, nd, &next_inner, edge_node, stack, key_a, key_b, cost, ins_v) ||
        !tree_cost(list, count, &r.t, ops, edge_node, stack, &total))
      goto done;
    if (!k)
    {
      if (score) *score = (unsigned int)total;
      rc = PLL_SUCCESS;
      goto done;
    }
    /* labels of the new tips: taxa[j] is the row of clv index T + ord[j] */
    for (j = 0; j < k; ++j)
    {
      pll_unode_t * tip = fresh[4 * j];
      tip->clv_index = T + (unsigned int)ord[j];
      if (labels && labels[ord[j]] && !(tip->label = strdup(labels[ord[j]])))
      {
        pars_error(PLL_ERROR_MEM_ALLOC, "Cannot copy a label");
        goto done;
      }
    }
    /* the surgery, in insertion order: taxon j on the edge above ins_v[j] through the ring fresh[4j+1 ..] */
    for (j = 0; j < k; ++j)
    {
      pll_unode_t * tip = fresh[4 * j], * x0 = fresh[4 * j + 1], * x1 = fresh[4 * j + 2], * x2 = fresh[4 * j + 3];
      pll_unode_t * rv = r.up[ins_v[j]], * ru = rv->back;
      const int xid = (int)(N + T - 2 + j);
      x0->next = x1; x1->next = x2; x2->next = x0;
      x0->back = ru; ru->back = x0;          /* x0: up */
      x1->back = rv; rv->back = x1;          /* x1: down to v */
      x2->back = tip; tip->back = x2;        /* x2: the new tip */
      x0->length = ru->length = x1->length = rv->length = x2->length = tip->length = 0.1;
      x0->clv_index = x1->clv_index = x2->clv_index = (unsigned int)xid;
      r.up[xid] = x0;
      r.up[taxa[j]] = tip;
    }
    /* clv indices and the node table: tips by clv, inner clv = id */
    for (i = 0; i < T; ++i) newnodes[tree->nodes[i]->clv_index] = tree->nodes[i];
    for (j = 0; j < k; ++j) newnodes[fresh[4 * j]->clv_index] = fresh[4 * j];
    for (i = T; i < nold; ++i)
    {
      pll_unode_t * x = tree->nodes[i];
      const unsigned int c = x->clv_index + k;
      x->clv_index = x->next->clv_index = x->next->next->clv_index = c;
      newnodes[c] = x;
    }
    for (j = 0; j < k; ++j) newnodes[N + T - 2 + j] = fresh[4 * j + 1];
    /* node, scaler and branch matrix indices as build_utree gives them */
    unsigned int edge = N;
    for (i = 0; i < N; ++i)
    {
      pll_unode_t * x = newnodes[i];
      x->node_index = i;
      x->scaler_index = PLL_SCALE_BUFFER_NONE;
      x->pmatrix_index = x->back->pmatrix_index = i;
    }
    for (i = N; i < nodes; ++i)
    {
      pll_unode_t * x = newnodes[i];
      for (j = 0; j < 3; ++j, x = x->next)
      {
        x->node_index = N + 3 * (i - N) + j;
        x->scaler_index = (int)(i - N);
        if (x->back->clv_index > i) x->pmatrix_index = x->back->pmatrix_index = edge++;
      }
    }
    pll_unode_t ** old = tree->nodes;
    tree->nodes = newnodes;
    newnodes = NULL;
    free(old);
    tree->tip_count = N;
    tree->inner_count = N - 2;
    tree->edge_count = 2 * N - 3;
    for (j = 0; j < 4 * k; ++j) fresh[j] = NULL;       /* owned by the tree now */
    if (score) *score = (unsigned int)total;
    rc = PLL_SUCCESS;
  }
done:
  if (fresh)
    for (j = 0; j < 4 * k; ++j)
      if (fresh[j]) { free(fresh[j]->label); free(fresh[j]); }
  free(fresh); free(newnodes); free(tab); free(taxa); free(ord); free(ins_v); free(ops); free(edge_node); free(stack);
  free(key_a); free(key_b); free(cost);
  rtree_free(&r);
  if (rng) pll_random_destroy(rng);
  return rc;
}

/* ------------------------------------------------------------------ */
/* SPR rounds                                                         */
/* ------------------------------------------------------------------ */

/* State of one round.  The tree is rooted at r0 (row 0); an edge is named by its lower node.  Pruning v (parent p,
   sibling s, grandparent pp) gives T': p removed, s hung below pp.  Per prune the schedule (kernels_parsimony.hpp,
   k_pars_spr) holds the new down sets of the path pp .. c0 (scratch slots 0 ..), the up sets U' of the nodes of T'
   off that path (scratch slots from tips - 2 on; path nodes keep their up sets U) and one counted edge op per
   candidate edge, the first one for s (the reference: v back where it was). */
typedef struct
{
  rtree_t r;
  unsigned int N, nodes;
  const int * gid;                /* [nodes]: constraint group of inner nodes (clv_valid), NULL: unconstrained */
  int * tin, * tout;              /* preorder interval of every node (ancestor tests) */
  int * pidx, * slot, * mark;     /* per prune: path index, U' slot, counted; -1 / 0 when unset */
  int * touched;                  /* nodes whose pidx / slot / mark this prune set */
  unsigned int ntouched;
  int * pre;                      /* edge ops of the member being built */
  int * edge_x;                   /* the lower node of each of its counted ops */
  int g;                          /* constraint group of p */
  unsigned int npre, ncount, nslot;
  int need_path;                  /* deepest path index the member reads */
  int v, p, s, pp, w;             /* the prune */
} spr_t;

#define PLLHIP_PARS_PRE_INTS 5
#define SRC(src, i) ((int)(((unsigned int)(i) << 2) | (unsigned int)(src)))

static void spr_touch(spr_t * q, int x)
{
  if (q->pidx[x] < 0 && q->slot[x] < 0 && !q->mark[x]) q->touched[q->ntouched++] = x;
}

static void spr_intervals(spr_t * q, int * stack)
{
  const ptree_t * t = &q->r.t;
  unsigned int sp = 0;
  int clock = 0;
  stack[sp++] = t->c0;
  while (sp)
  {
    const int y = stack[--sp];
    if (y < 0) { q->tout[-y - 1] = clock; continue; }
    q->tin[y] = clock++;
    stack[sp++] = -y - 1;
    if (y >= (int)t->tips) { stack[sp++] = t->child[2 * y + 1]; stack[sp++] = t->child[2 * y]; }
  }
  q->tin[t->r0] = -1;
  q->tout[t->r0] = clock;
}

static int in_sub(const spr_t * q, int x, int v) { return q->tin[v] <= q->tin[x] && q->tin[x] < q->tout[v]; }

/* parent and sibling in T' */
static int par_t(const spr_t * q, int x) { return x == q->s ? q->pp : q->r.t.parent[x]; }
static int sib_t(const spr_t * q, int x)
{
  const ptree_t * t = &q->r.t;
  if (x == q->s) return q->w;
  if (x == q->w) return q->s;
  const int y = t->parent[x];
  return t->child[2 * y] == x ? t->child[2 * y + 1] : t->child[2 * y];
}

static int dsrc(spr_t * q, int x)
{
  if (q->pidx[x] >= 0)
  {
    if (q->pidx[x] > q->need_path) q->need_path = q->pidx[x];
    return SRC(PLLHIP_PARS_SRC_X, q->pidx[x]);
  }
  return SRC(PLLHIP_PARS_SRC_D, x);
}

/* whether the set above x in T' is at hand without an op of this member */
static int up_ready(const spr_t * q, int x) { return par_t(q, x) == q->r.t.r0 || q->pidx[x] >= 0 || q->slot[x] >= 0; }

static int upsrc(const spr_t * q, int x)
{
  if (par_t(q, x) == q->r.t.r0) return SRC(PLLHIP_PARS_SRC_D, q->r.t.r0);
  if (q->pidx[x] >= 0) return SRC(PLLHIP_PARS_SRC_U, x);
  return SRC(PLLHIP_PARS_SRC_X, q->slot[x]);
}

/* one edge op: the set above x in T' (stored for x's children if x is an inner node off the path), counted or not */
static void spr_emit(spr_t * q, int x, int count)
{
  int * op = q->pre + PLLHIP_PARS_PRE_INTS * q->npre++;
  op[0] = dsrc(q, x);
  if (up_ready(q, x))
  {
    op[1] = upsrc(q, x);
    op[2] = -1;
    op[3] = -1;
  }
  else
  {
    op[1] = upsrc(q, par_t(q, x));
    op[2] = dsrc(q, sib_t(q, x));
    op[3] = -1;
    if (x >= (int)q->N)
    {
      spr_touch(q, x);
      q->slot[x] = (int)(q->N - 2 + q->nslot++);
      op[3] = q->slot[x];
    }
  }
  op[4] = count;
  if (count)
  {
    spr_touch(q, x);
    q->mark[x] = 1;
    q->edge_x[q->ncount++] = x;
  }
}

/* whether x (a node of T', not s) is an allowed regraft edge for a prune from group g */
static int spr_allowed(const spr_t * q, int x, int g)
{
  if (!q->gid) return 1;
  if (x >= (int)q->N && q->gid[x] == g) return 1;
  const int y = par_t(q, x);
  return y != q->r.t.r0 && q->gid[y] == g;
}

/* a counted op for x, after the ops of the up sets it needs (counted too where they are allowed edges, so that
   no node has two ops) */
static void spr_edge(spr_t * q, int x, int * chain)
{
  unsigned int n = 0;
  int y;
  if (q->mark[x]) return;
  for (y = par_t(q, x); y != q->r.t.r0 && !up_ready(q, y); y = par_t(q, y)) chain[n++] = y;
  while (n)
  {
    y = chain[--n];
    spr_emit(q, y, spr_allowed(q, y, q->g));
  }
  spr_emit(q, x, 1);
}

/* Builds the member of prune v into ops (down ops then edge ops); returns the number of ints, 0 if no edge is
   allowed.  edge_x: the lower node of every counted op. */
static unsigned int spr_member(spr_t * q, int v, int * ops, int * edge_x, unsigned int * ndown, unsigned int * npre,
                               unsigned int * ncount, int * chain)
{
  const ptree_t * t = &q->r.t;
  unsigned int i, L = 0;
  int y;
  q->v = v;
  q->p = t->parent[v];
  q->s = t->child[2 * q->p] == v ? t->child[2 * q->p + 1] : t->child[2 * q->p];
  q->pp = t->parent[q->p];
  q->w = q->pp == t->r0 ? -1 : (t->child[2 * q->pp] == q->p ? t->child[2 * q->pp + 1] : t->child[2 * q->pp]);
  q->npre = q->ncount = q->nslot = 0;
  q->need_path = -1;
  q->ntouched = 0;
  for (y = q->pp; y != t->r0; y = t->parent[y])
  {
    spr_touch(q, y);
    q->pidx[y] = (int)L++;
  }
  const int g = q->gid ? q->gid[q->p] : 0;
  q->g = g;
  q->edge_x = edge_x;
  spr_emit(q, q->s, 1);                           /* the reference; its up set is at hand or one op away */
  if (!q->gid)
  {
    for (i = 0; i < q->nodes; ++i)
      if ((int)i != t->r0 && (int)i != q->p && !q->mark[i] && !in_sub(q, (int)i, v)) spr_edge(q, (int)i, chain);
  }
  else
    for (i = q->N; i < q->nodes; ++i)
    {
      if (q->gid[i] != g || (int)i == q->p || in_sub(q, (int)i, v)) continue;
      /* the edge above i and the edges below it in T' (below pp: s and w) */
      const int c[3] = { (int)i, (int)i == q->pp ? q->s : t->child[2 * i], (int)i == q->pp ? q->w : t->child[2 * i + 1] };
      unsigned int k;
      for (k = 0; k < 3; ++k)
      {
        const int x = c[k];
        if (x == q->s || q->mark[x] || !spr_allowed(q, x, g)) continue;
        spr_edge(q, x, chain);
      }
    }
  unsigned int n = 0;
  if (q->ncount > 1)
  {
    /* the path's down sets, pp first: children in T' */
    for (y = q->pp, L = 0; y != t->r0 && (int)L <= q->need_path; y = t->parent[y], ++L)
    {
      const int a = t->child[2 * y], b = t->child[2 * y + 1];
      ops[3 * L] = (int)L;
      ops[3 * L + 1] = dsrc(q, a == q->p ? q->s : a);
      ops[3 * L + 2] = dsrc(q, b == q->p ? q->s : b);
    }
    n = 3 * L;
    memcpy(ops + n, q->pre, sizeof(int) * PLLHIP_PARS_PRE_INTS * q->npre);
    n += PLLHIP_PARS_PRE_INTS * q->npre;
    *ndown = L;
    *npre = q->npre;
    *ncount = q->ncount;
  }
  for (i = 0; i < q->ntouched; ++i)
  {
    const int x = q->touched[i];
    q->pidx[x] = q->slot[x] = -1;
    q->mark[x] = 0;
  }
  return n;
}

/* the whole tree's down and up sets on the device, and its cost */
static int spr_refresh(pll_parsimony_t * const * list, unsigned int count, spr_t * q, int * ops, int * post,
                       int * stack, unsigned long long * cost, unsigned long long * total)
{
  const ptree_t * t = &q->r.t;
  const unsigned int ndown = full_down_ops(t, ops, post, stack);
  const unsigned int npre = preorder_ops(t, ops + 3 * ndown, post, stack);
  if (!walk_all(list, count, ops, ndown, npre, t->r0, cost, total)) return PLL_FAILURE;
  spr_intervals(q, stack);
  return PLL_SUCCESS;
}

static int cmp_uint(const void * a, const void * b)
{
  const unsigned int x = *(const unsigned int *)a, y = *(const unsigned int *)b;
  return x < y ? -1 : x > y;
}

int pll_fastparsimony_stepwise_spr_round(pll_utree_t * tree, pll_parsimony_t ** list, unsigned int count,
                                         const unsigned int * tip_msa_idmap, unsigned int seed,
                                         const int * clv_valid, unsigned int * cost)
{
  if (!tree || !cost)
  {
    pars_error(PLL_ERROR_PARAM_INVALID, "No tree or no cost target given");
    return PLL_FAILURE;
  }
  if (!check_list(list, count)) return PLL_FAILURE;
  const unsigned int N = list[0]->tips;
  if (N < 3 || tree->tip_count != N)
  {
    pars_error(PLL_ERROR_STEPWISE_TIPS, "The tree and the partitions differ in tips, or there are fewer than 3");
    return PLL_FAILURE;
  }
  if (!check_map(tip_msa_idmap, N) || !check_tree_shape(tree)) return PLL_FAILURE;
  const unsigned int nodes = 2 * N - 2;
  unsigned int i, j;
  int rc = PLL_FAILURE;
  spr_t q;
  memset(&q, 0, sizeof(q));
  q.N = N;
  q.nodes = nodes;
  clv_id_t * tab = (clv_id_t *)malloc(sizeof(*tab) * nodes);
  unsigned int * inner_clv = (unsigned int *)malloc(sizeof(unsigned int) * nodes);
  int * gid = clv_valid ? (int *)malloc(sizeof(int) * nodes) : NULL;
  int * order = (int *)malloc(sizeof(int) * nodes);
  int * wops = (int *)malloc(sizeof(int) * (3 * nodes + 4 * nodes + 8));
  int * post = (int *)malloc(sizeof(int) * nodes);
  int * stack = (int *)malloc(sizeof(int) * 2 * nodes);
  int * chain = (int *)malloc(sizeof(int) * nodes);
  int * key_a = (int *)malloc(sizeof(int) * N);
  int * key_b = (int *)malloc(sizeof(int) * N);
  unsigned long long * wcost = (unsigned long long *)malloc(sizeof(unsigned long long) * nodes);
  q.tin = (int *)malloc(sizeof(int) * nodes);
  q.tout = (int *)malloc(sizeof(int) * nodes);
  q.pidx = (int *)malloc(sizeof(int) * nodes);
  q.slot = (int *)malloc(sizeof(int) * nodes);
  q.mark = (int *)calloc(nodes, sizeof(int));
  q.touched = (int *)malloc(sizeof(int) * nodes);
  q.pre = (int *)malloc(sizeof(int) * PLLHIP_PARS_PRE_INTS * nodes);
  pll_random_state * rng = pll_random_create(seed);
  /* the batch: PLLHIP_PARS_SPR_BATCH forces it, otherwise what fills the chip */
  unsigned int B = 0;
  int * mops = NULL, * members = NULL, * medge = NULL, * mv = NULL;
  unsigned long long * acc = NULL;
  if (!tab || !inner_clv || (clv_valid && !gid) || !order || !wops || !post || !stack || !chain || !key_a ||
      !key_b || !wcost || !q.tin || !q.tout || !q.pidx || !q.slot || !q.mark || !q.touched || !q.pre || !rng)
  {
    pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate SPR round state");
    goto done;
  }
  /* node ids: tips their rows, inner nodes N + rank of their clv index */
  {
    unsigned int ni = 0;
    pll_unode_t * r0rec = NULL;
    for (i = N; i < nodes; ++i) inner_clv[ni++] = tree->nodes[i]->clv_index;
    qsort(inner_clv, ni, sizeof(unsigned int), cmp_uint);
    for (i = 0; i < nodes; ++i)
    {
      const unsigned int c = tree->nodes[i]->clv_index;
      tab[i].clv = c;
      if (i < N)
      {
        if (c >= N)
        {
          pars_error(PLL_ERROR_PARAM_INVALID, "A tip's clv index is not below the tip count");
          goto done;
        }
        tab[i].id = (int)(tip_msa_idmap ? tip_msa_idmap[c] : c);
        if (tab[i].id == 0) r0rec = tree->nodes[i];
      }
      else
        tab[i].id = (int)(N + (unsigned int)((const unsigned int *)bsearch(&c, inner_clv, ni, sizeof(unsigned int),
                                                                             cmp_uint) - inner_clv));
    }
    qsort(tab, nodes, sizeof(*tab), cmp_clv_id);
    for (i = 1; i < nodes; ++i)
      if (tab[i].clv == tab[i - 1].clv)
      {
        pars_error(PLL_ERROR_PARAM_INVALID, "The tree names a clv index twice");
        goto done;
      }
    if (!rtree_build(&q.r, tree, r0rec, tab, nodes, N, nodes)) goto done;
    if (gid)
      for (i = 0; i < nodes; ++i) gid[i] = i < N ? -1 : clv_valid[q.r.up[i]->clv_index];
    q.gid = gid;
  }
  for (i = 0; i < nodes; ++i) { q.pidx[i] = q.slot[i] = -1; }
  /* the batch */
  {
    const char * env = getenv("PLLHIP_PARS_SPR_BATCH");
    unsigned int want = env && atoi(env) > 0 ? (unsigned int)atoi(env) : 0;
    if (!want)
    {
      want = ~0u;
      for (i = 0; i < count; ++i)
      {
        const unsigned int h = pllhip_pars_dev_spr_hint(((pars_obj_t *)list[i])->dev);
        if (h < want) want = h;
      }
    }
    B = want;
    for (i = 0; i < count; ++i)
    {
      const unsigned int b = pllhip_pars_dev_spr_reserve(((pars_obj_t *)list[i])->dev, B);
      if (!b) goto done;
      if (b < B) B = b;
    }
  }
  mops = (int *)malloc(sizeof(int) * (size_t)B * 8 * nodes);
  members = (int *)malloc(sizeof(int) * 5 * (size_t)B);
  medge = (int *)malloc(sizeof(int) * (size_t)B * nodes);
  mv = (int *)malloc(sizeof(int) * 2 * (size_t)B);
  acc = (unsigned long long *)malloc(sizeof(unsigned long long) * (size_t)B * nodes);
  if (!mops || !members || !medge || !mv || !acc)
  {
    pars_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate SPR batch state");
    goto done;
  }
  /* visit order: the stepwise shuffle of all node ids */
  for (i = 0; i < nodes; ++i) order[i] = (int)i;
  for (i = nodes - 1; i >= 1; --i)
  {
    const unsigned int k = (unsigned int)pll_random_getint(rng, (int)i + 1);
    const int x = order[i];
    order[i] = order[k];
    order[k] = x;
  }
  unsigned long long total = 0;
  if (!spr_refresh(list, count, &q, wops, post, stack, wcost, &total)) goto done;
  for (i = 0; i < nodes;)
  {
    /* up to B prunes against the current tree */
    unsigned int nm = 0, nops = 0, nout = 0, next = i;
    while (next < nodes && nm < B)
    {
      const int v = order[next++];
      unsigned int nd = 0, np = 0, nc = 0;
      if (v == q.r.t.r0 || v == q.r.t.c0) continue;
      const unsigned int n = spr_member(&q, v, mops + nops, medge + nout, &nd, &np, &nc, chain);
      if (!n) continue;
      int * m = members + 5 * nm;
      m[0] = (int)nops; m[1] = (int)nd; m[2] = (int)np; m[3] = v; m[4] = (int)nout;
      mv[2 * nm] = (int)(next - 1);
      mv[2 * nm + 1] = (int)nc;
      nops += n;
      nout += nc;
      ++nm;
    }
    if (!nm) break;
    for (j = 0; j < count; ++j)
      if (!pllhip_pars_dev_spr_launch(((pars_obj_t *)list[j])->dev, mops, nops, members, nm, nout)) goto done;
    memset(acc, 0, sizeof(*acc) * nout);
    for (j = 0; j < count; ++j)
      if (!pllhip_pars_dev_spr_collect(((pars_obj_t *)list[j])->dev, acc)) goto done;
    /* the first member, in visit order, with a strictly better edge moves */
    i = next;
    for (j = 0; j < nm; ++j)
    {
      const unsigned long long * c = acc + members[5 * j + 4];
      const int * ex = medge + members[5 * j + 4];
      const unsigned int nc = (unsigned int)mv[2 * j + 1];
      const int v = members[5 * j + 3];
      unsigned int e, best = 1;
      for (e = 2; e < nc; ++e)
        if (c[e] < c[best]) best = e;
      if (c[best] >= c[0]) continue;
      for (e = 1; e < nc; ++e)
      {
        if (c[e] != c[best] || e == best) continue;
        const unsigned int na = subtree_tips(&q.r.t, ex[best], v, key_a, stack);
        const unsigned int nb = subtree_tips(&q.r.t, ex[e], v, key_b, stack);
        unsigned int m = 0;
        while (m < na && m < nb && key_a[m] == key_b[m]) ++m;
        if ((m < na && m < nb) ? key_b[m] < key_a[m] : nb < na) best = e;
      }
      /* the move: p with its subtree v onto the edge above x, on the caller's records */
      ptree_t * t = &q.r.t;
      const int x = ex[best], p = t->parent[v];
      const int s = t->child[2 * p] == v ? t->child[2 * p + 1] : t->child[2 * p];
      const int pp = t->parent[p];
      pll_unode_t * pv = q.r.up[v]->back;
      if (!pll_utree_spr(pv, q.r.up[x], NULL, NULL, NULL)) goto done;
      q.r.up[p] = pv->next->next;
      t->parent[s] = pp;
      if (pp == t->r0) t->c0 = s;
      else t->child[2 * pp + (t->child[2 * pp] == p ? 0 : 1)] = s;
      const int y = t->parent[x];
      t->parent[p] = y;
      t->child[2 * p] = x;
      t->child[2 * p + 1] = v;
      t->parent[x] = p;
      if (y == t->r0) t->c0 = p;
      else t->child[2 * y + (t->child[2 * y] == x ? 0 : 1)] = p;
      if (!spr_refresh(list, count, &q, wops, post, stack, wcost, &total)) goto done;
      i = (unsigned int)mv[2 * j] + 1;
      break;
    }
  }
  if (total > 0xFFFFFFFFULL)
  {
    pars_error(PLL_ERROR_PARAM_INVALID, "The parsimony score does not fit an unsigned int");
    goto done;
  }
  *cost = (unsigned int)total;
  rc = PLL_SUCCESS;
done:
  free(tab); free(inner_clv); free(gid); free(order); free(wops); free(post); free(stack); free(chain);
  free(key_a); free(key_b); free(wcost); free(q.tin); free(q.tout); free(q.pidx); free(q.slot); free(q.mark);
  free(q.touched); free(q.pre); free(mops); free(members); free(medge); free(mv); free(acc);
  rtree_free(&q.r);
  if (rng) pll_random_destroy(rng);
  return rc;
}
