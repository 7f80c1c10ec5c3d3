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

/* tips of the subtree of v, sorted, into out; returns the count */
static unsigned int subtree_tips(const ptree_t * t, int v, int * out, int * stack)
{
  unsigned int n = 0, sp = 0, i, j;
  stack[sp++] = v;
  while (sp)
  {
    const int x = stack[--sp];
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
  unsigned int i, k;
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
  for (k = 3; k < tips; ++k)
  {
    const int taxon = (int)order[k];
    const unsigned int npre = preorder_ops(&t, ops + 3 * ndown, edge_node, stack);
    if (!walk_all(list, count, ops, ndown, npre, taxon, cost, NULL)) goto done;
    unsigned int best = 0;
    for (i = 1; i < npre; ++i)
      if (cost[i] < cost[best]) best = i;
    for (i = 0; i < npre; ++i)
    {
      if (cost[i] != cost[best] || i == best) continue;
      /* tie: the smaller split key (tips below the edge, sorted; a prefix is smaller) */
      const unsigned int na = subtree_tips(&t, edge_node[best], key_a, stack);
      const unsigned int nb = subtree_tips(&t, edge_node[i], key_b, stack);
      unsigned int m = 0;
      while (m < na && m < nb && key_a[m] == key_b[m]) ++m;
      if ((m < na && m < nb) ? key_b[m] < key_a[m] : nb < na) best = i;
    }
    /* insert the taxon on edge (v, parent of v) through the new inner node x */
    const int v = edge_node[best], u = t.parent[v], x = next_inner++;
    t.parent[x] = u;
    t.child[2 * x] = v;
    t.child[2 * x + 1] = taxon;
    t.parent[v] = x;
    t.parent[taxon] = x;
    if (v == t.c0) t.c0 = x;
    else t.child[2 * u + (t.child[2 * u] == v ? 0 : 1)] = x;
    ndown = 0;
    for (int y = x; y != t.r0; y = t.parent[y])
    {
      ops[3 * ndown] = y;
      ops[3 * ndown + 1] = t.child[2 * y];
      ops[3 * ndown + 2] = t.child[2 * y + 1];
      ++ndown;
    }
  }
  /* the final cost: a whole postorder pass plus the join with r0 */
  {
    unsigned int sp = 0, n = 0;
    unsigned long long total = 0;
    int * post = edge_node;            /* inner nodes in postorder */
    stack[sp++] = t.c0;
    while (sp)                         /* reverse of a (node, right, left) preorder is a postorder */
    {
      const int y = stack[--sp];
      post[n++] = y;
      for (i = 0; i < 2; ++i)
        if (t.child[2 * y + i] >= (int)tips) stack[sp++] = t.child[2 * y + i];
    }
    for (i = 0; i < n; ++i)
    {
      const int y = post[n - 1 - i];
      ops[3 * i] = y;
      ops[3 * i + 1] = t.child[2 * y];
      ops[3 * i + 2] = t.child[2 * y + 1];
    }
    ops[3 * n] = -1; ops[3 * n + 1] = t.c0; ops[3 * n + 2] = t.r0;
    if (!walk_all(list, count, ops, n + 1, 0, -1, NULL, &total)) goto done;
    if (total > 0xFFFFFFFFULL)
    {
      pars_error(PLL_ERROR_PARAM_INVALID, "The parsimony score does not fit an unsigned int");
      goto done;
    }
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
