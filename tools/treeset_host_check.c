/* treeset_host_check.c -- the tree set's host side (csrc/host/pllhip_treeset.c: label table, validation, split plan,
 * transfer program) under the host sanitizers, as a program of its own: no device, no Python.
 *
 * Build and run from the repository root:
 *
 *   gcc -std=gnu99 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined \
 *       -Iinclude -Ipll-modules_amd/csrc -o /tmp/treeset_host_check tools/treeset_host_check.c \
 *       pll-modules_amd/csrc/host/pllhip_treeset.c pll-modules_amd/csrc/host/pll_utree.c -lm
 *   python -c "import json; d = json.load(open('tests/golden/tree_support_fixtures.json')); \
 *     [print('labels', *c['labels']) or [print('tree', t) for t in [c['ref']] + c['trees']] for c in d['cases']]" \
 *     | /tmp/treeset_host_check
 *
 * Input lines: `labels l0 l1 ...` starts a label table, `tree <newick>` flattens a tree against it.  After the input
 * come trees made here: caterpillars of 300 and 5000 tips (the recursive Newick parser sets the limit), and trees that
 * must be rejected.  Every accepted tree's plan is checked: the intervals nest or are disjoint, the program's stack stays within 1 + floor(log2 T) and ends
 * with one entry of T - 1 tips, and the sorted splits ascend.  Exit status 0 and "ok" when all of it held.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pll.h"
#include "treeset_plan.h"

__thread int pll_errno;
__thread char pll_errmsg[200];

static unsigned int checked = 0, rejected = 0;

static void die(const char * what)
{
  fprintf(stderr, "treeset_host_check: %s (pll_errno %d: %s)\n", what, pll_errno, pll_errmsg);
  exit(1);
}

/* PLL_SUCCESS: accepted and checked */
static int check_tree(const char * newick, unsigned int T, const pllhip_ts_labels_t * labels)
{
  pll_utree_t * tree = pll_utree_parse_newick_string(newick);
  const unsigned int R = T - 3u, len = pllhip_ts_words(T);
  uint32_t * order = (uint32_t *)malloc((T - 1u) * sizeof(uint32_t)), * lo = (uint32_t *)malloc(R * sizeof(uint32_t));
  uint32_t * hi = (uint32_t *)malloc(R * sizeof(uint32_t)), * perm = (uint32_t *)malloc(R * sizeof(uint32_t));
  uint32_t * words = (uint32_t *)malloc((size_t)R * len * sizeof(uint32_t));
  uint64_t * hash = (uint64_t *)malloc(R * sizeof(uint64_t));
  pll_unode_t ** edge = (pll_unode_t **)malloc(R * sizeof(pll_unode_t *));
  pllhip_ts_step_t * program = (pllhip_ts_step_t *)malloc((2u * T - 3u) * sizeof(pllhip_ts_step_t));
  unsigned int deepest = 0, i, bound = 1, sp = 0;
  unsigned int sizes[PLLHIP_TS_MAX_STACK];
  int ok;
  if (!tree) die("a tree does not parse");
  ok = pllhip_ts_flatten(tree, T, labels, order, lo, hi, edge, program, &deepest);
  if (ok)
  {
    for (i = T; i > 1u; i >>= 1) ++bound;
    if (deepest > bound) die("stack bound");
    for (i = 0; i < R; ++i)
    {
      unsigned int k;
      if (lo[i] + 2u > hi[i] || hi[i] > T - 1u || !edge[i] || !edge[i]->next) die("interval");
      for (k = 0; k < i; ++k)
        if (!(hi[k] <= lo[i] || hi[i] <= lo[k] || (lo[k] <= lo[i] && hi[i] <= hi[k]) || (lo[i] <= lo[k] && hi[k] <= hi[i])))
          die("intervals neither nest nor are disjoint");
      if (T > 2000u && i > 64u) break;                           /* quadratic: the start of a long tree is enough */
    }
    for (i = 0; i < 2u * T - 3u; ++i)
    {
      if (program[i].kind == PLLHIP_TS_PUSH)
      {
        if (sp >= PLLHIP_TS_MAX_STACK || program[i].arg >= T) die("push");
        sizes[sp++] = 1;
      }
      else
      {
        if (sp < 2u) die("combine");
        sizes[sp - 2u] += sizes[sp - 1u];
        --sp;
        if (sizes[sp - 1u] != program[i].arg) die("a combine step's size");
      }
    }
    if (sp != 1u || sizes[0] != T - 1u) die("the program's end");
    pllhip_ts_plan_splits(T, order, lo, hi, words, hash);
    pllhip_ts_sort_splits(T, R, words, perm);
    for (i = 0; i < R; ++i)
    {
      if (!(words[(size_t)perm[i] * len] & 1u)) die("a split is not normalised");
      if (i && memcmp(words + (size_t)perm[i - 1u] * len, words + (size_t)perm[i] * len, len * 4u) == 0) die("equal splits");
    }
    ++checked;
  }
  else
    ++rejected;
  pll_utree_destroy(tree, NULL);
  free(order); free(lo); free(hi); free(perm); free(words); free(hash); free(edge); free(program);
  return ok;
}

static char * caterpillar(unsigned int T, char *** names_out)
{
  char ** names = (char **)malloc(T * sizeof(char *));
  char * text = (char *)malloc((size_t)T * 12u + 16u), * at = text;
  unsigned int i;
  for (i = 0; i < T; ++i)
  {
    names[i] = (char *)malloc(12);
    snprintf(names[i], 12, "c%u", i);
  }
  /* the spine c1, c2, ..., c(T-1), with c0 in the place of c(T/2) and c(T/2) at the far end */
  at += sprintf(at, "(c1,c2,");
  for (i = 3; i < T; ++i) at += sprintf(at, "(c%u,", i == T / 2u ? 0u : i);
  at += sprintf(at, "c%u", T / 2u);
  for (i = 3; i < T; ++i) *at++ = ')';
  sprintf(at, ");");
  *names_out = names;
  return text;
}

int main(void)
{
  char * line = NULL;
  size_t cap = 0;
  pllhip_ts_labels_t * labels = NULL;
  unsigned int T = 0, k;
  static const unsigned int LONG[2] = {300u, 5000u};
  while (getline(&line, &cap, stdin) > 0)
  {
    line[strcspn(line, "\n")] = 0;
    if (!strncmp(line, "labels ", 7))
    {
      char ** list = NULL, * tok;
      char * copy = strdup(line + 7);
      T = 0;
      for (tok = strtok(copy, " "); tok; tok = strtok(NULL, " "))
      {
        list = (char **)realloc(list, (T + 1u) * sizeof(char *));
        list[T++] = tok;
      }
      pllhip_ts_labels_destroy(labels);
      labels = pllhip_ts_labels_create(T, (const char * const *)list);
      if (!labels) die("label table");
      if (pllhip_ts_labels_find(labels, list[T - 1u]) != (long)T - 1 || pllhip_ts_labels_find(labels, "no such") != -1)
        die("label lookup");
      free(list);
      free(copy);
    }
    else if (!strncmp(line, "tree ", 5))
    {
      if (!labels || !check_tree(line + 5, T, labels)) die("a tree of the input is rejected");
    }
  }
  free(line);
  pllhip_ts_labels_destroy(labels);

  for (k = 0; k < 2u; ++k)
  {
    char ** names;
    char * text = caterpillar(LONG[k], &names);
    labels = pllhip_ts_labels_create(LONG[k], (const char * const *)names);
    if (!labels || !check_tree(text, LONG[k], labels)) die("caterpillar");
    pllhip_ts_labels_destroy(labels);
    for (T = 0; T < LONG[k]; ++T) free(names[T]);
    free(names);
    free(text);
  }

  {
    static const char * NAMES[6] = {"a", "b", "c", "d", "e", "f"}, * TWICE[6] = {"a", "b", "c", "d", "e", "a"};
    static const char * BAD[5] = {"((a,b),(c,d),(e,zz));", "((a,b),(c,d),(e,e));", "((a,b),(c,d),e);", "((a,b),c,d,(e,f));",
                                  "((a,b,c),d,(e,f));"};
    static const int CODE[5] = {PLL_ERROR_PARAM_INVALID, PLL_ERROR_PARAM_INVALID, PLL_ERROR_TREE_INVALID,
                                PLL_ERROR_TREE_INVALID, PLL_ERROR_TREE_INVALID};
    if (pllhip_ts_labels_create(6, TWICE) || pll_errno != PLL_ERROR_PARAM_INVALID) die("a label given twice is accepted");
    labels = pllhip_ts_labels_create(6, NAMES);
    for (k = 0; k < 5u; ++k)
    {
      pll_errno = 0;
      if (check_tree(BAD[k], 6, labels) || pll_errno != CODE[k]) die(BAD[k]);
    }
    if (!check_tree("((a,b),(c,d),(e,f));", 6, labels)) die("a good tree is rejected");
    if (!check_tree("((a,b),(c,d),(e,f));", 6, NULL)) die("a good tree is rejected by node_index");
    pllhip_ts_labels_destroy(labels);
  }
  printf("ok: %u trees checked, %u rejected\n", checked, rejected);
  return 0;
}
