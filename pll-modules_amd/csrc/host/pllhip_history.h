/*
 * pllhip_history.h -- the host tables of the sampled substitution histories ("Sampled substitution
 * histories"), shared between the driver's host path (pllhip_eval.c, which builds them) and the device call
 * (pll_history_dev.hip, which uploads them).  Not installed; the public interface is include/pllhip.h and
 * include/pllhip_eval.h.
 */
#ifndef PLLHIP_HISTORY_H_INCLUDED
#define PLLHIP_HISTORY_H_INCLUDED

#include "pll.h"

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLLHIP_HIST_STREAM 0x40000000u      /* + (matrix << 11) + i: jump count and steps; + 1024 + i: event times */
#define PLLHIP_HIST_MAX_MATRIX (1u << 19)

typedef struct pllhip_history_tables
{
  unsigned int states, cats, edge_count;
  unsigned int kmax;            /* powers held per rate matrix: the longest Poisson table, at least 2 */
  unsigned int nmat;            /* distinct rate matrices among params_indices */
  unsigned int * slot;          /* [cats]: which Rpow table category r reads */
  double * mu;                  /* [nmat] */
  double * rpow;                /* [nmat][kmax][states][states] */
  double * tau;                 /* [edge][cats] */
  unsigned int * len;           /* [edge][cats]: entries of the Poisson table */
  unsigned long long * off;     /* [edge][cats]: its first entry in pois */
  double * pois;
  unsigned long long pois_count;
} pllhip_history_tables_t;

/* NULL with pll_errno set (PLL_ERROR_PARAM_INVALID: a negative or non-finite length, a table beyond the cap, a matrix
   index of 2^19 or more, a parameter index out of range, an eigen system that is not valid, pattern weights that add
   up to 2^31 or more; PLL_ERROR_MEM_ALLOC).  Reads the partition only. */
pllhip_history_tables_t * pllhip_history_tables_create(const pll_partition_t * partition, unsigned int edge_count,
                                                       const unsigned int * matrix_indices,
                                                       const unsigned int * params_indices,
                                                       const double * branch_lengths, const char * who);
void pllhip_history_tables_destroy(pllhip_history_tables_t * t);

#ifdef __cplusplus
}
#endif

#endif
