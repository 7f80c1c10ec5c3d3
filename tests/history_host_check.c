/* history_host_check.c -- the host stage of the sampled substitution histories (include/pllhip_eval.h:
 * pllhip_history_rate_table, pllhip_history_poisson, pllhip_history_summary) on fixed inputs, as a program of its own:
 * tests/test_history_cpu.py builds it with -fsanitize=address,undefined and runs it.
 *
 * The eigen system is Jukes-Cantor's in libpll's storage (P = inv_eigenvecs diag(exp(lambda t)) eigenvecs) with rate 1/3
 * between any two states: Q = -4/3 (I - J/4), mu = 1, R = J/3 off the diagonal and 0 on it, and
 * Rpow[k][a][b] = 1/4 + (a == b ? 3/4 : -1/4) (-1/3)^k. */
#include "pllhip_eval.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define S 4
#define SP 4
#define K 12

static int failures;

static void check(int ok, const char * what)
{
  if (ok) return;
  ++failures;
  printf("FAILED: %s\n", what);
}

int main(void)
{
  /* an orthonormal basis: the constant vector (eigenvalue 0) and three contrasts (eigenvalue -4/3) */
  const double h = 0.5;
  const double W[S * SP] = { h, h, h, h,   h, h, -h, -h,   h, -h, h, -h,   h, -h, -h, h };
  double V[S * SP], lambda[S] = { 0.0, -4.0 / 3.0, -4.0 / 3.0, -4.0 / 3.0 };
  double * rpow = (double *)malloc(sizeof(double) * K * S * S);          /* exactly K tables: one more write is caught */
  double * pois = (double *)malloc(sizeof(double) * PLLHIP_HIST_MAX_TABLE);
  double mu = -1.0, sum, total = -1.0;
  unsigned int a, b, k, len = 0;
  if (!rpow || !pois) return 2;
  for (a = 0; a < S; ++a) for (b = 0; b < S; ++b) V[a * SP + b] = W[b * SP + a];

  check(pllhip_history_rate_table(S, SP, W, V, lambda, K, &mu, rpow) == PLL_SUCCESS, "rate table");
  check(fabs(mu - 1.0) < 1e-15, "mu = 1");
  for (k = 0; k < K; ++k)
    for (a = 0; a < S; ++a)
      for (b = 0; b < S; ++b)
      {
        const double want = 0.25 + (a == b ? 0.75 : -0.25) * pow(-1.0 / 3.0, (double)k);
        check(fabs(rpow[(k * S + a) * S + b] - want) < 1e-14, "Rpow in closed form");
        check(rpow[(k * S + a) * S + b] >= 0.0, "no negative entry");
      }
  check(pllhip_history_rate_table(S, SP, W, V, lambda, 1, &mu, rpow) == PLL_SUCCESS, "K = 1 writes the identity alone");
  check(pllhip_history_rate_table(S, SP, W, V, lambda, 0, &mu, rpow) == PLL_FAILURE, "K = 0 is refused");
  memset(lambda, 0, sizeof(lambda));
  check(pllhip_history_rate_table(S, SP, W, V, lambda, 3, &mu, rpow) == PLL_SUCCESS && mu == 0.0, "mu = 0");
  for (a = 0; a < S; ++a)
    for (b = 0; b < S; ++b) check(rpow[(2 * S + a) * S + b] == (a == b ? 1.0 : 0.0), "mu = 0 gives R = I");

  /* the Poisson table: its rule, its sum, its first entries, the cap */
  check(pllhip_history_poisson(0.0, pois, &len) == PLL_SUCCESS && len == 1 && pois[0] == 1.0, "lambda = 0");
  check(pllhip_history_poisson(2.5, pois, &len) == PLL_SUCCESS && len > 2 && len < 60, "lambda = 2.5");
  for (sum = 0.0, k = 0; k < len; ++k) sum += pois[k];
  check(fabs(sum - 1.0) < 1e-14 && fabs(pois[0] - exp(-2.5)) < 1e-16 && fabs(pois[3] - exp(-2.5) * 2.5 * 2.5 * 2.5 / 6.0) < 1e-15,
        "the Poisson masses");
  check(exp((double)len * log(2.5) - 2.5 - lgamma((double)len + 1.0)) < 0x1.0p-70 * sum, "the table ends by its rule");
  check(pllhip_history_poisson(700.0, pois, &len) == PLL_SUCCESS && len > 700 && len <= PLLHIP_HIST_MAX_TABLE, "lambda = 700");
  check(pllhip_history_poisson(900.0, pois, &len) == PLL_FAILURE, "beyond the cap");
  check(pllhip_history_poisson(-1.0, pois, &len) == PLL_FAILURE && pllhip_history_poisson(NAN, pois, &len) == PLL_FAILURE,
        "a negative or undefined lambda");

  /* the summary: two categories, a cell that went through a negative intermediate sum */
  {
    unsigned long long counts_int[S * S] = { 0 }, units[2 * S] = { 0 };
    double counts[S * S], dwell[S], tau[2] = { 0.5, 2.0 };
    counts_int[0 * S + 1] = 3; counts_int[2 * S + 3] = 5;
    units[0 * S + 0] = 0ULL - 7ULL;                  /* -7 units, two's complement */
    units[0 * S + 1] = 1ULL << 32;
    units[1 * S + 1] = 3ULL << 31;
    check(pllhip_history_summary(S, 2, tau, counts_int, units, counts, dwell, &total) == PLL_SUCCESS, "summary");
    check(total == 8.0 && counts[1] == 3.0 && counts[2 * S + 3] == 5.0, "counts as doubles");
    check(dwell[0] == -7.0 * 0.5 * 0x1.0p-32 && dwell[1] == 0.5 + 2.0 * 1.5 && dwell[2] == 0.0, "dwell in rate-scaled time");
    check(pllhip_history_summary(S, 2, NULL, counts_int, units, counts, dwell, &total) == PLL_FAILURE, "a NULL argument");
  }
  free(rpow);
  free(pois);
  printf(failures ? "history host check: %d failures\n" : "history host check: ok\n", failures);
  return failures != 0;
}
