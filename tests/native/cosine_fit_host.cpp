// Stand-alone host program for tests/test_cosine_fit_host.py: the cosine fit's host forms (csrc/cosine_fit_ref.h: the objective and
// the four-parameter Powell machine behind nlml_cosine_fit_host) on the columns of a text file, built with
// -fsanitize=address,undefined and run directly.  Every row lives in a heap block of exactly its size, so a read past a row's end
// is reported.
//
//   file:  "<C> <ld>" then C lines "<n> <ld y values> <ld w values> <4 start values>", floats in C99 hex notation
//   out:   "fit <f> <x0> <x1> <x2> <x3> <fun> <nfev> <nit> <status>" per column (hex floats), then "cosine fit host ok"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../nlml_hpe_amd/csrc/cosine_fit_ref.h"

using namespace nlml;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int C = 0, ld = 0;
  if (std::fscanf(f, "%d %d", &C, &ld) != 2 || C < 0 || ld < 1) return 2;
  for (int k = 0; k < C; ++k) {
    int n = 0;
    if (std::fscanf(f, "%d", &n) != 1 || n < 1 || n > ld || n > CF_ROWS_MAX) return 2;
    std::vector<double> row(2 * ld + 4);
    char tok[64];
    for (double& v : row) {
      if (std::fscanf(f, "%63s", tok) != 1) return 2;
      v = std::strtod(tok, nullptr);
    }
    // exactly n samples and n angles: nothing beyond them may be read
    double* y = new double[n];
    double* w = new double[n];
    for (int i = 0; i < n; ++i) { y[i] = row[i]; w[i] = row[ld + i]; }
    double x[4], fun = 0.0;
    int32_t nfev = 0, nit = 0, status = 0;
    cf_fit_host(y, w, n, &row[2 * ld], 1e-4, 1e-4, x, &fun, &nfev, &nit, &status);
    if (cf_objective(y, w, n, x) != fun && fun == fun) {   // the end point's value is the value of an evaluated point
      std::printf("column %d: fun %a is not the objective at x (%a)\n", k, fun, cf_objective(y, w, n, x));
      return 1;
    }
    std::printf("fit %d %a %a %a %a %a %d %d %d\n", k, x[0], x[1], x[2], x[3], fun, (int)nfev, (int)nit, (int)status);
    delete[] y;
    delete[] w;
  }
  std::fclose(f);
  // the row-count limits on blocks of exactly that size, and a NaN column (status 4 after 1 + 3 * 4 evaluations)
  for (int n : {1, CF_ROWS_MAX}) {
    double* y = new double[n];
    double* w = new double[n];
    for (int i = 0; i < n; ++i) { y[i] = 0.3 + 0.01 * i; w[i] = -50.0 + 100.0 * i / CF_ROWS_MAX; }
    const double x0[4] = {0.2, 1.0, 0.1, 0.0};
    double x[4], fun;
    int32_t nfev, nit, status;
    cf_fit_host(y, w, n, x0, 1e-4, 1e-4, x, &fun, &nfev, &nit, &status);
    if (status < PW_CONVERGED || status > PW_MAXITER || nfev < 1 || nfev > 4000) return 1;
    y[0] = NAN;
    cf_fit_host(y, w, n, x0, 1e-4, 1e-4, x, &fun, &nfev, &nit, &status);
    if (status != PW_NAN || nfev != 1 + 3 * CF_NPAR) return 1;
    delete[] y;
    delete[] w;
  }
  std::printf("cosine fit host ok\n");
  return 0;
}
