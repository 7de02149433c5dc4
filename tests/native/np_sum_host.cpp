// Host run of the shipped pairwise sum (nlml_hpe_amd/csrc/np_sum.h, the statement the kernels and the host restatements compile) for
// tests/test_np_sum_host.py:  np_sum_host ROWS SUMS  reads rows from ROWS -- each an int32 length n followed by n float64 values --
// and writes np_pairwise_sum of every row, float64, to SUMS.  On standard output: the leaf tables of NpTree<N> for the N below, one
// line each:  N leaves balanced off(0) .. off(leaves).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../nlml_hpe_amd/csrc/np_sum.h"

template <int N>
static void print_tree() {
  typedef nlml::NpTree<N> T;
  printf("%d %d %d", N, T::leaves, T::balanced ? 1 : 0);
  for (int L = 0; L <= T::leaves; ++L) printf(" %d", T::off(L));
  for (int L = 0; L < T::leaves; ++L)
    if (T::len(L) != T::off(L + 1) - T::off(L)) printf(" bad-len");
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  print_tree<129>();
  print_tree<136>();
  print_tree<468>();
  print_tree<1000>();
  print_tree<1404>();
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<double> sums, row;
  int32_t n;
  while (fread(&n, sizeof n, 1, in) == 1) {
    if (n < 0) return 6;
    row.resize((size_t)n);
    if (fread(row.data(), sizeof(double), (size_t)n, in) != (size_t)n) return 6;
    sums.push_back(nlml::np_pairwise_sum(row.data(), n));
  }
  fclose(in);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 4;
  const bool ok = fwrite(sums.data(), sizeof(double), sums.size(), out) == sums.size();
  return (fclose(out) == 0) & ok ? 0 : 5;
}
