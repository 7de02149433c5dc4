// Host run of the shipped IPD normalisation (nlml_hpe_amd/csrc/ipd_norm.h, the statement every kernel compiles) for
// tests/test_ipd_exact_host.py:  ipd_norm_host RAW OUT IPD  reads raw faces float32[B,1404] from RAW and writes the normalised
// float32[B,1404] to OUT and the float64[B] ipds to IPD -- the set-up once per face, div_ipd per element, as K1 does it.
// -DIPD_NORM_OLD_RESIDUAL: the chain with the residual as it stood before the sign fix, r = n - q d added back, which loses the sign of a
// -0.0 numerator; the test builds it to show that it would have been caught.
#include <stdio.h>

#include <vector>

#include "../../nlml_hpe_amd/csrc/ipd_norm.h"

static double divide(double n, double d, double y) {
#ifdef IPD_NORM_OLD_RESIDUAL
  const double q = nlml::div_ipd_quotient(n, y);
  const double r = fma(-q, d, n);
  return fma(r, y, q);
#else
  return nlml::div_ipd(n, d, y);
#endif
}

int main(int argc, char** argv) {
  constexpr int F = 1404;
  if (argc != 4) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<float> raw;
  float row[F];
  while (fread(row, sizeof(float), F, in) == (size_t)F) raw.insert(raw.end(), row, row + F);
  fclose(in);
  const size_t B = raw.size() / F;
  std::vector<float> out(raw.size());
  std::vector<double> ipds(B);
  for (size_t b = 0; b < B; ++b) {
    const float* p = raw.data() + b * F;
    double ipd, rcp, ref[3];
    nlml::ipd_setup(p, ipd, rcp, ref[0], ref[1], ref[2]);
    ipds[b] = ipd;
    for (int k = 0; k < F; ++k) out[b * F + k] = (float)divide((double)p[k] - ref[k % 3], ipd, rcp);
  }
  FILE* fo = fopen(argv[2], "wb");
  FILE* fi = fopen(argv[3], "wb");
  if (!fo || !fi) return 4;
  const bool ok = fwrite(out.data(), sizeof(float), out.size(), fo) == out.size() && fwrite(ipds.data(), sizeof(double), B, fi) == B;
  return (fclose(fo) == 0) & (fclose(fi) == 0) & ok ? 0 : 5;
}
