// Host build of the device's correctly rounded sin and derivative entry (nlml_hpe_amd/csrc/cr_cos.h) for tests/test_td_gradient_host.py.
#include "../../nlml_hpe_amd/csrc/cr_cos.h"
extern "C" void cr_sin_array(const double* x, double* y, long n) {
  for (long i = 0; i < n; ++i) y[i] = nlml::cr_sin(x[i]);
}
// fast[i] = cr_f32_nab_sin (library sin unless the float could depend on its last bits); slow[i] = the double-double sin alone
extern "C" void cr_dfvalue_arrays(const double* a, const double* b, const double* t, float* fast, float* slow, long n) {
  for (long i = 0; i < n; ++i) {
    fast[i] = nlml::cr_f32_nab_sin(a[i], b[i], t[i]);
    slow[i] = (float)((-a[i] * b[i]) * nlml::cr_sin(t[i]));
  }
}
