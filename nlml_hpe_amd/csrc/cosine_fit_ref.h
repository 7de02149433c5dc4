// cosine_fit_ref.h -- the objective of the pose factors' cosine fit, stated once for host and device.
//
// The reference fits every column U_j of the three pose factor matrices by a cos(b w + c) + d over its angle bins w (degrees):
// TD_Trainer.Train (TD_Trainer.py:232-351) runs scipy.optimize.minimize(objective, guess, method='Powell') per column over
// (a, b, c, d), with
//     objective(params) = 1/2 sum_i (U_j[i] - (a cos(b radians(w_i) + c) + d))^2                                   (:37-42)
// as an interpreted loop.  All of it is f64 (the f32 column entry is promoted by the subtraction), one operation at a time:
//
//     wr_i  = w_deg[i] * 0.017453292519943295          np.radians: bit for bit this product (checked on the integer degrees
//                                                      -180..180 and on 100,000 random values)
//     t_i   = b * wr_i + c                             product and sum rounded on their own
//     m_i   = a * cos(t_i) + d
//     e_i   = y[i] - m_i
//     q_i   = e_i * e_i
//     s     = (((0 + q_0) + q_1) + ...) + q_{n-1}      sequential, i ascending
//     value = s / 2
//
// Two library functions of the reference's objective are NOT correctly rounded in glibc, so no second implementation can return
// numpy's bits; both are replaced by their correctly rounded values -- the rule cr_cos.h sets for the f-vectors' cos, for the
// reason its header gives (two libraries cannot be made to agree, but both can be held to the exact result):
//   np.cos           -> cr_cos (cr_cos.h)
//   scalar e ** 2    -> e * e.  numpy's scalar power is libm pow(e, 2.0), which differs from the correctly rounded square e * e on
//                       174 of 200,000 random values; e * e IS the correctly rounded square.
// With math.pow(e, 2.0) in place of e * e a plain restatement of the above is bit-equal to the reference, so the rest of the order
// is the reference's.  The two replacements move about 1 objective value in 2,000 by one unit in the last place, and a Powell end
// point by 3e-8..1e-7 -- the distance between two hosts' runs of the reference itself.
//
// cf_fit_host is the whole fit on the CPU: powell.h's machine with four parameters (scipy's maxiter = maxfev = 4000) resumed with
// this objective.  The device kernel (cosine_fit.hip, K8) evaluates the same cf_term per lane and the same sequential sum.
#pragma once
#include <stdint.h>

#include "cr_cos.h"
#include "powell.h"

namespace nlml {

constexpr int CF_NPAR = 4;            // (a, b, c, d)
constexpr int CF_ROWS_MAX = 64;       // NLML_COSINE_FIT_ROWS_MAX: one row per lane of a wave
constexpr double CF_DEG2RAD = 0.017453292519943295;

typedef PowellStateT<CF_NPAR, PowellDimFixed<CF_NPAR>> PowellState4;   // the four-parameter machine: maxiter = maxfev = 4000

NLML_HD double cf_radians(double w_deg) {
  NLML_FP_STRICT
  return w_deg * CF_DEG2RAD;
}

// q_i: the squared residual of one row at the parameters (a, b, c, d); wr = cf_radians(w_deg[i])
NLML_HD double cf_term(double y, double wr, double a, double b, double c, double d) {
  NLML_FP_STRICT
  const double t = b * wr + c;
  const double m = a * cr_cos(t) + d;
  const double e = y - m;
  return e * e;
}

// the objective value of n rows at p = (a, b, c, d)
NLML_HD double cf_objective(const double* y, const double* w_deg, int n, const double* p) {
  NLML_FP_STRICT
  double s = 0.0;
  for (int i = 0; i < n; ++i) s = s + cf_term(y[i], cf_radians(w_deg[i]), p[0], p[1], p[2], p[3]);
  return s / 2.0;
}

// One fit on the host: x f64[4], the others may be null.
inline void cf_fit_host(const double* y, const double* w_deg, int n, const double* x0, double xtol, double ftol, double* x, double* fun,
                        int32_t* nfev, int32_t* nit, int32_t* status) {
  PowellState4 s;
  powell_init(s, x0, xtol, ftol);
  double f = 0.0;
  bool need = powell_step(s, f);
  for (int round = 0; need && round < s.maxfun + 16; ++round) {
    f = cf_objective(y, w_deg, n, s.xeval);
    need = powell_step(s, f);
  }
  for (int k = 0; k < CF_NPAR; ++k) x[k] = s.x[k];
  if (fun) *fun = s.fval;
  if (nfev) *nfev = s.nfev;
  if (nit) *nit = s.iter;
  if (status) *status = need ? PW_RUNNING : s.status;
}

}  // namespace nlml
