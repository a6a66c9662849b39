// scoary_ttail.hpp -- the two-sided tail of Student's t of spec S24 (scoary_score.hip: the linear score test).
#ifndef SCOARY_TTAIL_HPP
#define SCOARY_TTAIL_HPP

namespace {

// The continued fraction of the regularised incomplete beta function I_x(a, b) without its front factor, by the
// modified Lentz recurrence; it converges quickly for x < (a + 1) / (a + b + 2), which the caller sees to.
__device__ __forceinline__ double tt_beta_cf(double a, double b, double x) {
  const double tiny = 1e-300;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= 4000; ++m) {
    const double m2 = 2.0 * (double)m;
    double aa = (double)m * (b - (double)m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + (double)m) * (qab + (double)m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < 1e-15) break;
  }
  return h;
}

// S24: P(|T_df| >= |t|) = I_x(df / 2, 1 / 2) at x = df / (df + t^2), df >= 1.  x and 1 - x are both formed without a
// subtraction (from t^2 / df), their logarithms by log1p; the fraction is taken on the side where it converges and
// the other side is the complement, which is only used where the tail is above a half.  A value, not bits (within
// 1e-10 relative of the true tail above 1e-290).
__device__ __forceinline__ double t_tail(double t, int df) {
  if (t != t || df < 1) return 1.0;
  const double t2 = t * t;
  if (!(t2 > 0.0)) return 1.0;
  if (t2 == __builtin_inf()) return 0.0;
  const double a = 0.5 * (double)df, b = 0.5;
  const double r = t2 / (double)df;                     // x = 1 / (1 + r), 1 - x = r / (1 + r)
  const double x = 1.0 / (1.0 + r), y = r / (1.0 + r);
  const double lx = -log1p(r), ly = r < 1.0 ? log(r) - log1p(r) : -log1p(1.0 / r);
  // log(Gamma(a + 1/2) / Gamma(a)): past a = 20 by its asymptotic series (the next term is below 1e-13 there), so
  // that two logarithms of Gamma of some thousands are never subtracted; log(Gamma(1/2)) = log(pi) / 2
  double lg;
  if (a >= 20.0) {
    const double ia = 1.0 / a, ia2 = ia * ia;
    lg = 0.5 * log(a) - ia * (1.0 / 8.0 - ia2 * (1.0 / 192.0 - ia2 * (1.0 / 640.0 - ia2 * (17.0 / 14336.0))));
  } else {
    lg = lgamma(a + b) - lgamma(a);
  }
  const double front = exp(((a * lx + b * ly) + lg) - 0.57236494292470008707);
  if (x < (a + 1.0) / (a + b + 2.0)) return fmin(front * tt_beta_cf(a, b, x) / a, 1.0);
  return fmin(fmax(1.0 - front * tt_beta_cf(b, a, y) / b, 0.0), 1.0);
}

}  // namespace
#endif
