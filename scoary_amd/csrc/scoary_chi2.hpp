// scoary_chi2.hpp -- the chi-square upper tail of spec S14, shared by the translation units that report a chi-square
// p (scoary_cmh.hip: the homogeneity test; scoary_categorical.hip: spec S20), so that both compile the same text.
#ifndef SCOARY_CHI2_HPP
#define SCOARY_CHI2_HPP
#include "scoary_common.hpp"

namespace {

// S14: the upper tail Q(df / 2, stat / 2) of the chi-square distribution, 1 <= df <= 1023.  The finite sum of the
// tail (all terms positive, plus erfc for an odd df) taken outward from its largest term, which is the one value
// that goes through exp / log / lgamma; a value, not bits (within 1e-10 relative of the true tail above 1e-290).
__device__ __forceinline__ double chi2_tail(double stat, int df) {
  if (!(stat > 0.0)) return 1.0;
  if (stat == __builtin_inf()) return 0.0;
  const double y = stat / 2.0;
  const int h = df >> 1;                                                  // the number of terms
  const bool odd = df & 1;
  const double base = odd ? erfc(sqrt(y)) : 0.0;
  if (h == 0) return fmin(base, 1.0);
  const double a0 = odd ? 0.5 : 0.0;                                      // term i: y^(a0 + i) e^-y / Gamma(a0 + i + 1)
  const int top_i = (int)fmin(fmax(floor(y - a0), 0.0), (double)(h - 1));
  const double top = exp(((a0 + (double)top_i) * log(y) - y) - lgamma((a0 + (double)top_i) + 1.0));
  double sum = top, term = top;
  for (int i = top_i; i > 0; --i) {
    term = (term * (a0 + (double)i)) / y;
    sum += term;
    if (term < sum * 1e-20) break;
  }
  term = top;
  for (int i = top_i + 1; i < h; ++i) {
    term = (term * y) / (a0 + (double)i);
    sum += term;
    if (term < sum * 1e-20) break;
  }
  return fmin(base + sum, 1.0);
}

}  // namespace
#endif
