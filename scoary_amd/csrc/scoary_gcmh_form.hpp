// scoary_gcmh_form.hpp -- the form of a (trait, gene) of the generalized CMH test (spec S21) and the quadratic Q of a
// table under it, which k_gcmh_observed and the hot kernels of scoary_gcmh.hip (specs S21 and S22) compute by this one
// text, so that an identical table gives identical bits.
#ifndef SCOARY_GCMH_FORM_HPP
#define SCOARY_GCMH_FORM_HPP
#include "scoary_cat_planes.hpp"

namespace {

constexpr int kGcmhMults = kCatPlanes * (kCatPlanes - 1) / 2;
constexpr int kGcmhForm = kCatPlanes + kGcmhMults + kCatPlanes;       // E[7], f[21], invp[7]

__host__ __device__ constexpr int gcmh_f(int i, int j) { return i * (i - 1) / 2 + j; }   // f_ij, j < i

// Q of the counts a under a form, over the first NC contrasts (the others add +0.0 where their form entries are 0:
// the same bits for every NC that covers the trait's contrasts).  fp64, every operation rounded on its own.
template <int NC>
__device__ __forceinline__ double gcmh_q(const double* __restrict__ form, const uint32_t (&a)[kCatPlanes]) {
  double y[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    double x = (double)a[i] - form[i];
#pragma unroll
    for (int j = 0; j < i; ++j) x = x - form[kCatPlanes + gcmh_f(i, j)] * y[j];
    y[i] = x;
  }
  double q = 0.0;
#pragma unroll
  for (int j = 0; j < NC; ++j) q += (y[j] * y[j]) * form[kCatPlanes + kGcmhMults + j];
  return q;
}

// the last class (1-based) with n_k > 0 among the first K; wave-uniform
__device__ __forceinline__ int gcmh_klast(const int32_t* __restrict__ nkt, int K) {
  int klast = 0;
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k)
    if (k < K && nkt[k] > 0) klast = k + 1;
  return klast;
}

}  // namespace
#endif
