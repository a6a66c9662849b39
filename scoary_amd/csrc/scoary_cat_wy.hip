// scoary_cat_wy.hip -- Westfall-Young single-step maxT over the statistics of the categorical traits (spec S22 of
// DESIGN.md): the observed side.  The hot kernels live with the kernels they extend -- k_cat_maxt in
// scoary_categorical.hip, k_gcmh_maxt in scoary_gcmh.hip -- and share their block through scoary_cat_planes.hpp.
//
// A cell (gene g, permuted code row pi) of trait t has the table a_k the categorical kernels count.  Its statistic is
//     chi-square:  s = (sum over k of ((double)c_k (double)c_k) inv[t][k]) ivm[t][g],   c_k = n a_k - m n_k (int32),
//                  inv = 1 / n_k where n_k > 0, ivm = 1 / (m (n - m)) where the gene is testable, else 0 -- X2 in the
//                  reals, 0 in every row of an untestable gene
//     gcmh:        s = Q of the table under the gene's form, as k_gcmh_permute computes it: k_gcmh_observed wrote its
//                  observed value and comparison point, nothing is prepared here
// and maxs[t][pi] = max over the genes of s.
//
//   k_cat_wy_prepare  (observed)      inv, ivm, s_obs = s of the observed table by the device function the hot path
//                                     uses (cat_wy_add), and thr = s_obs (1 - 1e-9), the comparison point of the
//                                     chi-square maximum
#include "scoary_cat_planes.hpp"
#include "scoary_common.hpp"
#include "scoary_gcmh_form.hpp"

namespace {

constexpr double kCatWyBand = 1e-9;               // thr = s_obs (1 - band): S3's band

// inv of the trait (block column 0 writes it), and ivm, s_obs and thr of the genes of a block of 256 of trait
// blockIdx.y.  n, K' and the testable rule are k_cat_observed's; the divisions are fp64, correctly rounded.
__global__ __launch_bounds__(256) void k_cat_wy_prepare(const int32_t* __restrict__ aobs,
                                                        const int32_t* __restrict__ nk, int G, int K,
                                                        double* __restrict__ d_inv, double* __restrict__ d_ivm,
                                                        double* __restrict__ d_sobs, double* __restrict__ d_thr) {
  const int t = blockIdx.y, tid = threadIdx.x;
  int nkk[kCatMaxClasses], n = 0, kp = 0;
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k) {
    nkk[k] = k < K ? max(nk[t * kCatMaxClasses + k], 0) : 0;
    n += nkk[k];
    kp += nkk[k] > 0;
  }
  if (blockIdx.x == 0 && tid < kCatMaxClasses) {
    const int x = tid < K ? max(nk[t * kCatMaxClasses + tid], 0) : 0;
    d_inv[t * kCatMaxClasses + tid] = x > 0 ? 1.0 / (double)x : 0.0;
  }
  const int g = blockIdx.x * 256 + tid;
  if (g >= G) return;
  const int64_t o = (int64_t)t * G + g;
  const int4* ao = reinterpret_cast<const int4*>(aobs + o * kCatMaxClasses);
  const int4 a0 = ao[0], a1 = ao[1];
  const int a[kCatMaxClasses] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  int m = 0;
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k) m += a[k];
  const bool testable = n >= 2 && m > 0 && m < n && kp >= 2;
  const double ivm = testable ? 1.0 / ((double)m * (double)(n - m)) : 0.0;
  double tot = 0.0;
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k)
    tot = cat_wy_add(tot, n, a[k], m * nkk[k], nkk[k] > 0 ? 1.0 / (double)nkk[k] : 0.0);
  const double s = tot * ivm;
  d_ivm[o] = ivm;
  d_sobs[o] = s;
  d_thr[o] = s * (1.0 - kCatWyBand);
}

}  // namespace

extern "C" {

int scoary_cat_wy_prepare(scoary_handle h, const int32_t* d_a, const int32_t* d_nk, int64_t G, int64_t T, int64_t K,
                          double* d_inv, double* d_ivm, double* d_sobs, double* d_thr, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = cat_check(h, "scoary_cat_wy_prepare", d_a && d_nk && d_inv && d_ivm && d_sobs && d_thr, G, T, 1, K, 1, 1))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  KernelTimer kt(h, s, "k_cat_wy_prepare");
  hipLaunchKernelGGL(k_cat_wy_prepare, dim3((unsigned)((G + 255) / 256), (unsigned)T), dim3(256), 0, s, d_a, d_nk,
                     (int)G, (int)K, d_inv, d_ivm, d_sobs, d_thr);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
