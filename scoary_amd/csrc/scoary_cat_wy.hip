// scoary_cat_wy.hip -- Westfall-Young single-step maxT over the statistics of the categorical traits: the chi-square
// test (S20) and the generalized CMH test (S21), each under its own statistic (spec S22 of DESIGN.md).
//
// A cell (gene g, permuted code row pi) of trait t has the table a_k the categorical kernels count.  Its statistic is
//     chi-square:  s = (sum over k of ((double)c_k (double)c_k) inv[t][k]) ivm[t][g],   c_k = n a_k - m n_k (int32),
//                  inv = 1 / n_k where n_k > 0, ivm = 1 / (m (n - m)) where the gene is testable, else 0 -- X2 in the
//                  reals, 0 in every row of an untestable gene
//     gcmh:        s = Q of the table under the gene's form, as k_gcmh_permute computes it
// and maxs[t][pi] = max over the genes of s.
//
//   k_cat_wy_prepare  (observed)      inv, ivm, s_obs = s of the observed table by the device function the hot path
//                                     uses, and thr = s_obs (1 - 1e-9), the comparison point of the chi-square maximum
//   k_cat_maxt        (the hot path)  k_cat_permute's block (scoary_categorical.hip: a stage of 64 permutations of one
//                                     trait x a strided share of the gene groups, class planes in LDS, a lane is a
//                                     permutation) with both reductions behind a gene's last chunk: the exceedance
//                                     count, decided in integers as there, and s into a running maximum that a lane
//                                     keeps in a register over all gene groups its block walks; at the end of the block
//                                     one 64-bit unsigned atomic maximum per lane on the bits of the non-negative
//                                     double -- independent of the order of the blocks
//   k_gcmh_maxt       (the hot path)  k_gcmh_permute's block (scoary_gcmh.hip) with the running maximum of the Q it
//                                     computes for the count, and the same atomic
#include "scoary_cat_planes.hpp"
#include "scoary_common.hpp"
#include "scoary_gcmh_form.hpp"

namespace {

constexpr double kCatWyBand = 1e-9;               // thr = s_obs (1 - band): S3's band

// One class of the chi-square statistic of a cell: tot + ((double)c (double)c) inv, c = n a - mnk exact in int32
// (|c| <= 16320^2 < 2^29), one rounding each for the square, the product and the sum.  The observed and the permuted
// cells go through this one function, so equal tables tie exactly; a class without a member adds +0.0.
__device__ __forceinline__ double cat_wy_add(double tot, int n, int a, int mnk, double inv) {
  const int c = n * a - mnk;
  const double e = (double)c * (double)c;
  const double term = e * inv;
  return tot + term;
}

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

// a lane's maximum into its column of maxs: the bits of a non-negative double order as unsigned integers
__device__ __forceinline__ void cat_wy_combine(double* __restrict__ col, double mx) {
  atomicMax(reinterpret_cast<unsigned long long*>(col), (unsigned long long)__double_as_longlong(mx));
}

// k_cat_permute's block, planes, walk and integer comparison (scoary_categorical.hip; restated here so that that
// kernel compiles exactly as it did): block = stage blockIdx.x % S (64 permutations) of trait blockIdx.y x the gene
// groups rng, rng + ranges, .. of kCatGroup genes; wavefront w of a group counts its genes kCatHold w .. + kCatHold - 1;
// a lane is a permutation.  Behind the last chunk, per gene and lane, next to the comparison of S20: the class's term
// of s from the same a_k (n, m n_k, inv[k] and ivm[g] are wave-uniform), and mx = max(mx, s).  mx lives across all
// gene groups the block walks; at the end every lane whose permutation is < P combines it into maxs[t][64 s + lane]:
// one atomic per lane and block, never one per gene.  Permutations past P and genes >= G reach neither d_r nor maxs.
__global__ __launch_bounds__(kCatThreads) void k_cat_maxt(const uint32_t* __restrict__ tiled, int64_t Gp, int G, int N,
                                                          const int16_t* __restrict__ rows, int64_t P, int S,
                                                          const int32_t* __restrict__ aobs,
                                                          const int32_t* __restrict__ nk,
                                                          const uint64_t* __restrict__ wt,
                                                          const double* __restrict__ d_inv,
                                                          const double* __restrict__ d_ivm, int ranges, int lds_words,
                                                          int32_t* __restrict__ d_r, double* __restrict__ d_maxs,
                                                          int64_t maxs_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t* planes = reinterpret_cast<uint32_t*>(lds);
  const int t = blockIdx.y, s = blockIdx.x % S, rng = blockIdx.x / S;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int32_t* nkt = nk + t * kCatMaxClasses;
  int klast = 0, n = 0;
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k)
    if (nkt[k] > 0) klast = k + 1, n += nkt[k];
  const bool wide = klast > 4;
  const int nf = wide ? kCatPlanes : 3;
  const uint64_t* w = wt + (int64_t)t * 2 * kCatMaxClasses;
  const double* inv = d_inv + t * kCatMaxClasses;
  const int nw = (N + 31) / 32;
  const int nchunks = (nw + kCatChunkWords - 1) / kCatChunkWords;
  const int ngroups = (G + kCatGroup - 1) / kCatGroup;
  const bool counted = (int64_t)s * 64 + lane < P;

  // chunk c -> LDS: wavefront iteration = (permutation p, word pair wp); lanes 0 and 1 write the two words of a plane
  auto load = [&](int c) {
    const int npairs = lds_words / 2;
    for (int it = wave; it < 64 * npairs; it += kCatWaves) {
      const int p = it / npairs, wp = it - p * npairs;
      const int64_t col = (int64_t)s * 64 + p;
      const int i = (c * kCatChunkWords + 2 * wp) * 32 + lane;
      int code = 0;
      if (i < N && col < P) code = rows[((int64_t)t * P + col) * N + i];
      for (int k = 0; k < nf; ++k) {
        const uint64_t m64 = __ballot(code == k + 1);
        if (lane < 2) planes[(k * lds_words + 2 * wp + lane) * 64 + p] = lane ? (uint32_t)(m64 >> 32) : (uint32_t)m64;
      }
    }
  };

  double mx = 0.0;
  bool loaded = false;
  for (int grp = rng; grp < ngroups; grp += ranges) {
    const int g0 = grp * kCatGroup + wave * kCatHold;
    uint32_t cnt[kCatHold][kCatPlanes];
#pragma unroll
    for (int j = 0; j < kCatHold; ++j)
#pragma unroll
      for (int k = 0; k < kCatPlanes; ++k) cnt[j][k] = 0u;
    for (int c = 0; c < nchunks; ++c) {
      if (!loaded || nchunks > 1) {
        __syncthreads();
        load(c);
        __syncthreads();
        loaded = true;
      }
      const int nquads = (min(kCatChunkWords, nw - c * kCatChunkWords) + 3) / 4;
      const uint4* tq = reinterpret_cast<const uint4*>(tiled) + (int64_t)c * (kCatChunkWords / 4) * Gp + g0;
      if (wide) cat_count<kCatPlanes>(planes + lane, lds_words, tq, Gp, nquads, cnt);
      else cat_count<3>(planes + lane, lds_words, tq, Gp, nquads, cnt);
    }
#pragma unroll
    for (int j = 0; j < kCatHold; ++j) {
      const int g = g0 + j;
      if (g >= G) break;
      const int32_t* ao = aobs + ((int64_t)t * G + g) * kCatMaxClasses;
      int m = 0;
#pragma unroll
      for (int k = 0; k < kCatMaxClasses; ++k) m += ao[k];
      __int128 H = 0, Lo = 0;
      int sum = 0;
      double tot = 0.0;
#pragma unroll 1                                   // (unrolled, the sixteen limbs wait in SGPRs across the count)
      for (int k = 0; k < klast; ++k) {
        int a;
        if (k < klast - 1) {
          a = (int)cnt[j][0];
#pragma unroll
          for (int x = 1; x < kCatPlanes; ++x) a = k == x ? (int)cnt[j][x] : a;
          sum += a;
        } else {
          a = m - sum;
        }
        const int64_t o = ao[k];
        const int64_t d = (int64_t)a * a - o * o;
        H += cat_mul(d, w[2 * k + 1]);
        Lo += cat_mul(d, w[2 * k]);
        tot = cat_wy_add(tot, n, a, m * nkt[k], inv[k]);
      }
      const bool ge = H + (Lo >> 64) >= 0;
      const int hits = __popcll(__ballot(ge && counted));
      if (lane == 0 && hits) atomicAdd(d_r + (int64_t)t * G + g, hits);
      mx = fmax(mx, tot * d_ivm[(int64_t)t * G + g]);
    }
  }
  if (counted) cat_wy_combine(d_maxs + (int64_t)t * maxs_stride + (int64_t)s * 64 + lane, mx);
}

// k_gcmh_permute's block, planes, walk, quadratic and count (scoary_gcmh.hip; restated here so that that kernel
// compiles exactly as it did), with mx = max(mx, Q) next to the count and k_cat_maxt's combine at the end of the
// block.  A form of zeros (df = 0) has Q = 0, the identity of the maximum.
__global__ __launch_bounds__(kCatThreads) void k_gcmh_maxt(const uint32_t* __restrict__ tiled, int64_t Gp, int G, int N,
                                                           const int16_t* __restrict__ rows, int64_t P, int S,
                                                           const double* __restrict__ form,
                                                           const double* __restrict__ thr,
                                                           const int32_t* __restrict__ nk, int ranges, int lds_words,
                                                           int32_t* __restrict__ d_r, double* __restrict__ d_maxs,
                                                           int64_t maxs_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t* planes = reinterpret_cast<uint32_t*>(lds);
  const int t = blockIdx.y, s = blockIdx.x % S, rng = blockIdx.x / S;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool wide = gcmh_klast(nk + t * kCatMaxClasses, kCatMaxClasses) > 4;
  const int nf = wide ? kCatPlanes : 3;
  const int nw = (N + 31) / 32;
  const int nchunks = (nw + kCatChunkWords - 1) / kCatChunkWords;
  const int ngroups = (G + kCatGroup - 1) / kCatGroup;
  const bool counted = (int64_t)s * 64 + lane < P;

  // chunk c -> LDS: wavefront iteration = (permutation p, word pair wp); lanes 0 and 1 write the two words of a plane
  auto load = [&](int c) {
    const int npairs = lds_words / 2;
    for (int it = wave; it < 64 * npairs; it += kCatWaves) {
      const int p = it / npairs, wp = it - p * npairs;
      const int64_t col = (int64_t)s * 64 + p;
      const int i = (c * kCatChunkWords + 2 * wp) * 32 + lane;
      int code = 0;
      if (i < N && col < P) code = rows[((int64_t)t * P + col) * N + i];
      for (int k = 0; k < nf; ++k) {
        const uint64_t m64 = __ballot(code == k + 1);
        if (lane < 2) planes[(k * lds_words + 2 * wp + lane) * 64 + p] = lane ? (uint32_t)(m64 >> 32) : (uint32_t)m64;
      }
    }
  };

  double mx = 0.0;
  bool loaded = false;
  for (int grp = rng; grp < ngroups; grp += ranges) {
    const int g0 = grp * kCatGroup + wave * kCatHold;
    uint32_t cnt[kCatHold][kCatPlanes];
#pragma unroll
    for (int j = 0; j < kCatHold; ++j)
#pragma unroll
      for (int k = 0; k < kCatPlanes; ++k) cnt[j][k] = 0u;
    for (int c = 0; c < nchunks; ++c) {
      if (!loaded || nchunks > 1) {
        __syncthreads();
        load(c);
        __syncthreads();
        loaded = true;
      }
      const int nquads = (min(kCatChunkWords, nw - c * kCatChunkWords) + 3) / 4;
      const uint4* tq = reinterpret_cast<const uint4*>(tiled) + (int64_t)c * (kCatChunkWords / 4) * Gp + g0;
      if (wide) cat_count<kCatPlanes>(planes + lane, lds_words, tq, Gp, nquads, cnt);
      else cat_count<3>(planes + lane, lds_words, tq, Gp, nquads, cnt);
    }
#pragma unroll 1                                     // (unrolled, four forms wait in SGPRs across the count)
    for (int j = 0; j < kCatHold; ++j) {
      const int g = g0 + j;
      if (g >= G) break;
      const int64_t o = (int64_t)t * G + g;
      const double* fo = form + o * kGcmhForm;         // wave-uniform
      uint32_t a[kCatPlanes];
#pragma unroll
      for (int k = 0; k < kCatPlanes; ++k) {
        a[k] = cnt[0][k];
#pragma unroll
        for (int x = 1; x < kCatHold; ++x) a[k] = j == x ? cnt[x][k] : a[k];
      }
      const double q = wide ? gcmh_q<kCatPlanes>(fo, a) : gcmh_q<3>(fo, a);
      const bool ge = q >= thr[o];
      const int hits = __popcll(__ballot(ge && counted));
      if (lane == 0 && hits) atomicAdd(d_r + o, hits);
      mx = fmax(mx, q);
    }
  }
  if (counted) cat_wy_combine(d_maxs + (int64_t)t * maxs_stride + (int64_t)s * 64 + lane, mx);
}

// the checks the entry points share: cat_check's of scoary_categorical.hip (S = 1) and gcmh_check's of scoary_gcmh.hip
int cwy_check(scoary_handle h, const char* what, bool ok, int64_t G, int64_t T, int64_t N, int64_t K, int64_t S,
              int64_t P) {
  if (int rc = check_args(h, what, ok && G >= 1 && T >= 1 && N >= 1 && S >= 1 && P >= 1)) return rc;
  if (K < 1 || K > kCatMaxClasses)
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": K outside [1, scoary_categorical_max_classes()]");
  if (S > scoary_perm_max_strata())
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": more strata than scoary_perm_max_strata()");
  if (N > scoary_ranksum_max_isolates())
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": more isolates than scoary_ranksum_max_isolates()");
  if (T > 65535 || G > 0x7fffffffLL - 256 || P > 0x7fffffffLL)
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": T > 65535, G >= 2^31 or P >= 2^31");
  return SCOARY_OK;
}

// k_cat_permute's launch: the LDS for the seven planes of eight classes (the opt-in above 64 KB is asked for at every
// such launch -- a host call per batch of permutations -- so that the handle keeps no state for it) and the gene
// ranges per stage: enough blocks for four rounds over the CUs, where the gene groups allow it
struct CatWyLaunch {
  int64_t lds_words, lds, S, ranges;
};
template <typename Kernel>
int cwy_launch_plan(scoary_handle h, const char* what, Kernel kernel, int64_t G, int64_t T, int64_t N, int64_t P,
                    CatWyLaunch* out) {
  out->lds_words = round_up(std::min<int64_t>((N + 31) / 32, kCatChunkWords), 4);
  out->lds = kCatPlanes * out->lds_words * 256;
  if (out->lds > 64 * 1024)
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kCatPlanes * kCatChunkWords * 256));
  const int64_t ngroups = (G + kCatGroup - 1) / kCatGroup;
  out->S = (P + 63) / 64;
  out->ranges =
      std::min<int64_t>(ngroups, std::max<int64_t>(1, (4 * (int64_t)h->num_cu + out->S * T - 1) / (out->S * T)));
  if (out->S * out->ranges > 0x7fffffffLL) return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": grid too large");
  return SCOARY_OK;
}

}  // namespace

extern "C" {

int scoary_cat_wy_prepare(scoary_handle h, const int32_t* d_a, const int32_t* d_nk, int64_t G, int64_t T, int64_t K,
                          double* d_inv, double* d_ivm, double* d_sobs, double* d_thr, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = cwy_check(h, "scoary_cat_wy_prepare", d_a && d_nk && d_inv && d_ivm && d_sobs && d_thr, G, T, 1, K, 1, 1))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  KernelTimer kt(h, s, "k_cat_wy_prepare");
  hipLaunchKernelGGL(k_cat_wy_prepare, dim3((unsigned)((G + 255) / 256), (unsigned)T), dim3(256), 0, s, d_a, d_nk,
                     (int)G, (int)K, d_inv, d_ivm, d_sobs, d_thr);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_permute_cat_wy(scoary_handle h, const uint32_t* d_tiled, const int16_t* d_rows, const int32_t* d_a,
                          const int32_t* d_nk, const uint64_t* d_w, const double* d_inv, const double* d_ivm,
                          int64_t G, int64_t T, int64_t N, int64_t P, int32_t* d_r, double* d_maxs,
                          int64_t maxs_stride, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = cwy_check(h, "scoary_permute_cat_wy",
                         d_tiled && d_rows && d_a && d_nk && d_w && d_inv && d_ivm && d_r && d_maxs &&
                             maxs_stride >= P,
                         G, T, N, 1, 1, P))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CatWyLaunch lp;
  if (int rc = cwy_launch_plan(h, "scoary_permute_cat_wy", &k_cat_maxt, G, T, N, P, &lp)) return rc;
  KernelTimer kt(h, s, "k_cat_maxt");
  hipLaunchKernelGGL(k_cat_maxt, dim3((unsigned)(lp.S * lp.ranges), (unsigned)T), dim3(kCatThreads), (size_t)lp.lds, s,
                     d_tiled, scoary_tiled_genes(G), (int)G, (int)N, d_rows, P, (int)lp.S, d_a, d_nk, d_w, d_inv, d_ivm,
                     (int)lp.ranges, (int)lp.lds_words, d_r, d_maxs, maxs_stride);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_permute_gcmh_wy(scoary_handle h, const uint32_t* d_tiled, const int16_t* d_rows, const double* d_form,
                           const double* d_thr, const int32_t* d_nk, int64_t G, int64_t T, int64_t N, int64_t P,
                           int32_t* d_r, double* d_maxs, int64_t maxs_stride, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = cwy_check(h, "scoary_permute_gcmh_wy",
                         d_tiled && d_rows && d_form && d_thr && d_nk && d_r && d_maxs && maxs_stride >= P, G, T, N, 1,
                         1, P))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CatWyLaunch lp;
  if (int rc = cwy_launch_plan(h, "scoary_permute_gcmh_wy", &k_gcmh_maxt, G, T, N, P, &lp)) return rc;
  KernelTimer kt(h, s, "k_gcmh_maxt");
  hipLaunchKernelGGL(k_gcmh_maxt, dim3((unsigned)(lp.S * lp.ranges), (unsigned)T), dim3(kCatThreads), (size_t)lp.lds,
                     s, d_tiled, scoary_tiled_genes(G), (int)G, (int)N, d_rows, P, (int)lp.S, d_form, d_thr, d_nk,
                     (int)lp.ranges, (int)lp.lds_words, d_r, d_maxs, maxs_stride);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
