// scoary_categorical.hip -- categorical traits: the Pearson chi-square test of a gene against a label of up to eight
// classes (a 2 x K table per gene), with label permutations (spec S20 of DESIGN.md) and their Westfall-Young maxima
// (spec S22).
//
// The host numbers a trait's classes 1 .. K (0 = missing): a trait is its row of class codes (int16), the class sizes
// n_k over the isolates with a code, and the weights w_k = lcm{n_k > 0} / n_k as two 64-bit limbs.  Everything per
// gene is the vector a_k = |gene & class k|; the permutation null shuffles the codes over the isolates that have one
// -- spec S15's value shuffle, made by scoary_ranksum_perm_generate with the codes in the place of the ranks.
//
//   k_cat_observed  (observed)      a[8], m, X2, p and Cramer's V of every (trait, gene): k_ranksum's shape, a bit
//                                   walk over the tiled matrix with the trait's code row in LDS; not the hot path
//   k_cat_permute   (the hot path)  block = one stage of 64 permutations of one trait x a strided share of the gene
//                                   groups (CatStage, scoary_cat_planes.hpp).  The stage's 64 code rows stand in LDS
//                                   as class bit planes, a word per (class, 32 isolates, permutation); a lane is a
//                                   permutation, a wavefront takes four genes at a time and adds popc(gene word &
//                                   plane word) per class; behind a gene's last chunk of isolates the permuted table
//                                   is compared exactly with the observed one and the lanes' verdicts are counted
//   k_cat_maxt      (the hot path)  the same block (k_cat_permute_t<true>) with S22's statistic s of the same a_k
//                                   next to the comparison and a running maximum of it that a lane keeps in a register
//                                   over all gene groups its block walks; at the end of the block one 64-bit unsigned
//                                   atomic maximum per lane.  inv, ivm: k_cat_wy_prepare's (scoary_cat_wy.hip)
#include "scoary_cat_planes.hpp"
#include "scoary_chi2.hpp"
#include "scoary_common.hpp"

namespace {

// Observed table and statistic.  Block = 256 genes of one trait, a gene per lane; the trait's code row in LDS, a byte
// per isolate.  A lane counts the classes 1 .. 8 of its gene's isolates in eight 16-bit fields of two 64-bit words.
__global__ __launch_bounds__(256) void k_cat_observed(const uint4* __restrict__ tiled, int64_t Gp, int G, int N, int K,
                                                      const int16_t* __restrict__ codes,
                                                      const int32_t* __restrict__ nk, int32_t* __restrict__ d_a,
                                                      int32_t* __restrict__ d_m, double* __restrict__ d_x2,
                                                      double* __restrict__ d_p, double* __restrict__ d_v) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int t = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < N; i += 256)
    lds[i] = (unsigned char)min(max((int)codes[(int64_t)t * N + i], 0), kCatMaxClasses);
  __syncthreads();
  const int g = blockIdx.x * 256 + tid;
  if (g >= G) return;
  const int nw = (N + 31) / 32;
  uint64_t lo = 0, hi = 0;
  for (int q = 0; 4 * q < nw; ++q) {
    const uint4 x = tiled[(int64_t)q * Gp + g];
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int w = 4 * q + j;
      if (w >= nw) break;
      uint32_t bits = xs[j];
      if (32 * w + 32 > N) bits &= (1u << (N - 32 * w)) - 1u;
      while (bits) {
        const int c = lds[32 * w + __builtin_ctz(bits)];
        bits &= bits - 1u;
        if (c >= 5) hi += 1ull << (16 * (c - 5));
        else if (c >= 1) lo += 1ull << (16 * (c - 1));
      }
    }
  }
  int a[kCatMaxClasses], m = 0;
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k) {
    a[k] = (int)(((k < 4 ? lo : hi) >> (16 * (k & 3))) & 0xffffull);
    m += a[k];
  }
  int64_t n = 0;
  int kp = 0;
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k) {
    const int nkk = k < K ? nk[t * kCatMaxClasses + k] : 0;
    if (nkk > 0) n += nkk, ++kp;
  }
  // X2 in the form of spec S20: c_k = n a_k - m n_k exact, the sum in ascending k, every operation rounded on its own
  double x2 = 0.0, p = 1.0, v = 0.0;
  if (n >= 2 && m > 0 && m < n && kp >= 2) {
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < kCatMaxClasses; ++k) {
      const int nkk = k < K ? nk[t * kCatMaxClasses + k] : 0;
      if (nkk > 0) {
        const int64_t c = n * (int64_t)a[k] - (int64_t)m * (int64_t)nkk;
        sum += (double)(c * c) / (double)nkk;
      }
    }
    x2 = sum / ((double)m * (double)(n - m));
    p = chi2_tail(x2, kp - 1);
    v = sqrt(x2 / (double)n);
  }
  const int64_t o = (int64_t)t * G + g;
  int4* ao = reinterpret_cast<int4*>(d_a + o * kCatMaxClasses);
  ao[0] = int4{a[0], a[1], a[2], a[3]};
  ao[1] = int4{a[4], a[5], a[6], a[7]};
  d_m[o] = m;
  d_x2[o] = x2;
  d_p[o] = p;
  d_v[o] = v;
}

// The block of k_cat_permute (MAXT = false) and of k_cat_maxt (true): CatStage's, see scoary_cat_planes.hpp.  Behind
// the last chunk, per gene and lane: a_k = the count, the last non-empty class a = m - the others, d_k = a_k^2 -
// a_obs,k^2, H = sum d_k w_hi,k, Lo = sum d_k w_lo,k, and the permutation counts iff H + (Lo >> 64) >= 0 (spec S20:
// the sign of sum d_k L / n_k in integers).  MAXT, next to it: the class's term of s from the same a_k (n, m n_k,
// inv[k] and ivm[g] are wave-uniform) and mx = max(mx, s); mx lives across all gene groups the block walks, and at
// the end every lane whose permutation is < P combines it into maxs[t][64 s + lane]: one atomic per lane and block,
// never one per gene.  Permutations past P and genes >= G reach neither d_r nor maxs.
template <bool MAXT>
__device__ __forceinline__ void k_cat_permute_t(const uint32_t* tiled, int64_t Gp, int G, int N, const int16_t* rows,
                                                int64_t P, int S, const int32_t* aobs, const int32_t* nk,
                                                const uint64_t* wt, const double* d_inv, const double* d_ivm,
                                                int ranges, int lds_words, int32_t* d_r, double* d_maxs,
                                                int64_t maxs_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t* planes = reinterpret_cast<uint32_t*>(lds);
  const int t = blockIdx.y;
  const int32_t* nkt = nk + t * kCatMaxClasses;
  int klast = 0, n = 0;
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k)
    if (nkt[k] > 0) klast = k + 1, n += nkt[k];
  CatStage st(N, G, P, S, klast);
  const int lane = st.lane;
  const uint64_t* w = wt + (int64_t)t * 2 * kCatMaxClasses;
  const double* inv = d_inv + t * kCatMaxClasses;

  double mx = 0.0;
  for (int grp = st.rng; grp < st.ngroups; grp += ranges) {
    const int g0 = st.first_gene(grp);
    uint32_t cnt[kCatHold][kCatPlanes] = {};
    st.count_group(grp, planes, lds_words, tiled, Gp, rows, P, N, cnt);
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
        if constexpr (MAXT) tot = cat_wy_add(tot, n, a, m * nkt[k], inv[k]);
      }
      cat_hits(H + (Lo >> 64) >= 0, st.counted, lane, d_r + (int64_t)t * G + g);
      if constexpr (MAXT) mx = fmax(mx, tot * d_ivm[(int64_t)t * G + g]);
    }
  }
  if constexpr (MAXT)
    if (st.counted) cat_wy_combine(d_maxs + (int64_t)t * maxs_stride + (int64_t)st.s * 64 + lane, mx);
}

// The two kernels: plain functions around the template's instances, so that their names stay the ones the build's
// resource rules (which count instances by substring) and the timers know.
__global__ __launch_bounds__(kCatThreads) void k_cat_permute(const uint32_t* __restrict__ tiled, int64_t Gp, int G,
                                                             int N, const int16_t* __restrict__ rows, int64_t P, int S,
                                                             const int32_t* __restrict__ aobs,
                                                             const int32_t* __restrict__ nk,
                                                             const uint64_t* __restrict__ wt, int ranges,
                                                             int lds_words, int32_t* __restrict__ d_r) {
  k_cat_permute_t<false>(tiled, Gp, G, N, rows, P, S, aobs, nk, wt, nullptr, nullptr, ranges, lds_words, d_r, nullptr, 0);
}

__global__ __launch_bounds__(kCatThreads) void k_cat_maxt(const uint32_t* __restrict__ tiled, int64_t Gp, int G, int N,
                                                          const int16_t* __restrict__ rows, int64_t P, int S,
                                                          const int32_t* __restrict__ aobs,
                                                          const int32_t* __restrict__ nk,
                                                          const uint64_t* __restrict__ wt,
                                                          const double* __restrict__ d_inv,
                                                          const double* __restrict__ d_ivm, int ranges, int lds_words,
                                                          int32_t* __restrict__ d_r, double* __restrict__ d_maxs,
                                                          int64_t maxs_stride) {
  k_cat_permute_t<true>(tiled, Gp, G, N, rows, P, S, aobs, nk, wt, d_inv, d_ivm, ranges, lds_words, d_r, d_maxs,
                        maxs_stride);
}

}  // namespace

extern "C" {

int64_t scoary_categorical_max_classes(void) { return kCatMaxClasses; }

int scoary_categorical(scoary_handle h, const uint32_t* d_tiled, const int16_t* d_codes, const int32_t* d_nk, int64_t G,
                       int64_t T, int64_t N, int64_t K, int32_t* d_a, int32_t* d_m, double* d_x2, double* d_p,
                       double* d_v, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = cat_check(h, "scoary_categorical", d_tiled && d_codes && d_nk && d_a && d_m && d_x2 && d_p && d_v, G, T,
                         N, K, 1, 1))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  KernelTimer kt(h, s, "k_cat_observed");
  hipLaunchKernelGGL(k_cat_observed, dim3((unsigned)((G + 255) / 256), (unsigned)T), dim3(256),
                     (size_t)round_up(N, 16), s, reinterpret_cast<const uint4*>(d_tiled), scoary_tiled_genes(G), (int)G,
                     (int)N, (int)K, d_codes, d_nk, d_a, d_m, d_x2, d_p, d_v);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_permute_categorical(scoary_handle h, const uint32_t* d_tiled, const int16_t* d_rows, const int32_t* d_a,
                               const int32_t* d_nk, const uint64_t* d_w, int64_t G, int64_t T, int64_t N, int64_t P,
                               int32_t* d_r, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = cat_check(h, "scoary_permute_categorical", d_tiled && d_rows && d_a && d_nk && d_w && d_r, G, T, N, 1, 1,
                         P))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CatLaunch lp;
  if (int rc = cat_launch_plan(h, "scoary_permute_categorical", &k_cat_permute, kCatOptinPermute, G, T, N, P, &lp))
    return rc;
  KernelTimer kt(h, s, "k_cat_permute");
  hipLaunchKernelGGL(k_cat_permute, dim3((unsigned)(lp.S * lp.ranges), (unsigned)T), dim3(kCatThreads), (size_t)lp.lds,
                     s, d_tiled, scoary_tiled_genes(G), (int)G, (int)N, d_rows, P, (int)lp.S, d_a, d_nk, d_w,
                     (int)lp.ranges, (int)lp.lds_words, d_r);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_permute_cat_wy(scoary_handle h, const uint32_t* d_tiled, const int16_t* d_rows, const int32_t* d_a,
                          const int32_t* d_nk, const uint64_t* d_w, const double* d_inv, const double* d_ivm,
                          int64_t G, int64_t T, int64_t N, int64_t P, int32_t* d_r, double* d_maxs,
                          int64_t maxs_stride, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = cat_check(h, "scoary_permute_cat_wy",
                         d_tiled && d_rows && d_a && d_nk && d_w && d_inv && d_ivm && d_r && d_maxs &&
                             maxs_stride >= P,
                         G, T, N, 1, 1, P))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CatLaunch lp;
  if (int rc = cat_launch_plan(h, "scoary_permute_cat_wy", &k_cat_maxt, kCatOptinMaxt, G, T, N, P, &lp)) return rc;
  KernelTimer kt(h, s, "k_cat_maxt");
  hipLaunchKernelGGL(k_cat_maxt, dim3((unsigned)(lp.S * lp.ranges), (unsigned)T), dim3(kCatThreads), (size_t)lp.lds, s,
                     d_tiled, scoary_tiled_genes(G), (int)G, (int)N, d_rows, P, (int)lp.S, d_a, d_nk, d_w, d_inv, d_ivm,
                     (int)lp.ranges, (int)lp.lds_words, d_r, d_maxs, maxs_stride);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
