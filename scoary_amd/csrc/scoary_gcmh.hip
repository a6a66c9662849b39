// scoary_gcmh.hip -- categorical traits over strata: the generalized Cochran-Mantel-Haenszel test of a gene against a
// label of up to eight classes (a 2 x K x S table per gene), with label permutations within the strata (spec S21 of
// DESIGN.md) and their Westfall-Young maxima (spec S22).
//
// A trait is its row of class codes (int16, 1 .. K, 0 = missing), its pooled class sizes n_k and the per-stratum
// class sizes n_sk; the strata are the CMH entry points' (the stratum of every isolate and the isolates by stratum).
// A shuffle of the codes within the strata keeps every per-stratum margin -- the gene's m_s, n_sk, n_s -- so the
// expectation E and the covariance V of the pooled counts a_k = |gene & class k| are constants of the (trait, gene):
// the observed kernel factorises V once into the FORM of the (trait, gene), 35 doubles, and a permuted labelling
// enters the statistic through its a_k alone,
//     Q = sum_j y_j^2 invp_j,   y_i = (a_i - E_i) - sum_{j < i} f_ij y_j.
//
//   k_gcmh_observed  (observed)      a[8], m, E[8], the form, Q, df, p and the threshold of every (trait, gene):
//                                    k_vanelteren's walk over the segment table with the trait's code row in LDS, E and
//                                    V folded at every change of stratum, LDL' without pivoting; not the hot path
//   k_gcmh_permute   (the hot path)  k_cat_permute's blocks, class planes and popcount walk (CatStage,
//                                    scoary_cat_planes.hpp); behind a gene's last chunk of isolates a lane computes its
//                                    permutation's Q from the form (wave-uniform reads) and the lanes with Q >= thr are
//                                    counted
//   k_gcmh_maxt      (the hot path)  the same block (k_gcmh_permute_t<true>) with a lane's running maximum of the Q it
//                                    computes for the count, and k_cat_maxt's atomic at the end of the block
#include "scoary_cat_planes.hpp"
#include "scoary_chi2.hpp"
#include "scoary_common.hpp"
#include "scoary_gcmh_form.hpp"

namespace {

constexpr int kGcmhThreads = 256;                 // k_gcmh_observed: a gene per lane
constexpr double kGcmhTheta = 1e-8;               // pivot j is skipped iff p_j <= theta V_jj (measured, DESIGN S21)
constexpr double kGcmhTau = 1e-6;                 // thr = Q_obs (1 - tau): S10's band

// Observed statistic.  Block = 256 genes of one trait, a gene per lane; the trait's code row in LDS, a byte per
// isolate, clamped into [0, 8].  The lane walks the segment table as k_vanelteren does (stratum and word clamped: a
// bad plan gives wrong numbers, never a wild access): per segment m_s and the pooled class counts (eight 16-bit fields)
// grow by the gene's labelled isolates of that (stratum, word), and every change of stratum folds m_s into E and V --
// ascending s, the order S21 fixes.  Strata without a member have no segment and add nothing.
__global__ __launch_bounds__(kGcmhThreads) void k_gcmh_observed(
    const uint4* __restrict__ tiled, int64_t Gp, int G, int N, int K, int S, const int16_t* __restrict__ codes,
    const int32_t* __restrict__ nk, const int32_t* __restrict__ nsk, const CmhSegments* __restrict__ segs,
    int32_t* __restrict__ d_a, int32_t* __restrict__ d_m, double* __restrict__ d_e, double* __restrict__ d_form,
    double* __restrict__ d_q, int32_t* __restrict__ d_df, double* __restrict__ d_p, double* __restrict__ d_thr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int t = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < N; i += kGcmhThreads)
    lds[i] = (unsigned char)min(max((int)codes[(int64_t)t * N + i], 0), kCatMaxClasses);
  __syncthreads();
  const int g = blockIdx.x * kGcmhThreads + tid;
  if (g >= G) return;
  const int nw = (N + 31) / 32;

  double E[kCatMaxClasses], V[kCatPlanes][kCatPlanes];
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k) E[k] = 0.0;
#pragma unroll
  for (int j = 0; j < kCatPlanes; ++j)
#pragma unroll
    for (int k = 0; k <= j; ++k) V[j][k] = 0.0;
  uint64_t lo = 0, hi = 0;
  int m = 0, ms = 0;
  auto fold = [&](int s) {
    const int32_t* row = nsk + ((int64_t)t * S + s) * kCatMaxClasses;        // wave-uniform
    int64_t r[kCatMaxClasses], n = 0;
#pragma unroll
    for (int k = 0; k < kCatMaxClasses; ++k) {
      r[k] = k < K ? max(row[k], 0) : 0;
      n += r[k];
    }
    if (n >= 1) {
#pragma unroll
      for (int k = 0; k < kCatMaxClasses; ++k) E[k] += (double)((int64_t)ms * r[k]) / (double)n;
    }
    if (n >= 2) {
      const double c = ((double)ms * (double)(n - ms)) / (((double)n * (double)n) * (double)(n - 1));
#pragma unroll
      for (int j = 0; j < kCatPlanes; ++j)
#pragma unroll
        for (int k = 0; k <= j; ++k) V[j][k] += c * (double)((j == k ? n * r[j] : 0) - r[j] * r[k]);
    }
    m += ms;
    ms = 0;
  };
  const int nseg = min((int)segs->count, N);
  int cur_s = -1, cur_q = -1;
  uint4 gq = make_uint4(0, 0, 0, 0);
  for (int i = 0; i < nseg; ++i) {
    const uint2 sg = segs->seg[i];                                            // wave-uniform
    const int s = min((int)(sg.x >> 16), S - 1), w = min((int)(sg.x & 0xffffu), nw - 1);
    if (s != cur_s) {
      if (cur_s >= 0) fold(cur_s);
      cur_s = s;
    }
    if ((w >> 2) != cur_q) {
      cur_q = w >> 2;
      gq = tiled[(int64_t)cur_q * Gp + g];
    }
    const int c4 = w & 3;
    uint32_t bits = (c4 == 0 ? gq.x : c4 == 1 ? gq.y : c4 == 2 ? gq.z : gq.w) & sg.y;
    if (32 * w + 32 > N) bits &= (1u << (N - 32 * w)) - 1u;
    while (bits) {
      const int c = lds[32 * w + __builtin_ctz(bits)];
      bits &= bits - 1u;
      if (c >= 5) hi += 1ull << (16 * (c - 5));
      else if (c >= 1) lo += 1ull << (16 * (c - 1));
      ms += c >= 1;
    }
  }
  if (cur_s >= 0) fold(cur_s);

  // LDL' without pivoting in class order over the contrasts j < nc = klast - 1; the rows from nc on count as zero
  const int nc = gcmh_klast(nk + t * kCatMaxClasses, K) - 1;
  double form[kGcmhForm], u[kCatPlanes][kCatPlanes];
  int df = 0;
#pragma unroll
  for (int j = 0; j < kCatPlanes; ++j) {
#pragma unroll
    for (int k = 0; k < j; ++k) {
      double x = j < nc ? V[j][k] : 0.0;
#pragma unroll
      for (int l = 0; l < k; ++l) x = x - u[j][l] * form[kCatPlanes + gcmh_f(k, l)];
      u[j][k] = x;
      form[kCatPlanes + gcmh_f(j, k)] = x * form[kCatPlanes + kGcmhMults + k];
    }
    const double vjj = j < nc ? V[j][j] : 0.0;
    double p = vjj;
#pragma unroll
    for (int k = 0; k < j; ++k) p = p - u[j][k] * form[kCatPlanes + gcmh_f(j, k)];
    const bool keep = !(p <= kGcmhTheta * vjj);
    form[kCatPlanes + kGcmhMults + j] = keep ? 1.0 / p : 0.0;
    df += keep;
    form[j] = j < nc ? E[j] : 0.0;
  }
  uint32_t a[kCatMaxClasses];
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k) a[k] = (uint32_t)(((k < 4 ? lo : hi) >> (16 * (k & 3))) & 0xffffull);
  const uint32_t a7[kCatPlanes] = {a[0], a[1], a[2], a[3], a[4], a[5], a[6]};
  const double q = gcmh_q<kCatPlanes>(form, a7);
  const double p = df > 0 ? chi2_tail(q, df) : 1.0;

  const int64_t o = (int64_t)t * G + g;
  int4* ao = reinterpret_cast<int4*>(d_a + o * kCatMaxClasses);
  ao[0] = int4{(int)a[0], (int)a[1], (int)a[2], (int)a[3]};
  ao[1] = int4{(int)a[4], (int)a[5], (int)a[6], (int)a[7]};
  d_m[o] = m;
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k) d_e[o * kCatMaxClasses + k] = E[k];
#pragma unroll
  for (int x = 0; x < kGcmhForm; ++x) d_form[o * kGcmhForm + x] = form[x];
  d_q[o] = q;
  d_df[o] = df;
  d_p[o] = p;
  d_thr[o] = q * (1.0 - kGcmhTau);
}

// The block of k_gcmh_permute (MAXT = false) and of k_gcmh_maxt (true): CatStage's, see scoary_cat_planes.hpp.  Behind
// the last chunk, per gene and lane: Q of the counts of the classes before the last non-empty one -- that one needs no
// plane and no count -- under the gene's form, read wave-uniformly (three contrasts while the last non-empty class is
// at most the fourth, else seven), and the permutation counts iff Q >= thr.  A form of zeros (df = 0) has Q = 0 = thr
// by itself.  MAXT: mx = max(mx, Q) next to the count -- Q = 0 is the identity of the maximum -- kept across all gene
// groups the block walks, and one combine per lane whose permutation is < P at the end of the block.
template <bool MAXT>
__device__ __forceinline__ void k_gcmh_permute_t(const uint32_t* tiled, int64_t Gp, int G, int N, const int16_t* rows,
                                                 int64_t P, int S, const double* form, const double* thr,
                                                 const int32_t* nk, int ranges, int lds_words, int32_t* d_r,
                                                 double* d_maxs, int64_t maxs_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t* planes = reinterpret_cast<uint32_t*>(lds);
  const int t = blockIdx.y;
  CatStage st(N, G, P, S, gcmh_klast(nk + t * kCatMaxClasses, kCatMaxClasses));
  const int lane = st.lane;

  double mx = 0.0;
  for (int grp = st.rng; grp < st.ngroups; grp += ranges) {
    const int g0 = st.first_gene(grp);
    uint32_t cnt[kCatHold][kCatPlanes] = {};
    st.count_group(grp, planes, lds_words, tiled, Gp, rows, P, N, cnt);
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
      const double q = st.wide ? gcmh_q<kCatPlanes>(fo, a) : gcmh_q<3>(fo, a);
      cat_hits(q >= thr[o], st.counted, lane, d_r + o);
      if constexpr (MAXT) mx = fmax(mx, q);
    }
  }
  if constexpr (MAXT)
    if (st.counted) cat_wy_combine(d_maxs + (int64_t)t * maxs_stride + (int64_t)st.s * 64 + lane, mx);
}

// The two kernels: plain functions around the template's instances, so that their names stay the ones the build's
// resource rules (which count instances by substring) and the timers know.
__global__ __launch_bounds__(kCatThreads) void k_gcmh_permute(const uint32_t* __restrict__ tiled, int64_t Gp, int G,
                                                              int N, const int16_t* __restrict__ rows, int64_t P, int S,
                                                              const double* __restrict__ form,
                                                              const double* __restrict__ thr,
                                                              const int32_t* __restrict__ nk, int ranges,
                                                              int lds_words, int32_t* __restrict__ d_r) {
  k_gcmh_permute_t<false>(tiled, Gp, G, N, rows, P, S, form, thr, nk, ranges, lds_words, d_r, nullptr, 0);
}

__global__ __launch_bounds__(kCatThreads) void k_gcmh_maxt(const uint32_t* __restrict__ tiled, int64_t Gp, int G, int N,
                                                           const int16_t* __restrict__ rows, int64_t P, int S,
                                                           const double* __restrict__ form,
                                                           const double* __restrict__ thr,
                                                           const int32_t* __restrict__ nk, int ranges, int lds_words,
                                                           int32_t* __restrict__ d_r, double* __restrict__ d_maxs,
                                                           int64_t maxs_stride) {
  k_gcmh_permute_t<true>(tiled, Gp, G, N, rows, P, S, form, thr, nk, ranges, lds_words, d_r, d_maxs, maxs_stride);
}

}  // namespace

extern "C" {

int64_t scoary_gcmh_form_doubles(void) { return kGcmhForm; }

int scoary_gcmh(scoary_handle h, const uint32_t* d_tiled, const int16_t* d_codes, const int32_t* d_nk,
                const int32_t* d_nsk, const uint16_t* d_strata, const int32_t* d_members, int64_t G, int64_t T,
                int64_t N, int64_t K, int64_t S, int32_t* d_a, int32_t* d_m, double* d_e, double* d_form, double* d_q,
                int32_t* d_df, double* d_p, double* d_thr, void* d_scratch, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = cat_check(h, "scoary_gcmh", d_tiled && d_codes && d_nk && d_nsk && d_strata && d_members && d_a &&
                                                d_m && d_e && d_form && d_q && d_df && d_p && d_thr && d_scratch,
                         G, T, N, K, S, 1))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = scoary_cmh_segments_launch(h, s, d_strata, d_members, N, S, d_scratch, "k_cmh_segments")) return rc;
  KernelTimer kt(h, s, "k_gcmh_observed");
  hipLaunchKernelGGL(k_gcmh_observed, dim3((unsigned)((G + kGcmhThreads - 1) / kGcmhThreads), (unsigned)T),
                     dim3(kGcmhThreads), (size_t)round_up(N, 16), s, reinterpret_cast<const uint4*>(d_tiled),
                     scoary_tiled_genes(G), (int)G, (int)N, (int)K, (int)S, d_codes, d_nk, d_nsk,
                     static_cast<const CmhSegments*>(d_scratch), d_a, d_m, d_e, d_form, d_q, d_df, d_p, d_thr);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_permute_gcmh(scoary_handle h, const uint32_t* d_tiled, const int16_t* d_rows, const double* d_form,
                        const double* d_thr, const int32_t* d_nk, int64_t G, int64_t T, int64_t N, int64_t P,
                        int32_t* d_r, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = cat_check(h, "scoary_permute_gcmh", d_tiled && d_rows && d_form && d_thr && d_nk && d_r, G, T, N, 1, 1,
                         P))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CatLaunch lp;
  if (int rc = cat_launch_plan(h, "scoary_permute_gcmh", &k_gcmh_permute, kGcmhOptinPermute, G, T, N, P, &lp)) return rc;
  KernelTimer kt(h, s, "k_gcmh_permute");
  hipLaunchKernelGGL(k_gcmh_permute, dim3((unsigned)(lp.S * lp.ranges), (unsigned)T), dim3(kCatThreads),
                     (size_t)lp.lds, s, d_tiled, scoary_tiled_genes(G), (int)G, (int)N, d_rows, P, (int)lp.S, d_form,
                     d_thr, d_nk, (int)lp.ranges, (int)lp.lds_words, d_r);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_permute_gcmh_wy(scoary_handle h, const uint32_t* d_tiled, const int16_t* d_rows, const double* d_form,
                           const double* d_thr, const int32_t* d_nk, int64_t G, int64_t T, int64_t N, int64_t P,
                           int32_t* d_r, double* d_maxs, int64_t maxs_stride, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = cat_check(h, "scoary_permute_gcmh_wy",
                         d_tiled && d_rows && d_form && d_thr && d_nk && d_r && d_maxs && maxs_stride >= P, G, T, N, 1,
                         1, P))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CatLaunch lp;
  if (int rc = cat_launch_plan(h, "scoary_permute_gcmh_wy", &k_gcmh_maxt, kGcmhOptinMaxt, G, T, N, P, &lp)) return rc;
  KernelTimer kt(h, s, "k_gcmh_maxt");
  hipLaunchKernelGGL(k_gcmh_maxt, dim3((unsigned)(lp.S * lp.ranges), (unsigned)T), dim3(kCatThreads), (size_t)lp.lds,
                     s, d_tiled, scoary_tiled_genes(G), (int)G, (int)N, d_rows, P, (int)lp.S, d_form, d_thr, d_nk,
                     (int)lp.ranges, (int)lp.lds_words, d_r, d_maxs, maxs_stride);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
