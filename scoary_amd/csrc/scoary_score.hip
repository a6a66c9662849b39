// scoary_score.hip -- covariate-adjusted score tests (spec S24 of DESIGN.md): the Rao score test of a gene in a
// logistic model of a binary trait, or in a linear model of a measured trait, next to up to eight covariates.
//
// The host fits the null model (trait on intercept and covariates, no gene) once per trait and hands over, per
// isolate, the residual r_i and the weighted design row z_ij = w_i x_ij (j < q, z_i0 = w_i; all zero outside the
// trait's valid set), the lower Cholesky factor L of A = sum w_i x_i x_i' packed by rows, and for the linear kind the
// null model's residual sum of squares.  Per (trait, gene) what is left is q + 1 sums over the carriers and a
// triangular solve of q unknowns.
//
//   k_score_observed<Q>   block = 256 genes of one trait, a gene per lane (k_cat_observed's shape); the trait's q + 1
//                         rows pass through LDS in chunks of 512 isolates, the q + 1 running sums stay in registers
//                         across the chunks; Q = q is a template parameter, so that the sums and the solve are
//                         unrolled over registers and nothing is indexed.  The walk is dense: every lane of a
//                         wavefront reads the same LDS address (a broadcast, no bank conflict) and adds the value or
//                         +0.0 -- which never changes a running sum that started at +0.0, so the bits are those of a
//                         walk over the carriers alone.
#include "scoary_chi2.hpp"
#include "scoary_common.hpp"
#include "scoary_ttail.hpp"

namespace {

constexpr int kScoreMaxCovariates = 8;
constexpr int kScoreMaxQ = kScoreMaxCovariates + 1;          // design columns: the intercept and the covariates
constexpr int kScoreChunkWords = 16;                         // words (of 32 isolates) of a chunk: four quads
constexpr int kScoreChunk = 32 * kScoreChunkWords;           // 512 isolates: (q + 1) x 4 KB of LDS, at most 40 KB
static_assert(kScoreChunkWords % 4 == 0 && (kScoreMaxQ + 1) * kScoreChunk * 8 <= 64 * 1024,
              "a chunk is whole quads and its rows fit the LDS a kernel has without asking");

// word w of a trait's validity row, isolates >= N cleared
__device__ __forceinline__ uint32_t score_valid_word(const uint32_t* __restrict__ vrow, int w, int N) {
  uint32_t v = vrow[w];
  if (32 * w + 32 > N) v &= (1u << (N - 32 * w)) - 1u;
  return v;
}

template <int Q>
__global__ __launch_bounds__(256) void k_score_observed(const uint4* __restrict__ tiled, int64_t Gp, int G, int N,
                                                        int Wp, int linear, const double* __restrict__ rows,
                                                        const uint32_t* __restrict__ valid,
                                                        const double* __restrict__ chol,
                                                        const double* __restrict__ rss, int32_t* __restrict__ d_m,
                                                        double* __restrict__ d_u, double* __restrict__ d_b,
                                                        double* __restrict__ d_vg, double* __restrict__ d_stat,
                                                        double* __restrict__ d_beta, double* __restrict__ d_se,
                                                        double* __restrict__ d_p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int s_n;
  double* s_rows = reinterpret_cast<double*>(lds);           // [Q + 1][kScoreChunk]
  const int t = blockIdx.y, tid = threadIdx.x;
  const uint32_t* vrow = valid + (int64_t)t * Wp;
  const double* trow = rows + (int64_t)t * (Q + 1) * N;
  const int nw = (N + 31) / 32;
  if (tid == 0) s_n = 0;
  __syncthreads();
  int cnt = 0;
  for (int w = tid; w < nw; w += 256) cnt += __popc(score_valid_word(vrow, w, N));
  if (cnt) atomicAdd(&s_n, cnt);
  const int g = blockIdx.x * 256 + tid;
  const bool live = g < G;

  int m = 0;
  double acc[Q + 1];                                         // U, b_0 .. b_{Q-1}: unrolled, registers
#pragma unroll
  for (int j = 0; j <= Q; ++j) acc[j] = 0.0;
  for (int i0 = 0; i0 < N; i0 += kScoreChunk) {
    __syncthreads();                                         // the chunk before is read (and s_n is complete)
    const int len = min(kScoreChunk, N - i0);
    for (int k = tid; k < (Q + 1) * kScoreChunk; k += 256) {
      const int j = k / kScoreChunk, i = k % kScoreChunk;
      s_rows[k] = i < len ? trow[(int64_t)j * N + i0 + i] : 0.0;
    }
    __syncthreads();
    if (live) {
      const int w0 = i0 / 32;
#pragma unroll 1
      for (int qd = 0; qd < kScoreChunkWords / 4; ++qd) {
        if (w0 + 4 * qd >= nw) break;
        const uint4 x = tiled[(int64_t)(w0 / 4 + qd) * Gp + g];
        const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int jw = 0; jw < 4; ++jw) {
          const int w = w0 + 4 * qd + jw;
          if (w >= nw) break;
          const uint32_t bits = xs[jw] & score_valid_word(vrow, w, N);
          m += __popc(bits);
          const double* col = s_rows + 32 * (4 * qd + jw);
#pragma unroll 4
          for (int b = 0; b < 32; ++b) {
            const bool on = (bits >> b) & 1u;
#pragma unroll
            for (int j = 0; j <= Q; ++j) acc[j] += on ? col[j * kScoreChunk + b] : 0.0;
          }
        }
      }
    }
  }
  if (!live) return;
  const int n = s_n;

  // L u = b by forward substitution, rows and columns ascending; Vg = b_0 - sum u_j^2, ascending j
  const double* L = chol + (int64_t)t * (Q * (Q + 1) / 2);
  double u[Q], sq = 0.0;
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    double s = acc[1 + i];
#pragma unroll
    for (int j = 0; j < i; ++j) s -= L[i * (i + 1) / 2 + j] * u[j];
    u[i] = s / L[i * (i + 1) / 2 + i];
    sq += u[i] * u[i];
  }
  const double U = acc[0], b0 = acc[1], vg = b0 - sq;
  double stat = 0.0, beta = 0.0, se = 0.0, p = 1.0;
  const int df = n - Q - 1;
  if (m > 0 && m < n && vg > 0x1p-26 * b0 && (!linear || df >= 1)) {
    beta = U / vg;
    if (!linear) {
      stat = (U * U) / vg;
      se = 1.0 / sqrt(vg);
      p = chi2_tail(stat, 1);
    } else {
      const double rss1 = rss[t] - (U * U) / vg;
      if (rss1 > 0.0) {
        se = sqrt((rss1 / (double)df) / vg);
        stat = beta / se;
        p = t_tail(stat, df);
      } else if (U != 0.0) {                                 // the gene leaves no residual: an infinite t
        stat = U > 0.0 ? __builtin_inf() : -__builtin_inf();
        p = 0.0;
      }
    }
  }
  const int64_t o = (int64_t)t * G + g;
  d_m[o] = m;
  d_u[o] = U;
#pragma unroll
  for (int j = 0; j < Q; ++j) d_b[o * Q + j] = acc[1 + j];
  d_vg[o] = vg;
  d_stat[o] = stat;
  d_beta[o] = beta;
  d_se[o] = se;
  d_p[o] = p;
}

template <int Q>
void score_launch(dim3 grid, hipStream_t s, const uint4* tiled, int64_t Gp, int G, int N, int Wp, int linear,
                  const double* rows, const uint32_t* valid, const double* chol, const double* rss, int32_t* d_m,
                  double* d_u, double* d_b, double* d_vg, double* d_stat, double* d_beta, double* d_se, double* d_p) {
  hipLaunchKernelGGL(k_score_observed<Q>, grid, dim3(256), (size_t)(Q + 1) * kScoreChunk * 8, s, tiled, Gp, G, N, Wp,
                     linear, rows, valid, chol, rss, d_m, d_u, d_b, d_vg, d_stat, d_beta, d_se, d_p);
}

}  // namespace

extern "C" {

int64_t scoary_score_max_covariates(void) { return kScoreMaxCovariates; }

int scoary_score(scoary_handle h, const uint32_t* d_tiled, const double* d_rows, const uint32_t* d_valid,
                 const double* d_chol, const double* d_rss, int64_t G, int64_t T, int64_t N, int64_t q, int64_t linear,
                 int32_t* d_m, double* d_u, double* d_b, double* d_vg, double* d_stat, double* d_beta, double* d_se,
                 double* d_p, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = check_args(h, "scoary_score",
                          d_tiled && d_rows && d_valid && d_chol && (d_rss || linear == 0) && d_m && d_u && d_b &&
                              d_vg && d_stat && d_beta && d_se && d_p && G >= 1 && T >= 1 && N >= 1 &&
                              (linear == 0 || linear == 1)))
    return rc;
  if (q < 1 || q > kScoreMaxQ)
    return fail(h, SCOARY_ERR_SIZE, "scoary_score: q outside [1, scoary_score_max_covariates() + 1]");
  if (T > 65535 || G > 0x7fffffffLL - 256 || N > 0x7fffffffLL - kScoreChunk)
    return fail(h, SCOARY_ERR_SIZE, "scoary_score: T > 65535, G or N >= 2^31");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((G + 255) / 256), (unsigned)T);
  const uint4* tiled = reinterpret_cast<const uint4*>(d_tiled);
  const int64_t Gp = scoary_tiled_genes(G);
  const int Wp = (int)scoary_row_words(N);
  KernelTimer kt(h, s, "k_score_observed");
#define SCOARY_SCORE_CASE(Q)                                                                                        \
  case Q:                                                                                                           \
    score_launch<Q>(grid, s, tiled, Gp, (int)G, (int)N, Wp, (int)linear, d_rows, d_valid, d_chol, d_rss, d_m, d_u,  \
                    d_b, d_vg, d_stat, d_beta, d_se, d_p);                                                          \
    break;
  switch ((int)q) {
    SCOARY_SCORE_CASE(1)
    SCOARY_SCORE_CASE(2)
    SCOARY_SCORE_CASE(3)
    SCOARY_SCORE_CASE(4)
    SCOARY_SCORE_CASE(5)
    SCOARY_SCORE_CASE(6)
    SCOARY_SCORE_CASE(7)
    SCOARY_SCORE_CASE(8)
    SCOARY_SCORE_CASE(9)
  }
#undef SCOARY_SCORE_CASE
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
