// scoary_score_spa.hip -- the saddlepoint-corrected p of the logistic score test (spec S25 of DESIGN.md): for every
// (trait, gene) whose score chi-square of S24 reaches the cutoff, the two tails of S = sum g~_i (y_i - mu_i) by the
// Lugannani-Rice / Barndorff-Nielsen formula at the root of K'(t) = +-|U|, K the cumulant generating function of S
// under the null model.  The normal approximation behind Score_p is weakest for rare genes and unbalanced traits,
// which is where a run's strongest rows are.
//
//   k_spa_select      every pair: status 0, SPA_p = the bits of Score_p, z = t = 0; a pair whose statistic is not
//                     below cutoff^2 is appended to the work list in scratch through one atomic counter (hipcc folds
//                     a wavefront's additions into one atomic).  The order of the list is free: pairs are independent.
//   k_score_spa<Q>    the search, where the time goes: one wavefront per work item, grid-stride over the list, whose
//                     length it reads from device memory (no host round trip).  The lanes stride over the isolates; an
//                     isolate without its validity bit (or at or past N) is skipped by that bit and adds nothing.  The
//                     projected gene g~_i is formed from c = A^-1 b at every evaluation (q - 1 loads, q multiplications
//                     and subtractions beside the about hundred fp64 instructions of expm1 and the reciprocal): nothing
//                     of an item is kept in LDS or scratch, so N has no limit from a memory.  K' and K'' are reduced
//                     across the wavefront by an exchange in which every lane ends with the same bits, and made scalar
//                     (readfirstlane): the Newton search and its bracket are scalar code.  Per side it leaves t^ and
//                     what kind of side it is (beyond the support, the point mass, a root, no root within the cap).
//                     The cap is 100 evaluations, the restatement's: the rule counted in Python over the tests'
//                     problems (profiles/score_spa_tests.txt) takes up to 64 where the bracket's upper end sits at
//                     K'' ~ 0 and the search goes on by midpoints, and a side at the cap costs its pair the answer.
//   k_spa_sums<Q>     the same walk once more per side: K and K'' at the root, or the logarithm of the point mass.
//   k_spa_finish      one lane per work item: omega, v, z, the two tails, SPA_p and the status.
// Three kernels behind the list and not one, because hipcc keeps the coefficients of every fp64 library function
// of a kernel in registers from its first instruction on: with expm1, log1p, log, exp and erfc in one kernel an
// instance had 190 to 244 VGPRs (two wavefronts per SIMD) and kept 21 to 56 SGPRs in VGPR lanes; the search, which
// is nearly all of the time, now holds expm1's alone: 100 to 166 VGPRs, four wavefronts per SIMD up to q = 7.
#include "scoary_common.hpp"

namespace {

constexpr int kSpaMaxQ = 9;                          // design columns: S24's limit
constexpr int kSpaMaxIsolates = 65536;               // an item is one wavefront's walk: 1024 isolates per lane at most
constexpr int kSpaMaxEvals = 100;                    // evaluations of K' and K'' a side's search may take (S25)
constexpr double kSpaStep = 1e-11;                   // the search ends with an applied step of at most this, relative
constexpr double kSpaEdge = 1e-9;                    // S25's epsilon: |x - s_hi| <= epsilon s_hi is the point mass
constexpr int kSpaHeadBytes = 256;                   // the counter's own lines in front of the work list
// the most blocks (of four wavefronts) a launch has: 8 per CU.  At the 100 to 178 VGPRs of the search and the sums
// three or four wavefronts fit a SIMD, so up to half of such a grid waits for a slot; the blocks are not meant to be
// resident together (nothing waits for another block), the stride only bounds the grid.
constexpr int kSpaMaxBlocks = 2048;
// what a side is, from the search to the finish (in spa_z, as a double, until k_spa_finish writes z there)
constexpr int kSpaBeyond = 0, kSpaPoint = 1, kSpaRoot = 2, kSpaNoRoot = 3;

__host__ __device__ constexpr int64_t spa_list_bytes(int64_t pairs) { return (4 * pairs + 7) / 8 * 8; }

struct SpaArgs {
  const uint32_t* tiled;
  int64_t Gp;
  int G, N, Wp;
  const double* spa_rows;
  const double* rows;
  const uint32_t* valid;
  const double* chol;
  const double *d_u, *d_b, *d_vg, *d_stat, *d_p;
  double cutoff2;
  double *spa_p, *spa_z, *spa_t;
  int32_t* spa_status;
  int32_t* counter;
  int32_t* list;
  double* sums;                                      // [work item][side][2]: K and K'' at the root, or log of the mass
};

__global__ __launch_bounds__(256) void k_spa_select(SpaArgs a, int64_t pairs) {
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < pairs; o += (int64_t)gridDim.x * 256) {
    a.spa_p[o] = a.d_p[o];
    a.spa_z[2 * o] = 0.0;
    a.spa_z[2 * o + 1] = 0.0;
    a.spa_t[2 * o] = 0.0;
    a.spa_t[2 * o + 1] = 0.0;
    a.spa_status[o] = 0;
    if (!(a.d_stat[o] < a.cutoff2)) a.list[atomicAdd(a.counter, 1)] = (int32_t)o;
  }
}

// the sum over the wavefront, the same bits in every lane (a + b = b + a at every exchange), as a scalar
__device__ __forceinline__ double spa_wave_sum(double v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// what a work item's walks read: the trait's rows and bits, the gene's column of the tiled matrix, c = A^-1 b
template <int Q>
struct SpaItem {
  const double* mu;                                  // spa_rows row 0
  const double* x;                                   // spa_rows row 1 (ones; not read), rows 2 .. Q the covariates
  const double* w;                                   // S24's weights mu (1 - mu)
  const uint32_t* vrow;
  const uint32_t* gene;                              // word w of the gene: gene[((w >> 2) * Gp) * 4 + (w & 3)]
  int64_t Gp;
  int N;
  double c[Q];

  __device__ __forceinline__ SpaItem(const SpaArgs& a, int o) {
    const int t = o / a.G, g = o % a.G;
    const double* srow = a.spa_rows + (int64_t)t * (Q + 1) * a.N;
    mu = srow;
    x = srow + a.N;
    w = a.rows + ((int64_t)t * (Q + 1) + 1) * a.N;
    vrow = a.valid + (int64_t)t * a.Wp;
    gene = a.tiled + (int64_t)g * 4;
    Gp = a.Gp;
    N = a.N;
    // L u = b as S24 does, then L' c = u.  The same in every lane, but through vector loads into vector registers
    // (vz is a zero the compiler cannot see through): as scalars, L, u and c do not fit the scalar registers.
    int vz = 0;
    asm volatile("" : "+v"(vz));
    const double* L = a.chol + (int64_t)t * (Q * (Q + 1) / 2) + vz;
    double u[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      double s = a.d_b[(int64_t)o * Q + i + vz];
#pragma unroll
      for (int j = 0; j < i; ++j) s -= L[i * (i + 1) / 2 + j] * u[j];
      u[i] = s / L[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = Q - 1; i >= 0; --i) {
      double s = u[i];
#pragma unroll
      for (int j = Q - 1; j > i; --j) s -= L[j * (j + 1) / 2 + i] * c[j];
      c[i] = s / L[i * (i + 1) / 2 + i];
    }
  }

  // isolate i: false without its validity bit; else g~_i, mu_i and w_i
  __device__ __forceinline__ bool at(int i, double& gt, double& m, double& wi) const {
    const int wd = i >> 5, bit = i & 31;
    if (!((vrow[wd] >> bit) & 1u)) return false;
    const uint32_t gw = gene[((int64_t)(wd >> 2) * Gp) * 4 + (wd & 3)];
    double s = (double)((gw >> bit) & 1u);
    s -= c[0];                                       // x_i0 = 1
    // one running address, which hipcc is kept from turning back into a scalar base per row: those are 2 (q - 1)
    // SGPRs for every walk of the kernel, and at q >= 4 they no longer fit
    const double* xi = x + i;
#pragma unroll
    for (int j = 1; j < Q; ++j) {
      xi += N;
      asm volatile("" : "+v"(xi));
      s -= *xi * c[j];
    }
    gt = s;
    m = mu[i];
    wi = w[i];
    return true;
  }
};

// K' and K'' (and K) of the side sg = +-1 at sg t, t >= 0, in the side's own coordinates h_i = sg g~_i: with
// a = t h_i, e = expm1(-|a|) and pi = mu (a <= 0) or 1 - mu (a > 0), d = 1 + pi e: S25's two branches in one text
// (their terms differ by exact sign changes only).  K' is the side's, that is sg K'(sg t).
template <int Q, bool WITH_K>
__device__ __forceinline__ void spa_eval(const SpaItem<Q>& it, int lane, double sg, double t, double& K, double& K1,
                                         double& K2) {
  double k0 = 0.0, k1 = 0.0, k2 = 0.0;
#pragma unroll 1
  for (int i = lane; i < it.N; i += 64) {
    double gt, m, wi;
    if (!it.at(i, gt, m, wi)) continue;
    const double h = sg * gt, a = t * h;
    const bool pos = a > 0.0;
    const double e = expm1(-fabs(a));
    const double pi = pos ? 1.0 - m : m;
    const double r = 1.0 / (1.0 + pi * e);
    if (WITH_K) k0 += log1p(pi * e) + fabs(a) * pi;
    k1 += ((pos ? -h : h) * wi) * e * r;
    k2 += (wi * (h * h)) * (e + 1.0) * (r * r);
  }
  if (WITH_K) K = spa_wave_sum(k0);
  K1 = spa_wave_sum(k1);
  K2 = spa_wave_sum(k2);
}

template <int Q>
__global__ __launch_bounds__(256) void k_score_spa(SpaArgs a) {
  const double inf = __builtin_inf();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int count = *a.counter;
  for (int64_t k = (int64_t)blockIdx.x * 4 + wave; k < count; k += (int64_t)gridDim.x * 4) {   // count < 2^31
    const int o = a.list[k];
    const SpaItem<Q> it(a, o);
    // the ends of the support: s_hi and -s_lo
    double up = 0.0, dn = 0.0;
#pragma unroll 1
    for (int i = lane; i < a.N; i += 64) {
      double gt, m, wi;
      if (!it.at(i, gt, m, wi)) continue;
      up += gt > 0.0 ? gt * (1.0 - m) : -gt * m;
      dn += gt > 0.0 ? gt * m : -gt * (1.0 - m);
    }
    up = spa_wave_sum(up);
    dn = spa_wave_sum(dn);
    const double x = fabs(a.d_u[o]), vg = a.d_vg[o];
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {           // x = +|U|, then x = -|U|: one text, in the side's coordinates
      const double sg = side ? -1.0 : 1.0, shi = side ? dn : up;
      int kind;
      double that = sg * inf;
      if (x > shi * (1.0 + kSpaEdge)) {
        kind = kSpaBeyond;
      } else if (fabs(x - shi) <= kSpaEdge * shi) {
        kind = kSpaPoint;
      } else {
        // the root of K'(t) = x in (0, inf): Newton from x / Vg (the step from 0, K''(0) = Vg), kept in a bracket
        double lo = 0.0, hi = inf, t = x / vg, K, K1, K2;
        bool found = false;
#pragma unroll 1
        for (int ev = 0; ev < kSpaMaxEvals && !found; ++ev) {
          spa_eval<Q, false>(it, lane, sg, t, K, K1, K2);
          const double f = K1 - x;
          if (f > 0.0) hi = t; else lo = t;
          double tn = t - f / K2;
          if (hi == inf) {
            if (!(tn > lo && tn <= 4.0 * t)) tn = 4.0 * t;
          } else if (!(tn > lo && tn < hi)) {
            tn = 0.5 * (lo + hi);
          }
          found = fabs(tn - t) <= kSpaStep * fabs(tn);
          t = tn;
        }
        kind = found ? kSpaRoot : kSpaNoRoot;
        that = sg * t;
      }
      if (lane == 0) {
        a.spa_z[2 * (int64_t)o + side] = (double)kind;
        a.spa_t[2 * (int64_t)o + side] = that;
      }
    }
  }
}

template <int Q>
__global__ __launch_bounds__(256) void k_spa_sums(SpaArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int count = *a.counter;
  for (int64_t k = (int64_t)blockIdx.x * 4 + wave; k < count; k += (int64_t)gridDim.x * 4) {   // count < 2^31
    const int o = a.list[k];
    const SpaItem<Q> it(a, o);
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
      const double sg = side ? -1.0 : 1.0;
      const int kind = (int)a.spa_z[2 * (int64_t)o + side];
      double s0 = 0.0, s1 = 0.0;
      if (kind == kSpaRoot) {
        double K1;
        spa_eval<Q, true>(it, lane, sg, fabs(a.spa_t[2 * (int64_t)o + side]), s0, K1, s1);
      } else if (kind == kSpaPoint) {                // log of the mass at the end of the support
        double lp = 0.0;
#pragma unroll 1
        for (int i = lane; i < a.N; i += 64) {
          double gt, m, wi;
          if (!it.at(i, gt, m, wi)) continue;
          const double h = sg * gt;
          lp += h > 0.0 ? log(m) : (h < 0.0 ? log1p(-m) : 0.0);
        }
        s0 = spa_wave_sum(lp);
      }
      if (lane == 0) {
        a.sums[(2 * (int64_t)k + side) * 2] = s0;
        a.sums[(2 * (int64_t)k + side) * 2 + 1] = s1;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_spa_finish(SpaArgs a) {
  const double inf = __builtin_inf();
  const int count = *a.counter;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < count; k += (int64_t)gridDim.x * 256) {
    const int o = a.list[k];
    const double x = fabs(a.d_u[o]);
    double both = 0.0;
    bool ok = true;
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
      const double sg = side ? -1.0 : 1.0;
      const int kind = (int)a.spa_z[2 * (int64_t)o + side];
      const double s0 = a.sums[(2 * (int64_t)k + side) * 2], K2 = a.sums[(2 * (int64_t)k + side) * 2 + 1];
      double z = 0.0;
      if (kind == kSpaPoint) {
        both += exp(s0);
      } else if (kind == kSpaRoot) {
        const double t = fabs(a.spa_t[2 * (int64_t)o + side]), q2 = t * x - s0;
        bool good = q2 > 0.0 && q2 < inf && K2 > 0.0 && K2 < inf;
        if (good) {
          const double om = sqrt(2.0 * q2), v = t * sqrt(K2), ratio = v / om;
          good = ratio > 0.0 && ratio < inf;
          if (good) {
            const double zs = om + log(ratio) / om;
            z = sg * zs;
            good = zs > 0.0;                         // the sign of z is the side's
            if (good) both += 0.5 * erfc(zs * 0.70710678118654752440);
          }
        }
        ok = ok && good;
      } else if (kind != kSpaBeyond) {
        ok = false;
      }
      a.spa_z[2 * (int64_t)o + side] = z;
    }
    a.spa_p[o] = ok ? fmin(1.0, both) : a.d_p[o];
    a.spa_status[o] = ok ? 1 : 2;
  }
}

}  // namespace

extern "C" {

int64_t scoary_score_spa_max_isolates(void) { return kSpaMaxIsolates; }

int64_t scoary_score_spa_scratch_bytes(int64_t G, int64_t T) {
  if (G < 1 || T < 1 || T > 65535 || G > 0x7fffffffLL / T) return 0;
  return kSpaHeadBytes + spa_list_bytes(G * T) + 32 * G * T;
}

int scoary_score_spa(scoary_handle h, const uint32_t* d_tiled, const double* d_spa_rows, const double* d_rows,
                     const uint32_t* d_valid, const double* d_chol, const double* d_u, const double* d_b,
                     const double* d_vg, const double* d_stat, const double* d_p, int64_t G, int64_t T, int64_t N,
                     int64_t q, double cutoff2, double* d_spa_p, double* d_spa_z, double* d_spa_t,
                     int32_t* d_spa_status, void* d_scratch, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = check_args(h, "scoary_score_spa",
                          d_tiled && d_spa_rows && d_rows && d_valid && d_chol && d_u && d_b && d_vg && d_stat &&
                              d_p && d_spa_p && d_spa_z && d_spa_t && d_spa_status && d_scratch &&
                              reinterpret_cast<uintptr_t>(d_scratch) % 8 == 0 && G >= 1 && T >= 1 &&
                              N >= 1 && cutoff2 >= 0.1 * 0.1 && cutoff2 < __builtin_inf()))
    return rc;
  if (q < 1 || q > kSpaMaxQ)
    return fail(h, SCOARY_ERR_SIZE, "scoary_score_spa: q outside [1, scoary_score_max_covariates() + 1]");
  if (N > kSpaMaxIsolates)
    return fail(h, SCOARY_ERR_SIZE, "scoary_score_spa: more isolates than scoary_score_spa_max_isolates()");
  if (T > 65535 || G > 0x7fffffffLL / T)
    return fail(h, SCOARY_ERR_SIZE, "scoary_score_spa: T > 65535 or G T >= 2^31");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t pairs = G * T;
  char* scratch = static_cast<char*>(d_scratch);
  SpaArgs a;
  a.tiled = d_tiled;
  a.Gp = scoary_tiled_genes(G);
  a.G = (int)G;
  a.N = (int)N;
  a.Wp = (int)scoary_row_words(N);
  a.spa_rows = d_spa_rows;
  a.rows = d_rows;
  a.valid = d_valid;
  a.chol = d_chol;
  a.d_u = d_u;
  a.d_b = d_b;
  a.d_vg = d_vg;
  a.d_stat = d_stat;
  a.d_p = d_p;
  a.cutoff2 = cutoff2;
  a.spa_p = d_spa_p;
  a.spa_z = d_spa_z;
  a.spa_t = d_spa_t;
  a.spa_status = d_spa_status;
  a.counter = reinterpret_cast<int32_t*>(scratch);
  a.list = reinterpret_cast<int32_t*>(scratch + kSpaHeadBytes);
  a.sums = reinterpret_cast<double*>(scratch + kSpaHeadBytes + spa_list_bytes(pairs));
  const dim3 per_lane((unsigned)std::min<int64_t>((pairs + 255) / 256, kSpaMaxBlocks));
  // a wavefront per four pairs at the most: a list of every pair is then walked in four strides at any size, and a
  // list at the default cutoff (a twentieth of the pairs under the null) still finds the wavefronts to spread over
  const dim3 per_wave((unsigned)std::min<int64_t>((pairs + 15) / 16, kSpaMaxBlocks));
  KernelTimer kt(h, s, "k_score_spa");
  HIP_TRY(h, hipMemsetAsync(a.counter, 0, kSpaHeadBytes, s));
  hipLaunchKernelGGL(k_spa_select, per_lane, dim3(256), 0, s, a, pairs);
#define SCOARY_SPA_CASE(Q)                                                        \
  case Q:                                                                         \
    hipLaunchKernelGGL(k_score_spa<Q>, per_wave, dim3(256), 0, s, a);             \
    hipLaunchKernelGGL(k_spa_sums<Q>, per_wave, dim3(256), 0, s, a);              \
    break;
  switch ((int)q) {
    SCOARY_SPA_CASE(1)
    SCOARY_SPA_CASE(2)
    SCOARY_SPA_CASE(3)
    SCOARY_SPA_CASE(4)
    SCOARY_SPA_CASE(5)
    SCOARY_SPA_CASE(6)
    SCOARY_SPA_CASE(7)
    SCOARY_SPA_CASE(8)
    SCOARY_SPA_CASE(9)
  }
#undef SCOARY_SPA_CASE
  hipLaunchKernelGGL(k_spa_finish, per_lane, dim3(256), 0, s, a);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
