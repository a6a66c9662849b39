// scoary_cmh_exact.hip -- the exact conditional test over the strata (spec S12 of DESIGN.md): under the S9 null
// the pooled count of a (trait, gene) is the sum of independent hypergeometrics, one per stratum, so its
// distribution is their convolution.  From that one pmf: the two-sided p of every count of the support under the
// probability-ordering rule (R's mantelhaen.test(exact = TRUE); Fisher's exact test when there is one stratum), the
// observed count's own entry, and the exact mass of S10's rejection region.
//
//   k_cmh_exact : one work group of 256 lanes per (trait, gene) row, rows in the CSR order of scoary_cmh_minp_plan.
//     1. the lanes stride over the segment table of k_cmh_segments, gather the gene's words from the tiled matrix
//        and add popc(gene & valid & mask) into m[s] in LDS;
//     2. a lane per stratum (a few strata each): the support sizes, their offsets (block_scan of
//        scoary_common.hpp, as every scan of this file) and the stratum's
//        pmf by the ratio recurrence outward from the mode, normalised to sum 1 -- all strata at once, side by side
//        in one LDS buffer of at most N / 2 + S doubles;
//     3. the running pmf is convolved with one stratum after the other between two LDS buffers, lane = output
//        index (neighbouring lanes read neighbouring words, the stratum's entry is a broadcast), strata with a
//        single support point skipped: they only shift the support;
//     4. prefix sums from the left and suffix sums from the right, and the mode; f is log-concave, so the set
//        {y : f(y) <= gamma f(x)} is a left tail and a right tail, found by two binary searches: p(x) is two
//        reads of the sums.  Tails are summed from their small end, so a p of 1e-190 keeps its relative accuracy;
//     5. the row's run of the table is written with contiguous stores; the observed p is read back from it.
//   k_cmh_odds_exact (spec S13; further down): steps 1 to 3 through the same function (exact_pmf), then the conditional
//     maximum-likelihood odds ratio and its exact confidence limits, three roots solved in lockstep.
//   The table is built by scoary_cmh_segments_launch and the arguments are checked by strata_check (scoary_cmh.hip,
//   scoary_common.hpp).  Every index is clamped: a bad plan gives wrong values, never a wild access.  LDS per work group follows N and S
//   (three buffers of N / 2 + 1 doubles): 25 KB at N = 2000, 115 KB at the limit of 8190 isolates.
#include "scoary_common.hpp"

namespace {

constexpr int kExactThreads = 256;
constexpr int kExactMaxIsolates = 8190;               // the support is then at most 4096 entries
constexpr double kExactGamma = 1.0 + 1e-7;            // S12 step 3: the relErr of R's fisher.test / mantelhaen.test
constexpr int64_t kExactRows = (int64_t)1 << 30;      // (trait, gene) rows per launch

// the most entries a support can have: every stratum adds at most n_s / 2 to hi - lo
inline int exact_cap(int64_t N) { return (int)(N / 2 + 1); }
inline int64_t exact_lds_bytes(int64_t N, int64_t S) {
  return (3 * (int64_t)exact_cap(N) + S) * (int64_t)sizeof(double) + (2 * S + 1) * (int64_t)sizeof(int32_t);
}

struct ExactOut {
  double *p, *p_region, *tab;
};

// exclusive prefix sum of v over the lanes of the block in the order of `idx` (a permutation of 0 .. 255); every
// partial sum is a sum of the terms themselves (no subtraction), so sums of positive terms keep their accuracy
__device__ __forceinline__ double exact_scan(double* s_d, int idx, double v) {
  s_d[idx] = v;
  block_scan<kExactThreads>(s_d, idx, [](double x, double y) { return x + y; });
  const double before = idx > 0 ? s_d[idx - 1] : 0.0;
  __syncthreads();
  return before;
}

// steps 1 to 3 of k_cmh_exact for the row (t, g), shared with k_cmh_odds_exact: the stratum counts, the strata's pmfs
// and their convolution in the dynamic LDS of exact_lds_bytes(N, S) at `lds`.  -> L, the entries of the support; the
// pmf is cur[0 .. L), nxt and fs (cap and cap + S doubles) are free.  Ends on a barrier whenever L > 1.
__device__ __forceinline__ int exact_pmf(double* lds, int* s_i, const uint32_t* __restrict__ tiled,
                                         const uint32_t* __restrict__ masks, const int32_t* __restrict__ smargins,
                                         const CmhSegments* __restrict__ segs, int64_t Gp, int N, int Wp, int S, int cap,
                                         int t, int64_t g, double*& cur, double*& nxt, double*& fs) {
  cur = lds;                                           // [cap] the running pmf
  nxt = lds + cap;                                     // [cap]
  fs = lds + 2 * cap;                                  // [cap + S] the strata's pmfs side by side
  uint32_t* m = reinterpret_cast<uint32_t*>(fs + cap + S);   // [S]
  int* zoff = reinterpret_cast<int*>(m + S);           // [S + 1] offsets of the informative strata's pmfs in fs
  const int fs_cap = cap + S;
  const int tid = threadIdx.x;

  // 1. m[s] = popc(gene & valid & stratum s)
  for (int s = tid; s < S; s += kExactThreads) m[s] = 0;
  __syncthreads();
  const int nseg = min((int)segs->count, N);
  for (int i = tid; i < nseg; i += kExactThreads) {
    const uint2 sg = segs->seg[i];
    const int s = min((int)(sg.x >> 16), S - 1), w = min((int)(sg.x & 0xffffu), Wp - 1);
    const uint32_t gw = tiled[((int64_t)(w >> 2) * Gp + g) * 4 + (w & 3)];
    const uint32_t v = gw & sg.y & masks[(int64_t)t * Wp + w];
    if (v) atomicAdd(&m[s], (uint32_t)__popc(v));
  }
  __syncthreads();

  // 2. the strata of this lane: [s0, s1); a stratum is informative when its support has more than one point
  const int per = (S + kExactThreads - 1) / kExactThreads;
  const int s0 = min(tid * per, S), s1 = min(s0 + per, S);
  const int2* __restrict__ kn = reinterpret_cast<const int2*>(smargins) + (int64_t)t * S;
  auto shape = [&](int s, int& k, int& n, int& mm, int& lo_s) {         // -> the size of the stratum's support
    const int2 v = kn[s];
    k = v.x, n = v.y, mm = (int)m[s];
    if (n <= 0) return 0;
    lo_s = max(0, k + mm - n);
    const int z = min(k, mm) - lo_s + 1;
    return z > 1 ? z : 0;
  };
  int mine = 0;
  for (int s = s0; s < s1; ++s) {
    int k, n, mm, lo_s;
    mine += min(shape(s, k, n, mm, lo_s), fs_cap + 1);                 // (no overflow of the sum, whatever the plan)
  }
  s_i[tid] = mine;                                                      // the lanes' sizes, clamped (no overflow)
  block_scan<kExactThreads>(s_i, tid, [&](int x, int y) { return min(x + y, 2 * fs_cap); });
  int at = s_i[tid] - mine;
  if (tid == kExactThreads - 1) zoff[S] = s_i[tid];
  for (int s = s0; s < s1; ++s) {
    int k, n, mm, lo_s;
    const int z = min(shape(s, k, n, mm, lo_s), fs_cap + 1);
    zoff[s] = at;
    if (z > 1 && at + z <= fs_cap) {
      // f(x) = C(m, x) C(n - m, k - x) / C(n, k) on [lo_s, lo_s + z): the mode's weight 1, its neighbours by the
      // ratio f(x + 1) / f(x) = (m - x)(k - x) / ((x + 1)(n - m - k + x + 1)); products of counts are exact
      double* f = fs + at;
      const int hi_s = lo_s + z - 1;
      const int xm = min(max((int)(((int64_t)(mm + 1) * (k + 1)) / (n + 2)), lo_s), hi_s);
      const int c = n - mm - k;
      double w = 1.0, sum = 1.0;
      f[xm - lo_s] = 1.0;
      for (int x = xm; x < hi_s; ++x) {
        w = (w * ((double)(mm - x) * (double)(k - x))) / ((double)(x + 1) * (double)(c + x + 1));
        f[x + 1 - lo_s] = w;
        sum += w;
      }
      w = 1.0;
      for (int x = xm; x > lo_s; --x) {
        w = (w * ((double)x * (double)(c + x))) / ((double)(mm - x + 1) * (double)(k - x + 1));
        f[x - 1 - lo_s] = w;
        sum += w;
      }
      for (int j = 0; j < z; ++j) f[j] = f[j] / sum;
    }
    at = min(at + z, 2 * fs_cap);
  }
  if (tid == 0) cur[0] = 1.0;
  __syncthreads();

  // 3. the convolution, strata in ascending order
  int L = 1;
  for (int s = 0; s < S; ++s) {
    const int o = zoff[s], z = zoff[s + 1] - o;                         // block-uniform
    if (z <= 1) continue;
    if (o + z > fs_cap || L + z - 1 > cap) break;                       // not with a sound plan
    const double* __restrict__ f = fs + o;
    const int Ln = L + z - 1;
    for (int j = tid; j < Ln; j += kExactThreads) {
      const int i0 = max(0, j - L + 1), i1 = min(z - 1, j);
      double acc = 0.0;
      for (int i = i0; i <= i1; ++i) acc += cur[j - i] * f[i];        // (unrolled 4 or 8 times: 1 to 19 % slower)
      nxt[j] = acc;
    }
    __syncthreads();
    double* const swap = cur;
    cur = nxt, nxt = swap;
    L = Ln;
  }
  return L;
}

__global__ __launch_bounds__(kExactThreads) void k_cmh_exact(
    const uint32_t* __restrict__ tiled, const uint32_t* __restrict__ masks, const int32_t* __restrict__ smargins,
    const CmhSegments* __restrict__ segs, const int32_t* __restrict__ a_obs, const uint32_t* __restrict__ crit,
    const int64_t* __restrict__ off, const int32_t* __restrict__ lo, int64_t G, int64_t Gp, int N, int Wp, int S,
    int cap, int64_t r0, int64_t entries, ExactOut out) {
  extern __shared__ double lds[];
  __shared__ double s_d[kExactThreads];
  __shared__ int s_i[kExactThreads];
  const int tid = threadIdx.x;
  const int64_t row = r0 + blockIdx.x;                 // < T * G: the launches cover the rows exactly
  const int t = (int)(row / G);
  const int64_t g = row % G;
  double *cur, *nxt, *fs;
  const int L = exact_pmf(lds, s_i, tiled, masks, smargins, segs, Gp, N, Wp, S, cap, t, g, cur, nxt, fs);

  // 4. left[j] = f(0) + ... + f(j), right[j] = f(j) + ... + f(L - 1), and the mode (the first largest entry)
  double* left = nxt;
  double* right = fs;
  const int chunk = (L + kExactThreads - 1) / kExactThreads;
  const int c0 = min(tid * chunk, L), c1 = min(c0 + chunk, L);
  double sum = 0.0, best = -1.0;
  int best_at = 0x7fffffff;
  for (int j = c0; j < c1; ++j) {
    const double v = cur[j];
    sum += v;
    if (v > best) best = v, best_at = j;
  }
  double run = exact_scan(s_d, tid, sum);
  for (int j = c0; j < c1; ++j) left[j] = (run += cur[j]);
  sum = 0.0;
  for (int j = c1 - 1; j >= c0; --j) sum += cur[j];
  run = exact_scan(s_d, kExactThreads - 1 - tid, sum);
  for (int j = c1 - 1; j >= c0; --j) right[j] = (run += cur[j]);
  s_d[tid] = best, s_i[tid] = best_at;
  __syncthreads();
  for (int o = kExactThreads / 2; o > 0; o >>= 1) {
    if (tid < o && (s_d[tid + o] > s_d[tid] || (s_d[tid + o] == s_d[tid] && s_i[tid + o] < s_i[tid])))
      s_d[tid] = s_d[tid + o], s_i[tid] = s_i[tid + o];
    __syncthreads();
  }
  const int mode = min(max(s_i[0], 0), L - 1);
  const double total = left[L - 1];

  // S12 step 3 at the count lo + x: the entries up to gamma f(x) are [0, nl) and [rb, L)
  auto p_at = [&](int x) {
    const double thr = kExactGamma * cur[x];
    int a = 0, b = mode;                                  // nl: the first entry of [0, mode) above thr (rising side)
    while (a < b) {
      const int c = (a + b) >> 1;
      if (cur[c] <= thr) a = c + 1; else b = c;
    }
    const int nl = a;
    a = mode, b = L;                                      // rb: the first entry of [mode, L) not above thr (falling side)
    while (a < b) {
      const int c = (a + b) >> 1;
      if (cur[c] <= thr) b = c; else a = c + 1;
    }
    const int rb = a;
    if (nl >= rb) return 1.0;                             // the whole support: x is a mode
    const double tails = (nl > 0 ? left[nl - 1] : 0.0) + (rb < L ? right[rb] : 0.0);
    return fmin(1.0, tails / total);
  };

  // 5. the row's run of the table, the observed count's entry and the mass of the region
  const int64_t o0 = min(max(off[row], (int64_t)0), entries), o1 = min(max(off[row + 1], o0), entries);
  const int64_t ntab = out.tab ? o1 - o0 : 0;
  for (int64_t x = tid; x < ntab; x += kExactThreads) out.tab[o0 + x] = x < L ? p_at((int)x) : 1.0;
  const int64_t lo_row = lo[row];
  if (out.p) {
    const int xa = (int)min(max((int64_t)a_obs[row] - lo_row, (int64_t)0), (int64_t)(L - 1));
    if (tid == (xa & (kExactThreads - 1))) out.p[row] = xa < ntab ? out.tab[o0 + xa] : p_at(xa);   // this lane's own store
  }
  if (out.p_region && tid == 0) {
    const uint2 br = reinterpret_cast<const uint2*>(crit)[row];
    double pr = 1.0;                                      // the region (0, 0): every count
    if (br.y != 0) {
      const int nl = (int)min(max((int64_t)br.x - lo_row, (int64_t)0), (int64_t)L);
      const int rb = (int)min(max((int64_t)br.x + (int64_t)br.y - lo_row, (int64_t)nl), (int64_t)L);
      const double tails = (nl > 0 ? left[nl - 1] : 0.0) + (rb < L ? right[rb] : 0.0);
      pr = fmin(1.0, tails / total);
    }
    out.p_region[row] = pr;
  }
}

// ---- spec S13: the conditional maximum-likelihood odds ratio and its exact confidence limits ------------------
constexpr int kOddsSums = 12;                         // the sums one block reduction carries (odds_solve)
constexpr int kOddsWaves = kExactThreads / kWave;
constexpr double kOddsTheta = 700.0;                  // theta = log psi is searched in [-700, 700]
constexpr double kOddsStep = 1e-13;                   // a step or a bracket below it ends a search
constexpr int kOddsMaxIter = 128;                     // (a bound on the loop; 5 to 9 iterations are the rule)
constexpr double kOddsTiny = 1e-290;                  // S12's TINY

struct OddsOut {
  double *odds, *lo, *hi;
};

// one root search: the trial theta, its bracket and whether it has ended
struct OddsRoot {
  double th, lo, hi;
  bool done;
};

// the largest exponent lf(j) + th (j - xa) over [j0, j1]: lf is concave, so the exponents rise up to their maximum
// and fall behind it -- a binary search on the sign of the forward difference, every lane its own (no barrier)
__device__ __forceinline__ double odds_peak(const double* lf, int j0, int j1, int xa, double th) {
  int a = j0, b = j1;
  while (a < b) {
    const int c = (a + b) >> 1;
    if (lf[c + 1] - lf[c] + th > 0.0) a = c + 1; else b = c;
  }
  return lf[a] + th * (double)(a - xa);
}

// safeguarded Newton: h (increasing in theta) and its derivative dh at r.th tighten the bracket; the Newton step is
// taken while it stays inside the bracket, the bracket is bisected otherwise (h = +-inf and a nan step among it:
// one side of a ratio underflowed far from the root).  Ends on a step or a bracket below kOddsStep.
__device__ __forceinline__ void odds_step(OddsRoot& r, double h, double dh) {
  if (r.done) return;
  r.hi = h > 0.0 ? r.th : r.hi;
  r.lo = h < 0.0 ? r.th : r.lo;
  const double dn = -h / dh;
  const bool small = fabs(dn) < kOddsStep;
  double nt = r.th + dn;
  if (!(nt > r.lo && nt < r.hi)) nt = small ? r.th : 0.5 * (r.lo + r.hi);
  r.done = small || fabs(nt - r.th) < kOddsStep || r.hi - r.lo < kOddsStep;
  r.th = nt;
}

// psi = exp(theta); a search that ran into an end of [-700, 700] has its root outside: 0 or +inf
__device__ __forceinline__ double odds_psi(double th) {
  return th <= -kOddsTheta + 1e-9 ? 0.0 : (th >= kOddsTheta - 1e-9 ? HUGE_VAL : exp(th));
}

//   k_cmh_odds_exact : one work group of 256 lanes per (trait, gene) row, in k_cmh_exact's row order.  Steps 1 to 3 are
//     k_cmh_exact's (exact_pmf); then, with x = j - xa the distance to the observed count and w(j) = f(j) psi^x,
//       the estimate    : log sum{w x : x > 0} - log sum{w |x| : x < 0} = 0          (E_psi[X] = A)
//       the lower limit : log sum{w : x >= 0} - log sum{w : x < 0} = logit(half)     (P_psi(X >= A) = half)
//       the upper limit : log sum{w : x > 0} - log sum{w : x <= 0} = -logit(half)    (P_psi(X <= A) = half)
//     all three increasing in theta = log psi with a derivative of at least 1 (the distance between the means of
//     the two sides) and close to linear far from the root, where a plain P - half or E - A is flat.  lf(j) = log(f(j) / f(A)) is written over nxt once; every
//     iteration takes one pass over a lane's entries for the three trial thetas (terms exp(lf + theta x - M), M the
//     largest exponent: odds_peak), one reduction of the kOddsSums sums -- shuffles inside a wavefront, the four
//     wavefronts through LDS, double-buffered: ONE barrier per iteration -- and the same Newton step in every lane.
__global__ __launch_bounds__(kExactThreads) void k_cmh_odds_exact(
    const uint32_t* __restrict__ tiled, const uint32_t* __restrict__ masks, const int32_t* __restrict__ smargins,
    const CmhSegments* __restrict__ segs, const int32_t* __restrict__ a_obs, const int32_t* __restrict__ lo, int64_t G,
    int64_t Gp, int N, int Wp, int S, int cap, int64_t r0, double half, OddsOut out) {
  extern __shared__ double lds[];
  __shared__ double s_red[2][kOddsWaves][kOddsSums];
  __shared__ int s_i[kExactThreads];
  const int tid = threadIdx.x;
  const int64_t row = r0 + blockIdx.x;                 // < T * G: the launches cover the rows exactly
  const int t = (int)(row / G);
  const int64_t g = row % G;
  double *cur, *nxt, *fs;
  const int L = exact_pmf(lds, s_i, tiled, masks, smargins, segs, Gp, N, Wp, S, cap, t, g, cur, nxt, fs);
  if (L <= 1) {                                        // no informative stratum (block-uniform)
    if (tid == 0) out.odds[row] = __builtin_nan(""), out.lo[row] = 0.0, out.hi[row] = HUGE_VAL;
    return;
  }
  const int xa = (int)min(max((int64_t)a_obs[row] - (int64_t)lo[row], (int64_t)0), (int64_t)(L - 1));

  // lf = log(f / f(A)) over nxt, and [j0, j1] = the entries with f > 0 (a run: f is log-concave)
  double* lf = nxt;
  const double fa = cur[xa];
  const double ref = fa >= kOddsTiny ? fa : 1.0;       // (below TINY the values are unspecified: no overflow of f / ref)
  if (tid == 0) s_i[0] = L - 1, s_i[1] = 0;
  __syncthreads();
  int first = L, last = -1;
  for (int j = tid; j < L; j += kExactThreads) {
    const double v = cur[j];
    lf[j] = log(v / ref);                              // -inf where f underflowed
    if (v > 0.0) first = min(first, j), last = j;
  }
  if (last >= 0) atomicMin(&s_i[0], first), atomicMax(&s_i[1], last);
  __syncthreads();
  const int j0 = min(s_i[0], xa), j1 = max(max(s_i[1], xa), j0);     // block-uniform, inside [0, L)

  const double target = log(half) - log1p(-half);      // logit(half)
  OddsRoot est{0.0, -kOddsTheta, kOddsTheta, !(xa > 0 && xa < L - 1)};
  OddsRoot low{0.0, -kOddsTheta, kOddsTheta, !(xa > 0)};
  OddsRoot upp{0.0, -kOddsTheta, kOddsTheta, !(xa < L - 1)};
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  for (int it = 0; it < kOddsMaxIter && !(est.done && low.done && upp.done); ++it) {
    const double m_est = odds_peak(lf, j0, j1, xa, est.th);
    const double m_low = odds_peak(lf, j0, j1, xa, low.th);
    const double m_upp = odds_peak(lf, j0, j1, xa, upp.th);
    double acc[kOddsSums];
#pragma unroll
    for (int k = 0; k < kOddsSums; ++k) acc[k] = 0.0;
    for (int j = j0 + tid; j <= j1; j += kExactThreads) {
      const double l = lf[j], x = (double)(j - xa);
      if (!est.done) {                                 // (the three tests are block-uniform)
        const double w = exp(l + est.th * x - m_est), wx = w * fabs(x), wxx = wx * fabs(x);
        const bool up = j > xa;                        // (the entry x = 0 adds 0 to either side)
        acc[0] += up ? wx : 0.0, acc[1] += up ? wxx : 0.0, acc[2] += up ? 0.0 : wx, acc[11] += up ? 0.0 : wxx;
      }
      if (!low.done) {
        const double w = exp(l + low.th * x - m_low), wx = w * x;
        const bool up = j >= xa;
        acc[3] += up ? w : 0.0, acc[4] += up ? wx : 0.0, acc[5] += up ? 0.0 : w, acc[6] += up ? 0.0 : wx;
      }
      if (!upp.done) {
        const double w = exp(l + upp.th * x - m_upp), wx = w * x;
        const bool up = j > xa;
        acc[7] += up ? w : 0.0, acc[8] += up ? wx : 0.0, acc[9] += up ? 0.0 : w, acc[10] += up ? 0.0 : wx;
      }
    }
#pragma unroll
    for (int k = 0; k < kOddsSums; ++k) {
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);   // the same bits in every lane
    }
    double (*red)[kOddsSums] = s_red[it & 1];
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kOddsSums; ++k) red[wave][k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kOddsSums; ++k) acc[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    odds_step(est, log(acc[0]) - log(acc[2]), acc[1] / acc[0] + acc[11] / acc[2]);
    odds_step(low, log(acc[3]) - log(acc[5]) - target, acc[4] / acc[3] - acc[6] / acc[5]);
    odds_step(upp, log(acc[7]) - log(acc[9]) + target, acc[8] / acc[7] - acc[10] / acc[9]);
  }
  if (tid == 0) {
    out.odds[row] = xa == 0 ? 0.0 : (xa == L - 1 ? HUGE_VAL : odds_psi(est.th));
    out.lo[row] = xa == 0 ? 0.0 : odds_psi(low.th);
    out.hi[row] = xa == L - 1 ? HUGE_VAL : odds_psi(upp.th);
  }
}

// What the two entry points (``who``) do after their own argument check: the sizes both kernels refuse, the
// opt-in to more than 64 KB of LDS (``optin``: the kernel's own flag in the handle -- it is per kernel function),
// the segment table, and the launches in blocks of kExactRows rows.  The kernels' parameter lists differ in the
// middle, so ``block(s, nrows, lds_bytes, r0)`` launches ``kernel`` for the rows r0 .. r0 + nrows - 1.
template <class... Args, class Block>
int launch_exact(scoary_handle h, const std::string& who, void (*kernel)(Args...), const char* timer, int* optin,
                 const uint16_t* d_strata, const int32_t* d_members, void* d_scratch, int64_t G, int64_t T, int64_t N,
                 int64_t S, scoary_stream_t stream, Block block) {
  if (G > (int64_t)1 << 30) return fail(h, SCOARY_ERR_SIZE, who + ": G > 2^30");
  if (N > kExactMaxIsolates)
    return fail(h, SCOARY_ERR_SIZE, who + ": more isolates than scoary_cmh_exact_max_isolates() = " +
                                        std::to_string(kExactMaxIsolates) + " (the pmf of a gene is held in LDS)");
  const int64_t lds_bytes = exact_lds_bytes(N, S);
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (lds_bytes > 64 * 1024 && !*optin) {
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)exact_lds_bytes(kExactMaxIsolates, scoary_perm_max_strata())));
    *optin = 1;
  }
  if (int rc = scoary_cmh_segments_launch(h, s, d_strata, d_members, N, S, d_scratch, "k_cmh_segments")) return rc;
  const int64_t M = T * G;
  KernelTimer kt(h, s, timer);
  for (int64_t r0 = 0; r0 < M; r0 += kExactRows) {
    block(s, dim3((unsigned)std::min(kExactRows, M - r0)), (size_t)lds_bytes, r0);
    HIP_TRY(h, hipGetLastError());
  }
  return SCOARY_OK;
}

}  // namespace

extern "C" {

int64_t scoary_cmh_exact_max_isolates(void) { return kExactMaxIsolates; }

int scoary_cmh_exact(scoary_handle h, const uint32_t* d_tiled, const uint32_t* d_masks, const uint16_t* d_strata,
                     const int32_t* d_members, const int32_t* d_offsets, const int32_t* d_smargins, int64_t G,
                     int64_t T, int64_t N, int64_t S, const int32_t* d_a, const uint32_t* d_crit,
                     const int64_t* d_off, const int32_t* d_lo, int64_t entries, double* d_p, double* d_p_region,
                     double* d_tab, void* d_scratch, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = strata_check(h, "scoary_cmh_exact", d_tiled && d_masks && d_strata && d_members && d_offsets &&
                                                        d_smargins && d_a && d_crit && d_off && d_lo && d_scratch &&
                                                        (d_p || d_p_region || d_tab) && G >= 1 && entries >= T * G,
                            T, N, S))
    return rc;
  const ExactOut out{d_p, d_p_region, d_tab};
  return launch_exact(h, "scoary_cmh_exact", k_cmh_exact, "k_cmh_exact", &h->cmh_exact_lds_optin, d_strata, d_members,
                      d_scratch, G, T, N, S, stream, [&](hipStream_t s, dim3 nrows, size_t lds_bytes, int64_t r0) {
                        hipLaunchKernelGGL(k_cmh_exact, nrows, dim3(kExactThreads), lds_bytes, s, d_tiled, d_masks,
                                           d_smargins, static_cast<const CmhSegments*>(d_scratch), d_a, d_crit, d_off,
                                           d_lo, G, scoary_tiled_genes(G), (int)N, (int)scoary_row_words(N), (int)S,
                                           exact_cap(N), r0, entries, out);
                      });
}

int scoary_cmh_exact_odds(scoary_handle h, const uint32_t* d_tiled, const uint32_t* d_masks, const uint16_t* d_strata,
                          const int32_t* d_members, const int32_t* d_offsets, const int32_t* d_smargins, int64_t G,
                          int64_t T, int64_t N, int64_t S, const int32_t* d_a, const int64_t* d_off, const int32_t* d_lo,
                          int64_t entries, double half, double* d_or, double* d_or_lo, double* d_or_hi, void* d_scratch,
                          scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = strata_check(h, "scoary_cmh_exact_odds", d_tiled && d_masks && d_strata && d_members && d_offsets &&
                                                             d_smargins && d_a && d_off && d_lo && d_scratch && d_or &&
                                                             d_or_lo && d_or_hi && G >= 1 && entries >= T * G &&
                                                             half > 0.0 && half < 0.5,
                            T, N, S))
    return rc;
  const OddsOut out{d_or, d_or_lo, d_or_hi};
  return launch_exact(h, "scoary_cmh_exact_odds", k_cmh_odds_exact, "k_cmh_odds_exact", &h->cmh_exact_odds_lds_optin,
                      d_strata, d_members, d_scratch, G, T, N, S, stream,
                      [&](hipStream_t s, dim3 nrows, size_t lds_bytes, int64_t r0) {
                        hipLaunchKernelGGL(k_cmh_odds_exact, nrows, dim3(kExactThreads), lds_bytes, s, d_tiled, d_masks,
                                           d_smargins, static_cast<const CmhSegments*>(d_scratch), d_a, d_lo, G,
                                           scoary_tiled_genes(G), (int)N, (int)scoary_row_words(N), (int)S,
                                           exact_cap(N), r0, half, out);
                      });
}

}  // extern "C"
