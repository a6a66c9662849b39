// scoary_cmh.hip -- the Cochran-Mantel-Haenszel test over the per-stratum 2x2 tables (spec S10 of DESIGN.md):
// per (trait, gene) the stratified chi-square with its p, the Mantel-Haenszel common odds ratio, and the
// rejection region of the pooled overlap count that the permutation kernels consume under the S9 null.
//
//   k_cmh_segments : once per call, one block: the strata as a SEGMENT TABLE -- (32-bit word of the isolate row,
//       stratum, mask of that stratum's isolates inside the word), sorted by (stratum, word).  The members array
//       of the strata plan is ordered by (stratum, isolate), so a segment is a run of consecutive members with
//       the same key: at most N of them, about W + S when the isolates of a stratum are adjacent.
//   cmh_walk : THE walk of a lane over the table (k_cmh and k_cmh_support pass it what they do per segment, per
//       stratum and for the strata without a member); cmh_stat : THE statistic at a pooled count (k_cmh, k_cmh_fill).
//   k_cmh : one lane per gene on the tiled matrix (a wavefront's quad loads are 1 KiB coalesced), kTraits traits
//       per block with their fp64 accumulators in registers.  A lane walks the table: per segment two AND +
//       popcounts per trait against wave-uniform label / validity words, and on every change of stratum the
//       stratum's (a, m) is folded into the accumulators -- strata in ascending order, the operations of S10
//       each rounded on its own (the library is built with -ffp-contract=off).  The cost follows the number of
//       segments, not S; nothing is re-tiled and the per-stratum tables exist only in registers (d_scounts, for
//       callers that want them, is the one exception).
//
// The Westfall-Young tables of the CMH statistic (spec S11): what scoary_permute_minp / scoary_permute_stepdown
// gather from, in the CSR layout of scoary_minp_plan / _fill, indexed by the pooled count a' = popc(gene & label).
//   k_cmh_support : cmh_walk over the same segment table with the validity words alone -- per stratum
//       m = popc(gene & valid & stratum), folded into the two integer sums lo = sum max(0, k + m - n) and
//       hi = sum min(k, m): the support of a' under within-stratum shuffles.  A kernel of its own, so that k_cmh
//       compiles to what it compiled to before there were tables.  k_minp_scan (scoary_common.hpp) turns the sizes
//       into offsets.
//   k_cmh_fill : one wavefront per (trait, gene); its lanes stride over the gene's entries, so a wavefront's stores
//       are one contiguous run of the table.  u(x) = 1 / (1 + cmh_stat(x)) from d_e2 and d_var as scoary_cmh wrote
//       them: a few flops per entry, no table list, 64-bit entry indices throughout.
//
// The homogeneity of the odds ratios over the strata (spec S14): the Breslow-Day statistic with Tarone's correction.
//   k_cmh_homog : k_cmh's geometry (two traits per block) and cmh_walk once more, counting (a, m) per segment as k_cmh does; the fold fits
//       every informative stratum's table to the common odds ratio scoary_cmh wrote to d_odds (read, never recomputed)
//       and sums the three terms of the statistic; chi2_tail gives the upper tail at up to 1023 degrees of freedom.
//       A kernel of its own, so that k_cmh, k_cmh_support and k_cmh_fill compile to what they compiled to before.
//
// The entry points check their arguments with strata_check / check_args and build the table through
// scoary_cmh_segments_launch (both declared in scoary_common.hpp, shared with scoary_cmh_exact.hip).
#include <cstddef>

#include "scoary_chi2.hpp"
#include "scoary_common.hpp"

namespace {

constexpr int kCmhTraits = 4;        // traits per block: 9 accumulator registers each, far from a spill
constexpr int kCmhThreads = 256;     // = kGeneAlign: a block is 256 consecutive genes
constexpr int kSegThreads = 1024;
constexpr double kCmhTau = 1e-6;     // S10: the tie tolerance of the region, above the fp64 error of E2

// the isolate at position j of the members array and its segment key; every index clamped (a bad plan gives
// wrong counts, never a wild access)
__device__ __forceinline__ uint32_t seg_key(const int32_t* __restrict__ members, const uint16_t* __restrict__ strata,
                                            int j, int N, int S, int& isolate) {
  isolate = min(max(members[j], 0), N - 1);
  const uint32_t s = min((int)strata[isolate], S - 1);
  return (s << 16) | (uint32_t)(isolate >> 5);
}

__global__ __launch_bounds__(kSegThreads) void k_cmh_segments(const uint16_t* __restrict__ strata,
                                                              const int32_t* __restrict__ members, int N, int S,
                                                              CmhSegments* __restrict__ out) {
  __shared__ int heads[kSegThreads];
  const int tid = threadIdx.x;
  const int per = (N + kSegThreads - 1) / kSegThreads;
  const int j0 = min(tid * per, N), j1 = min(j0 + per, N);
  // a member starts a segment when its key differs from its predecessor's
  auto is_head = [&](int j) {
    int i;
    return j == 0 || seg_key(members, strata, j, N, S, i) != seg_key(members, strata, j - 1, N, S, i);
  };
  int mine = 0;
  for (int j = j0; j < j1; ++j) mine += is_head(j);
  heads[tid] = mine;
  block_scan<kSegThreads>(heads, tid, [](int x, int y) { return x + y; });   // the per-thread head counts
  int slot = heads[tid] - mine;
  if (tid == kSegThreads - 1) out->count = (uint32_t)heads[tid];
  for (int j = j0; j < j1; ++j) {
    if (!is_head(j)) continue;
    int i;
    const uint32_t key = seg_key(members, strata, j, N, S, i);
    uint32_t mask = 1u << (i & 31);
    for (int k = j + 1; k < N; ++k) {                   // the run of this key: at most 32 members of a sound plan
      if (seg_key(members, strata, k, N, S, i) != key) break;
      mask |= 1u << (i & 31);
    }
    out->seg[slot++] = make_uint2(key, mask);           // slot < number of heads <= N
  }
}

// THE walk of the segment table by the lane of gene g (k_cmh, k_cmh_support): seg(w, gene word & segment mask) per
// segment, fold(s) on every change of stratum and at the end, empty(s0, s1) for the strata [s0, s1) without a
// member.  Stratum and word are clamped (a bad table gives wrong counts, never a wild access); the quad of the gene
// row is reloaded only when the word leaves it.
template <class Seg, class Fold, class Empty>
__device__ __forceinline__ void cmh_walk(const uint32_t* __restrict__ tiled, const CmhSegments* __restrict__ segs,
                                         int64_t Gp, int64_t g, int N, int Wp, int S, Seg seg, Fold fold,
                                         Empty empty) {
  const uint4* __restrict__ quads = reinterpret_cast<const uint4*>(tiled);
  const int nseg = min((int)segs->count, N);
  int cur_s = -1, cur_q = -1;
  uint4 gq = make_uint4(0, 0, 0, 0);
  for (int i = 0; i < nseg; ++i) {
    const uint2 sg = segs->seg[i];                                        // wave-uniform
    const int s = min((int)(sg.x >> 16), S - 1), w = min((int)(sg.x & 0xffffu), Wp - 1);
    if (s != cur_s) {
      if (cur_s >= 0) fold(cur_s);
      empty(cur_s + 1, s);
      cur_s = s;
    }
    if ((w >> 2) != cur_q) {
      cur_q = w >> 2;
      gq = quads[(int64_t)cur_q * Gp + g];
    }
    const int c = w & 3;
    seg(w, (c == 0 ? gq.x : c == 1 ? gq.y : c == 2 ? gq.z : gq.w) & sg.y);
  }
  if (cur_s >= 0) fold(cur_s);
  empty(cur_s + 1, S);
}

// S10 / S11: the continuity-corrected statistic at the pooled count x, half = E2 / 2, v != 0; every operation
// rounded on its own, so k_cmh's stat and k_cmh_fill's entry at the same count are the same double
__device__ __forceinline__ double cmh_stat(double x, double half, double v) {
  const double delta = fabs(x - half);
  const double y = fmin(0.5, delta);
  return ((delta - y) * (delta - y)) / v;
}

struct CmhOut {
  double *stat, *p, *odds, *e2, *var;
  int32_t* a;
  uint32_t* crit;
  int32_t* scounts;
};

__global__ __launch_bounds__(kCmhThreads) void k_cmh(const uint32_t* __restrict__ tiled,
                                                     const uint32_t* __restrict__ labels,
                                                     const uint32_t* __restrict__ masks,
                                                     const int32_t* __restrict__ smargins,
                                                     const CmhSegments* __restrict__ segs, int64_t G, int64_t Gp,
                                                     int T, int N, int Wp, int S, CmhOut out) {
  const int64_t g = (int64_t)blockIdx.x * kCmhThreads + threadIdx.x;      // < Gp: the grid covers Gp exactly
  const int t0 = blockIdx.y * kCmhTraits;

  int32_t A[kCmhTraits], K[kCmhTraits];     // K: the positives of the counted strata (wave-uniform)
  double E2[kCmhTraits], V[kCmhTraits], R[kCmhTraits], Q[kCmhTraits];
  uint32_t a[kCmhTraits], m[kCmhTraits];
#pragma unroll
  for (int j = 0; j < kCmhTraits; ++j) A[j] = K[j] = 0, E2[j] = V[j] = R[j] = Q[j] = 0.0, a[j] = m[j] = 0;

  // trait j of the block, clamped for reading (the surplus traits of the last block are computed and dropped)
  auto trait = [&](int j) { return min(t0 + j, T - 1); };
  auto put_scounts = [&](int j, int s, uint32_t aa, uint32_t mm) {
    if (out.scounts && g < G && t0 + j < T)
      reinterpret_cast<int2*>(out.scounts)[((int64_t)(t0 + j) * G + g) * S + s] = make_int2((int)aa, (int)mm);
  };
  // S10, accumulation: stratum s with this lane's (a, m) and the stratum's margins (k, n)
  auto fold = [&](int s) {
#pragma unroll
    for (int j = 0; j < kCmhTraits; ++j) {
      const int2 kn = reinterpret_cast<const int2*>(smargins)[(int64_t)trait(j) * S + s];
      const int64_t k = kn.x, n = kn.y, mm = m[j], aa = a[j];
      put_scounts(j, s, a[j], m[j]);
      a[j] = m[j] = 0;
      if (n <= 0) continue;
      const double dn = (double)n;
      A[j] += (int32_t)aa;
      K[j] += (int32_t)k;
      E2[j] += (double)(2 * k * mm) / dn;
      if (n >= 2)
        V[j] += (((double)k * (double)(n - k)) * ((double)mm * (double)(n - mm))) / ((dn * dn) * (double)(n - 1));
      const int64_t b = k - aa, c = mm - aa, d = n - k - mm + aa;
      R[j] += (double)(aa * d) / dn;
      Q[j] += (double)(b * c) / dn;
    }
  };

  cmh_walk(
      tiled, segs, Gp, g, N, Wp, S,
      [&](int w, uint32_t gw) {
#pragma unroll
        for (int j = 0; j < kCmhTraits; ++j) {
          const int64_t row = (int64_t)trait(j) * Wp + w;
          bcnt_acc(m[j], gw & masks[row]);
          bcnt_acc(a[j], gw & labels[row]);
        }
      },
      fold,
      [&](int s0, int s1) {                                               // strata without a member: all-zero tables
        for (int z = s0; z < s1; ++z)
          for (int j = 0; j < kCmhTraits; ++j) put_scounts(j, z, 0, 0);
      });

  if (g >= G) return;
#pragma unroll
  for (int j = 0; j < kCmhTraits; ++j) {
    if (t0 + j >= T) continue;
    const int64_t o = (int64_t)(t0 + j) * G + g;
    const double dA = (double)A[j];
    double stat = __builtin_nan(""), p = 1.0;
    int64_t lo = 0, hi = -1;                                              // the accepted integers; empty: (0, 0)
    if (V[j] != 0.0) {
      stat = cmh_stat(dA, 0.5 * E2[j], V[j]);
      p = erfc(sqrt(stat / 2.0));
      const double diff = 2.0 * dA - E2[j];
      if (diff > kCmhTau) {
        lo = (int64_t)floor((E2[j] - dA) + kCmhTau) + 1, hi = (int64_t)A[j] - 1;
      } else if (diff < -kCmhTau) {
        lo = (int64_t)A[j] + 1, hi = (int64_t)ceil((E2[j] - dA) - kCmhTau) - 1;
      }
    }
    if (lo < 0) lo = 0;
    if (hi > K[j]) hi = K[j];           // no pooled count exceeds the positives; the list kernels want base + span <= npos + 1
    const int64_t span = hi - lo + 1;
    out.stat[o] = stat;
    out.p[o] = p;
    out.odds[o] = Q[j] != 0.0 ? R[j] / Q[j] : (R[j] > 0.0 ? __builtin_inf() : __builtin_nan(""));
    out.e2[o] = E2[j];
    out.var[o] = V[j];
    out.a[o] = A[j];
    reinterpret_cast<uint2*>(out.crit)[o] = span > 0 ? make_uint2((uint32_t)lo, (uint32_t)span) : make_uint2(0u, 0u);
  }
}


// ---- S11: the tables of the Westfall-Young passes over the CMH statistic ----

constexpr int64_t kCmhFillRows = (int64_t)1 << 28;   // (trait, gene) rows per k_cmh_fill launch: 2^26 blocks

// S11 step 1.  k_cmh's geometry (lane = gene, kCmhTraits traits per block) and cmh_walk with the validity words alone;
// the stratum's m of a trait is folded at every change of stratum, strata without a valid isolate skipped as in S10.
__global__ __launch_bounds__(kCmhThreads) void k_cmh_support(const uint32_t* __restrict__ tiled,
                                                             const uint32_t* __restrict__ masks,
                                                             const int32_t* __restrict__ smargins,
                                                             const CmhSegments* __restrict__ segs, int64_t G,
                                                             int64_t Gp, int T, int N, int Wp, int S,
                                                             int64_t* __restrict__ off, int32_t* __restrict__ lo_out) {
  const int64_t g = (int64_t)blockIdx.x * kCmhThreads + threadIdx.x;      // < Gp: the grid covers Gp exactly
  const int t0 = blockIdx.y * kCmhTraits;

  int32_t lo[kCmhTraits], hi[kCmhTraits];
  uint32_t m[kCmhTraits];
#pragma unroll
  for (int j = 0; j < kCmhTraits; ++j) lo[j] = hi[j] = 0, m[j] = 0;
  auto trait = [&](int j) { return min(t0 + j, T - 1); };
  auto fold = [&](int s) {
#pragma unroll
    for (int j = 0; j < kCmhTraits; ++j) {
      const int2 kn = reinterpret_cast<const int2*>(smargins)[(int64_t)trait(j) * S + s];
      const int mm = (int)m[j];
      m[j] = 0;
      if (kn.y <= 0) continue;
      lo[j] += max(0, kn.x + mm - kn.y);
      hi[j] += min(kn.x, mm);
    }
  };

  cmh_walk(
      tiled, segs, Gp, g, N, Wp, S,
      [&](int w, uint32_t gw) {
#pragma unroll
        for (int j = 0; j < kCmhTraits; ++j) bcnt_acc(m[j], gw & masks[(int64_t)trait(j) * Wp + w]);
      },
      fold, [](int, int) {});

  if (g >= G) return;
#pragma unroll
  for (int j = 0; j < kCmhTraits; ++j) {
    if (t0 + j >= T) continue;
    const int64_t o = (int64_t)(t0 + j) * G + g;
    off[o] = max(hi[j] - lo[j], 0) + 1;       // a sound plan has hi >= lo; any other still gets a table of one entry
    lo_out[o] = lo[j];
  }
}

// S11 steps 2 and 3 for the rows [r0, r0 + nrows) of the [T * G] (trait, gene) pairs: wavefront = row, lane l writes
// the entries l, l + 64, ... of the row's run tab[off[i] .. off[i + 1]).  The run is clamped into [0, entries): a
// bad offset array writes wrong values, never outside the table.
__global__ __launch_bounds__(kCmhThreads) void k_cmh_fill(const double* __restrict__ e2, const double* __restrict__ var,
                                                          const int64_t* __restrict__ off,
                                                          const int32_t* __restrict__ lo, int64_t r0, int64_t nrows,
                                                          int64_t entries, double* __restrict__ tab) {
  const int64_t r = (int64_t)blockIdx.x * (kCmhThreads / kWave) + (threadIdx.x / kWave);
  if (r >= nrows) return;
  const int64_t i = r0 + r;                                               // wave-uniform
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t o0 = min(max(off[i], (int64_t)0), entries), o1 = min(max(off[i + 1], o0), entries);
  const double v = var[i];
  double e = e2[i];
  const double whole = rint(e);
  if (fabs(e - whole) <= kCmhTau) e = whole;                               // step 2: the snap
  const double half = 0.5 * e;
  const double x0 = (double)lo[i];
  for (int64_t k = lane; k < o1 - o0; k += kWave) {
    double u = 1.0;
    if (v != 0.0) u = 1.0 / (1.0 + cmh_stat(x0 + (double)k, half, v));   // lo + k is an exact integer
    tab[o0 + k] = u;
  }
}

// ---- S14: the Breslow-Day test of homogeneity with Tarone's correction ----

// traits per block: two -- 64 VGPRs, eight wavefronts per SIMD.  Measured at cfg3's shape against one, four and eight
// (50 / 64 / 96 / 185 VGPRs): the fp64 sqrt and divisions of a fold want the wavefronts more than the walk wants the
// gene quad shared by more traits (profiles/cmh_homog.txt)
constexpr int kHomogTraits = 2;

struct CmhHomogOut {
  double *stat_bd, *stat_tarone, *p;
  int32_t* df;
};

__global__ __launch_bounds__(kCmhThreads) void k_cmh_homog(const uint32_t* __restrict__ tiled,
                                                           const uint32_t* __restrict__ labels,
                                                           const uint32_t* __restrict__ masks,
                                                           const int32_t* __restrict__ smargins,
                                                           const CmhSegments* __restrict__ segs,
                                                           const double* __restrict__ odds, int64_t G, int64_t Gp,
                                                           int T, int N, int Wp, int S, CmhHomogOut out) {
  const int64_t g = (int64_t)blockIdx.x * kCmhThreads + threadIdx.x;      // < Gp: the grid covers Gp exactly
  const int t0 = blockIdx.y * kHomogTraits;

  // trait j of the block, clamped for reading (the surplus traits of the last block are computed and dropped)
  auto trait = [&](int j) { return min(t0 + j, T - 1); };
  double psi[kHomogTraits], A1[kHomogTraits], BD[kHomogTraits], SD[kHomogTraits], SV[kHomogTraits];
  int32_t L[kHomogTraits];
  uint32_t a[kHomogTraits], m[kHomogTraits];
#pragma unroll
  for (int j = 0; j < kHomogTraits; ++j) {
    const double o = odds[(int64_t)trait(j) * G + min(g, G - 1)];         // the lanes past G read gene G - 1
    psi[j] = o > 0.0 && o < __builtin_inf() ? o : __builtin_nan("");      // nan: a row without a result
    A1[j] = 1.0 - psi[j];
    BD[j] = SD[j] = SV[j] = 0.0, L[j] = 0, a[j] = m[j] = 0;
  }

  // S14, steps 1-7: stratum s with this lane's (a, m) and the stratum's margins (k, n)
  auto fold = [&](int s) {
#pragma unroll
    for (int j = 0; j < kHomogTraits; ++j) {
      const int2 kn = reinterpret_cast<const int2*>(smargins)[(int64_t)trait(j) * S + s];
      const int k = kn.x, n = kn.y, mm = (int)m[j], aa = (int)a[j];
      a[j] = m[j] = 0;
      if (!(n > 0 && 0 < k && k < n && 0 < mm && mm < n) || psi[j] != psi[j]) continue;
      const double dk = (double)k, dm = (double)mm;
      const int r = n - k - mm, km = k - mm;                              // (products of these stay below 2^31)
      const double rest = (double)r;
      const double B = rest + psi[j] * (double)(k + mm);
      const double C = psi[j] * (dk * dm);
      // the discriminant B B + 4 (1 - psi) C as a sum of non-negative terms: no cancellation at a large psi
      const double root = sqrt(((double)(r * r) + (psi[j] * psi[j]) * (double)(km * km)) +
                               (2.0 * psi[j]) * (double)(k * (n - k) + mm * (n - mm)));
      const double x = B >= 0.0 ? (2.0 * C) / (B + root) : (root - B) / (2.0 * A1[j]);
      const double w = ((1.0 / x + 1.0 / (dk - x)) + 1.0 / (dm - x)) + 1.0 / (rest + x);
      const double d = (double)aa - x;
      BD[j] += (d * d) * w;
      SD[j] += d;
      SV[j] += 1.0 / w;
      L[j] += 1;
    }
  };

  cmh_walk(
      tiled, segs, Gp, g, N, Wp, S,
      [&](int w, uint32_t gw) {
#pragma unroll
        for (int j = 0; j < kHomogTraits; ++j) {
          const int64_t row = (int64_t)trait(j) * Wp + w;
          bcnt_acc(m[j], gw & masks[row]);
          bcnt_acc(a[j], gw & labels[row]);
        }
      },
      fold, [](int, int) {});

  if (g >= G) return;
#pragma unroll
  for (int j = 0; j < kHomogTraits; ++j) {
    if (t0 + j >= T) continue;
    const int64_t o = (int64_t)(t0 + j) * G + g;
    double bd = __builtin_nan(""), tarone = __builtin_nan(""), p = 1.0;
    int32_t df = 0;
    if (L[j] >= 2) {
      bd = BD[j];
      tarone = fmax(BD[j] - (SD[j] * SD[j]) / SV[j], 0.0);
      df = L[j] - 1;
      p = chi2_tail(tarone, df);
    }
    out.stat_bd[o] = bd;
    out.stat_tarone[o] = tarone;
    out.df[o] = df;
    out.p[o] = p;
  }
}

}  // namespace

int scoary_cmh_segments_launch(scoary_handle h, hipStream_t s, const uint16_t* d_strata, const int32_t* d_members,
                               int64_t N, int64_t S, void* d_scratch, const char* event) {
  KernelTimer kt(h, s, event);
  hipLaunchKernelGGL(k_cmh_segments, dim3(1), dim3(kSegThreads), 0, s, d_strata, d_members, (int)N, (int)S,
                     static_cast<CmhSegments*>(d_scratch));
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

extern "C" {

int64_t scoary_cmh_scratch_bytes(int64_t N) {
  return N < 1 ? 0 : (int64_t)offsetof(CmhSegments, seg) + N * (int64_t)sizeof(uint2);
}

int scoary_cmh(scoary_handle h, const uint32_t* d_tiled, const uint32_t* d_labels, const uint32_t* d_masks,
               const uint16_t* d_strata, const int32_t* d_members, const int32_t* d_offsets,
               const int32_t* d_smargins, int64_t G, int64_t T, int64_t N, int64_t S, double* d_stat, double* d_p,
               double* d_odds, double* d_e2, double* d_var, int32_t* d_a, uint32_t* d_crit, int32_t* d_scounts,
               void* d_scratch, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = strata_check(h, "scoary_cmh", d_tiled && d_labels && d_masks && d_strata && d_members && d_offsets &&
                                                  d_smargins && d_stat && d_p && d_odds && d_e2 && d_var && d_a &&
                                                  d_crit && d_scratch && G >= 1, T, N, S))
    return rc;
  const int64_t Gp = scoary_tiled_genes(G);
  if (Gp / kCmhThreads > 0x7fffffffLL) return fail(h, SCOARY_ERR_SIZE, "scoary_cmh: grid too large");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = scoary_cmh_segments_launch(h, s, d_strata, d_members, N, S, d_scratch, "k_cmh_segments")) return rc;
  const CmhOut out{d_stat, d_p, d_odds, d_e2, d_var, d_a, d_crit, d_scounts};
  KernelTimer kt(h, s, "k_cmh");
  hipLaunchKernelGGL(k_cmh, dim3((unsigned)(Gp / kCmhThreads), (unsigned)((T + kCmhTraits - 1) / kCmhTraits)),
                     dim3(kCmhThreads), 0, s, d_tiled, d_labels, d_masks, d_smargins,
                     static_cast<const CmhSegments*>(d_scratch), G, Gp, (int)T, (int)N, (int)scoary_row_words(N), (int)S,
                     out);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}


int scoary_cmh_minp_plan(scoary_handle h, const uint32_t* d_tiled, const uint32_t* d_masks, const uint16_t* d_strata,
                         const int32_t* d_members, const int32_t* d_offsets, const int32_t* d_smargins, int64_t G,
                         int64_t T, int64_t N, int64_t S, void* d_scratch, int64_t* d_off, int32_t* d_lo,
                         int64_t* entries_out, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = strata_check(h, "scoary_cmh_minp_plan", d_tiled && d_masks && d_strata && d_members && d_offsets &&
                                                            d_smargins && d_scratch && d_off && d_lo && entries_out &&
                                                            G >= 1, T, N, S))
    return rc;
  if (G > (int64_t)1 << 30) return fail(h, SCOARY_ERR_SIZE, "scoary_cmh_minp_plan: G > 2^30");
  const int64_t Gp = scoary_tiled_genes(G);
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t M = T * G;
  {
    KernelTimer kt(h, s, "k_cmh_minp_plan");           // the one event of the plan's three launches
    if (int rc = scoary_cmh_segments_launch(h, s, d_strata, d_members, N, S, d_scratch, nullptr)) return rc;
    hipLaunchKernelGGL(k_cmh_support, dim3((unsigned)(Gp / kCmhThreads), (unsigned)((T + kCmhTraits - 1) / kCmhTraits)),
                       dim3(kCmhThreads), 0, s, d_tiled, d_masks, d_smargins, static_cast<const CmhSegments*>(d_scratch),
                       G, Gp, (int)T, (int)N, (int)scoary_row_words(N), (int)S, d_off, d_lo);
    hipLaunchKernelGGL(k_minp_scan, dim3(1), dim3(1024), 0, s, d_off, M);
    HIP_TRY(h, hipGetLastError());
  }
  // the one read-back of the path, as in scoary_minp_plan: the caller sizes the table with it
  HIP_TRY(h, hipMemcpyAsync(entries_out, d_off + M, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return SCOARY_OK;
}

int scoary_cmh_minp_fill(scoary_handle h, const double* d_e2, const double* d_var, const int64_t* d_off,
                         const int32_t* d_lo, int64_t T, int64_t G, int64_t entries, double* d_tab,
                         scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = check_args(h, "scoary_cmh_minp_fill",
                          d_e2 && d_var && d_off && d_lo && d_tab && T >= 1 && G >= 1 && entries >= T * G))
    return rc;
  if (T > 65535 || G > (int64_t)1 << 30)
    return fail(h, SCOARY_ERR_SIZE, "scoary_cmh_minp_fill: T > 65535 or G > 2^30");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t M = T * G;
  constexpr int rows_per_block = kCmhThreads / kWave;
  KernelTimer kt(h, s, "k_cmh_minp_fill");
  for (int64_t r0 = 0; r0 < M; r0 += kCmhFillRows) {
    const int64_t nrows = std::min(kCmhFillRows, M - r0);
    hipLaunchKernelGGL(k_cmh_fill, dim3((unsigned)((nrows + rows_per_block - 1) / rows_per_block)), dim3(kCmhThreads),
                       0, s, d_e2, d_var, d_off, d_lo, r0, nrows, entries, d_tab);
    HIP_TRY(h, hipGetLastError());
  }
  return SCOARY_OK;
}

int scoary_cmh_homogeneity(scoary_handle h, const uint32_t* d_tiled, const uint32_t* d_labels,
                           const uint32_t* d_masks, const uint16_t* d_strata, const int32_t* d_members,
                           const int32_t* d_offsets, const int32_t* d_smargins, int64_t G, int64_t T, int64_t N,
                           int64_t S, const double* d_odds, double* d_stat_bd, double* d_stat_tarone, int32_t* d_df,
                           double* d_p, void* d_scratch, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = strata_check(h, "scoary_cmh_homogeneity",
                            d_tiled && d_labels && d_masks && d_strata && d_members && d_offsets && d_smargins &&
                                d_odds && d_stat_bd && d_stat_tarone && d_df && d_p && d_scratch && G >= 1, T, N, S))
    return rc;
  const int64_t Gp = scoary_tiled_genes(G);
  if (Gp / kCmhThreads > 0x7fffffffLL) return fail(h, SCOARY_ERR_SIZE, "scoary_cmh_homogeneity: grid too large");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = scoary_cmh_segments_launch(h, s, d_strata, d_members, N, S, d_scratch, "k_cmh_segments")) return rc;
  const CmhHomogOut out{d_stat_bd, d_stat_tarone, d_p, d_df};
  KernelTimer kt(h, s, "k_cmh_homog");
  hipLaunchKernelGGL(k_cmh_homog, dim3((unsigned)(Gp / kCmhThreads), (unsigned)((T + kHomogTraits - 1) / kHomogTraits)),
                     dim3(kCmhThreads), 0, s, d_tiled, d_labels, d_masks, d_smargins,
                     static_cast<const CmhSegments*>(d_scratch), d_odds, G, Gp, (int)T, (int)N,
                     (int)scoary_row_words(N), (int)S, out);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
