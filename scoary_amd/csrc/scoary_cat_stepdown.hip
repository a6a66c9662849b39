// scoary_cat_stepdown.hip -- Westfall-Young step-down maxT over the statistics of the categorical traits (spec S23 of
// DESIGN.md): S22's statistic s -- the chi-square one or the generalized CMH Q -- with the genes of a trait walked in
// rank order (descending comparison point thr), the gene at rank k compared per permuted code row with u[k] = the
// maximum of s over the ranks k and behind.
//
// The blocks are CatStage's (scoary_cat_planes.hpp): a lane is a permutation, wavefront w of a block counts the
// positions 64 grp + 4 w + j of gene group grp.  A suffix maximum over the ranks is lane-local where a wavefront
// walks consecutive ranks, and the gather arranges that: with Gs = G rounded up to 1024 and a SUPERGROUP sg = 16
// consecutive groups, position 1024 sg + 64 i + 4 w + j holds rank 1024 sg + 64 w + 4 i + j (a transpose of quads
// inside the supergroup, an involution), so wavefront w walks the 64 consecutive ranks of RUN rho = 16 sg + w over
// the groups i = 0 .. 15: no barrier, no LDS exchange and no shuffle beyond what count_group already has.
//
//   k_cat_sd_gather   (once per analysis)  every trait's gene rows copied into position order as a tiled matrix of
//                                          width Gs, and next to them what the hot loop reads per gene (chi-square:
//                                          a_obs[8], ivm, thr; gcmh: the form and thr); a position whose rank is >= G
//                                          holds a zero row, zeros and thr = +inf
//   k_cat_sd_max, k_gcmh_sd_max  (pass A)  k_cat_maxt's / k_gcmh_maxt's loop body over every ranges-th supergroup:
//                                          the plain exceedance count by rank position, and a lane's maximum of s
//                                          over each run, stored to gmax[t][rho][column] -- one owner per cell
//   k_cat_sd_suffix                        one lane per (trait, column) walks the runs from the last to the first:
//                                          gmax becomes the maximum over the runs BEHIND each run, the overall
//                                          maximum goes to maxs (S22's, bit for bit)
//   k_cat_sd_count, k_gcmh_sd_count  (pass B)  the same counts again, a run walked from its last rank to its first
//                                          with u kept in a register, started from the run's suffix: u = max(u, s),
//                                          and u >= thr is counted per rank
// No block waits for another: the order of the work is the order of three launches on one stream.
#include "scoary_cat_planes.hpp"
#include "scoary_common.hpp"
#include "scoary_gcmh_form.hpp"

namespace {

constexpr int kSdSuper = 16;                                  // groups of a supergroup: a run is 16 x kCatHold ranks
constexpr int kSdSuperGenes = kSdSuper * kCatGroup;           // 1024 positions
constexpr int kSdRun = kSdSuper * kCatHold;                   // 64 ranks
static_assert(kSdSuper == kCatWaves, "the transpose of quads swaps a supergroup's groups with a group's wavefronts");
// further bits of cat_lds_optin, behind scoary_cat_planes.hpp's four
enum : int { kCatSdOptinMax = 16, kCatSdOptinCount = 32, kGcmhSdOptinMax = 64, kGcmhSdOptinCount = 128 };

// the rank that position p holds
__host__ __device__ constexpr int64_t sd_rank_of(int64_t p) {
  return (p & ~(int64_t)(kSdSuperGenes - 1)) + ((p >> 2) & 15) * kSdRun + ((p >> 6) & 15) * kCatHold + (p & 3);
}
static_assert(sd_rank_of(sd_rank_of(1024 + 64 * 3 + 4 * 5 + 2)) == 1024 + 64 * 3 + 4 * 5 + 2 &&
                  sd_rank_of(64 * 3 + 4 * 5 + 2) == 64 * 5 + 4 * 3 + 2,
              "position 64 i + 4 w + j holds rank 64 w + 4 i + j, and back");

// A wave-uniform value that only vector instructions need (the address of a lane's store, of lane 0's atomic, of a
// load every lane takes alike) kept in vector registers: the hot kernels have vector registers to spare and none of
// the scalar ones (their siblings already keep SGPRs in VGPR lanes).
template <class V>
__device__ __forceinline__ V sd_in_vgprs(V x) {
  asm volatile("" : "+v"(x));
  return x;
}

// d_scratch: byte offsets of its parts.  Everything before gmax is what the gather writes and does not depend on P.
struct CatSdLayout {
  int64_t Gs, Qs, runs, cols;       // padded positions, quads per row, runs of 64 ranks, padded columns
  int64_t rows, a, ivm, form, thr, gmax, total;
};
CatSdLayout cat_sd_layout(int64_t G, int64_t T, int64_t N, int64_t P, bool gcmh) {
  CatSdLayout l;
  l.Gs = round_up(G, kSdSuperGenes);
  l.Qs = ((N + 31) / 32 + 3) / 4;
  l.runs = l.Gs / kSdRun;
  l.cols = (P + 63) / 64 * 64;
  l.rows = 0;
  l.a = l.form = l.rows + T * l.Qs * l.Gs * 16;
  l.ivm = l.a + T * l.Gs * kCatMaxClasses * 4;
  l.thr = gcmh ? l.form + T * l.Gs * kGcmhForm * 8 : l.ivm + T * l.Gs * 8;
  l.gmax = l.thr + T * l.Gs * 8;
  l.total = l.gmax + T * l.runs * l.cols * 8;
  return l;
}

// position p of trait blockIdx.z, quad blockIdx.y: the row of gene order[t][rank of p], zero where that is no gene.
// The blocks of quad 0 copy the per-gene values too: `na` 64-bit words a gene from src_a (a_obs as four words, or
// the form's 35), one from src_b where there is one (ivm), and thr.
__global__ __launch_bounds__(256) void k_cat_sd_gather(const uint4* __restrict__ tiled, int64_t Gp,
                                                       const int32_t* __restrict__ order, int G, int64_t Gs, int Qs,
                                                       const uint64_t* __restrict__ src_a, int na,
                                                       const double* __restrict__ src_b,
                                                       const double* __restrict__ src_thr, uint4* __restrict__ rows,
                                                       uint64_t* __restrict__ dst_a, double* __restrict__ dst_b,
                                                       double* __restrict__ dst_thr) {
  const int t = blockIdx.z, q = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= Gs) return;
  const int64_t k = sd_rank_of(p);
  int g = k < G ? order[(int64_t)t * G + k] : -1;
  if ((unsigned)g >= (unsigned)G) g = -1;          // (an index that is no gene reads nothing)
  rows[((int64_t)t * Qs + q) * Gs + p] = g >= 0 ? tiled[(int64_t)q * Gp + g] : make_uint4(0u, 0u, 0u, 0u);
  if (q == 0) {
    const int64_t o = (int64_t)t * G + g, d = (int64_t)t * Gs + p;
    for (int x = 0; x < na; ++x) dst_a[d * na + x] = g >= 0 ? src_a[o * na + x] : 0ull;
    if (src_b) dst_b[d] = g >= 0 ? src_b[o] : 0.0;
    dst_thr[d] = g >= 0 ? src_thr[o] : __builtin_huge_val();
  }
}

// The block of k_cat_sd_max (kCount = false) and of k_cat_sd_count (true): CatStage's over the gathered matrix of
// width Gs, stage s of trait t x the supergroups rng, rng + ranges, ..  Behind a group's last chunk, per position and
// lane, the table a_k and S22's statistic s of it exactly as k_cat_maxt forms them (cat_wy_add over the classes up to
// the last non-empty one, one multiplication by ivm).  Pass A: S20's integer comparison with the observed table,
// counted into d_out[t][rank], and u = the maximum of s over the run, stored behind its 16th group.  Pass B: the run
// from its last rank to its first, u from gmax (the maximum behind the run), u = max(u, s), and u >= thr counted
// into d_out[t][rank].  A position whose rank is >= G reaches no count: a test of the rank, not of the data (a zero
// table would pass the integer comparison).  All wavefronts of a block walk the same groups, so count_group's
// barriers are met by all of them whatever their ranks.
template <bool kCount>
__device__ __forceinline__ void cat_sd_block(const uint32_t* rows_all, int64_t Gs, int Qs, int G, int N,
                                             const int16_t* rows, int64_t P, int S, const int32_t* aobs,
                                             const double* d_ivm, const double* d_thr, const int32_t* nk,
                                             const uint64_t* wt, const double* d_inv, int ranges, int lds_words,
                                             int32_t* d_out, double* gmax) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t* planes = reinterpret_cast<uint32_t*>(lds);
  const int t = blockIdx.y;
  const int32_t* nkt = nk + t * kCatMaxClasses;
  int klast = 0, n = 0;
#pragma unroll
  for (int k = 0; k < kCatMaxClasses; ++k)
    if (nkt[k] > 0) klast = k + 1, n += nkt[k];
  CatStage st(N, (int)Gs, P, S, klast);
  const int lane = st.lane;
  const uint64_t* w = wt + (int64_t)t * 2 * kCatMaxClasses;
  const double* inv = d_inv + t * kCatMaxClasses;
  const uint32_t* tiled = rows_all + (int64_t)t * Qs * Gs * 4;
  const int32_t* aot = aobs + (int64_t)t * Gs * kCatMaxClasses;
  const double* ivt = sd_in_vgprs(d_ivm + (int64_t)t * Gs);
  const double* tht = sd_in_vgprs(d_thr + (int64_t)t * Gs);
  int32_t* out = sd_in_vgprs(d_out + (int64_t)t * G);
  const int64_t cols = (int64_t)S * 64;
  // the lane's cell of run 16 rng + wave, and the way to the block's next supergroup
  double* gm = gmax + ((int64_t)t * (Gs / kSdRun) + st.rng * kSdSuper + st.wave) * cols + (int64_t)st.s * 64 + lane;
  const int64_t gm_step = sd_in_vgprs((int64_t)ranges * kSdSuper * cols);

  for (int sg = st.rng; sg < st.ngroups / kSdSuper; sg += ranges, gm += gm_step) {
    double u = 0.0;
    if constexpr (kCount) u = *gm;
#pragma unroll 1
    for (int ii = 0; ii < kSdSuper; ++ii) {
      const int i = kCount ? kSdSuper - 1 - ii : ii;
      const int grp = sg * kSdSuper + i;
      const int p0 = st.first_gene(grp), k0 = sg * kSdSuperGenes + st.wave * kSdRun + i * kCatHold;
      uint32_t cnt[kCatHold][kCatPlanes] = {};
      st.count_group(grp, planes, lds_words, tiled, Gs, rows, P, N, cnt);
#pragma unroll
      for (int jj = 0; jj < kCatHold; ++jj) {
        const int j = kCount ? kCatHold - 1 - jj : jj;
        if (k0 + j >= G) {
          if constexpr (kCount) continue;
          else break;
        }
        const int o = p0 + j;
        const int32_t* ao = aot + (int64_t)o * kCatMaxClasses;
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
          if constexpr (!kCount) {
            const int64_t ob = ao[k];
            const int64_t d = (int64_t)a * a - ob * ob;
            H += cat_mul(d, w[2 * k + 1]);
            Lo += cat_mul(d, w[2 * k]);
          }
          tot = cat_wy_add(tot, n, a, m * nkt[k], inv[k]);
        }
        u = fmax(u, tot * ivt[o]);
        if constexpr (kCount) cat_hits(u >= tht[o], st.counted, lane, out + k0 + j);
        else cat_hits(H + (Lo >> 64) >= 0, st.counted, lane, out + k0 + j);
      }
    }
    if constexpr (!kCount) *gm = u;
  }
}

// The same block around k_gcmh_maxt's body: Q of the counts under the position's form, read wave-uniformly.  Pass A
// counts Q >= thr by rank position, as k_gcmh_permute counts it by gene.
template <bool kCount>
__device__ __forceinline__ void gcmh_sd_block(const uint32_t* rows_all, int64_t Gs, int Qs, int G, int N,
                                              const int16_t* rows, int64_t P, int S, const double* form,
                                              const double* d_thr, const int32_t* nk, int ranges, int lds_words,
                                              int32_t* d_out, double* gmax) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t* planes = reinterpret_cast<uint32_t*>(lds);
  const int t = blockIdx.y;
  CatStage st(N, (int)Gs, P, S, gcmh_klast(nk + t * kCatMaxClasses, kCatMaxClasses));
  const int lane = st.lane;
  const uint32_t* tiled = rows_all + (int64_t)t * Qs * Gs * 4;
  const double* fot = form + (int64_t)t * Gs * kGcmhForm;
  const double* tht = sd_in_vgprs(d_thr + (int64_t)t * Gs);
  int32_t* out = sd_in_vgprs(d_out + (int64_t)t * G);
  const int64_t cols = (int64_t)S * 64;
  // the lane's cell of run 16 rng + wave, and the way to the block's next supergroup
  double* gm = gmax + ((int64_t)t * (Gs / kSdRun) + st.rng * kSdSuper + st.wave) * cols + (int64_t)st.s * 64 + lane;
  const int64_t gm_step = sd_in_vgprs((int64_t)ranges * kSdSuper * cols);

  for (int sg = st.rng; sg < st.ngroups / kSdSuper; sg += ranges, gm += gm_step) {
    double u = 0.0;
    if constexpr (kCount) u = *gm;
#pragma unroll 1
    for (int ii = 0; ii < kSdSuper; ++ii) {
      const int i = kCount ? kSdSuper - 1 - ii : ii;
      const int grp = sg * kSdSuper + i;
      const int p0 = st.first_gene(grp), k0 = sg * kSdSuperGenes + st.wave * kSdRun + i * kCatHold;
      uint32_t cnt[kCatHold][kCatPlanes] = {};
      st.count_group(grp, planes, lds_words, tiled, Gs, rows, P, N, cnt);
#pragma unroll 1                                     // (unrolled, four forms wait in SGPRs across the count)
      for (int jj = 0; jj < kCatHold; ++jj) {
        const int j = kCount ? kCatHold - 1 - jj : jj;
        if (k0 + j >= G) {
          if constexpr (kCount) continue;
          else break;
        }
        const int o = p0 + j;
        const double* fo = fot + (int64_t)o * kGcmhForm;   // wave-uniform
        uint32_t a[kCatPlanes];
#pragma unroll
        for (int k = 0; k < kCatPlanes; ++k) {
          a[k] = cnt[0][k];
#pragma unroll
          for (int x = 1; x < kCatHold; ++x) a[k] = j == x ? cnt[x][k] : a[k];
        }
        const double q = st.wide ? gcmh_q<kCatPlanes>(fo, a) : gcmh_q<3>(fo, a);
        u = fmax(u, q);
        cat_hits((kCount ? u : q) >= tht[o], st.counted, lane, out + k0 + j);
      }
    }
    if constexpr (!kCount) *gm = u;
  }
}

// The four hot kernels: plain functions around the templates' instances, so that the build's resource rules and the
// timers know them by these names.
__global__ __launch_bounds__(kCatThreads) void k_cat_sd_max(const uint32_t* __restrict__ rows_all, int64_t Gs, int Qs,
                                                            int G, int N, const int16_t* __restrict__ rows, int64_t P,
                                                            int S, const int32_t* __restrict__ aobs,
                                                            const double* __restrict__ d_ivm,
                                                            const int32_t* __restrict__ nk,
                                                            const uint64_t* __restrict__ wt,
                                                            const double* __restrict__ d_inv, int ranges,
                                                            int lds_words, int32_t* __restrict__ d_r,
                                                            double* __restrict__ gmax) {
  cat_sd_block<false>(rows_all, Gs, Qs, G, N, rows, P, S, aobs, d_ivm, nullptr, nk, wt, d_inv, ranges, lds_words, d_r,
                      gmax);
}

__global__ __launch_bounds__(kCatThreads) void k_cat_sd_count(const uint32_t* __restrict__ rows_all, int64_t Gs,
                                                              int Qs, int G, int N, const int16_t* __restrict__ rows,
                                                              int64_t P, int S, const int32_t* __restrict__ aobs,
                                                              const double* __restrict__ d_ivm,
                                                              const double* __restrict__ d_thr,
                                                              const int32_t* __restrict__ nk,
                                                              const double* __restrict__ d_inv, int ranges,
                                                              int lds_words, int32_t* __restrict__ d_c,
                                                              double* __restrict__ gmax) {
  cat_sd_block<true>(rows_all, Gs, Qs, G, N, rows, P, S, aobs, d_ivm, d_thr, nk, nullptr, d_inv, ranges, lds_words,
                     d_c, gmax);
}

__global__ __launch_bounds__(kCatThreads) void k_gcmh_sd_max(const uint32_t* __restrict__ rows_all, int64_t Gs, int Qs,
                                                             int G, int N, const int16_t* __restrict__ rows,
                                                             int64_t P, int S, const double* __restrict__ form,
                                                             const double* __restrict__ d_thr,
                                                             const int32_t* __restrict__ nk, int ranges,
                                                             int lds_words, int32_t* __restrict__ d_r,
                                                             double* __restrict__ gmax) {
  gcmh_sd_block<false>(rows_all, Gs, Qs, G, N, rows, P, S, form, d_thr, nk, ranges, lds_words, d_r, gmax);
}

__global__ __launch_bounds__(kCatThreads) void k_gcmh_sd_count(const uint32_t* __restrict__ rows_all, int64_t Gs,
                                                               int Qs, int G, int N, const int16_t* __restrict__ rows,
                                                               int64_t P, int S, const double* __restrict__ form,
                                                               const double* __restrict__ d_thr,
                                                               const int32_t* __restrict__ nk, int ranges,
                                                               int lds_words, int32_t* __restrict__ d_c,
                                                               double* __restrict__ gmax) {
  gcmh_sd_block<true>(rows_all, Gs, Qs, G, N, rows, P, S, form, d_thr, nk, ranges, lds_words, d_c, gmax);
}

// lane = (trait blockIdx.y, column): gmax[t][run][column] <- the maximum over the runs behind it (0.0 behind the
// last), and the maximum over all of them to maxs[t][perm_base + column] where the column is a permutation
__global__ __launch_bounds__(256) void k_cat_sd_suffix(double* __restrict__ gmax, int runs, int64_t cols, int64_t P,
                                                       int64_t perm_base, double* __restrict__ maxs,
                                                       int64_t maxs_stride) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int t = blockIdx.y;
  if (col >= cols) return;
  double* g = gmax + (int64_t)t * runs * cols + col;
  double run = 0.0;
#pragma unroll 8
  for (int ri = runs - 1; ri >= 0; --ri) {
    const double v = g[(int64_t)ri * cols];
    g[(int64_t)ri * cols] = run;
    run = fmax(run, v);
  }
  if (col < P) maxs[(int64_t)t * maxs_stride + perm_base + col] = run;
}

// cat_check's rules, and a padded gene count that stays an int
int cat_sd_check(scoary_handle h, const char* what, bool ok, int64_t G, int64_t T, int64_t N, int64_t P) {
  if (int rc = cat_check(h, what, ok, G, T, N, 1, 1, P)) return rc;
  if (G > 0x7fffffffLL - kSdSuperGenes) return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": G >= 2^31 - 1024");
  return SCOARY_OK;
}

// the launch of a pass: cat_launch_plan's LDS figures and opt-in, the ranges counted over supergroups
template <typename Kernel>
int cat_sd_plan(scoary_handle h, const char* what, Kernel kernel, int optin_bit, int64_t Gs, int64_t T, int64_t N,
                int64_t P, CatLaunch* lp) {
  if (int rc = cat_launch_plan(h, what, kernel, optin_bit, Gs, T, N, P, lp)) return rc;
  lp->ranges = std::min<int64_t>(Gs / kSdSuperGenes,
                                 std::max<int64_t>(1, (4 * (int64_t)h->num_cu + lp->S * T - 1) / (lp->S * T)));
  if (lp->S * lp->ranges > 0x7fffffffLL || (lp->S * 64 + 255) / 256 > 0x7fffffffLL)
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": grid too large");
  return SCOARY_OK;
}

int cat_sd_gather(scoary_handle h, const char* what, const uint32_t* d_tiled, const int32_t* d_order,
                  const void* src_a, int na, const double* src_b, const double* src_thr, int64_t G, int64_t T,
                  int64_t N, void* d_scratch, bool gcmh, hipStream_t s) {
  DeviceGuard guard(h->device);
  const CatSdLayout l = cat_sd_layout(G, T, N, 1, gcmh);
  if (l.Gs / 256 > 0x7fffffffLL) return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": grid too large");
  unsigned char* base = static_cast<unsigned char*>(d_scratch);
  KernelTimer kt(h, s, "k_cat_sd_gather");
  hipLaunchKernelGGL(k_cat_sd_gather, dim3((unsigned)(l.Gs / 256), (unsigned)l.Qs, (unsigned)T), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(d_tiled), scoary_tiled_genes(G), d_order, (int)G, l.Gs, (int)l.Qs,
                     static_cast<const uint64_t*>(src_a), na, src_b, src_thr, reinterpret_cast<uint4*>(base + l.rows),
                     reinterpret_cast<uint64_t*>(base + l.a), reinterpret_cast<double*>(base + l.ivm),
                     reinterpret_cast<double*>(base + l.thr));
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int cat_sd_suffix(scoary_handle h, hipStream_t s, const CatSdLayout& l, double* gmax, int64_t T, int64_t P,
                  int64_t perm_base, double* d_maxs, int64_t maxs_stride) {
  KernelTimer kt(h, s, "k_cat_sd_suffix");
  hipLaunchKernelGGL(k_cat_sd_suffix, dim3((unsigned)((l.cols + 255) / 256), (unsigned)T), dim3(256), 0, s, gmax,
                     (int)l.runs, l.cols, P, perm_base, d_maxs, maxs_stride);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // namespace

extern "C" {

int64_t scoary_cat_stepdown_scratch_bytes(scoary_handle h, int64_t G, int64_t T, int64_t N, int64_t P, int64_t gcmh) {
  if (!h || G < 1 || T < 1 || N < 1 || P < 1 || G > 0x7fffffffLL - kSdSuperGenes) return 0;
  return cat_sd_layout(G, T, N, P, gcmh != 0).total;
}

int scoary_cat_stepdown_gather(scoary_handle h, const uint32_t* d_tiled, const int32_t* d_order, const int32_t* d_a,
                               const double* d_ivm, const double* d_thr, int64_t G, int64_t T, int64_t N,
                               void* d_scratch, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  const char* what = "scoary_cat_stepdown_gather";
  if (int rc = cat_sd_check(h, what, d_tiled && d_order && d_a && d_ivm && d_thr && d_scratch, G, T, N, 1)) return rc;
  return cat_sd_gather(h, what, d_tiled, d_order, d_a, kCatMaxClasses / 2, d_ivm, d_thr, G, T, N, d_scratch, false,
                       static_cast<hipStream_t>(stream));
}

int scoary_gcmh_stepdown_gather(scoary_handle h, const uint32_t* d_tiled, const int32_t* d_order, const double* d_form,
                                const double* d_thr, int64_t G, int64_t T, int64_t N, void* d_scratch,
                                scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  const char* what = "scoary_gcmh_stepdown_gather";
  if (int rc = cat_sd_check(h, what, d_tiled && d_order && d_form && d_thr && d_scratch, G, T, N, 1)) return rc;
  return cat_sd_gather(h, what, d_tiled, d_order, d_form, kGcmhForm, nullptr, d_thr, G, T, N, d_scratch, true,
                       static_cast<hipStream_t>(stream));
}

int scoary_permute_cat_stepdown(scoary_handle h, void* d_scratch, const int16_t* d_rows, const int32_t* d_nk,
                                const uint64_t* d_w, const double* d_inv, int64_t G, int64_t T, int64_t N, int64_t P,
                                int64_t perm_base, int32_t* d_r_rank, int32_t* d_c_rank, double* d_maxs,
                                int64_t maxs_stride, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  const char* what = "scoary_permute_cat_stepdown";
  if (int rc = cat_sd_check(h, what,
                            d_scratch && d_rows && d_nk && d_w && d_inv && d_r_rank && d_c_rank && d_maxs &&
                                perm_base >= 0 && P >= 1 && maxs_stride - perm_base >= P,
                            G, T, N, P))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CatSdLayout l = cat_sd_layout(G, T, N, P, false);
  CatLaunch la, lb;
  if (int rc = cat_sd_plan(h, what, &k_cat_sd_max, kCatSdOptinMax, l.Gs, T, N, P, &la)) return rc;
  if (int rc = cat_sd_plan(h, what, &k_cat_sd_count, kCatSdOptinCount, l.Gs, T, N, P, &lb)) return rc;
  unsigned char* base = static_cast<unsigned char*>(d_scratch);
  const uint32_t* rows_all = reinterpret_cast<const uint32_t*>(base + l.rows);
  const int32_t* aobs = reinterpret_cast<const int32_t*>(base + l.a);
  const double* ivm = reinterpret_cast<const double*>(base + l.ivm);
  const double* thr = reinterpret_cast<const double*>(base + l.thr);
  double* gmax = reinterpret_cast<double*>(base + l.gmax);
  {
    KernelTimer kt(h, s, "k_cat_sd_max");
    hipLaunchKernelGGL(k_cat_sd_max, dim3((unsigned)(la.S * la.ranges), (unsigned)T), dim3(kCatThreads),
                       (size_t)la.lds, s, rows_all, l.Gs, (int)l.Qs, (int)G, (int)N, d_rows, P, (int)la.S, aobs, ivm,
                       d_nk, d_w, d_inv, (int)la.ranges, (int)la.lds_words, d_r_rank, gmax);
    HIP_TRY(h, hipGetLastError());
  }
  if (int rc = cat_sd_suffix(h, s, l, gmax, T, P, perm_base, d_maxs, maxs_stride)) return rc;
  {
    KernelTimer kt(h, s, "k_cat_sd_count");
    hipLaunchKernelGGL(k_cat_sd_count, dim3((unsigned)(lb.S * lb.ranges), (unsigned)T), dim3(kCatThreads),
                       (size_t)lb.lds, s, rows_all, l.Gs, (int)l.Qs, (int)G, (int)N, d_rows, P, (int)lb.S, aobs, ivm,
                       thr, d_nk, d_inv, (int)lb.ranges, (int)lb.lds_words, d_c_rank, gmax);
    HIP_TRY(h, hipGetLastError());
  }
  return SCOARY_OK;
}

int scoary_permute_gcmh_stepdown(scoary_handle h, void* d_scratch, const int16_t* d_rows, const int32_t* d_nk,
                                 int64_t G, int64_t T, int64_t N, int64_t P, int64_t perm_base, int32_t* d_r_rank,
                                 int32_t* d_c_rank, double* d_maxs, int64_t maxs_stride, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  const char* what = "scoary_permute_gcmh_stepdown";
  if (int rc = cat_sd_check(h, what,
                            d_scratch && d_rows && d_nk && d_r_rank && d_c_rank && d_maxs && perm_base >= 0 &&
                                P >= 1 && maxs_stride - perm_base >= P,
                            G, T, N, P))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CatSdLayout l = cat_sd_layout(G, T, N, P, true);
  CatLaunch la, lb;
  if (int rc = cat_sd_plan(h, what, &k_gcmh_sd_max, kGcmhSdOptinMax, l.Gs, T, N, P, &la)) return rc;
  if (int rc = cat_sd_plan(h, what, &k_gcmh_sd_count, kGcmhSdOptinCount, l.Gs, T, N, P, &lb)) return rc;
  unsigned char* base = static_cast<unsigned char*>(d_scratch);
  const uint32_t* rows_all = reinterpret_cast<const uint32_t*>(base + l.rows);
  const double* form = reinterpret_cast<const double*>(base + l.form);
  const double* thr = reinterpret_cast<const double*>(base + l.thr);
  double* gmax = reinterpret_cast<double*>(base + l.gmax);
  {
    KernelTimer kt(h, s, "k_gcmh_sd_max");
    hipLaunchKernelGGL(k_gcmh_sd_max, dim3((unsigned)(la.S * la.ranges), (unsigned)T), dim3(kCatThreads),
                       (size_t)la.lds, s, rows_all, l.Gs, (int)l.Qs, (int)G, (int)N, d_rows, P, (int)la.S, form, thr,
                       d_nk, (int)la.ranges, (int)la.lds_words, d_r_rank, gmax);
    HIP_TRY(h, hipGetLastError());
  }
  if (int rc = cat_sd_suffix(h, s, l, gmax, T, P, perm_base, d_maxs, maxs_stride)) return rc;
  {
    KernelTimer kt(h, s, "k_gcmh_sd_count");
    hipLaunchKernelGGL(k_gcmh_sd_count, dim3((unsigned)(lb.S * lb.ranges), (unsigned)T), dim3(kCatThreads),
                       (size_t)lb.lds, s, rows_all, l.Gs, (int)l.Qs, (int)G, (int)N, d_rows, P, (int)lb.S, form, thr,
                       d_nk, (int)lb.ranges, (int)lb.lds_words, d_c_rank, gmax);
    HIP_TRY(h, hipGetLastError());
  }
  return SCOARY_OK;
}

}  // extern "C"
