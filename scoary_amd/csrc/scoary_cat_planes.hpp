// scoary_cat_planes.hpp -- everything the kernels that count a gene's 2 x K table under label permutations have in
// common (scoary_categorical.hip: k_cat_permute and k_cat_maxt, specs S20 and S22; scoary_gcmh.hip: k_gcmh_permute and
// k_gcmh_maxt, specs S21 and S22), once: the block of a stage of 64 permuted code rows (CatStage: its decode, the
// class bit planes in LDS, the chunk walk and the popcount walk over them), the count of the lanes' verdicts, the
// 128-bit product of S20's integer comparison, the term and the combine of S22's maximum -- which k_cat_wy_prepare
// (scoary_cat_wy.hip) shares with the hot path -- and, on the host, the argument check and the launch plan of their
// entry points.  A kernel keeps what is its own: the loop over a wavefront's four genes behind the last chunk.
#ifndef SCOARY_CAT_PLANES_HPP
#define SCOARY_CAT_PLANES_HPP
#include "scoary_common.hpp"

namespace {

constexpr int kCatMaxClasses = 8;
constexpr int kCatThreads = 1024;                 // sixteen wavefronts
constexpr int kCatWaves = kCatThreads / 64;
constexpr int kCatHold = 4;                       // genes a wavefront counts at a time: one read of a plane word serves four
constexpr int kCatGroup = kCatWaves * kCatHold;   // genes of a block's step
constexpr int kCatPlanes = kCatMaxClasses - 1;    // the last non-empty class needs no plane: its count is m - the others
// words (of 32 isolates) of a chunk: whole quads of the tiled matrix whose seven class planes x 64 permutations stay
// under the 160 KB of a CU (133 KB).  A matrix of up to 2432 isolates is loaded once per block; beyond that a block
// reloads the chunks for every gene group.
constexpr int kCatChunkWords = 76;
constexpr int kCatChunk = 32 * kCatChunkWords;
static_assert(kCatChunkWords % 4 == 0 && kCatPlanes * kCatChunkWords * 256 <= 160 * 1024,
              "a chunk is whole quads and its planes fit the LDS");

// The walk of one gene group over the chunks, for NF class planes (3 while the trait's last non-empty class is at most
// the fourth, else 7).  LDS holds planes[k][w][lane]: bit b of the word = isolate 32 w + b of the chunk has class k + 1
// under the lane's permutation.  cnt[j][k] += popc(gene j's word & plane k's word): a plane word is read once for the
// wavefront's four genes, whose words of a quad are 64 contiguous bytes of the tiled matrix (wave-uniform).
template <int NF>
__device__ __forceinline__ void cat_count(const uint32_t* __restrict__ planes, int lds_words, const uint4* __restrict__ tq,
                                          int64_t Gp, int nquads, uint32_t (&cnt)[kCatHold][kCatPlanes]) {
  for (int q = 0; q < nquads; ++q) {
    uint4 gw[kCatHold];
#pragma unroll
    for (int j = 0; j < kCatHold; ++j) gw[j] = tq[(int64_t)q * Gp + j];
#pragma unroll
    for (int w4 = 0; w4 < 4; ++w4) {
      uint32_t pl[NF];
#pragma unroll
      for (int k = 0; k < NF; ++k) pl[k] = planes[(k * lds_words + 4 * q + w4) * 64];
#pragma unroll
      for (int j = 0; j < kCatHold; ++j) {
        const uint32_t g = w4 == 0 ? gw[j].x : w4 == 1 ? gw[j].y : w4 == 2 ? gw[j].z : gw[j].w;
#pragma unroll
        for (int k = 0; k < NF; ++k) bcnt_acc(cnt[j][k], g & pl[k]);
      }
    }
  }
}

// A block of the hot kernels: stage s = blockIdx.x % S (64 permutations) of trait t = blockIdx.y x the gene groups
// rng, rng + ranges, .. of kCatGroup genes; wavefront `wave` of a group counts its genes first_gene(grp) .. +
// kCatHold - 1; a lane is a permutation, `counted` iff it is one of the P.  klast = the trait's last non-empty class
// (1-based): three planes while it is at most the fourth, else seven.
struct CatStage {
  int t, s, rng, lane, wave, nf, nw, nchunks, ngroups;
  bool wide, counted, loaded;

  __device__ __forceinline__ CatStage(int N, int G, int64_t P, int S, int klast)
      : t(blockIdx.y), s(blockIdx.x % S), rng(blockIdx.x / S), lane(threadIdx.x & 63),
        wave(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)), nf(klast > 4 ? kCatPlanes : 3), nw((N + 31) / 32),
        nchunks((nw + kCatChunkWords - 1) / kCatChunkWords), ngroups((G + kCatGroup - 1) / kCatGroup),
        wide(klast > 4), counted((int64_t)s * 64 + lane < P), loaded(false) {}

  __device__ __forceinline__ int first_gene(int grp) const { return grp * kCatGroup + wave * kCatHold; }

  // chunk c of the stage's 64 code rows -> LDS as class planes: wavefront iteration = (permutation p, word pair wp),
  // 64 isolates of one row read coalesced, a ballot per class gives two plane words; lanes 0 and 1 write them.
  // Isolates past N and permutations past P have no class, and a code that is none of 1 .. 8 matches no plane: no
  // mask is needed and a bad row gives wrong numbers only.
  __device__ __forceinline__ void load(int c, uint32_t* planes, int lds_words, const int16_t* rows, int64_t P,
                                       int N) const {
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
  }

  // cnt[j][k] += |gene first_gene(grp) + j & class k + 1| under the lane's permutation, over all chunks of kCatChunk
  // isolates.  With one chunk in all the planes are built once per block; else every group reloads every chunk.
  // The kernel hands in zeros (`cnt[..][..] = {}` at its own level): zeroed in here, the walk is optimised around an
  // array in memory before it is inlined, and k_cat_permute compiled to 85 VGPRs where it needs at most 64.
  __device__ __forceinline__ void count_group(int grp, uint32_t* planes, int lds_words, const uint32_t* tiled,
                                              int64_t Gp, const int16_t* rows, int64_t P, int N,
                                              uint32_t (&cnt)[kCatHold][kCatPlanes]) {
    for (int c = 0; c < nchunks; ++c) {
      if (!loaded || nchunks > 1) {
        __syncthreads();
        load(c, planes, lds_words, rows, P, N);
        __syncthreads();
        loaded = true;
      }
      const int nquads = (min(kCatChunkWords, nw - c * kCatChunkWords) + 3) / 4;
      const uint4* tq = reinterpret_cast<const uint4*>(tiled) + (int64_t)c * (kCatChunkWords / 4) * Gp + first_gene(grp);
      if (wide) cat_count<kCatPlanes>(planes + lane, lds_words, tq, Gp, nquads, cnt);
      else cat_count<3>(planes + lane, lds_words, tq, Gp, nquads, cnt);
    }
  }
};

// the lanes of a wavefront whose permutation counts (ge) and is one of the P, added to the gene's cell of d_r
__device__ __forceinline__ void cat_hits(bool ge, bool counted, int lane, int32_t* d_r_cell) {
  const int hits = __popcll(__ballot(ge && counted));
  if (lane == 0 && hits) atomicAdd(d_r_cell, hits);
}

// d w as a signed 128-bit integer, d signed and w unsigned
__device__ __forceinline__ __int128 cat_mul(int64_t d, uint64_t w) {
  const uint64_t ud = (uint64_t)d;
  const uint64_t hi = __umul64hi(ud, w) - (d < 0 ? w : 0ull);
  return (__int128)(((unsigned __int128)hi << 64) | (unsigned __int128)(ud * w));
}

// One class of S22's chi-square statistic of a cell: tot + ((double)c (double)c) inv, c = n a - mnk exact in int32
// (|c| <= 16320^2 < 2^29), one rounding each for the square, the product and the sum.  The observed cells
// (k_cat_wy_prepare) and the permuted ones (k_cat_maxt) go through this one function, so equal tables tie exactly; a
// class without a member adds +0.0.
__device__ __forceinline__ double cat_wy_add(double tot, int n, int a, int mnk, double inv) {
  const int c = n * a - mnk;
  const double e = (double)c * (double)c;
  const double term = e * inv;
  return tot + term;
}

// a lane's maximum into its column of maxs: the bits of a non-negative double order as unsigned integers, so the
// result does not depend on the order of the blocks
__device__ __forceinline__ void cat_wy_combine(double* __restrict__ col, double mx) {
  atomicMax(reinterpret_cast<unsigned long long*>(col), (unsigned long long)__double_as_longlong(mx));
}

// the argument rules of every entry point of the three units (those without strata pass S = 1, without rows P = 1)
int cat_check(scoary_handle h, const char* what, bool ok, int64_t G, int64_t T, int64_t N, int64_t K, int64_t S,
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

// The launch of a hot kernel: the LDS for the seven planes of eight classes (the trait's classes are on the device),
// opted in above 64 KB once per handle and kernel (optin_bit: its bit of h->cat_lds_optin), and the gene ranges per
// stage: enough blocks for four rounds over the CUs, where the gene groups allow it; a range is every ranges-th group,
// so that a table sorted by gene frequency spreads evenly.
enum : int { kCatOptinPermute = 1, kCatOptinMaxt = 2, kGcmhOptinPermute = 4, kGcmhOptinMaxt = 8 };
struct CatLaunch {
  int64_t lds_words, lds, S, ranges;
};
template <typename Kernel>
int cat_launch_plan(scoary_handle h, const char* what, Kernel kernel, int optin_bit, int64_t G, int64_t T, int64_t N,
                    int64_t P, CatLaunch* out) {
  out->lds_words = round_up(std::min<int64_t>((N + 31) / 32, kCatChunkWords), 4);
  out->lds = kCatPlanes * out->lds_words * 256;
  if (out->lds > 64 * 1024 && !(h->cat_lds_optin & optin_bit)) {
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kCatPlanes * kCatChunkWords * 256));
    h->cat_lds_optin |= optin_bit;
  }
  const int64_t ngroups = (G + kCatGroup - 1) / kCatGroup;
  out->S = (P + 63) / 64;
  out->ranges =
      std::min<int64_t>(ngroups, std::max<int64_t>(1, (4 * (int64_t)h->num_cu + out->S * T - 1) / (out->S * T)));
  if (out->S * out->ranges > 0x7fffffffLL) return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": grid too large");
  return SCOARY_OK;
}

}  // namespace
#endif
