// scoary_cat_planes.hpp -- the class bit planes of a stage of permuted code rows and the popcount walk over them,
// shared by the translation units that count a gene's 2 x K table under label permutations (scoary_categorical.hip:
// spec S20; scoary_gcmh.hip: spec S21; scoary_cat_wy.hip: spec S22), so that all compile the same text; and the
// 128-bit product of S20's integer comparison, which scoary_categorical.hip and scoary_cat_wy.hip make alike.
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

// d w as a signed 128-bit integer, d signed and w unsigned
__device__ __forceinline__ __int128 cat_mul(int64_t d, uint64_t w) {
  const uint64_t ud = (uint64_t)d;
  const uint64_t hi = __umul64hi(ud, w) - (d < 0 ? w : 0ull);
  return (__int128)(((unsigned __int128)hi << 64) | (unsigned __int128)(ud * w));
}

}  // namespace
#endif
