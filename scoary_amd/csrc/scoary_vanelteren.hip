// scoary_vanelteren.hip -- quantitative traits over strata: the van Elteren (stratified rank-sum) test of a measured
// value against gene presence, with value permutations within the strata (spec S16 of DESIGN.md).
//
// The host ranks the values inside every stratum and weighs them (engine.vanelteren_plan): a trait is its row of
// scores a_i = w_s Rc_i (int16, 0 for an isolate without a value; |a| <= 16319 as S15's Rc), its validity bits, the
// per-stratum (w, n) and variance factors c, and L, the scores of its valid isolates in (stratum, isolate) order.
// Everything per gene is again one integer,
//     D[g] = sum over the isolates that carry the gene of a,
// and the permutation null shuffles the scores among the valid isolates of each stratum.
//
//   k_vanelteren         (observed)    D, m, var, AUC and the normal-approximation p of every (trait, gene): the walk
//                                      of the CMH kernels over the segment table (scoary_cmh_segments_launch) with
//                                      the trait's score row in LDS, a stratum's m folded into var (fp64) and den
//                                      (int64) at every change of stratum; not the hot path
//   k_vanelteren_labels  (per batch)   the permuted score rows of (trait, permutation): k_ranksum_labels' LDS bitonic
//                                      sort over the composites (stratum | 50 - b random bits | isolate), so that the
//                                      ranks of a stratum's isolates are that stratum's positions in L; the row goes
//                                      out plain (int16 [T][P][N]) or as the B operand of k_permute_ranksum
//
// The permutation GEMM is scoary_permute_ranksum (scoary_ranksum.hip), as it is: it takes any int16 rows with
// |score| <= 16319.
#include "scoary_common.hpp"

namespace {

constexpr int kVeMaxIsolates = 16320;             // = scoary_ranksum_max_isolates(): the hi digit fits a signed byte
constexpr uint32_t kDomRank = 0x53434F51u;        // "SCOQ": S15's sort keys
constexpr int kVeThreads = 256;                   // k_vanelteren: a gene per lane
constexpr int kVeChunkSteps = 8;                  // k_permute_ranksum's B operand: K-steps (of 32 isolates) per chunk,
constexpr int kVeStepBytes = 4 * kFragBytes;      // bytes of a K-step x 64 permutations: [plane][column tile][lane] x 16
constexpr int kVeLabelThreads = 1024;
constexpr int kVeLabelHold = 16;                  // sorted entries a lane of k_vanelteren_labels holds
static_assert(kVeLabelHold * kVeLabelThreads >= kVeMaxIsolates && kVeMaxIsolates < (1 << 14),
              "a block of k_vanelteren_labels holds a whole row; an isolate index fits the 14 low bits of a composite");

// chunks of kVeChunkSteps K-steps that cover N isolates; B is padded with zero rows to that many
__host__ __device__ constexpr int64_t ve_chunks(int64_t N) {
  return ((N + 31) / 32 + kVeChunkSteps - 1) / kVeChunkSteps;
}
inline int ve_pow2(int64_t n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}
// k_vanelteren_labels' LDS: the composites (later the finished row), then L / the isolates of the valid positions
inline int64_t ve_label_key_bytes(int64_t N) {
  return std::max<int64_t>({8 * (int64_t)ve_pow2(N), 2 * 32 * kVeChunkSteps * ve_chunks(N), 2048});
}
inline int64_t ve_label_lds(int64_t N) { return ve_label_key_bytes(N) + round_up(2 * N, 16); }
// bits of a stratum index: 0 for one stratum, else the bit length of S - 1
inline int ve_strata_bits(int64_t S) {
  int b = 0;
  while (((int64_t)1 << b) < S) ++b;
  return b;
}

// word w of a trait's validity row, isolates >= N cleared
__device__ __forceinline__ uint32_t ve_valid_word(const uint32_t* __restrict__ vrow, int w, int N) {
  uint32_t v = vrow[w];
  if (32 * w + 32 > N) v &= (1u << (N - 32 * w)) - 1u;
  return v;
}

// Observed statistic.  Block = 256 genes of one trait, a gene per lane; the trait's score row in LDS.  The lane
// walks the segment table as cmh_walk does (stratum and word clamped: a bad plan gives wrong numbers, never a wild
// access; the quad of the gene row reloaded only when the word leaves it): per segment m_s and D grow by the gene's
// valid isolates of that (stratum, word), and every change of stratum folds m_s -- ascending s, the order S16 fixes
// for var.  Strata without a member have no segment and add nothing.
__global__ __launch_bounds__(kVeThreads) void k_vanelteren(
    const uint4* __restrict__ tiled, int64_t Gp, int G, int N, int S, const int16_t* __restrict__ score,
    const uint32_t* __restrict__ valid, int Wp, const CmhSegments* __restrict__ segs, const int32_t* __restrict__ wn,
    const double* __restrict__ cfac, int32_t* __restrict__ d_d, int32_t* __restrict__ d_m, double* __restrict__ d_var,
    double* __restrict__ d_auc, double* __restrict__ d_p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  int16_t* s_a = reinterpret_cast<int16_t*>(lds);
  const int t = blockIdx.y, tid = threadIdx.x;
  const uint32_t* vrow = valid + (int64_t)t * Wp;
  const int nw = (N + 31) / 32;
  for (int i = tid; i < N; i += kVeThreads) s_a[i] = score[(int64_t)t * N + i];
  __syncthreads();
  const int g = blockIdx.x * kVeThreads + tid;
  if (g >= G) return;

  int D = 0, m = 0, ms = 0;
  int64_t den = 0;
  double var = 0.0;
  auto fold = [&](int s) {
    const int2 x = reinterpret_cast<const int2*>(wn)[(int64_t)t * S + s];     // (w_s, n_s)
    const int64_t mm = (int64_t)ms * (int64_t)(x.y - ms);
    var += cfac[(int64_t)t * S + s] * ((double)ms * (double)(x.y - ms));
    den += (int64_t)x.x * mm;
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
    const int c = w & 3;
    uint32_t bits = (c == 0 ? gq.x : c == 1 ? gq.y : c == 2 ? gq.z : gq.w) & sg.y & ve_valid_word(vrow, w, N);
    ms += __popc(bits);
    while (bits) {
      D += s_a[32 * w + __builtin_ctz(bits)];
      bits &= bits - 1u;
    }
  }
  if (cur_s >= 0) fold(cur_s);

  // the normal approximation in the order spec S16 fixes; no continuity correction
  double auc = 0.5, p = 1.0;
  if (var > 0.0) {
    const double z = (fabs((double)D) * 0.5) / sqrt(var);
    p = erfc(z / sqrt(2.0));
    auc = 0.5 + (double)D / (2.0 * (double)den);
  }
  const int64_t o = (int64_t)t * G + g;
  d_d[o] = D;
  d_m[o] = m;
  d_var[o] = var;
  d_auc[o] = auc;
  d_p[o] = p;
}

// The permuted score row of (trait blockIdx.y, permutation perm_base + blockIdx.x).  The valid isolates are
// compacted in ascending order; their composites -- the stratum in the top `sbits` bits, under it Philox words 0
// and 1 of counter (i, pi, t, "SCOQ") without their 14 low bits, moved down by sbits, and the isolate in the 14 low
// bits -- are sorted, and the isolate whose composite lands at position k takes lrow[k]: the stratum leads, so the
// positions of a stratum's isolates are that stratum's run of L (the scores of the valid isolates by (stratum,
// isolate), built on the host).  The stratum is clamped to S - 1 < 2^sbits.  `rows`: the plain row; `bfrag`: the
// row as hi and lo digits in k_permute_ranksum's B layout,
//     [t][stage of 64 permutations][K-step][plane hi, lo][column tile][lane] x 16 bytes,
// lane l of a fragment = permutation 64 stage + 32 tile + (l & 31), isolates 32 K-step + 16 (l >> 5) .. + 15, one
// per byte; K-steps up to whole chunks, isolates >= N and the columns from P to the end of the last stage are
// written as zeros (the grid covers whole stages when it writes B).
__global__ __launch_bounds__(kVeLabelThreads) void k_vanelteren_labels(
    const int16_t* __restrict__ lrows, const uint32_t* __restrict__ valid, const uint16_t* __restrict__ strata, int N,
    int Wp, int S, int sbits, int64_t P, int64_t perm_base, int64_t trait_base, uint32_t k0, uint32_t k1,
    int key_bytes, int16_t* __restrict__ rows, unsigned char* __restrict__ bfrag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t* s_scan = reinterpret_cast<uint32_t*>(lds);             // 512 counts, in the keys' bytes before the keys
  uint64_t* keys = reinterpret_cast<uint64_t*>(lds);
  int16_t* row = reinterpret_cast<int16_t*>(lds);                  // the keys' bytes, once the keys are read
  int16_t* Lc = reinterpret_cast<int16_t*>(lds + key_bytes);
  uint16_t* idx = reinterpret_cast<uint16_t*>(lds + key_bytes);    // the same bytes: isolate of the k-th valid one
  const int p = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const uint32_t* vrow = valid + (int64_t)t * Wp;
  const int16_t* lrow = lrows + (int64_t)t * N;
  const int nw = (N + 31) / 32;                                    // <= 510
  const int rowlen = 32 * kVeChunkSteps * (int)ve_chunks(N);

  // the columns from P to the end of the last stage have blocks of their own, which write them as zeros: a block
  // without a valid isolate
  const bool pad = p >= P;
  const uint32_t mine = tid < nw && !pad ? ve_valid_word(vrow, tid, N) : 0u;
  if (tid < 512) s_scan[tid] = __popc(mine);
  __syncthreads();
  for (int o = 1; o < 512; o <<= 1) {
    uint32_t v = 0;
    if (tid < 512 && tid >= o) v = s_scan[tid - o];
    __syncthreads();
    if (tid < 512) s_scan[tid] += v;
    __syncthreads();
  }
  const int n = (int)s_scan[511];
  if (tid < nw) {                                                  // (idx lies behind the counts: key_bytes >= 2048)
    int k = (int)s_scan[tid] - __popc(mine);
    for (uint32_t bits = mine; bits; bits &= bits - 1u) idx[k++] = (uint16_t)(32 * tid + __builtin_ctz(bits));
  }
  __syncthreads();
  int np = 1;
  while (np < n) np <<= 1;
  const uint32_t pi = (uint32_t)(perm_base + p), tt = (uint32_t)(trait_base + t);
  for (int k = tid; k < np; k += kVeLabelThreads) {
    uint64_t c = ~0ull;
    if (k < n) {
      const uint32_t i = idx[k];
      uint32_t r[4];
      philox4x32_10(i, pi, tt, kDomRank, k0, k1, r);
      const uint64_t key64 = (uint64_t)r[1] << 32 | r[0];
      c = (((key64 >> 14) >> sbits) << 14) | i;
      if (sbits) c |= (uint64_t)min((int)strata[i], S - 1) << (64 - sbits);
      Lc[k] = lrow[k];
    }
    keys[k] = c;
  }
  __syncthreads();
  for (int k = 2; k <= np; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = tid; e < (np >> 1); e += kVeLabelThreads) {
        const int lo = ((e & ~(j - 1)) << 1) | (e & (j - 1)), hi = lo | j;
        const uint64_t a = keys[lo], b = keys[hi];
        if ((a > b) == ((lo & k) == 0)) keys[lo] = b, keys[hi] = a;
      }
      __syncthreads();
    }
  // (isolate, score) of the sorted positions this lane owns, out of the keys before the row takes their place
  uint32_t held[kVeLabelHold];
#pragma unroll
  for (int e = 0; e < kVeLabelHold; ++e) {
    const int k = tid + e * kVeLabelThreads;
    held[e] = k < n ? ((uint32_t)(keys[k] & 0x3FFFull) << 16) | (uint16_t)Lc[k] : 0u;
  }
  __syncthreads();
  for (int x = tid; 2 * x < rowlen; x += kVeLabelThreads) reinterpret_cast<uint32_t*>(row)[x] = 0u;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kVeLabelHold; ++e)
    if (tid + e * kVeLabelThreads < n) row[held[e] >> 16] = (int16_t)(held[e] & 0xffffu);
  __syncthreads();

  if (rows && !pad) {
    int16_t* out = rows + ((int64_t)t * P + p) * N;
    for (int i = tid; i < N; i += kVeLabelThreads) out[i] = row[i];
  }
  if (bfrag) {
    const int64_t St = (P + 63) / 64, Wk = rowlen / 32;
    const int s = p >> 6, j = (p >> 5) & 1, col = p & 31;
    unsigned char* stage = bfrag + ((int64_t)t * St + s) * Wk * kVeStepBytes + j * kFragBytes + col * 16;
    for (int x = tid; 16 * x < rowlen; x += kVeLabelThreads) {      // isolates 16 x .. + 15: K-step x / 2, half x & 1
      uint32_t hi[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const int v = row[16 * x + b];
        const int l = ((v + 64) & 127) - 64;
        lo[b >> 2] |= (uint32_t)(l & 0xff) << (8 * (b & 3));
        hi[b >> 2] |= (uint32_t)(((v - l) >> 7) & 0xff) << (8 * (b & 3));
      }
      unsigned char* dst = stage + (int64_t)(x >> 1) * kVeStepBytes + (x & 1) * 512;
      *reinterpret_cast<uint4*>(dst) = uint4{hi[0], hi[1], hi[2], hi[3]};
      *reinterpret_cast<uint4*>(dst + 2 * kFragBytes) = uint4{lo[0], lo[1], lo[2], lo[3]};
    }
  }
}

// the checks the entry points share: strata_check's, then the rank-sum kernels' limit on N
int ve_check(scoary_handle h, const char* what, bool ok, int64_t T, int64_t N, int64_t S) {
  if (int rc = strata_check(h, what, ok, T, N, S)) return rc;
  if (N > kVeMaxIsolates)
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": more isolates than scoary_ranksum_max_isolates()");
  return SCOARY_OK;
}

int ve_generate(scoary_handle h, const char* what, const int16_t* d_l, const uint32_t* d_valid,
                const uint16_t* d_strata, int64_t T, int64_t N, int64_t S, int64_t P, int64_t perm_base,
                int64_t trait_base, uint64_t seed, int16_t* d_rows, void* d_bfrag, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = ve_check(h, what, d_l && d_valid && d_strata && (d_rows || d_bfrag) && P >= 1 && perm_base >= 0 &&
                                     trait_base >= 0, T, N, S))
    return rc;
  // (the last counter words are perm_base + P - 1 and trait_base + T - 1: both sums may be 2^32 itself)
  if (P > 0x7fffffffLL - 64 || perm_base + P > 0x100000000LL || trait_base + T > 0x100000000LL)
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": P >= 2^31 or a counter word past 2^32");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t lds = ve_label_lds(N);
  // past 64 KB of dynamic LDS (N > 4096) the kernel needs the opt-in; asked for at every such launch -- a host call
  // per batch of permutations -- so that the handle keeps no state for it
  if (lds > 64 * 1024)
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vanelteren_labels),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  KernelTimer kt(h, s, "k_vanelteren_labels");
  const int64_t columns = d_bfrag ? round_up(P, 64) : P;            // B: whole stages, the surplus columns zero
  hipLaunchKernelGGL(k_vanelteren_labels, dim3((unsigned)columns, (unsigned)T), dim3(kVeLabelThreads), (size_t)lds, s,
                     d_l, d_valid, d_strata, (int)N, (int)scoary_row_words(N), (int)S, ve_strata_bits(S), P, perm_base,
                     trait_base, (uint32_t)seed, (uint32_t)(seed >> 32), (int)ve_label_key_bytes(N), d_rows,
                     static_cast<unsigned char*>(d_bfrag));
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // namespace

extern "C" {

int scoary_vanelteren(scoary_handle h, const uint32_t* d_tiled, const int16_t* d_score, const uint32_t* d_valid,
                      const uint16_t* d_strata, const int32_t* d_members, const int32_t* d_wn, const double* d_c,
                      int64_t G, int64_t T, int64_t N, int64_t S, int32_t* d_d, int32_t* d_m, double* d_var,
                      double* d_auc, double* d_p, void* d_scratch, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = ve_check(h, "scoary_vanelteren", d_tiled && d_score && d_valid && d_strata && d_members && d_wn &&
                                                    d_c && d_d && d_m && d_var && d_auc && d_p && d_scratch && G >= 1,
                        T, N, S))
    return rc;
  if (G > 0x7fffffffLL - kVeThreads) return fail(h, SCOARY_ERR_SIZE, "scoary_vanelteren: G >= 2^31");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = scoary_cmh_segments_launch(h, s, d_strata, d_members, N, S, d_scratch, "k_cmh_segments")) return rc;
  KernelTimer kt(h, s, "k_vanelteren");
  hipLaunchKernelGGL(k_vanelteren, dim3((unsigned)((G + kVeThreads - 1) / kVeThreads), (unsigned)T), dim3(kVeThreads),
                     (size_t)round_up(2 * N, 16), s, reinterpret_cast<const uint4*>(d_tiled), scoary_tiled_genes(G),
                     (int)G, (int)N, (int)S, d_score, d_valid, (int)scoary_row_words(N),
                     static_cast<const CmhSegments*>(d_scratch), d_wn, d_c, d_d, d_m, d_var, d_auc, d_p);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_vanelteren_perm_generate(scoary_handle h, const int16_t* d_l, const uint32_t* d_valid,
                                    const uint16_t* d_strata, int64_t T, int64_t N, int64_t S, int64_t P,
                                    int64_t perm_base, int64_t trait_base, uint64_t seed, int16_t* d_rows,
                                    scoary_stream_t stream) {
  return ve_generate(h, "scoary_vanelteren_perm_generate", d_l, d_valid, d_strata, T, N, S, P, perm_base, trait_base,
                     seed, d_rows, nullptr, stream);
}

int scoary_vanelteren_perm_generate_bfrag(scoary_handle h, const int16_t* d_l, const uint32_t* d_valid,
                                          const uint16_t* d_strata, int64_t T, int64_t N, int64_t S, int64_t P,
                                          int64_t perm_base, int64_t trait_base, uint64_t seed, void* d_bfrag,
                                          scoary_stream_t stream) {
  return ve_generate(h, "scoary_vanelteren_perm_generate_bfrag", d_l, d_valid, d_strata, T, N, S, P, perm_base,
                     trait_base, seed, nullptr, d_bfrag, stream);
}

}  // extern "C"
