// scoary_ranksum.hip -- quantitative traits: the Wilcoxon-Mann-Whitney rank-sum test of a measured value against
// gene presence, with value permutations (spec S15 of DESIGN.md).
//
// The host ranks the values (engine.ranksum_plan): a trait is its row of centred doubled midranks Rc (int16, 0 for
// an isolate without a value), its validity bits and the tie sum.  Everything per gene is one integer,
//     D[g] = sum over the isolates that carry the gene of Rc,
// and the permutation null shuffles the values, that is Rc, over the valid isolates.
//
//   k_ranksum          (observed)      D, m, AUC and the normal-approximation p of every (trait, gene): a bit walk
//                                      over the tiled matrix with the trait's Rc row in LDS; not the hot path
//   k_ranksum_labels   (per batch)     the permuted Rc rows of (trait, permutation): one block sorts the composites
//                                      (50 random bits | isolate) of the valid isolates in LDS, bitonic, and writes
//                                      the row either plain (int16 [T][P][N]) or as the B operand of
//                                      k_permute_ranksum, split into the digits Rc = 128 hi + lo
//   k_permute_ranksum  (the hot path)  D[g][pi] = sum_i A[g][i] B[i][pi] on v_mfma_i32_32x32x32_i8: A expanded
//                                      from the gene bits to 0/1 bytes in registers, B the two digit planes,
//                                      K streamed through LDS by LDS-DMA in chunks of 256 isolates, the
//                                      comparison with |D_obs| and the count fused behind the last chunk of a
//                                      stage of 64 permutations
#include "scoary_common.hpp"

namespace {

typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kRsMaxIsolates = 16320;             // |Rc| <= 16319 = 127 * 128 + 63: the hi digit fits a signed byte
constexpr uint32_t kDomRank = 0x53434F51u;        // "SCOQ": the sort keys of the value shuffle
constexpr int kRsBlockGenes = 256;                // genes of a block: four wavefronts x 64
constexpr int kRsWaves = 4;
constexpr int kRsChunkSteps = 8;                  // K-steps (of 32 isolates) per chunk: two quads of the tiled matrix
constexpr int kRsStepBytes = 4 * kFragBytes;      // B of a K-step x 64 permutations: [plane][column tile][lane] x 16
constexpr int kRsBChunk = kRsChunkSteps * kRsStepBytes;                 // 32 KB
constexpr int kRsAChunk = (kRsChunkSteps / 4) * kRsBlockGenes * 16;     // 8 KB: [quad][gene] x 16 bytes of bits
constexpr int kRsBuf = kRsBChunk + kRsAChunk;
constexpr int kRsLds = 2 * kRsBuf;                // double buffer: two blocks per CU
constexpr int kRsLabelThreads = 1024;
constexpr int kRsLabelHold = 16;                  // sorted entries a lane of k_ranksum_labels holds (16 x 1024 in all)
static_assert(kRsLds * 2 <= 160 * 1024 && kRsLabelHold * kRsLabelThreads >= kRsMaxIsolates &&
                  kRsMaxIsolates < (1 << 14),
              "two blocks of k_permute_ranksum per CU; a block of k_ranksum_labels holds a whole row; an isolate "
              "index fits the 14 low bits of a composite");

// chunks of kRsChunkSteps K-steps that cover N isolates; B is padded with zero rows to that many
__host__ __device__ constexpr int64_t rs_chunks(int64_t N) {
  return ((N + 31) / 32 + kRsChunkSteps - 1) / kRsChunkSteps;
}
inline int rs_pow2(int64_t n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}
// k_ranksum_labels' LDS: the composites (later the finished row), then the Rc of the valid isolates in order
inline int64_t rs_label_key_bytes(int64_t N) {
  return std::max<int64_t>({8 * (int64_t)rs_pow2(N), 2 * 32 * kRsChunkSteps * rs_chunks(N), 2048});
}
inline int64_t rs_label_lds(int64_t N) { return rs_label_key_bytes(N) + round_up(2 * N, 16); }

// word w of a trait's validity row, isolates >= N cleared
__device__ __forceinline__ uint32_t rs_valid_word(const uint32_t* __restrict__ vrow, int w, int N) {
  uint32_t v = vrow[w];
  if (32 * w + 32 > N) v &= (1u << (N - 32 * w)) - 1u;
  return v;
}

// Observed statistic.  Block = 256 genes of one trait, a gene per lane; the trait's Rc row in LDS.
__global__ __launch_bounds__(256) void k_ranksum(const uint4* __restrict__ tiled, int64_t Gp, int G, int N, int Wp,
                                                 const int16_t* __restrict__ rc, const uint32_t* __restrict__ valid,
                                                 const int64_t* __restrict__ tiesum, int32_t* __restrict__ d_d,
                                                 int32_t* __restrict__ d_m, double* __restrict__ d_auc,
                                                 double* __restrict__ d_p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int s_n;
  int16_t* s_rc = reinterpret_cast<int16_t*>(lds);
  const int t = blockIdx.y, tid = threadIdx.x;
  const uint32_t* vrow = valid + (int64_t)t * Wp;
  const int nw = (N + 31) / 32;
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int i = tid; i < N; i += 256) s_rc[i] = rc[(int64_t)t * N + i];
  int cnt = 0;
  for (int w = tid; w < nw; w += 256) cnt += __popc(rs_valid_word(vrow, w, N));
  if (cnt) atomicAdd(&s_n, cnt);
  __syncthreads();
  const int g = blockIdx.x * 256 + tid;
  if (g >= G) return;
  const int n = s_n;
  int D = 0, m = 0;
  for (int q = 0; 4 * q < nw; ++q) {
    const uint4 x = tiled[(int64_t)q * Gp + g];
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int w = 4 * q + j;
      if (w >= nw) break;
      uint32_t bits = xs[j] & rs_valid_word(vrow, w, N);
      m += __popc(bits);
      while (bits) {
        D += s_rc[32 * w + __builtin_ctz(bits)];
        bits &= bits - 1u;
      }
    }
  }
  // the normal approximation with tie and continuity corrections, in the order spec S15 fixes
  double f = 0.0;
  if (n >= 2) f = (double)(n + 1) - (double)tiesum[t] / ((double)n * (double)(n - 1));
  double auc = 0.5, p = 1.0;
  if (n >= 2 && m > 0 && m < n && f > 0.0) {
    const double mm = (double)m * (double)(n - m);
    const double var = (mm / 12.0) * f;
    const double z = fmax(0.0, fabs((double)D) * 0.5 - 0.5) / sqrt(var);
    p = erfc(z / sqrt(2.0));
    auc = 0.5 + (double)D / (2.0 * mm);
  }
  const int64_t o = (int64_t)t * G + g;
  d_d[o] = D;
  d_m[o] = m;
  d_auc[o] = auc;
  d_p[o] = p;
}

// The permuted Rc row of (trait blockIdx.y, permutation perm_base + blockIdx.x).  The valid isolates are compacted
// in ascending order (k-th valid isolate: its index, then its Rc = L[k]); their composites (Philox words 0 and 1
// of counter (i, pi, t, "SCOQ") without the 14 low bits, | i -- among valid isolates i orders as the spec's valid
// index does) are sorted, and the isolate whose composite lands at position k takes L[k].  `rows`: the plain row;
// `bfrag`: the row as hi and lo digits in k_permute_ranksum's B layout,
//     [t][stage of 64 permutations][K-step][plane hi, lo][column tile][lane] x 16 bytes,
// lane l of a fragment = permutation 64 stage + 32 tile + (l & 31), isolates 32 K-step + 16 (l >> 5) .. + 15, one
// per byte; K-steps up to whole chunks and isolates >= N are written as zeros.
__global__ __launch_bounds__(kRsLabelThreads) void k_ranksum_labels(
    const int16_t* __restrict__ rc, const uint32_t* __restrict__ valid, int N, int Wp, int64_t P, int64_t perm_base,
    int64_t trait_base, uint32_t k0, uint32_t k1, int key_bytes, int16_t* __restrict__ rows,
    unsigned char* __restrict__ bfrag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t* s_scan = reinterpret_cast<uint32_t*>(lds);             // 512 counts, in the keys' bytes before the keys
  uint64_t* keys = reinterpret_cast<uint64_t*>(lds);
  int16_t* row = reinterpret_cast<int16_t*>(lds);                  // the keys' bytes, once the keys are read
  int16_t* Lc = reinterpret_cast<int16_t*>(lds + key_bytes);
  uint16_t* idx = reinterpret_cast<uint16_t*>(lds + key_bytes);    // the same bytes: isolate of the k-th valid one
  const int p = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const uint32_t* vrow = valid + (int64_t)t * Wp;
  const int16_t* rct = rc + (int64_t)t * N;
  const int nw = (N + 31) / 32;                                    // <= 510
  const int rowlen = 32 * kRsChunkSteps * (int)rs_chunks(N);

  const uint32_t mine = tid < nw ? rs_valid_word(vrow, tid, N) : 0u;
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
  if (tid < nw) {
    int k = (int)s_scan[tid] - __popc(mine);
    for (uint32_t bits = mine; bits; bits &= bits - 1u) idx[k++] = (uint16_t)(32 * tid + __builtin_ctz(bits));
  }
  __syncthreads();
  int np = 1;
  while (np < n) np <<= 1;
  const uint32_t pi = (uint32_t)(perm_base + p), tt = (uint32_t)(trait_base + t);
  for (int k = tid; k < np; k += kRsLabelThreads) {
    uint64_t c = ~0ull;
    if (k < n) {
      const uint32_t i = idx[k];
      uint32_t r[4];
      philox4x32_10(i, pi, tt, kDomRank, k0, k1, r);
      c = (((uint64_t)r[1] << 32 | r[0]) & ~0x3FFFull) | i;
      Lc[k] = rct[i];
    }
    keys[k] = c;
  }
  __syncthreads();
  for (int k = 2; k <= np; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = tid; e < (np >> 1); e += kRsLabelThreads) {
        const int lo = ((e & ~(j - 1)) << 1) | (e & (j - 1)), hi = lo | j;
        const uint64_t a = keys[lo], b = keys[hi];
        if ((a > b) == ((lo & k) == 0)) keys[lo] = b, keys[hi] = a;
      }
      __syncthreads();
    }
  // (isolate, value) of the sorted positions this lane owns, out of the keys before the row takes their place
  uint32_t held[kRsLabelHold];
#pragma unroll
  for (int e = 0; e < kRsLabelHold; ++e) {
    const int k = tid + e * kRsLabelThreads;
    held[e] = k < n ? ((uint32_t)(keys[k] & 0x3FFFull) << 16) | (uint16_t)Lc[k] : 0u;
  }
  __syncthreads();
  for (int x = tid; 2 * x < rowlen; x += kRsLabelThreads) reinterpret_cast<uint32_t*>(row)[x] = 0u;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kRsLabelHold; ++e)
    if (tid + e * kRsLabelThreads < n) row[held[e] >> 16] = (int16_t)(held[e] & 0xffffu);
  __syncthreads();

  if (rows) {
    int16_t* out = rows + ((int64_t)t * P + p) * N;
    for (int i = tid; i < N; i += kRsLabelThreads) out[i] = row[i];
  }
  if (bfrag) {
    const int64_t S = (P + 63) / 64, Wk = rowlen / 32;
    const int s = p >> 6, j = (p >> 5) & 1, col = p & 31;
    unsigned char* stage = bfrag + ((int64_t)t * S + s) * Wk * kRsStepBytes + j * kFragBytes + col * 16;
    for (int x = tid; 16 * x < rowlen; x += kRsLabelThreads) {      // isolates 16 x .. + 15: K-step x / 2, half x & 1
      uint32_t hi[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const int v = row[16 * x + b];
        const int l = ((v + 64) & 127) - 64;
        lo[b >> 2] |= (uint32_t)(l & 0xff) << (8 * (b & 3));
        hi[b >> 2] |= (uint32_t)(((v - l) >> 7) & 0xff) << (8 * (b & 3));
      }
      unsigned char* dst = stage + (int64_t)(x >> 1) * kRsStepBytes + (x & 1) * 512;
      *reinterpret_cast<uint4*>(dst) = uint4{hi[0], hi[1], hi[2], hi[3]};
      *reinterpret_cast<uint4*>(dst + 2 * kFragBytes) = uint4{lo[0], lo[1], lo[2], lo[3]};
    }
  }
}

// One 16-byte vector per lane, src + 16 * lane -> LDS address lds + 16 * lane, by LDS-DMA (k_permute_mfma's
// transfer): wave-uniform base in an SGPR pair, the lane offset in one VGPR, the LDS destination in M0.
__device__ __forceinline__ void rs_dma16(uint32_t lds, uint32_t lane_off, const unsigned char* src) {
  uint32_t m0_saved;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0"
               : "=&s"(m0_saved)
               : "s"(lds), "v"(lane_off), "s"(src)
               : "memory");
}

// four presence bits -> four 0/1 bytes
__device__ __forceinline__ int rs_bytes_of_bits4(uint32_t x) { return (int)((x * 0x00204081u) & 0x01010101u); }
// bits sh .. sh + 15 of a word of a gene's row (sh = 16 x the lane's half) -> the A fragment of that K-step
// (byte b = isolate b of the half)
__device__ __forceinline__ v4i rs_afrag(uint32_t word, uint32_t sh) {
  return v4i{rs_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh, 4u)),
             rs_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh + 4u, 4u)),
             rs_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh + 8u, 4u)),
             rs_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh + 12u, 4u))};
}

// Block = 256 genes x the stages [s0, s0 + ns) of 64 permutations of trait blockIdx.y.  Wavefront w owns the genes
// 64 w .. 64 w + 63 (two row tiles) against both column tiles and both digit planes: eight accumulator tiles.
// The block walks the linear sequence of (stage, chunk) -- B's own address order -- with two LDS buffers: chunk
// `it` is computed from buffer it & 1 while chunk it + 1 arrives in the other one by LDS-DMA (32 KB of B, and 8 KB
// of gene bits: quads 2 c and 2 c + 1 of the tiled matrix, 256 genes x 16 bytes each, contiguous).  Before the
// barrier of an iteration every wavefront has waited for its own transfers of that chunk, behind it the chunk is
// whole and the other buffer -- last read in the iteration before -- is free for the next transfer.
// A quad past the matrix (its pad in K) is read from the last quad instead: B holds zeros there.
// Behind a stage's last chunk: D = 128 D_hi + D_lo, |D| >= |D_obs[g]| counted per lane over the columns < P; the
// 32 lanes of a row meet once, at the end of the block, and add their count to d_r[t][g].
__global__ __launch_bounds__(kRsWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_permute_ranksum(const unsigned char* __restrict__ tiled, int64_t Gp, int Qp, int G, int nc,
                       const unsigned char* __restrict__ bfrag, const int32_t* __restrict__ dobs, int64_t P, int S,
                       int L, int nblk_genes, int32_t* __restrict__ d_r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int gb = blockIdx.x % nblk_genes, rng = blockIdx.x / nblk_genes, t = blockIdx.y;
  const int s0 = rng * L, ns = min(L, S - s0);
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)lds;
  const uint32_t lane_off = (uint32_t)lane * 16u;
  const int nit = ns * nc;

  const unsigned char* bsrc = bfrag + ((int64_t)t * S + s0) * nc * kRsBChunk + wave * (kRsBChunk / kRsWaves);
  // the wavefront's share of a chunk's gene bits: quad wave >> 1 of the chunk's two, genes 128 (wave & 1) .. + 127
  const unsigned char* asrc = tiled + ((int64_t)gb * kRsBlockGenes + (wave & 1) * 128) * 16;
  const uint32_t a_dst = kRsBChunk + (uint32_t)((wave >> 1) * kRsBlockGenes + (wave & 1) * 128) * 16u;
  // chunk `it` (chunk cq of its stage) into buffer it & 1; bsrc then points at the next chunk
  auto issue = [&](int it, int cq) {
    const uint32_t buf = lds0 + (uint32_t)(it & 1) * kRsBuf;
#pragma unroll
    for (int x = 0; x < kRsBChunk / kRsWaves / kFragBytes; ++x)
      rs_dma16(buf + wave * (kRsBChunk / kRsWaves) + x * kFragBytes, lane_off, bsrc + x * kFragBytes);
    bsrc += kRsBChunk;
    const unsigned char* aq = asrc + (int64_t)min(2 * cq + (wave >> 1), Qp - 1) * Gp * 16;
#pragma unroll
    for (int x = 0; x < 2; ++x) rs_dma16(buf + a_dst + x * kFragBytes, lane_off, aq + x * kFragBytes);
  };

  v16i acc[2][2][2];                               // [row tile][column tile][plane]
  uint32_t ex[2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) ex[i][r] = 0u;
  const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j][0] = zero, acc[i][j][1] = zero;

  const int gene0 = gb * kRsBlockGenes + wave * 64 + 4 * half;   // the gene of row tile 0, register 0
  const int32_t* thr = dobs + (int64_t)t * G;

  issue(0, 0);
  int c = 0, s = s0;
  for (int it = 0; it < nit; ++it) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (it + 1 < nit) issue(it + 1, c + 1 == nc ? 0 : c + 1);
    const unsigned char* buf = lds + (it & 1) * kRsBuf;
    const unsigned char* bb = buf + lane * 16;
    const unsigned char* ab = buf + kRsBChunk + (wave * 64 + l31) * 16;
#pragma unroll
    for (int qq = 0; qq < kRsChunkSteps / 4; ++qq) {
      v4i aw[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) aw[i] = *reinterpret_cast<const v4i*>(ab + (qq * kRsBlockGenes + i * 32) * 16);
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        const int k = qq * 4 + ww;
        v4i b[2][2];                               // [plane][column tile]
#pragma unroll
        for (int x = 0; x < 4; ++x)
          b[x >> 1][x & 1] = *reinterpret_cast<const v4i*>(bb + k * kRsStepBytes + x * kFragBytes);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const v4i a = rs_afrag((uint32_t)aw[i][ww], 16u * (uint32_t)half);
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
              acc[i][j][pl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[pl][j], acc[i][j][pl], 0, 0, 0);
        }
      }
    }
    if (++c == nc) {                               // the stage is whole: compare, count, start again
      const int64_t col0 = (int64_t)s * 64 + l31;
      const uint32_t v0 = col0 < P, v1 = col0 + 32 < P;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int g = gene0 + i * 32 + (r & 3) + 8 * (r >> 2);
          const int a = g < G ? abs(thr[min(g, G - 1)]) : 0x7fffffff;    // (the load itself is unconditional)
          const int d0 = acc[i][0][0][r] * 128 + acc[i][0][1][r], d1 = acc[i][1][0][r] * 128 + acc[i][1][1][r];
          ex[i][r] += ((uint32_t)(abs(d0) >= a) & v0) + ((uint32_t)(abs(d1) >= a) & v1);
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j][0] = zero, acc[i][j][1] = zero;
      c = 0, ++s;
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      uint32_t v = ex[i][r];
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
      const int g = gene0 + i * 32 + (r & 3) + 8 * (r >> 2);
      if (l31 == 0 && g < G && v) atomicAdd(d_r + (int64_t)t * G + g, (int32_t)v);
    }
}

int rs_check(scoary_handle h, const char* what, bool ok, int64_t N) {
  if (int rc = check_args(h, what, ok && N >= 1)) return rc;
  if (N > kRsMaxIsolates)
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": more isolates than scoary_ranksum_max_isolates()");
  return SCOARY_OK;
}

int rs_generate(scoary_handle h, const char* what, const int16_t* d_rc, const uint32_t* d_valid, int64_t T, int64_t N,
                int64_t P, int64_t perm_base, int64_t trait_base, uint64_t seed, int16_t* d_rows, void* d_bfrag,
                scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = rs_check(h, what, d_rc && d_valid && (d_rows || d_bfrag) && T >= 1 && P >= 1 && perm_base >= 0 &&
                                     trait_base >= 0, N))
    return rc;
  if (T > 65535 || P > 0x7fffffffLL || perm_base + P > 0xffffffffLL || trait_base + T > 0xffffffffLL)
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": T > 65535, P >= 2^31 or a counter word past 2^32");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t lds = rs_label_lds(N);
  if (lds > 64 * 1024 && !(h->ranksum_lds_optin & 1)) {
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ranksum_labels),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    h->ranksum_lds_optin |= 1;
  }
  KernelTimer kt(h, s, "k_ranksum_labels");
  hipLaunchKernelGGL(k_ranksum_labels, dim3((unsigned)P, (unsigned)T), dim3(kRsLabelThreads), (size_t)lds, s, d_rc,
                     d_valid, (int)N, (int)scoary_row_words(N), P, perm_base, trait_base, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (int)rs_label_key_bytes(N), d_rows,
                     static_cast<unsigned char*>(d_bfrag));
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // namespace

extern "C" {

int64_t scoary_ranksum_max_isolates(void) { return kRsMaxIsolates; }

int64_t scoary_ranksum_bfrag_bytes(int64_t N, int64_t P, int64_t T) {
  if (N < 1 || N > kRsMaxIsolates || P < 1 || T < 1) return 0;
  return T * ((P + 63) / 64) * rs_chunks(N) * kRsBChunk;
}

int scoary_ranksum(scoary_handle h, const uint32_t* d_tiled, const int16_t* d_rc, const uint32_t* d_valid,
                   const int64_t* d_tiesum, int64_t G, int64_t T, int64_t N, int32_t* d_d, int32_t* d_m,
                   double* d_auc, double* d_p, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = rs_check(h, "scoary_ranksum", d_tiled && d_rc && d_valid && d_tiesum && d_d && d_m && d_auc && d_p &&
                                                 G >= 1 && T >= 1, N))
    return rc;
  if (T > 65535 || G > 0x7fffffffLL - 256) return fail(h, SCOARY_ERR_SIZE, "scoary_ranksum: T > 65535 or G >= 2^31");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  KernelTimer kt(h, s, "k_ranksum");
  hipLaunchKernelGGL(k_ranksum, dim3((unsigned)((G + 255) / 256), (unsigned)T), dim3(256),
                     (size_t)round_up(2 * N, 16), s, reinterpret_cast<const uint4*>(d_tiled), scoary_tiled_genes(G),
                     (int)G, (int)N, (int)scoary_row_words(N), d_rc, d_valid, d_tiesum, d_d, d_m, d_auc, d_p);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_ranksum_perm_generate(scoary_handle h, const int16_t* d_rc, const uint32_t* d_valid, int64_t T, int64_t N,
                                 int64_t P, int64_t perm_base, int64_t trait_base, uint64_t seed, int16_t* d_rows,
                                 scoary_stream_t stream) {
  return rs_generate(h, "scoary_ranksum_perm_generate", d_rc, d_valid, T, N, P, perm_base, trait_base, seed, d_rows,
                     nullptr, stream);
}

int scoary_ranksum_perm_generate_bfrag(scoary_handle h, const int16_t* d_rc, const uint32_t* d_valid, int64_t T,
                                       int64_t N, int64_t P, int64_t perm_base, int64_t trait_base, uint64_t seed,
                                       void* d_bfrag, scoary_stream_t stream) {
  return rs_generate(h, "scoary_ranksum_perm_generate_bfrag", d_rc, d_valid, T, N, P, perm_base, trait_base, seed,
                     nullptr, d_bfrag, stream);
}

int scoary_permute_ranksum(scoary_handle h, const uint32_t* d_tiled, const void* d_bfrag, const int32_t* d_dobs,
                           int64_t G, int64_t T, int64_t N, int64_t P, int32_t* d_r, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = rs_check(h, "scoary_permute_ranksum", d_tiled && d_bfrag && d_dobs && d_r && G >= 1 && T >= 1 &&
                                                         P >= 1, N))
    return rc;
  if (T > 65535 || G > 0x7fffffffLL - 256 || P > 0x7fffffffLL)
    return fail(h, SCOARY_ERR_SIZE, "scoary_permute_ranksum: T > 65535, G >= 2^31 or P >= 2^31");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!(h->ranksum_lds_optin & 2)) {
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_permute_ranksum),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kRsLds));
    h->ranksum_lds_optin |= 2;
  }
  // stages per block: enough blocks for eight rounds over the CUs' two places each, where the stages allow it
  const int64_t S = (P + 63) / 64, nblk = (G + kRsBlockGenes - 1) / kRsBlockGenes;
  const int64_t want =
      std::min<int64_t>(S, std::max<int64_t>(1, (16 * (int64_t)h->num_cu + nblk * T - 1) / (nblk * T)));
  const int64_t L = (S + want - 1) / want, ranges = (S + L - 1) / L;
  if (nblk * ranges > 0x7fffffffLL) return fail(h, SCOARY_ERR_SIZE, "scoary_permute_ranksum: grid too large");
  KernelTimer kt(h, s, "k_permute_ranksum");
  hipLaunchKernelGGL(k_permute_ranksum, dim3((unsigned)(nblk * ranges), (unsigned)T), dim3(kRsWaves * 64), kRsLds, s,
                     reinterpret_cast<const unsigned char*>(d_tiled), scoary_tiled_genes(G),
                     (int)scoary_tiled_quads(N), (int)G, (int)rs_chunks(N), static_cast<const unsigned char*>(d_bfrag),
                     d_dobs, P, (int)S, (int)L, (int)nblk, d_r);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
