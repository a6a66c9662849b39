// scoary_rank_wy.hip -- Westfall-Young single-step maxT over the rank statistics of the quantitative traits: the
// rank-sum test (S15) and the van Elteren test (S16) under one statistic (spec S17 of DESIGN.md).
//
// A cell (gene g, permuted row pi) of trait t has the integer D the rank tests count by.  Its statistic is
//     s = ((double)E * (double)E) * iv[t][g],   E = max(0, |D| - cc),   iv = 1 / var where the gene is testable, else 0
// (cc = 1: S15's continuity correction, cc = 0: S16), 4 z^2 in the reals, strictly increasing in E for a gene with
// iv > 0 and 0 in every row of an untestable gene.  maxs[t][pi] = max over the genes of s.
//
//   k_ranksum_var      (observed)      S15's var of every (trait, gene), 0 where untestable (S16's is k_vanelteren's)
//   k_rank_wy_prepare  (observed)      iv and s_obs = s of the observed D, by the device function the hot path uses
//   k_rank_maxt        (the hot path)  k_permute_ranksum's GEMM (scoary_ranksum.hip: int8 matrix cores, gene bits
//                                      expanded in registers, B streamed by LDS-DMA through two 40 KB buffers, two
//                                      blocks per CU) with both reductions fused behind a stage's last chunk: the
//                                      exceedance count against |D_obs| as there, and the maximum of s over the block's
//                                      256 genes per column, combined into maxs by a 64-bit unsigned atomic maximum on
//                                      the bits of the non-negative double -- independent of the order of the blocks
#include "scoary_common.hpp"

namespace {

typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kWyMaxIsolates = 16320;             // = scoary_ranksum_max_isolates()
constexpr int kWyBlockGenes = 256;                // k_permute_ranksum's geometry, constant for constant
constexpr int kWyWaves = 4;
constexpr int kWyChunkSteps = 8;
constexpr int kWyStepBytes = 4 * kFragBytes;
constexpr int kWyBChunk = kWyChunkSteps * kWyStepBytes;                 // 32 KB
constexpr int kWyAChunk = (kWyChunkSteps / 4) * kWyBlockGenes * 16;     // 8 KB
constexpr int kWyBuf = kWyBChunk + kWyAChunk;
constexpr int kWyLds = 2 * kWyBuf;
static_assert(kWyLds * 2 <= 160 * 1024, "two blocks of k_rank_maxt per CU");

__host__ __device__ constexpr int64_t wy_chunks(int64_t N) {
  return ((N + 31) / 32 + kWyChunkSteps - 1) / kWyChunkSteps;
}

// The statistic of a cell: two conversions that are exact (E < 2^28) and two multiplications, each rounded on its
// own.  The observed and the permuted cells go through this one function, so equal E tie exactly.
__device__ __forceinline__ double wy_stat(int D, int cc, double iv) {
  const double e = (double)max(0, abs(D) - cc);
  const double e2 = e * e;
  return e2 * iv;
}

// word w of a trait's validity row, isolates >= N cleared
__device__ __forceinline__ uint32_t wy_valid_word(const uint32_t* __restrict__ vrow, int w, int N) {
  uint32_t v = vrow[w];
  if (32 * w + 32 > N) v &= (1u << (N - 32 * w)) - 1u;
  return v;
}

// S15's variance of the genes of a block of 256 of trait blockIdx.y, operations in k_ranksum's order; 0 where the
// gene is untestable (n < 2, m = 0, m = n or f <= 0).
__global__ __launch_bounds__(256) void k_ranksum_var(const int32_t* __restrict__ d_m,
                                                     const uint32_t* __restrict__ valid,
                                                     const int64_t* __restrict__ tiesum, int G, int N, int Wp,
                                                     double* __restrict__ d_var) {
  __shared__ int s_n;
  const int t = blockIdx.y, tid = threadIdx.x;
  const uint32_t* vrow = valid + (int64_t)t * Wp;
  const int nw = (N + 31) / 32;
  if (tid == 0) s_n = 0;
  __syncthreads();
  int cnt = 0;
  for (int w = tid; w < nw; w += 256) cnt += __popc(wy_valid_word(vrow, w, N));
  if (cnt) atomicAdd(&s_n, cnt);
  __syncthreads();
  const int g = blockIdx.x * 256 + tid;
  if (g >= G) return;
  const int n = s_n, m = d_m[(int64_t)t * G + g];
  double f = 0.0;
  if (n >= 2) f = (double)(n + 1) - (double)tiesum[t] / ((double)n * (double)(n - 1));
  double var = 0.0;
  if (n >= 2 && m > 0 && m < n && f > 0.0) {
    const double mm = (double)m * (double)(n - m);
    var = (mm / 12.0) * f;
  }
  d_var[(int64_t)t * G + g] = var;
}

// iv = 1 / var (fp64 division, correctly rounded) where var > 0, else 0; s_obs = the statistic of the observed D
__global__ __launch_bounds__(256) void k_rank_wy_prepare(const double* __restrict__ d_var,
                                                         const int32_t* __restrict__ dobs, int cc, int64_t cells,
                                                         double* __restrict__ d_iv, double* __restrict__ d_sobs) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= cells) return;
  const double var = d_var[o];
  const double iv = var > 0.0 ? 1.0 / var : 0.0;
  d_iv[o] = iv;
  d_sobs[o] = wy_stat(dobs[o], cc, iv);
}

// One 16-byte vector per lane, src + 16 * lane -> LDS address lds + 16 * lane, by LDS-DMA (k_permute_ranksum's
// transfer): wave-uniform base in an SGPR pair, the lane offset in one VGPR, the LDS destination in M0.
__device__ __forceinline__ void wy_dma16(uint32_t lds, uint32_t lane_off, const unsigned char* src) {
  uint32_t m0_saved;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0"
               : "=&s"(m0_saved)
               : "s"(lds), "v"(lane_off), "s"(src)
               : "memory");
}

// four presence bits -> four 0/1 bytes
__device__ __forceinline__ int wy_bytes_of_bits4(uint32_t x) { return (int)((x * 0x00204081u) & 0x01010101u); }
// bits sh .. sh + 15 of a word of a gene's row (sh = 16 x the lane's half) -> the A fragment of that K-step
__device__ __forceinline__ v4i wy_afrag(uint32_t word, uint32_t sh) {
  return v4i{wy_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh, 4u)),
             wy_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh + 4u, 4u)),
             wy_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh + 8u, 4u)),
             wy_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh + 12u, 4u))};
}

// k_permute_ranksum's block and main loop (scoary_ranksum.hip; restated here so that that kernel compiles exactly as
// it did): block = 256 genes x the stages [s0, s0 + ns) of 64 permutations of trait blockIdx.y, wavefront w owns the
// genes 64 w .. 64 w + 63 against both column tiles and both digit planes, the (stage, chunk) sequence streamed
// through two LDS buffers by LDS-DMA.
// Behind a stage's last chunk, per cell: D = 128 D_hi + D_lo; |D| >= |D_obs[g]| counted per lane over the columns
// < P as there; s = wy_stat(D, cc, iv[g]) with iv read once per row at a clamped index and 0 for the rows g >= G.
// A lane's accumulator registers are 32 rows of each of its two columns (32 tile + its l31): it keeps the running
// maximum of s per column, the two lane halves -- the other 32 rows of the same columns -- meet by one shuffle, and
// the lane of half h combines column tile h into maxs[t][64 s + 32 h + l31] where that column is < P: pad columns
// reach neither d_r nor maxs.  The combine is the atomic alone: reading the value first to skip atomics that cannot
// win was measured equal at N = 2000 and slower at N = 256 (profiles/rank_wy.txt) -- the atomic returns nothing and
// nobody waits for it, the read is waited for.
__global__ __launch_bounds__(kWyWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_rank_maxt(const unsigned char* __restrict__ tiled, int64_t Gp, int Qp, int G, int nc,
                 const unsigned char* __restrict__ bfrag, const int32_t* __restrict__ dobs,
                 const double* __restrict__ d_iv, int cc, int64_t P, int S, int L, int nblk_genes,
                 int32_t* __restrict__ d_r, unsigned long long* __restrict__ d_maxs, int64_t maxs_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int gb = blockIdx.x % nblk_genes, rng = blockIdx.x / nblk_genes, t = blockIdx.y;
  const int s0 = rng * L, ns = min(L, S - s0);
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)lds;
  const uint32_t lane_off = (uint32_t)lane * 16u;
  const int nit = ns * nc;

  const unsigned char* bsrc = bfrag + ((int64_t)t * S + s0) * nc * kWyBChunk + wave * (kWyBChunk / kWyWaves);
  const unsigned char* asrc = tiled + ((int64_t)gb * kWyBlockGenes + (wave & 1) * 128) * 16;
  const uint32_t a_dst = kWyBChunk + (uint32_t)((wave >> 1) * kWyBlockGenes + (wave & 1) * 128) * 16u;
  auto issue = [&](int it, int cq) {
    const uint32_t buf = lds0 + (uint32_t)(it & 1) * kWyBuf;
#pragma unroll
    for (int x = 0; x < kWyBChunk / kWyWaves / kFragBytes; ++x)
      wy_dma16(buf + wave * (kWyBChunk / kWyWaves) + x * kFragBytes, lane_off, bsrc + x * kFragBytes);
    bsrc += kWyBChunk;
    const unsigned char* aq = asrc + (int64_t)min(2 * cq + (wave >> 1), Qp - 1) * Gp * 16;
#pragma unroll
    for (int x = 0; x < 2; ++x) wy_dma16(buf + a_dst + x * kFragBytes, lane_off, aq + x * kFragBytes);
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

  const int gene0 = gb * kWyBlockGenes + wave * 64 + 4 * half;   // the gene of row tile 0, register 0
  const int32_t* thr = dobs + (int64_t)t * G;
  const double* ivt = d_iv + (int64_t)t * G;
  unsigned long long* mrow = d_maxs + (int64_t)t * maxs_stride + 32 * half + l31;

  issue(0, 0);
  int c = 0, s = s0;
  for (int it = 0; it < nit; ++it) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (it + 1 < nit) issue(it + 1, c + 1 == nc ? 0 : c + 1);
    const unsigned char* buf = lds + (it & 1) * kWyBuf;
    const unsigned char* bb = buf + lane * 16;
    const unsigned char* ab = buf + kWyBChunk + (wave * 64 + l31) * 16;
#pragma unroll
    for (int qq = 0; qq < kWyChunkSteps / 4; ++qq) {
      v4i aw[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) aw[i] = *reinterpret_cast<const v4i*>(ab + (qq * kWyBlockGenes + i * 32) * 16);
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        const int k = qq * 4 + ww;
        v4i b[2][2];                               // [plane][column tile]
#pragma unroll
        for (int x = 0; x < 4; ++x)
          b[x >> 1][x & 1] = *reinterpret_cast<const v4i*>(bb + k * kWyStepBytes + x * kFragBytes);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const v4i a = wy_afrag((uint32_t)aw[i][ww], 16u * (uint32_t)half);
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
              acc[i][j][pl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[pl][j], acc[i][j][pl], 0, 0, 0);
        }
      }
    }
    if (++c == nc) {                               // the stage is whole: compare, count, take the maxima, start again
      const int64_t col0 = (int64_t)s * 64 + l31;
      const uint32_t v0 = col0 < P, v1 = col0 + 32 < P;
      double mx0 = 0.0, mx1 = 0.0;
      // |D_obs| and iv are read here, stage by stage, at addresses made here: the first gene is made opaque so that
      // neither the 64 loads nor their addresses are hoisted out of the main loop, where their registers do not fit
      // next to the accumulators.  A row tile's 32 loads go out together, ahead of its first use (the pins below
      // keep them there): two memory latencies per stage, not one per row.
      int g0 = gene0;
      asm volatile("" : "+v"(g0));
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        int a[16];
        double iv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int g = g0 + i * 32 + (r & 3) + 8 * (r >> 2);
          const int gc = min(g, G - 1);                                    // (the loads themselves are unconditional)
          a[r] = thr[gc];
          iv[r] = ivt[gc];
        }
        __builtin_amdgcn_sched_barrier(0);         // (nothing that waits for a load moves up among the loads)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int g = g0 + i * 32 + (r & 3) + 8 * (r >> 2);
          a[r] = g < G ? abs(a[r]) : 0x7fffffff;
          iv[r] = g < G ? iv[r] : 0.0;
          const int d0 = acc[i][0][0][r] * 128 + acc[i][0][1][r], d1 = acc[i][1][0][r] * 128 + acc[i][1][1][r];
          ex[i][r] += ((uint32_t)(abs(d0) >= a[r]) & v0) + ((uint32_t)(abs(d1) >= a[r]) & v1);
          asm volatile("" : "+v"(ex[i][r]));       // counted here, row by row: not sunk behind the combine with |D| held
          mx0 = fmax(mx0, wy_stat(d0, cc, iv[r]));
          mx1 = fmax(mx1, wy_stat(d1, cc, iv[r]));
        }
      }
      mx0 = fmax(mx0, __shfl_xor(mx0, 32));
      mx1 = fmax(mx1, __shfl_xor(mx1, 32));
      const unsigned long long mine = (unsigned long long)__double_as_longlong(half ? mx1 : mx0);
      if (half ? v1 : v0) atomicMax(mrow + (int64_t)s * 64, mine);
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

// the checks the entry points share: rs_check's of scoary_ranksum.hip, and the limits on T and G
int wy_check(scoary_handle h, const char* what, bool ok, int64_t G, int64_t T, int64_t N) {
  if (int rc = check_args(h, what, ok && G >= 1 && T >= 1 && N >= 1)) return rc;
  if (N > kWyMaxIsolates)
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": more isolates than scoary_ranksum_max_isolates()");
  if (T > 65535 || G > 0x7fffffffLL - 256) return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": T > 65535 or G >= 2^31");
  return SCOARY_OK;
}

}  // namespace

extern "C" {

int scoary_ranksum_var(scoary_handle h, const int32_t* d_m, const uint32_t* d_valid, const int64_t* d_tiesum,
                       int64_t G, int64_t T, int64_t N, double* d_var, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = wy_check(h, "scoary_ranksum_var", d_m && d_valid && d_tiesum && d_var, G, T, N)) return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  KernelTimer kt(h, s, "k_ranksum_var");
  hipLaunchKernelGGL(k_ranksum_var, dim3((unsigned)((G + 255) / 256), (unsigned)T), dim3(256), 0, s, d_m, d_valid,
                     d_tiesum, (int)G, (int)N, (int)scoary_row_words(N), d_var);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_rank_wy_prepare(scoary_handle h, const double* d_var, const int32_t* d_dobs, int64_t cc, int64_t G,
                           int64_t T, double* d_iv, double* d_sobs, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = wy_check(h, "scoary_rank_wy_prepare", d_var && d_dobs && d_iv && d_sobs && (cc == 0 || cc == 1), G, T,
                        1))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t cells = G * T;
  KernelTimer kt(h, s, "k_rank_wy_prepare");
  hipLaunchKernelGGL(k_rank_wy_prepare, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, d_var, d_dobs, (int)cc,
                     cells, d_iv, d_sobs);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_permute_rank_wy(scoary_handle h, const uint32_t* d_tiled, const void* d_bfrag, const int32_t* d_dobs,
                           const double* d_iv, int64_t cc, int64_t G, int64_t T, int64_t N, int64_t P, int32_t* d_r,
                           double* d_maxs, int64_t maxs_stride, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = wy_check(h, "scoary_permute_rank_wy", d_tiled && d_bfrag && d_dobs && d_iv && d_r && d_maxs && P >= 1 &&
                                                         maxs_stride >= P && (cc == 0 || cc == 1), G, T, N))
    return rc;
  if (P > 0x7fffffffLL) return fail(h, SCOARY_ERR_SIZE, "scoary_permute_rank_wy: P >= 2^31");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // 80 KB of dynamic LDS need the opt-in; asked for at every launch -- a host call per batch of permutations -- so that
  // the handle keeps no state for it (k_vanelteren_labels' way)
  HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rank_maxt),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kWyLds));
  // scoary_permute_ranksum's launch rule: enough blocks for eight rounds over the CUs' two places each
  const int64_t S = (P + 63) / 64, nblk = (G + kWyBlockGenes - 1) / kWyBlockGenes;
  const int64_t want =
      std::min<int64_t>(S, std::max<int64_t>(1, (16 * (int64_t)h->num_cu + nblk * T - 1) / (nblk * T)));
  const int64_t L = (S + want - 1) / want, ranges = (S + L - 1) / L;
  if (nblk * ranges > 0x7fffffffLL) return fail(h, SCOARY_ERR_SIZE, "scoary_permute_rank_wy: grid too large");
  KernelTimer kt(h, s, "k_rank_maxt");
  hipLaunchKernelGGL(k_rank_maxt, dim3((unsigned)(nblk * ranges), (unsigned)T), dim3(kWyWaves * 64), kWyLds, s,
                     reinterpret_cast<const unsigned char*>(d_tiled), scoary_tiled_genes(G),
                     (int)scoary_tiled_quads(N), (int)G, (int)wy_chunks(N), static_cast<const unsigned char*>(d_bfrag),
                     d_dobs, d_iv, (int)cc, P, (int)S, (int)L, (int)nblk, d_r,
                     reinterpret_cast<unsigned long long*>(d_maxs), maxs_stride);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
