// scoary_rank_stepdown.hip -- Westfall-Young step-down maxT over the rank statistics of the quantitative traits
// (spec S18 of DESIGN.md): S17's statistic s, the genes of a trait walked in rank order (descending s_obs), the gene
// at rank k compared per permuted row with u[k] = the maximum of s over the ranks k and behind.
//
//   k_rank_sd_gather  (once per analysis)  every trait's gene rows copied from the tiled matrix into rank order, and
//                                          s_obs, iv and |D_obs| next to them; the positions behind G up to the block
//                                          hold zero rows, iv 0 and a threshold no |D| reaches
//   k_rank_sd_max     (pass A)             k_rank_maxt's GEMM (scoary_rank_wy.hip) over the rank-ordered rows: behind a
//                                          stage's last chunk the exceedance count |D| >= |D_obs| by rank position and
//                                          the maximum of s over each wavefront's 64 ranks per column, stored to
//                                          gmax[t][group of 64 ranks][column] -- one owner per cell, plain stores
//   k_rank_sd_suffix                       one lane per (trait, column) walks the groups from the last to the first:
//                                          gmax becomes the maximum over the groups BEHIND each group, the overall
//                                          maximum goes to maxs (S17's, bit for bit: a maximum does not depend on
//                                          the order it is taken in)
//   k_rank_sd_count   (pass B)             the same product again: per column the wavefront's 64 ranks are scanned
//                                          from the last to the first with a running maximum that starts from the
//                                          group's suffix -- u[k] -- and u[k] >= ss[k] is counted per rank
// No block waits for another: the order of the work is the order of three launches on one stream.
#include "scoary_common.hpp"

namespace {

typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kSdMaxIsolates = 16320;             // = scoary_ranksum_max_isolates()
constexpr int kSdBlockGenes = 256;                // k_rank_maxt's geometry, constant for constant
constexpr int kSdWaves = 4;
constexpr int kSdChunkSteps = 8;
constexpr int kSdStepBytes = 4 * kFragBytes;
constexpr int kSdBChunk = kSdChunkSteps * kSdStepBytes;                 // 32 KB
constexpr int kSdAChunk = (kSdChunkSteps / 4) * kSdBlockGenes * 16;     // 8 KB
constexpr int kSdBuf = kSdBChunk + kSdAChunk;
constexpr int kSdLds = 2 * kSdBuf;
constexpr int kSdPadThreshold = 0x7fffffff;       // |D_obs| of a position behind G: no |D| (< 2^28) reaches it
static_assert(kSdLds * 2 <= 160 * 1024, "two blocks of a pass per CU");
static_assert(kSdBlockGenes == kGeneAlign, "a padded gene count is whole blocks");

__host__ __device__ constexpr int64_t sd_chunks(int64_t N) {
  return ((N + 31) / 32 + kSdChunkSteps - 1) / kSdChunkSteps;
}

// S17's statistic of a cell, wy_stat of scoary_rank_wy.hip operation for operation (restated so that that file
// compiles exactly as it did; the library is built without contraction, so the roundings are the same two)
__device__ __forceinline__ double sd_stat(int D, int cc, double iv) {
  const double e = (double)max(0, abs(D) - cc);
  const double e2 = e * e;
  return e2 * iv;
}

// d_scratch: byte offsets of its parts.  Everything before gmax is what the gather writes and does not depend on P.
struct SdLayout {
  int64_t Gp, Qp, groups, cols;     // padded positions, quads per row, groups of 64 positions, padded columns
  int64_t rows, ss, iv, dabs, gmax, total;
};
SdLayout sd_layout(int64_t G, int64_t T, int64_t N, int64_t P) {
  SdLayout l;
  l.Gp = scoary_tiled_genes(G);
  l.Qp = scoary_tiled_quads(N);
  l.groups = l.Gp / 64;
  l.cols = (P + 63) / 64 * 64;
  l.rows = 0;
  l.ss = l.rows + T * l.Qp * l.Gp * 16;
  l.iv = l.ss + T * l.Gp * 8;
  l.dabs = l.iv + T * l.Gp * 8;
  l.gmax = l.dabs + T * l.Gp * 4;
  l.total = l.gmax + T * l.groups * l.cols * 8;
  return l;
}

// position k of trait blockIdx.z, quad blockIdx.y: the row of gene order[t][k], zero behind G
__global__ __launch_bounds__(256) void k_rank_sd_gather(const uint4* __restrict__ tiled,
                                                        const int32_t* __restrict__ order,
                                                        const double* __restrict__ sobs,
                                                        const double* __restrict__ d_iv,
                                                        const int32_t* __restrict__ dobs, int G, int64_t Gp, int Qp,
                                                        uint4* __restrict__ rows, double* __restrict__ ss,
                                                        double* __restrict__ iv, int32_t* __restrict__ dabs) {
  const int t = blockIdx.z, q = blockIdx.y;
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= Gp) return;
  int g = k < G ? order[(int64_t)t * G + k] : -1;
  if ((unsigned)g >= (unsigned)G) g = -1;          // (an index that is no gene reads nothing)
  rows[((int64_t)t * Qp + q) * Gp + k] = g >= 0 ? tiled[(int64_t)q * Gp + g] : make_uint4(0u, 0u, 0u, 0u);
  if (q == 0) {
    const int64_t o = (int64_t)t * G + g;
    ss[(int64_t)t * Gp + k] = g >= 0 ? sobs[o] : 0.0;
    iv[(int64_t)t * Gp + k] = g >= 0 ? d_iv[o] : 0.0;
    dabs[(int64_t)t * Gp + k] = g >= 0 ? abs(dobs[o]) : kSdPadThreshold;
  }
}

// One 16-byte vector per lane, src + 16 * lane -> LDS address lds + 16 * lane, by LDS-DMA (k_rank_maxt's transfer)
__device__ __forceinline__ void sd_dma16(uint32_t lds, uint32_t lane_off, const unsigned char* src) {
  uint32_t m0_saved;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0"
               : "=&s"(m0_saved)
               : "s"(lds), "v"(lane_off), "s"(src)
               : "memory");
}

__device__ __forceinline__ int sd_bytes_of_bits4(uint32_t x) { return (int)((x * 0x00204081u) & 0x01010101u); }
__device__ __forceinline__ v4i sd_afrag(uint32_t word, uint32_t sh) {
  return v4i{sd_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh, 4u)),
             sd_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh + 4u, 4u)),
             sd_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh + 8u, 4u)),
             sd_bytes_of_bits4(__builtin_amdgcn_ubfe(word, sh + 12u, 4u))};
}

// k_rank_maxt's block and main loop (scoary_rank_wy.hip; restated here so that that kernel compiles exactly as it
// did), over trait blockIdx.y's rank-ordered rows: block = 256 rank positions x the stages [s0, s0 + ns) of 64
// permutations, wavefront w owns the positions 64 w .. 64 w + 63 of the block -- one group of gmax -- against both
// column tiles and both digit planes.  A lane's accumulator registers are the rows 4 half + (r & 3) + 8 (r >> 2) +
// 32 i of its two columns (32 j + l31): runs of four consecutive ranks that alternate between the two lane halves.
//
// Behind a stage's last chunk, D = 128 D_hi + D_lo and s = sd_stat(D, cc, iv[k]) per cell.  The thresholds are read
// there, stage by stage, at a first position made opaque, so that neither the loads nor their addresses are hoisted
// into the main loop, where their registers do not fit next to the accumulators; the arrays are padded to the block,
// so no index is clamped and the positions behind G answer for themselves (iv 0: s = 0; threshold 2^31 - 1).
//
// kCount = false (pass A): |D| >= |D_obs| counted per lane over the columns < P, as k_rank_maxt counts it; the
// maximum of s over the lane's 32 rows per column, the two halves met by one shuffle, and the lane of half h stores
// column tile h to gmax[t][group][64 s + 32 h + l31].  Pad columns are stored too: their cells may hold anything.
//
// kCount = true (pass B): per column the 64 rows are scanned from the last to the first.  A run of four rows is
// scanned inside its lane (m[x] = the maximum of the run's rows x and behind); the running maximum `inc` enters the
// run of half 1 first (the higher ranks), leaves it as max(inc, m[0]), crosses to half 0 by one shuffle, and after
// that run crosses back: two shuffles per eight rows and column.  u[k] = max(what entered the run, m[x]);
// u[k] >= ss[k] is counted per lane over the columns < P.  Both halves execute both steps; each keeps what is its
// own (half 1: `inc`; half 0: what the first shuffle brought).
//
// Either way the counters of a row are summed over the 32 lanes that hold its columns behind the last stage and
// added to d_out[t][k], k < G, as k_rank_maxt adds d_r: several ranges of stages add to one position.
template <bool kCount>
__device__ __forceinline__ void sd_block(const unsigned char* __restrict__ rows, int64_t Gp, int Qp, int G, int nc,
                                         const unsigned char* __restrict__ bfrag, const int32_t* __restrict__ dabs,
                                         const double* __restrict__ ssr, const double* __restrict__ ivr, int cc,
                                         int64_t P, int S, int L, int nblk_genes, int32_t* __restrict__ d_out,
                                         double* __restrict__ gmax) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int gb = blockIdx.x % nblk_genes, rng = blockIdx.x / nblk_genes, t = blockIdx.y;
  const int s0 = rng * L, ns = min(L, S - s0);
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)lds;
  const uint32_t lane_off = (uint32_t)lane * 16u;
  const int nit = ns * nc;

  const unsigned char* bsrc = bfrag + ((int64_t)t * S + s0) * nc * kSdBChunk + wave * (kSdBChunk / kSdWaves);
  const unsigned char* asrc =
      rows + ((int64_t)t * Qp * Gp + (int64_t)gb * kSdBlockGenes + (wave & 1) * 128) * 16;
  const uint32_t a_dst = kSdBChunk + (uint32_t)((wave >> 1) * kSdBlockGenes + (wave & 1) * 128) * 16u;
  auto issue = [&](int it, int cq) {
    const uint32_t buf = lds0 + (uint32_t)(it & 1) * kSdBuf;
#pragma unroll
    for (int x = 0; x < kSdBChunk / kSdWaves / kFragBytes; ++x)
      sd_dma16(buf + wave * (kSdBChunk / kSdWaves) + x * kFragBytes, lane_off, bsrc + x * kFragBytes);
    bsrc += kSdBChunk;
    const unsigned char* aq = asrc + (int64_t)min(2 * cq + (wave >> 1), Qp - 1) * Gp * 16;
#pragma unroll
    for (int x = 0; x < 2; ++x) sd_dma16(buf + a_dst + x * kFragBytes, lane_off, aq + x * kFragBytes);
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

  const int rank0 = gb * kSdBlockGenes + wave * 64 + 4 * half;   // the position of row tile 0, register 0
  const int64_t cols = (int64_t)S * 64;
  const int32_t* thr = dabs + (int64_t)t * Gp;
  const double* sst = ssr + (int64_t)t * Gp;
  const double* ivt = ivr + (int64_t)t * Gp;
  double* gm = gmax + ((int64_t)t * (Gp / 64) + (gb * kSdWaves + wave)) * cols + l31;

  issue(0, 0);
  int c = 0, s = s0;
  for (int it = 0; it < nit; ++it) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (it + 1 < nit) issue(it + 1, c + 1 == nc ? 0 : c + 1);
    const unsigned char* buf = lds + (it & 1) * kSdBuf;
    const unsigned char* bb = buf + lane * 16;
    const unsigned char* ab = buf + kSdBChunk + (wave * 64 + l31) * 16;
#pragma unroll
    for (int qq = 0; qq < kSdChunkSteps / 4; ++qq) {
      v4i aw[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) aw[i] = *reinterpret_cast<const v4i*>(ab + (qq * kSdBlockGenes + i * 32) * 16);
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        const int k = qq * 4 + ww;
        v4i b[2][2];                               // [plane][column tile]
#pragma unroll
        for (int x = 0; x < 4; ++x)
          b[x >> 1][x & 1] = *reinterpret_cast<const v4i*>(bb + k * kSdStepBytes + x * kFragBytes);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const v4i a = sd_afrag((uint32_t)aw[i][ww], 16u * (uint32_t)half);
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
              acc[i][j][pl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[pl][j], acc[i][j][pl], 0, 0, 0);
        }
      }
    }
    if (++c == nc) {                               // the stage is whole
      const int64_t col0 = (int64_t)s * 64 + l31;
      const uint32_t v0 = col0 < P, v1 = col0 + 32 < P;
      int k0 = rank0;
      asm volatile("" : "+v"(k0));
      if constexpr (!kCount) {
        double mx0 = 0.0, mx1 = 0.0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          int a[16];
          double iv[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k = k0 + i * 32 + (r & 3) + 8 * (r >> 2);
            a[r] = thr[k];
            iv[r] = ivt[k];
          }
          __builtin_amdgcn_sched_barrier(0);       // (nothing that waits for a load moves up among the loads)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int d0 = acc[i][0][0][r] * 128 + acc[i][0][1][r], d1 = acc[i][1][0][r] * 128 + acc[i][1][1][r];
            ex[i][r] += ((uint32_t)(abs(d0) >= a[r]) & v0) + ((uint32_t)(abs(d1) >= a[r]) & v1);
            asm volatile("" : "+v"(ex[i][r]));
            mx0 = fmax(mx0, sd_stat(d0, cc, iv[r]));
            mx1 = fmax(mx1, sd_stat(d1, cc, iv[r]));
          }
        }
        mx0 = fmax(mx0, __shfl_xor(mx0, 32));
        mx1 = fmax(mx1, __shfl_xor(mx1, 32));
        gm[(int64_t)s * 64 + 32 * half] = half ? mx1 : mx0;
      } else {
        double inc0 = gm[(int64_t)s * 64], inc1 = gm[(int64_t)s * 64 + 32];   // the maximum behind this group
#pragma unroll
        for (int i = 1; i >= 0; --i) {
#pragma unroll
          for (int hb = 1; hb >= 0; --hb) {        // eight of the lane's rows at a time: two runs of four
            double ss[8], iv[8];
#pragma unroll
            for (int x = 0; x < 8; ++x) {
              const int k = k0 + i * 32 + (x & 3) + 8 * (2 * hb + (x >> 2));
              ss[x] = sst[k];
              iv[x] = ivt[k];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int blk = 1; blk >= 0; --blk) {
              double m0[4], m1[4];
#pragma unroll
              for (int x = 3; x >= 0; --x) {
                const int r = 8 * hb + 4 * blk + x;
                const int d0 = acc[i][0][0][r] * 128 + acc[i][0][1][r], d1 = acc[i][1][0][r] * 128 + acc[i][1][1][r];
                const double s0x = sd_stat(d0, cc, iv[4 * blk + x]), s1x = sd_stat(d1, cc, iv[4 * blk + x]);
                m0[x] = x == 3 ? s0x : fmax(s0x, m0[x + 1]);
                m1[x] = x == 3 ? s1x : fmax(s1x, m1[x + 1]);
              }
              const double t0 = __shfl_xor(fmax(inc0, m0[0]), 32), t1 = __shfl_xor(fmax(inc1, m1[0]), 32);
              const double e0 = half ? inc0 : t0, e1 = half ? inc1 : t1;     // what enters this lane's run
#pragma unroll
              for (int x = 0; x < 4; ++x) {
                const int r = 8 * hb + 4 * blk + x;
                ex[i][r] += ((uint32_t)(fmax(e0, m0[x]) >= ss[4 * blk + x]) & v0) +
                            ((uint32_t)(fmax(e1, m1[x]) >= ss[4 * blk + x]) & v1);
                asm volatile("" : "+v"(ex[i][r]));
              }
              inc0 = __shfl_xor(fmax(e0, m0[0]), 32);    // half 1 receives what left half 0's run
              inc1 = __shfl_xor(fmax(e1, m1[0]), 32);
            }
          }
        }
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
      const int k = rank0 + i * 32 + (r & 3) + 8 * (r >> 2);
      if (l31 == 0 && k < G && v) atomicAdd(d_out + (int64_t)t * G + k, (int32_t)v);
    }
}

__global__ __launch_bounds__(kSdWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_rank_sd_max(const unsigned char* __restrict__ rows, int64_t Gp, int Qp, int G, int nc,
                   const unsigned char* __restrict__ bfrag, const int32_t* __restrict__ dabs,
                   const double* __restrict__ ivr, int cc, int64_t P, int S, int L, int nblk_genes,
                   int32_t* __restrict__ d_r, double* __restrict__ gmax) {
  sd_block<false>(rows, Gp, Qp, G, nc, bfrag, dabs, nullptr, ivr, cc, P, S, L, nblk_genes, d_r, gmax);
}

__global__ __launch_bounds__(kSdWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_rank_sd_count(const unsigned char* __restrict__ rows, int64_t Gp, int Qp, int G, int nc,
                     const unsigned char* __restrict__ bfrag, const double* __restrict__ ssr,
                     const double* __restrict__ ivr, int cc, int64_t P, int S, int L, int nblk_genes,
                     int32_t* __restrict__ d_c, double* __restrict__ gmax) {
  sd_block<true>(rows, Gp, Qp, G, nc, bfrag, nullptr, ssr, ivr, cc, P, S, L, nblk_genes, d_c, gmax);
}

// lane = (trait blockIdx.y, column): gmax[t][g][column] <- the maximum over the groups behind g (0.0 behind the
// last), and the maximum over all of them to maxs[t][perm_base + column] where the column is a permutation
__global__ __launch_bounds__(256) void k_rank_sd_suffix(double* __restrict__ gmax, int groups, int64_t cols,
                                                        int64_t P, int64_t perm_base, double* __restrict__ maxs,
                                                        int64_t maxs_stride) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int t = blockIdx.y;
  if (col >= cols) return;
  double* g = gmax + (int64_t)t * groups * cols + col;
  double run = 0.0;
#pragma unroll 8
  for (int gi = groups - 1; gi >= 0; --gi) {
    const double v = g[(int64_t)gi * cols];
    g[(int64_t)gi * cols] = run;
    run = fmax(run, v);
  }
  if (col < P) maxs[(int64_t)t * maxs_stride + perm_base + col] = run;
}

// wy_check of scoary_rank_wy.hip: the refusals the S17 entry points make, in their order
int sd_check(scoary_handle h, const char* what, bool ok, int64_t G, int64_t T, int64_t N) {
  if (int rc = check_args(h, what, ok && G >= 1 && T >= 1 && N >= 1)) return rc;
  if (N > kSdMaxIsolates)
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": more isolates than scoary_ranksum_max_isolates()");
  if (T > 65535 || G > 0x7fffffffLL - 256) return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": T > 65535 or G >= 2^31");
  return SCOARY_OK;
}

}  // namespace

extern "C" {

int64_t scoary_rank_stepdown_scratch_bytes(scoary_handle h, int64_t G, int64_t T, int64_t N, int64_t P) {
  if (!h || G < 1 || T < 1 || N < 1 || P < 1) return 0;
  return sd_layout(G, T, N, P).total;
}

int scoary_rank_stepdown_gather(scoary_handle h, const uint32_t* d_tiled, const int32_t* d_order,
                                const double* d_sobs, const double* d_iv, const int32_t* d_dobs, int64_t G, int64_t T,
                                int64_t N, void* d_scratch, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = sd_check(h, "scoary_rank_stepdown_gather", d_tiled && d_order && d_sobs && d_iv && d_dobs && d_scratch,
                        G, T, N))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const SdLayout l = sd_layout(G, T, N, 1);
  if (l.Gp / 256 > 0x7fffffffLL) return fail(h, SCOARY_ERR_SIZE, "scoary_rank_stepdown_gather: grid too large");
  unsigned char* base = static_cast<unsigned char*>(d_scratch);
  KernelTimer kt(h, s, "k_rank_sd_gather");
  hipLaunchKernelGGL(k_rank_sd_gather, dim3((unsigned)(l.Gp / 256), (unsigned)l.Qp, (unsigned)T), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(d_tiled), d_order, d_sobs, d_iv, d_dobs, (int)G, l.Gp, (int)l.Qp,
                     reinterpret_cast<uint4*>(base + l.rows), reinterpret_cast<double*>(base + l.ss),
                     reinterpret_cast<double*>(base + l.iv), reinterpret_cast<int32_t*>(base + l.dabs));
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_permute_rank_stepdown(scoary_handle h, void* d_scratch, const void* d_bfrag, int64_t cc, int64_t G,
                                 int64_t T, int64_t N, int64_t P, int64_t perm_base, int32_t* d_r_rank,
                                 int32_t* d_c_rank, double* d_maxs, int64_t maxs_stride, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = sd_check(h, "scoary_permute_rank_stepdown",
                        d_scratch && d_bfrag && d_r_rank && d_c_rank && d_maxs && P >= 1 && perm_base >= 0 &&
                            maxs_stride - perm_base >= P && (cc == 0 || cc == 1), G, T, N))
    return rc;
  if (P > 0x7fffffffLL) return fail(h, SCOARY_ERR_SIZE, "scoary_permute_rank_stepdown: P >= 2^31");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // 80 KB of dynamic LDS need the opt-in; asked for at every launch, so that the handle keeps no state for it
  HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rank_sd_max),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kSdLds));
  HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rank_sd_count),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kSdLds));
  // scoary_permute_rank_wy's launch rule
  const SdLayout l = sd_layout(G, T, N, P);
  const int64_t S = l.cols / 64, nblk = l.Gp / kSdBlockGenes;
  const int64_t want =
      std::min<int64_t>(S, std::max<int64_t>(1, (16 * (int64_t)h->num_cu + nblk * T - 1) / (nblk * T)));
  const int64_t L = (S + want - 1) / want, ranges = (S + L - 1) / L;
  if (nblk * ranges > 0x7fffffffLL || (l.cols + 255) / 256 > 0x7fffffffLL)
    return fail(h, SCOARY_ERR_SIZE, "scoary_permute_rank_stepdown: grid too large");
  unsigned char* base = static_cast<unsigned char*>(d_scratch);
  const unsigned char* rows = base + l.rows;
  const double* ss = reinterpret_cast<const double*>(base + l.ss);
  const double* iv = reinterpret_cast<const double*>(base + l.iv);
  const int32_t* dabs = reinterpret_cast<const int32_t*>(base + l.dabs);
  double* gmax = reinterpret_cast<double*>(base + l.gmax);
  const dim3 grid((unsigned)(nblk * ranges), (unsigned)T);
  {
    KernelTimer kt(h, s, "k_rank_sd_max");
    hipLaunchKernelGGL(k_rank_sd_max, grid, dim3(kSdWaves * 64), kSdLds, s, rows, l.Gp, (int)l.Qp, (int)G,
                       (int)sd_chunks(N), static_cast<const unsigned char*>(d_bfrag), dabs, iv, (int)cc, P, (int)S,
                       (int)L, (int)nblk, d_r_rank, gmax);
    HIP_TRY(h, hipGetLastError());
  }
  {
    KernelTimer kt(h, s, "k_rank_sd_suffix");
    hipLaunchKernelGGL(k_rank_sd_suffix, dim3((unsigned)((l.cols + 255) / 256), (unsigned)T), dim3(256), 0, s, gmax,
                       (int)l.groups, l.cols, P, perm_base, d_maxs, maxs_stride);
    HIP_TRY(h, hipGetLastError());
  }
  {
    KernelTimer kt(h, s, "k_rank_sd_count");
    hipLaunchKernelGGL(k_rank_sd_count, grid, dim3(kSdWaves * 64), kSdLds, s, rows, l.Gp, (int)l.Qp, (int)G,
                       (int)sd_chunks(N), static_cast<const unsigned char*>(d_bfrag), ss, iv, (int)cc, P, (int)S,
                       (int)L, (int)nblk, d_c_rank, gmax);
    HIP_TRY(h, hipGetLastError());
  }
  return SCOARY_OK;
}

}  // extern "C"
