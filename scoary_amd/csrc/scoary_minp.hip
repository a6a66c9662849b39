// scoary_minp.hip -- the Westfall-Young kernels: single-step minP (spec S7 of DESIGN.md) and step-down minP (S8).
//
// SINGLE-STEP (S7): for every permuted labelling the smallest raw Fisher p over all genes.  The dense permutation
// kernels (scoary_assoc.hip) reduce a permuted table to one bit per gene -- inside or outside that gene's rejection
// region -- which cannot be compared across genes; here every permuted table is turned into its p-value and the
// minimum over the genes is kept.
//
// Two parts:
//   p tables, once per (gene matrix, trait group): for every (trait, gene) the doubles p_tg(a) for every
//     overlap count a of the support, CSR-style (k_minp_sizes -> k_minp_scan -> k_minp_tables -> k_fisher).
//     The entries come from k_fisher ITSELF, run over the enumerated tables: bit-identical to the
//     association step's p by construction (SciPy's arithmetic up to 170 isolates, the canonical
//     orientation), at the price of a table list in scratch memory (24 bytes per entry of a chunk).
//   k_permute_minp: the transpose of k_permute_reg.  A LANE OWNS A PERMUTATION: its label row stays in
//     VGPRs, the gene rows arrive wave-uniform through the scalar cache, four genes per 64-byte line of
//     the tiled matrix; a = popcount(gene & label) as in the dense kernels, then one gather of p_tg(a)
//     -- the 64 gathers of a wavefront fall inside one gene's table -- and a running minimum in a
//     register: no cross-lane reduction, one 64-bit atomic min per (block, permutation) at the end.
//
// STEP-DOWN (S8): the single-step form compares every gene with the smallest permuted p over ALL genes; here the
// gene at rank k (genes sorted ascending by their own p) is compared with the smallest permuted p over the genes at
// rank k and behind:
//   q_b[k] = min over j >= k of p_b[order[j]],   c[k] = #{ b : q_b[k] <= ps[k] }.
// Same data flow as k_permute_minp -- a LANE OWNS A PERMUTATION, its label row in VGPRs, gene rows wave-uniform
// through the scalar cache, a = popcount(gene & label), one gather from the gene's p table, a running minimum in a
// register -- but the genes are visited in DESCENDING RANK ORDER, so that the running minimum after position k IS
// q_b[k], and it is compared with ps[k] on the spot.
//
// The walk is sequential in k.  It is cut into nch chunks of the rank order and run as two passes of one body
// (template <bool COUNT>): pass A (no carry) leaves the minimum of every (trait, chunk, permutation) in a cell of
// its own -- a plain store, one owner per cell; pass B starts a chunk from the minimum of the LATER chunks' cells
// and counts.  No block ever waits for another block.  Chunk 0 is not needed by anyone and is skipped in pass A;
// with one chunk pass A is not launched.  The pass-B blocks of chunk 0 end with q_b[0], which is S7's minp[t][b].
//
// Counting: per wavefront and position popcount(ballot(q <= ps[k])) is a scalar; it is written into lane (k & 63)
// of one VGPR (a compare and a select), and every 64 positions that register goes out as one 64-byte line of bytes
// cnt[t][permutation group][k .. k + 63].  k_stepdown_sum adds the lines of all permutation groups into c: no
// atomics, and integer sums do not depend on the order.
//
// Rank order: k_stepdown_prep turns (order, off, lo) into per-POSITION arrays -- the gene index and a 16-byte
// descriptor (table offset, lo, last index) -- padded to a multiple of 64 positions, so the walk loads them
// straight by k, and k_stepdown_gather copies every trait's gene rows into rank order, group-major
// (rows[t][k / 4][q][k % 4] = tiled[q][gene[t][k]]: one more gene matrix per trait in scratch, 12.8 MB per trait
// at 50 000 x 2000), so the four positions of a group are one 64-byte line per quad as in k_permute_minp, the
// lines of a group are contiguous and one pointer with immediate offsets reaches them.  Chosen by measurement
// (profiles/r13_stepdown.txt): the variant without a copy -- tiled[q * Gp + gene[k]], one 16-byte scalar load per
// gene and quad -- took 73.7 ms against 47.3 ms for the same body at 50 000 x 2000 x 10, P = 10 000, and is not kept.
//
// Shared by the two: the launch shape (wy_shape), the clamped gather (wy_gather), the 64-bit atomic min that
// publishes a permutation's minimum (wy_publish) and the argument checks of the two entry points (wy_check).  The
// kernels themselves stay apart on purpose: k_stepdown_minp stages its scalar loads line by line (sd_arrived),
// k_permute_minp leaves them to the compiler (profiles/r13_stepdown.txt).
#include "scoary_common.hpp"

namespace {

constexpr int kMinpGenes = 4;            // genes per scalar load: one 64-byte line of the tiled matrix
constexpr int64_t kMinpFillChunk = (int64_t)1 << 24;   // table entries per k_fisher launch of the fill
constexpr int kSdGenes = 4;              // positions per group of the register-resident walk
constexpr int kChunkedGenes = 8;         // genes / positions per pass over the row of the two chunked kernels (GB)

// The launch shape of both permute entry points: permutation groups of 64 and enough wavefronts to fill the chip
// several times over -- the genes (S8: the rank positions) are split into nch chunks when there are few permutation
// groups; a chunk is a multiple of 64 genes and at least 256 unless there are fewer.  Gs = positions padded to whole
// 64-position lines (S8).
struct WyShape {
  int64_t groups, nch, gchunk, Gs;
};

inline WyShape wy_shape(int num_cu, int64_t G, int64_t T, int64_t P) {
  WyShape s;
  s.groups = (P + kWave - 1) / kWave;
  const int64_t want = (int64_t)num_cu * 4 * 8;
  int64_t nch = (want + s.groups * T - 1) / (s.groups * T);
  nch = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nch, (G + 255) / 256), 65535));
  s.gchunk = round_up((G + nch - 1) / nch, kWave);
  s.nch = (G + s.gchunk - 1) / s.gchunk;
  s.Gs = round_up(G, kWave);
  return s;
}

// What scoary_permute_minp and scoary_permute_stepdown check alike; `own` = the caller's further pointers and its
// rule for minp_stride.  SCOARY_OK or the failure, recorded under the caller's name `fn`.
int wy_check(scoary_handle h, const char* fn, bool own, const void* d_tiled, const void* d_perms, const void* d_off,
             const void* d_lo, const void* d_tab, int64_t G, int64_t T, int64_t N, int64_t P, int64_t perm_base) {
  if (!h) return SCOARY_ERR_ARG;
  if (!own || !d_tiled || !d_perms || !d_off || !d_lo || !d_tab || G < 1 || T < 1 || N < 1 || P < 1 || perm_base < 0)
    return fail(h, SCOARY_ERR_ARG, std::string(fn) + ": bad argument");
  if (T > 65535 || G > (int64_t)1 << 30 || P > (int64_t)1 << 36)
    return fail(h, SCOARY_ERR_SIZE, std::string(fn) + ": T > 65535, G > 2^30 or P > 2^36");
  if (!tiled_quads_ok(scoary_tiled_quads(N)))
    return fail(h, SCOARY_ERR_SIZE, std::string(fn) + ": unsupported tiled row size");
  return SCOARY_OK;
}

// p of overlap count a from the gene's table tab[o0 .. o1) (overlap counts lo, lo + 1, ...): a label row with the
// trait's margins cannot leave the support; the clamp keeps any other row inside the gene's own table.  (The end o1
// and not the last index: with it the instruction streams of both families are those of the two gathers this replaced;
// a step-down position passes off + last + 1, which folds back to its last.)
__device__ __forceinline__ double wy_gather(const double* __restrict__ tab, int64_t o0, int64_t o1, int lo,
                                            uint32_t a) {
  return tab[o0 + min(max((int)a - lo, 0), (int)(o1 - o0) - 1)];
}

// permutation pi's minimum m into minp[t][perm_base + pi]; p is a non-negative double: its bit pattern orders like
// the value
__device__ __forceinline__ void wy_publish(unsigned long long* __restrict__ minp, int t, int64_t stride,
                                           int64_t perm_base, int64_t pi, int64_t P, double m) {
  if (pi < P && m < 1.0)
    atomicMin(&minp[(int64_t)t * stride + perm_base + pi], (unsigned long long)__double_as_longlong(m));
}

// ---- S7: the p tables and the single-step kernels ----

// support of the overlap count of table c: [lo, hi]
__device__ __forceinline__ void minp_support(const int4 c, int& lo, int& hi) {
  const int npos = c.x + c.y, gm = c.x + c.z, nval = c.x + c.y + c.z + c.w;
  lo = max(0, npos + gm - nval);
  hi = min(npos, gm);
}

__global__ __launch_bounds__(256) void k_minp_sizes(const int4* __restrict__ counts, int64_t M,
                                                    int64_t* __restrict__ off, int32_t* __restrict__ lo_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  int lo, hi;
  minp_support(counts[i], lo, hi);
  off[i] = hi - lo + 1;
  lo_out[i] = lo;
}

// (k_minp_scan, the exclusive prefix sum of the sizes, is scoary_common.hpp's: scoary_cmh.hip plans its tables with it too)

// entries [e0, e0 + ne) of the table list: entry e belongs to the (trait, gene) i with off[i] <= e < off[i + 1]
// and is the table with overlap count lo[i] + e - off[i] and the margins of counts[i]
__global__ __launch_bounds__(256) void k_minp_tables(const int4* __restrict__ counts, const int64_t* __restrict__ off,
                                                     const int32_t* __restrict__ lo, int64_t M, int64_t e0,
                                                     int64_t ne, int4* __restrict__ tables) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ne) return;
  const int64_t e = e0 + k;
  int64_t a = 0, b = M - 1;              // the largest i with off[i] <= e
  while (a < b) {
    const int64_t mid = (a + b + 1) >> 1;
    if (off[mid] <= e) a = mid; else b = mid - 1;
  }
  const int4 c = counts[a];
  const int npos = c.x + c.y, gm = c.x + c.z, nval = c.x + c.y + c.z + c.w;
  const int x = lo[a] + (int)(e - off[a]);
  tables[k] = make_int4(x, npos - x, gm - x, nval - npos - gm + x);
}

// Register-resident instance: RQ quads of the lane's label row in VGPRs.
// grid = (permutation groups of 64, gene chunks, T), block = one wavefront.
template <int RQ>
__global__ __launch_bounds__(64) void k_permute_minp(const uint4* __restrict__ tiled, const uint4* __restrict__ perms,
                                                     const int64_t* __restrict__ off, const int32_t* __restrict__ lo,
                                                     const double* __restrict__ tab, int G, int Gp, int64_t P,
                                                     int gchunk, int64_t perm_base, int64_t stride,
                                                     unsigned long long* __restrict__ minp) {
  const int t = blockIdx.z;
  const int64_t pi = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int g0 = blockIdx.y * gchunk, g1 = min(G, g0 + gchunk);
  uint4 lab[RQ];
  {
    const uint4* row = perms + ((int64_t)t * P + min(pi, P - 1)) * RQ;    // ragged last group: the last row again
#pragma unroll
    for (int q = 0; q < RQ; ++q) lab[q] = row[q];
  }
  const int64_t* offt = off + (int64_t)t * G;
  const int32_t* lot = lo + (int64_t)t * G;
  double m = 1.0;
  double pend[kMinpGenes];                 // the gathers of the previous gene group: used one group later
#pragma unroll
  for (int j = 0; j < kMinpGenes; ++j) pend[j] = 1.0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (int g = g0; g < g1; g += kMinpGenes) {
    uint32_t acc[kMinpGenes];
#pragma unroll
    for (int j = 0; j < kMinpGenes; ++j) acc[j] = 0;
#pragma unroll
    for (int q = 0; q < RQ; ++q) {
      const uint4* gp = tiled + (int64_t)q * Gp + g;     // wave-uniform, 64 bytes -> two s_load_dwordx8
#pragma unroll
      for (int j = 0; j < kMinpGenes; ++j) {
        const uint4 s = gp[j];
        and_popc(acc[j], lab[q], s);
      }
    }
#pragma unroll
    for (int j = 0; j < kMinpGenes; ++j) {
      m = pend[j] < m ? pend[j] : m;
      pend[j] = 1.0;
      if (g + j < g1)                                     // wave-uniform
        pend[j] = wy_gather(tab, offt[g + j], offt[g + j + 1], lot[g + j], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kMinpGenes; ++j) m = pend[j] < m ? pend[j] : m;
  wy_publish(minp, t, stride, perm_base, pi, P, m);
}

// Rows too long for registers (more than kMaxRegQuads = 24 quads: N > 3072): CQ-quad chunks of the label row, GB genes
// accumulated per pass over the row, as k_permute_chunked does with permutations.
template <int CQ, int GB>
__global__ __launch_bounds__(64) void k_permute_minp_chunked(const uint4* __restrict__ tiled,
                                                             const uint4* __restrict__ perms,
                                                             const int64_t* __restrict__ off,
                                                             const int32_t* __restrict__ lo,
                                                             const double* __restrict__ tab, int G, int Gp, int Qp,
                                                             int64_t P, int gchunk, int64_t perm_base, int64_t stride,
                                                             unsigned long long* __restrict__ minp) {
  static_assert(GB % kMinpGenes == 0, "whole 64-byte lines of the tiled matrix");
  const int t = blockIdx.z;
  const int64_t pi = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int g0 = blockIdx.y * gchunk, g1 = min(G, g0 + gchunk);
  const uint4* row = perms + ((int64_t)t * P + min(pi, P - 1)) * Qp;
  const int64_t* offt = off + (int64_t)t * G;
  const int32_t* lot = lo + (int64_t)t * G;
  const int nchunks = Qp / CQ;
  double m = 1.0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (int g = g0; g < g1; g += GB) {                     // g + GB <= Gp: gchunk and Gp are multiples of GB
    uint32_t acc[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) acc[j] = 0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int c = 0; c < nchunks; ++c) {
      uint4 lab[CQ];
#pragma unroll
      for (int q = 0; q < CQ; ++q) lab[q] = row[c * CQ + q];
#pragma unroll
      for (int q = 0; q < CQ; ++q) {
        const uint4* gp = tiled + (int64_t)(c * CQ + q) * Gp + g;   // wave-uniform
#pragma unroll
        for (int j = 0; j < GB; ++j) {
          const uint4 s = gp[j];
          and_popc(acc[j], lab[q], s);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      if (g + j < g1) {                                   // wave-uniform
        const double v = wy_gather(tab, offt[g + j], offt[g + j + 1], lot[g + j], acc[j]);
        m = v < m ? v : m;
      }
    }
  }
  wy_publish(minp, t, stride, perm_base, pi, P, m);
}

// ---- S8: the step-down kernels ----

struct SdDesc {                          // one rank position: tab[off + clamp(a - lo, 0, last)]
  int64_t off;
  int32_t lo, last;
};
static_assert(sizeof(SdDesc) == 16, "one 16-byte scalar load per position");

// byte offsets into d_scratch
struct SdLayout {
  int64_t gene, desc, cells, cnt, rows, total;
};

inline SdLayout sd_layout(const WyShape& s, int64_t T, int64_t Qp, int64_t P) {
  SdLayout l;
  int64_t at = 0;
  auto take = [&at](int64_t bytes) {
    const int64_t o = at;
    at += round_up(bytes, 256);
    return o;
  };
  l.gene = take(T * s.Gs * (int64_t)sizeof(int32_t));
  l.desc = take(T * s.Gs * (int64_t)sizeof(SdDesc));
  l.cells = take(T * s.nch * P * (int64_t)sizeof(double));
  l.cnt = take(T * s.groups * s.Gs);
  l.rows = take(T * Qp * s.Gs * (int64_t)sizeof(uint4));                      // the rows in rank order
  l.total = at;
  return l;
}

// position arrays of every trait: the gene at rank k and its table descriptor; positions G .. Gs - 1 point at gene 0
// and a one-entry table (they are fetched by whole groups, never consumed)
__global__ __launch_bounds__(256) void k_stepdown_prep(const int64_t* __restrict__ off, const int32_t* __restrict__ lo,
                                                       const int32_t* __restrict__ order, int G, int Gs, int64_t M,
                                                       int32_t* __restrict__ gene, SdDesc* __restrict__ desc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const int64_t t = i / Gs;
  const int k = (int)(i - t * Gs);
  int gi = 0;
  SdDesc d = {0, 0, 0};
  if (k < G) {
    gi = min(max(order[t * G + k], 0), G - 1);          // a caller's bad index stays inside the matrix
    const int64_t o0 = off[t * G + gi], o1 = off[t * G + gi + 1];
    d.off = o0;
    d.lo = lo[t * G + gi];
    d.last = (int32_t)(o1 - o0) - 1;
  }
  gene[i] = gi;
  desc[i] = d;
}

// rows[t][k / GB][q][k % GB] = tiled[q][gene[t][k]]: the GB positions of a group side by side, its quads one
// after the other
__global__ __launch_bounds__(256) void k_stepdown_gather(const uint4* __restrict__ tiled,
                                                         const int32_t* __restrict__ gene, int Gp, int Gs, int Qp,
                                                         int GB, int64_t M, uint4* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const int j = (int)(i % GB);
  const int64_t gq = i / GB;
  const int q = (int)(gq % Qp);
  const int64_t tg = gq / Qp;                            // t * (Gs / GB) + k / GB
  const int64_t t = tg / (Gs / GB);
  const int k = (int)(tg - t * (Gs / GB)) * GB + j;
  rows[i] = tiled[(int64_t)q * Gp + gene[t * Gs + k]];
}

// the four rows of a line are in their scalar registers from here on (the compiler places its wait in front)
__device__ __forceinline__ void sd_arrived(uint4 (&c)[kSdGenes]) {
  asm volatile("" : "+s"(c[0].x), "+s"(c[0].y), "+s"(c[0].z), "+s"(c[0].w), "+s"(c[1].x), "+s"(c[1].y), "+s"(c[1].z),
               "+s"(c[1].w), "+s"(c[2].x), "+s"(c[2].y), "+s"(c[2].z), "+s"(c[2].w), "+s"(c[3].x), "+s"(c[3].y),
               "+s"(c[3].z), "+s"(c[3].w));
}

// position k (wave-uniform) with its permuted p `v`: the running minimum becomes q_b[k]; pass B counts it
template <bool COUNT>
__device__ __forceinline__ void sd_consume(double& m, uint32_t& cntv, const double v, const int k, const int k1,
                                           const bool valid, const double* __restrict__ pst,
                                           uint8_t* __restrict__ cntrow) {
  if (k < k1) {
    m = v < m ? v : m;
    if (COUNT) {
      const uint32_t n = (uint32_t)__popcll(__ballot(valid && m <= pst[k]));       // at most 64
      cntv = (int)threadIdx.x == (k & (kWave - 1)) ? n : cntv;        // lane (k & 63) keeps position k's count
      if ((k & (kWave - 1)) == 0) {                      // the line k .. k + 63 is complete
        cntrow[k + threadIdx.x] = (uint8_t)cntv;
        cntv = 0;
      }
    }
  }
}

// the minimum of the later chunks' cells: where pass B starts
__device__ __forceinline__ double sd_carry(const double* __restrict__ cells, int t, int chunk, int nch, int64_t P,
                                           int64_t pi) {
  double m = 1.0;
  for (int c = chunk + 1; c < nch; ++c) {
    const double v = cells[((int64_t)t * nch + c) * P + pi];
    m = v < m ? v : m;
  }
  return m;
}

template <bool COUNT>
__device__ __forceinline__ void sd_finish(const double m, int t, int chunk, int nch, int64_t P, int64_t pi,
                                          double* __restrict__ cells, int64_t perm_base, int64_t stride,
                                          unsigned long long* __restrict__ minp) {
  if (pi >= P) return;
  if (!COUNT)
    cells[((int64_t)t * nch + chunk) * P + pi] = m;                  // one owner per cell
  else if (chunk == 0 && minp != nullptr)                            // q_b[0] = S7's minimum over all genes
    wy_publish(minp, t, stride, perm_base, pi, P, m);
}

// Register-resident instance: RQ quads of the lane's label row in VGPRs.
// grid = (permutation groups of 64, chunks [pass A: all but chunk 0], T), block = one wavefront.
// rows: the rank-ordered copy of k_stepdown_gather (groups of four positions).
template <int RQ, bool COUNT>
__global__ __launch_bounds__(64) void k_stepdown_minp(const uint4* __restrict__ rows, const uint4* __restrict__ perms,
                                                      const SdDesc* __restrict__ desc, const double* __restrict__ tab,
                                                      const double* __restrict__ ps, int G, int Gs, int64_t P,
                                                      int gchunk, int nch, double* __restrict__ cells,
                                                      uint8_t* __restrict__ cnt,
                                                      int64_t perm_base, int64_t stride,
                                                      unsigned long long* __restrict__ minp) {
  const int t = blockIdx.z;
  const int chunk = COUNT ? blockIdx.y : blockIdx.y + 1;
  const int64_t pi = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int64_t pc = min(pi, P - 1);                     // ragged last group: the last row again, never counted
  const int k0 = chunk * gchunk, k1 = min(G, k0 + gchunk);
  uint4 lab[RQ];
  {
    const uint4* row = perms + ((int64_t)t * P + pc) * RQ;
#pragma unroll
    for (int q = 0; q < RQ; ++q) lab[q] = row[q];
  }
  const SdDesc* dt = desc + (int64_t)t * Gs;
  const double* pst = ps + (int64_t)t * G;
  const uint4* base = rows + (int64_t)t * RQ * Gs;
  uint8_t* cntrow = cnt + ((int64_t)t * gridDim.x + blockIdx.x) * Gs;
  double m = COUNT ? sd_carry(cells, t, chunk, nch, P, pc) : 1.0;
  uint32_t cntv = 0;
  double pend[kSdGenes];                   // the gathers of the previous group: consumed one group later
#pragma unroll
  for (int j = 0; j < kSdGenes; ++j) pend[j] = 1.0;
  const int ktop = (k1 + kSdGenes - 1) & ~(kSdGenes - 1);               // k0 is a multiple of 64
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (int kb = ktop - kSdGenes; kb >= k0; kb -= kSdGenes) {
    uint32_t acc[kSdGenes];
#pragma unroll
    for (int j = 0; j < kSdGenes; ++j) acc[j] = 0;
    const uint4* grp = base + (int64_t)kb * RQ;          // the group's RQ lines of 64 bytes; wave-uniform
    // Scalar loads return out of order, so a wait is a wait for all of them: line q + 1 is requested only once
    // line q has arrived, and travels while line q is counted.
    uint4 cur[kSdGenes];
#pragma unroll
    for (int j = 0; j < kSdGenes; ++j) cur[j] = grp[j];
#pragma unroll
    for (int q = 0; q < RQ; ++q) {
      sd_arrived(cur);
      uint4 nxt[kSdGenes];
#pragma unroll
      for (int j = 0; j < kSdGenes; ++j) nxt[j] = q + 1 < RQ ? grp[(q + 1) * kSdGenes + j] : cur[j];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < kSdGenes; ++j) {
        and_popc(acc[j], lab[q], cur[j]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < kSdGenes; ++j) cur[j] = nxt[j];
    }
#pragma unroll
    for (int j = kSdGenes - 1; j >= 0; --j)              // the group above this one, highest rank first
      sd_consume<COUNT>(m, cntv, pend[j], kb + kSdGenes + j, k1, pi < P, pst, cntrow);
#pragma unroll
    for (int j = 0; j < kSdGenes; ++j) {
      const SdDesc d = dt[kb + j];
      pend[j] = wy_gather(tab, d.off, d.off + d.last + 1, d.lo, acc[j]);
    }
  }
#pragma unroll
  for (int j = kSdGenes - 1; j >= 0; --j) sd_consume<COUNT>(m, cntv, pend[j], k0 + j, k1, pi < P, pst, cntrow);
  sd_finish<COUNT>(m, t, chunk, nch, P, pi, cells, perm_base, stride, minp);
}

// Rows too long for registers (more than 24 quads): CQ-quad chunks of the label row, GB positions accumulated per
// pass over the row, as k_permute_minp_chunked does.
template <int CQ, int GB, bool COUNT>
__global__ __launch_bounds__(64) void k_stepdown_minp_chunked(const uint4* __restrict__ rows,
                                                              const uint4* __restrict__ perms,
                                                              const SdDesc* __restrict__ desc,
                                                              const double* __restrict__ tab,
                                                              const double* __restrict__ ps, int G, int Gs, int Qp,
                                                              int64_t P, int gchunk, int nch,
                                                              double* __restrict__ cells, uint8_t* __restrict__ cnt,
                                                              int64_t perm_base, int64_t stride,
                                                              unsigned long long* __restrict__ minp) {
  static_assert(kWave % GB == 0, "whole groups per 64-position line");
  const int t = blockIdx.z;
  const int chunk = COUNT ? blockIdx.y : blockIdx.y + 1;
  const int64_t pi = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int64_t pc = min(pi, P - 1);
  const int k0 = chunk * gchunk, k1 = min(G, k0 + gchunk);
  const uint4* row = perms + ((int64_t)t * P + pc) * Qp;
  const SdDesc* dt = desc + (int64_t)t * Gs;
  const double* pst = ps + (int64_t)t * G;
  const uint4* base = rows + (int64_t)t * Qp * Gs;
  uint8_t* cntrow = cnt + ((int64_t)t * gridDim.x + blockIdx.x) * Gs;
  const int nparts = Qp / CQ;
  double m = COUNT ? sd_carry(cells, t, chunk, nch, P, pc) : 1.0;
  uint32_t cntv = 0;
  const int ktop = (k1 + GB - 1) & ~(GB - 1);
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (int kb = ktop - GB; kb >= k0; kb -= GB) {
    uint32_t acc[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) acc[j] = 0;
    const uint4* grp = base + (int64_t)kb * Qp;          // the group's Qp lines of GB rows
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int c = 0; c < nparts; ++c) {
      uint4 lab[CQ];
#pragma unroll
      for (int q = 0; q < CQ; ++q) lab[q] = row[c * CQ + q];
#pragma unroll
      for (int q = 0; q < CQ; ++q) {
#pragma unroll
        for (int j = 0; j < GB; ++j) {
          const uint4 s = grp[(c * CQ + q) * GB + j];
          and_popc(acc[j], lab[q], s);
        }
      }
    }
#pragma unroll
    for (int j = GB - 1; j >= 0; --j) {
      const SdDesc d = dt[kb + j];
      const double v = wy_gather(tab, d.off, d.off + d.last + 1, d.lo, acc[j]);
      sd_consume<COUNT>(m, cntv, v, kb + j, k1, pi < P, pst, cntrow);
    }
  }
  sd_finish<COUNT>(m, t, chunk, nch, P, pi, cells, perm_base, stride, minp);
}

// c[t][k] += the counts of position k over all permutation groups; a thread takes four positions (one dword of
// every group's line)
__global__ __launch_bounds__(256) void k_stepdown_sum(const uint8_t* __restrict__ cnt, int G, int Gs, int groups,
                                                      uint32_t* __restrict__ c) {
  const int t = blockIdx.y;
  const int k4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (k4 >= G) return;
  const uint32_t* line = reinterpret_cast<const uint32_t*>(cnt + (int64_t)t * groups * Gs + k4);
  const int64_t step = Gs / 4;
  uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (int g = 0; g < groups; ++g) {
    const uint32_t w = line[g * step];
    s0 += w & 255u;
    s1 += (w >> 8) & 255u;
    s2 += (w >> 16) & 255u;
    s3 += w >> 24;
  }
  uint32_t* out = c + (int64_t)t * G + k4;
  out[0] += s0;
  if (k4 + 1 < G) out[1] += s1;
  if (k4 + 2 < G) out[2] += s2;
  if (k4 + 3 < G) out[3] += s3;
}

}  // namespace

extern "C" {

int64_t scoary_minp_fill_scratch_bytes(int64_t entries) {
  if (entries < 1) return 0;
  return std::min(entries, kMinpFillChunk) * (int64_t)(sizeof(int4) + sizeof(double));
}

int scoary_minp_plan(scoary_handle h, const int32_t* d_counts, int64_t T, int64_t G, int64_t* d_off,
                     int32_t* d_lo, int64_t* entries_out, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (!d_counts || !d_off || !d_lo || !entries_out || T < 1 || G < 1)
    return fail(h, SCOARY_ERR_ARG, "scoary_minp_plan: bad argument");
  if (T > 65535 || G > (int64_t)1 << 30) return fail(h, SCOARY_ERR_SIZE, "scoary_minp_plan: T > 65535 or G > 2^30");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t M = T * G;
  {
    KernelTimer kt(h, s, "k_minp_plan");
    hipLaunchKernelGGL(k_minp_sizes, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const int4*>(d_counts), M, d_off, d_lo);
    hipLaunchKernelGGL(k_minp_scan, dim3(1), dim3(1024), 0, s, d_off, M);
    HIP_TRY(h, hipGetLastError());
  }
  // the one read-back of the path: the caller sizes the tables with it
  HIP_TRY(h, hipMemcpyAsync(entries_out, d_off + M, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return SCOARY_OK;
}

int scoary_minp_fill(scoary_handle h, const int32_t* d_counts, const int64_t* d_off, const int32_t* d_lo,
                     int64_t T, int64_t G, int64_t entries, void* d_scratch, double* d_tab,
                     scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (!d_counts || !d_off || !d_lo || !d_scratch || !d_tab || T < 1 || G < 1 || entries < T * G)
    return fail(h, SCOARY_ERR_ARG, "scoary_minp_fill: bad argument");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t chunk = std::min(entries, kMinpFillChunk);
  int4* tables = static_cast<int4*>(d_scratch);
  double* odds = reinterpret_cast<double*>(tables + chunk);      // k_fisher's second output: not kept
  KernelTimer kt(h, s, "k_minp_fill");
  for (int64_t e0 = 0; e0 < entries; e0 += chunk) {
    const int64_t ne = std::min(chunk, entries - e0);
    hipLaunchKernelGGL(k_minp_tables, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const int4*>(d_counts), d_off, d_lo, T * G, e0, ne, tables);
    HIP_TRY(h, hipGetLastError());
    const int rc = scoary_fisher(h, reinterpret_cast<const int32_t*>(tables), ne, d_tab + e0, odds, nullptr, stream);
    if (rc != SCOARY_OK) return rc;
  }
  return SCOARY_OK;
}

int scoary_permute_minp(scoary_handle h, const uint32_t* d_tiled, const uint32_t* d_perms, const int64_t* d_off,
                        const int32_t* d_lo, const double* d_tab, int64_t G, int64_t T, int64_t N, int64_t P,
                        int64_t perm_base, int64_t minp_stride, double* d_minp, scoary_stream_t stream) {
  const int rc = wy_check(h, "scoary_permute_minp", d_minp && minp_stride >= perm_base + P, d_tiled, d_perms, d_off,
                          d_lo, d_tab, G, T, N, P, perm_base);
  if (rc != SCOARY_OK) return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t Gp = scoary_tiled_genes(G), Qp = scoary_tiled_quads(N);
  const WyShape sh = wy_shape(h->num_cu, G, T, P);
  const dim3 grid((unsigned)sh.groups, (unsigned)sh.nch, (unsigned)T);
  const uint4* t4 = reinterpret_cast<const uint4*>(d_tiled);
  const uint4* p4 = reinterpret_cast<const uint4*>(d_perms);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(d_minp);
  KernelTimer kt(h, s, "k_permute_minp");
  const bool reg = with_reg_quads(Qp, [&](auto rq) {
    hipLaunchKernelGGL((k_permute_minp<decltype(rq)::value>), grid, dim3(kWave), 0, s, t4, p4, d_off, d_lo, d_tab,
                       (int)G, (int)Gp, P, (int)sh.gchunk, perm_base, minp_stride, out);
  });
  if (!reg)
    hipLaunchKernelGGL((k_permute_minp_chunked<kChunkQuads, kChunkedGenes>), grid, dim3(kWave), 0, s, t4, p4,
                       d_off, d_lo, d_tab, (int)G, (int)Gp, (int)Qp, P, (int)sh.gchunk, perm_base, minp_stride, out);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int64_t scoary_stepdown_chunks(scoary_handle h, int64_t G, int64_t T, int64_t P) {
  if (!h || G < 1 || T < 1 || P < 1) return 0;
  return wy_shape(h->num_cu, G, T, P).nch;
}

int64_t scoary_stepdown_scratch_bytes(scoary_handle h, int64_t G, int64_t T, int64_t N, int64_t P) {
  if (!h || G < 1 || T < 1 || N < 1 || P < 1) return 0;
  return sd_layout(wy_shape(h->num_cu, G, T, P), T, scoary_tiled_quads(N), P).total;
}

int scoary_permute_stepdown(scoary_handle h, const uint32_t* d_tiled, const uint32_t* d_perms, const int64_t* d_off,
                            const int32_t* d_lo, const double* d_tab, const int32_t* d_order,
                            const double* d_psorted, int64_t G, int64_t T, int64_t N, int64_t P, int64_t perm_base,
                            int64_t minp_stride, double* d_minp, uint32_t* d_c, void* d_scratch,
                            scoary_stream_t stream) {
  const int rc = wy_check(h, "scoary_permute_stepdown",
                          d_order && d_psorted && d_c && d_scratch && (!d_minp || minp_stride >= perm_base + P),
                          d_tiled, d_perms, d_off, d_lo, d_tab, G, T, N, P, perm_base);
  if (rc != SCOARY_OK) return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t Gp = scoary_tiled_genes(G), Qp = scoary_tiled_quads(N);
  const WyShape sh = wy_shape(h->num_cu, G, T, P);
  const SdLayout lay = sd_layout(sh, T, Qp, P);
  if (T * sh.Gs * Qp / 256 >= (int64_t)1 << 31)
    return fail(h, SCOARY_ERR_SIZE, "scoary_permute_stepdown: the rank-ordered rows of T traits exceed one launch");
  char* scratch = static_cast<char*>(d_scratch);
  int32_t* gene = reinterpret_cast<int32_t*>(scratch + lay.gene);
  SdDesc* desc = reinterpret_cast<SdDesc*>(scratch + lay.desc);
  double* cells = reinterpret_cast<double*>(scratch + lay.cells);
  uint8_t* cnt = reinterpret_cast<uint8_t*>(scratch + lay.cnt);
  uint4* rows = reinterpret_cast<uint4*>(scratch + lay.rows);
  const uint4* p4 = reinterpret_cast<const uint4*>(d_perms);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(d_minp);
  const int64_t M = T * sh.Gs;
  {
    KernelTimer kt(h, s, "k_stepdown_prep");
    hipLaunchKernelGGL(k_stepdown_prep, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, d_off, d_lo, d_order,
                       (int)G, (int)sh.Gs, M, gene, desc);
    hipLaunchKernelGGL(k_stepdown_gather, dim3((unsigned)((M * Qp + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(d_tiled), gene, (int)Gp, (int)sh.Gs, (int)Qp,
                       Qp <= kMaxRegQuads ? kSdGenes : kChunkedGenes, M * Qp, rows);
    HIP_TRY(h, hipGetLastError());
  }
  // one pass: cells (COUNT false, all chunks but chunk 0) or count (COUNT true)
  const auto pass = [&](auto count) {
    constexpr bool COUNT = decltype(count)::value;
    const dim3 grid((unsigned)sh.groups, (unsigned)(COUNT ? sh.nch : sh.nch - 1), (unsigned)T);
    KernelTimer kt(h, s, COUNT ? "k_stepdown_minp_count" : "k_stepdown_minp_cells");
    const bool reg = with_reg_quads(Qp, [&](auto rq) {
      hipLaunchKernelGGL((k_stepdown_minp<decltype(rq)::value, COUNT>), grid, dim3(kWave), 0, s, rows, p4, desc, d_tab,
                         d_psorted, (int)G, (int)sh.Gs, P, (int)sh.gchunk, (int)sh.nch, cells, cnt, perm_base,
                         minp_stride, out);
    });
    if (!reg)
      hipLaunchKernelGGL((k_stepdown_minp_chunked<kChunkQuads, kChunkedGenes, COUNT>), grid, dim3(kWave), 0, s, rows,
                         p4, desc, d_tab, d_psorted, (int)G, (int)sh.Gs, (int)Qp, P, (int)sh.gchunk, (int)sh.nch,
                         cells, cnt, perm_base, minp_stride, out);
  };
  if (sh.nch > 1) {                                      // with one chunk nobody needs a cell
    pass(std::false_type{});
    HIP_TRY(h, hipGetLastError());
  }
  pass(std::true_type{});
  HIP_TRY(h, hipGetLastError());
  {
    KernelTimer kt(h, s, "k_stepdown_sum");
    hipLaunchKernelGGL(k_stepdown_sum, dim3((unsigned)((G + 1023) / 1024), (unsigned)T), dim3(256), 0, s, cnt, (int)G,
                       (int)sh.Gs, (int)sh.groups, d_c);
    HIP_TRY(h, hipGetLastError());
  }
  return SCOARY_OK;
}

}  // extern "C"
