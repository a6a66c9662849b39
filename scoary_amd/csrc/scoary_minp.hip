// scoary_minp.hip -- Westfall-Young single-step minP (spec S7 of DESIGN.md): for every permuted labelling the
// smallest raw Fisher p over all genes.  The dense permutation kernels (scoary_assoc.hip) reduce a permuted
// table to one bit per gene -- inside or outside that gene's rejection region -- which cannot be compared
// across genes; here every permuted table is turned into its p-value and the minimum over the genes is kept.
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
#include "scoary_common.hpp"

namespace {

constexpr int kMinpGenes = 4;            // genes per scalar load: one 64-byte line of the tiled matrix
constexpr int64_t kMinpFillChunk = (int64_t)1 << 24;   // table entries per k_fisher launch of the fill

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

// exclusive prefix sum of off[0 .. M) in place, off[M] = total.  One block walks the array in tiles of
// 1024 with a running carry (once per trait group: 0.5 M entries are ~500 tiles).
__global__ __launch_bounds__(1024) void k_minp_scan(int64_t* __restrict__ off, int64_t M) {
  __shared__ int64_t s_wave[16];
  __shared__ int64_t s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < M; base += 1024) {
    const int64_t i = base + tid;
    const int64_t v = i < M ? off[i] : 0;
    int64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    int64_t before = s_carry;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (i < M) off[i] = before + x - v;
    __syncthreads();
    if (tid == 1023) s_carry = before + x;
    __syncthreads();
  }
  if (tid == 0) off[M] = s_carry;
}

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

__device__ __forceinline__ double minp_gather(const double* __restrict__ tab, int64_t o0, int64_t o1, int lo,
                                              uint32_t a) {
  // a label row with the trait's margins cannot leave the support; the clamp keeps any other row
  // inside the gene's own table
  const int idx = min(max((int)a - lo, 0), (int)(o1 - o0) - 1);
  return tab[o0 + idx];
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
        bcnt_acc(acc[j], lab[q].x & s.x);
        bcnt_acc(acc[j], lab[q].y & s.y);
        bcnt_acc(acc[j], lab[q].z & s.z);
        bcnt_acc(acc[j], lab[q].w & s.w);
      }
    }
#pragma unroll
    for (int j = 0; j < kMinpGenes; ++j) {
      m = pend[j] < m ? pend[j] : m;
      pend[j] = 1.0;
      if (g + j < g1)                                     // wave-uniform
        pend[j] = minp_gather(tab, offt[g + j], offt[g + j + 1], lot[g + j], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kMinpGenes; ++j) m = pend[j] < m ? pend[j] : m;
  // p is a non-negative double: its bit pattern orders like the value
  if (pi < P && m < 1.0)
    atomicMin(&minp[(int64_t)t * stride + perm_base + pi], (unsigned long long)__double_as_longlong(m));
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
          bcnt_acc(acc[j], lab[q].x & s.x);
          bcnt_acc(acc[j], lab[q].y & s.y);
          bcnt_acc(acc[j], lab[q].z & s.z);
          bcnt_acc(acc[j], lab[q].w & s.w);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      if (g + j < g1) {                                   // wave-uniform
        const double v = minp_gather(tab, offt[g + j], offt[g + j + 1], lot[g + j], acc[j]);
        m = v < m ? v : m;
      }
    }
  }
  if (pi < P && m < 1.0)
    atomicMin(&minp[(int64_t)t * stride + perm_base + pi], (unsigned long long)__double_as_longlong(m));
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
  if (!h) return SCOARY_ERR_ARG;
  if (!d_tiled || !d_perms || !d_off || !d_lo || !d_tab || !d_minp || G < 1 || T < 1 || N < 1 || P < 1 ||
      perm_base < 0 || minp_stride < perm_base + P)
    return fail(h, SCOARY_ERR_ARG, "scoary_permute_minp: bad argument");
  if (T > 65535 || G > (int64_t)1 << 30 || P > (int64_t)1 << 36)
    return fail(h, SCOARY_ERR_SIZE, "scoary_permute_minp: T > 65535, G > 2^30 or P > 2^36");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t Gp = scoary_tiled_genes(G), Qp = scoary_tiled_quads(N);
  if (Qp > kMaxRegQuads && Qp % kChunkQuads != 0)
    return fail(h, SCOARY_ERR_SIZE, "scoary_permute_minp: unsupported tiled row size");
  // enough wavefronts to fill the chip several times over: split the genes when there are few
  // permutation groups; a chunk is a multiple of 64 genes and at least 256
  const int64_t groups = (P + kWave - 1) / kWave;
  const int64_t want = (int64_t)h->num_cu * 4 * 8;
  int64_t nch = (want + groups * T - 1) / (groups * T);
  nch = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nch, (G + 255) / 256), 65535));
  const int64_t gchunk = round_up((G + nch - 1) / nch, kWave);
  nch = (G + gchunk - 1) / gchunk;
  const dim3 grid((unsigned)groups, (unsigned)nch, (unsigned)T);
  const uint4* t4 = reinterpret_cast<const uint4*>(d_tiled);
  const uint4* p4 = reinterpret_cast<const uint4*>(d_perms);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(d_minp);
  KernelTimer kt(h, s, "k_permute_minp");
  if (Qp <= kMaxRegQuads) {
    switch (Qp) {
#define CASE_RQ(RQ)                                                                                          \
  case RQ:                                                                                                   \
    hipLaunchKernelGGL((k_permute_minp<RQ>), grid, dim3(kWave), 0, s, t4, p4, d_off, d_lo, d_tab, (int)G,    \
                       (int)Gp, P, (int)gchunk, perm_base, minp_stride, out);                                \
    break;
      CASE_RQ(1) CASE_RQ(2) CASE_RQ(4) CASE_RQ(6) CASE_RQ(8) CASE_RQ(12) CASE_RQ(16) CASE_RQ(20)
      CASE_RQ(24)
#undef CASE_RQ
      default:
        return fail(h, SCOARY_ERR_SIZE, "scoary_permute_minp: unsupported tiled row size");
    }
  } else {
    hipLaunchKernelGGL((k_permute_minp_chunked<kChunkQuads, 8>), grid, dim3(kWave), 0, s, t4, p4, d_off, d_lo,
                       d_tab, (int)G, (int)Gp, (int)Qp, P, (int)gchunk, perm_base, minp_stride, out);
  }
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
