// scoary_common.hpp -- shared by the translation units of libscoary_hip.so: the
// handle, error / timing helpers, layout constants and the Philox generator of
// spec S4 (scoary_labels.hip).  Everything here is internal; the contract is include/scoary_hip.h.
#ifndef SCOARY_COMMON_HPP
#define SCOARY_COMMON_HPP
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "scoary_hip.h"

struct scoary_ctx {
  int device = 0;
  int num_cu = 256;
  std::string err;
  bool timing = false;
  int lists_lds_optin = 0;   // k_permute_lists instances (by tile width) with the 160 KB LDS opt-in done
  int labels_lds_optin = 0;  // k_labels instances with it
  int mfma_lds_optin = 0;    // k_permute_mfma with it
  int cmh_exact_lds_optin = 0;   // k_cmh_exact with it
  int cmh_exact_odds_lds_optin = 0;   // k_cmh_odds_exact with it
  int ranksum_lds_optin = 0;   // bit 0: k_ranksum_labels, bit 1: k_permute_ranksum with it
  int cat_lds_optin = 0;   // bits 0 .. 3: k_cat_permute, k_cat_maxt, k_gcmh_permute, k_gcmh_maxt with it; 4 .. 7: S23's
  int mfma_route = SCOARY_MFMA_ROUTE_AUTO;  // scoary_set_mfma_route: which list slots take the matrix-core kernel
  int fisher_route = SCOARY_FISHER_ROUTE_AUTO;     // scoary_set_fisher_route: the kernels of scoary_fisher_lists_chained
  uint32_t* scipy_primes = nullptr;  // scoary_fisher_scipy's prime table and reciprocals (device,
  float* scipy_inv = nullptr;        // built on the handle's first call, freed by scoary_destroy)
  int scipy_nprimes = 0;
  struct Timed {
    std::string name;
    hipEvent_t start, stop;
  };
  std::vector<Timed> timed;
};

// scoary_mfma.hip: the matrix-core kernel of the slots [0, k_split) of a list launch (scoary_lists.hip calls it
// between the region conversion and the list kernel); geometry = stages of 64 permutations per trait, Q = T x
// stages of them in all, cut into `ranges` ranges of L (the last one shorter), 256-slot gene blocks, blocks in
// all, and the plan's model cost in stage-times of one CU
struct MfmaGeom {
  int64_t stages, Q, ranges, L, gene_blocks, blocks;
  double cost;
};
MfmaGeom scoary_mfma_geom(int num_cu, int64_t k_split, int64_t T, int64_t P, int64_t ntiles);
int scoary_mfma_launch(scoary_handle h, hipStream_t s, const uint32_t* d_tiles, const void* d_panels, void* d_bfrag,
                       const uint32_t* d_lcrit, uint16_t* d_partial, int64_t k_split, int64_t G, int64_t T,
                       int64_t N, int64_t P, int64_t ntiles, int64_t gs, bool bfrag_ready);

// scoary_cmh.hip: the strata plan as the segment table (CmhSegments, below) in d_scratch = scoary_cmh_scratch_bytes(N)
// bytes -- THE launch of k_cmh_segments, for scoary_cmh, scoary_cmh_minp_plan and scoary_cmh_exact.  `event`: the
// timing event the launch is recorded under, or nullptr when the caller's own event covers it
int scoary_cmh_segments_launch(scoary_handle h, hipStream_t s, const uint16_t* d_strata, const int32_t* d_members,
                               int64_t N, int64_t S, void* d_scratch, const char* event);

namespace {

constexpr int kWave = 64;
constexpr int kGeneAlign = 256;

// Row sizes (in quads of four 32-bit words) for which a row is held entirely in VGPRs: the gene row by
// k_permute_reg, a lane's label row by k_permute_minp / k_stepdown_minp.  THE list: the instances, the padding
// of tiled_quads() and every dispatcher follow from it.
// Longer rows go to k_permute_chunked (measured 1.39x faster than registers at N=5000).
using RegQuads = std::integer_sequence<int, 1, 2, 4, 6, 8, 12, 16, 20, 24>;
constexpr int kChunkQuads = 8;  // k_permute_chunked: quads per register chunk

// the smallest size of the list that is >= q; 0 when there is none
template <int... Q>
constexpr int quads_at_least(std::integer_sequence<int, Q...>, int64_t q) {
  int r = 0;
  ((r = (Q >= q && (r == 0 || Q < r)) ? Q : r), ...);
  return r;
}
template <int... Q>
constexpr int quads_max(std::integer_sequence<int, Q...>) {
  int r = 0;
  ((r = Q > r ? Q : r), ...);
  return r;
}
constexpr int kMaxRegQuads = quads_max(RegQuads{});

// f(std::integral_constant<int, Q>{}) for the size Q of the list that equals Qp; false when Qp is none of them
template <int... Q, class F>
inline bool with_quads(std::integer_sequence<int, Q...>, int64_t Qp, F&& f) {
  return ((Qp == Q && (f(std::integral_constant<int, Q>{}), true)) || ...);
}
template <class F>
inline bool with_reg_quads(int64_t Qp, F&& f) {
  return with_quads(RegQuads{}, Qp, f);
}

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

inline int64_t tiled_quads(int64_t N) {
  int64_t q = (((N + 31) / 32) + 3) / 4;
  if (q < 1) q = 1;
  const int r = quads_at_least(RegQuads{}, q);
  return r ? r : round_up(q, kChunkQuads);
}

// the row sizes tiled_quads() produces: a RegQuads size up to kMaxRegQuads quads, multiples of kChunkQuads beyond
inline bool tiled_quads_ok(int64_t Qp) {
  return Qp > kMaxRegQuads ? Qp % kChunkQuads == 0 : with_reg_quads(Qp, [](auto) {});
}

// ---- list-driven permutation path: layout constants shared by scoary_lists.hip
// (kernels) and scoary_listbuild.hip (device-side list builder) ----
// TW = tile row width in dwords (32 permutations each): 16 while a tile of 512
// permutations x (N+1) rows fits in LDS (N <= 2559), 8 (tiles of 256) up to
// N <= 5119, 4 (tiles of 128) up to N <= 10239, 2 (tiles of 64, two words per lane)
// beyond.  A gene takes max(TW/4, 1) lanes and a wavefront 64 / that many genes of
// similar list length.  A two-dword tile fits LDS whole up to N = 20479; wider matrices
// (N <= 131070) cut the isolates into SEGMENTS of kSegRows rows: a block loads one segment
// of its tile at a time and a gene's list is one sub-list per segment (k_permute_seglists;
// the counter planes live across the reloads).  (Round 3 first did this with one-dword
// tiles, 32 permutations per lane: 2.1x slower per listed row, tools/sweep_isolates.py.)
constexpr int kSegRows = 20352;                      // 159 * 128: whole word quads; (rows + 1) * 8 B fit 160 KB
constexpr int kSegTW = 2;                            // dwords per row of a segmented tile
constexpr int kSegStride = ((kSegRows + 1) * kSegTW + 3) / 4 * 4;   // dwords from one segment of a tile to the next
constexpr int kSegPiece = 8;                         // 16-bit entries per lane and index vector (16 bytes) of a segmented sub-list
constexpr int kMaxListIsolates = 131070;             // N / 2 < 2^16: sixteen counter planes; at most 7 segments
__host__ __device__ constexpr int list_segments(int64_t N) {
  return N <= 20479 ? 1 : (N <= kMaxListIsolates ? (int)((N + kSegRows - 1) / kSegRows) : 0);
}
__host__ __device__ constexpr int list_tw(int64_t N) {
  return N <= 2559 ? 16 : (N <= 5119 ? 8 : (N <= 10239 ? 4 : (list_segments(N) ? 2 : 0)));
}
__host__ __device__ constexpr int list_lpg(int TW) { return TW >= 4 ? TW / 4 : 1; }   // lanes per gene
__host__ __device__ constexpr int list_nw(int TW) { return TW >= 4 ? 4 : TW; }        // words per lane
// dwords per label tile in HBM: rows 0..N plus padding to a 16-byte multiple
__host__ __device__ constexpr int64_t list_tile_dwords(int64_t N, int TW) {
  return ((N + 1) * TW + 3) / 4 * 4;
}
// the same for any N the list path takes; segmented tiles (N > 20479): kSegStride dwords per
// segment, each with its own all-zero row after its last isolate
__host__ __device__ constexpr int64_t list_tile_dwords_seg(int64_t N, int TW) {
  return list_segments(N) > 1 ? (int64_t)list_segments(N) * kSegStride : list_tile_dwords(N, TW);
}
// rows of segment s, and the first dword of row `row` inside a two-dword tile
__host__ __device__ constexpr int64_t list_seg_rows(int64_t N, int s) {
  return list_segments(N) > 1 ? (N - (int64_t)s * kSegRows < kSegRows ? N - (int64_t)s * kSegRows : kSegRows) : N;
}
__host__ __device__ constexpr int64_t list_row_dword(int64_t N, int64_t row) {
  return list_segments(N) > 1 ? row / kSegRows * kSegStride + row % kSegRows * kSegTW : row * kSegTW;
}

constexpr int kListPad = 16;        // list lengths are padded to a multiple of this many entries (half a 32-entry step)
constexpr int kListStartUnit = 32;  // d_lstart counts in units of this many entries (128 bytes)
constexpr int kListChunkMB = 2;     // MB of index lists per k_permute_lists block (an XCD's L2 is 4 MB)
constexpr int kListSlack = 256;     // zero entries after the last list (one wavefront index load)

int fail(scoary_handle h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

// the checks the entry points share; `what` names the entry point in the message
inline int check_args(scoary_handle h, const char* what, bool ok) {
  return ok ? SCOARY_OK : fail(h, SCOARY_ERR_ARG, std::string(what) + ": bad argument");
}
// the stratified entry points (S9 to S12): arguments, then the limits of the per-stratum tables
inline int strata_check(scoary_handle h, const char* what, bool ok, int64_t T, int64_t N, int64_t S) {
  if (int rc = check_args(h, what, ok && T >= 1 && N >= 1 && S >= 1)) return rc;
  if (T > 65535) return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": T > 65535");
  if (S > scoary_perm_max_strata())
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": more strata than scoary_perm_max_strata()");
  if (N > scoary_perm_strata_max_isolates())
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": more isolates than scoary_perm_strata_max_isolates()");
  return SCOARY_OK;
}

#define HIP_TRY(h, expr)                                                              \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail(h, SCOARY_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Sets the handle's device for the duration of a call and restores the
// caller's (torch's) current device afterwards.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

struct KernelTimer {
  scoary_handle h;
  hipStream_t s;
  hipEvent_t start = nullptr, stop = nullptr;
  KernelTimer(scoary_handle h_, hipStream_t s_, const char* name) : h(h_), s(s_) {   // no name: times nothing
    if (!name || !h->timing) return;
    if (hipEventCreate(&start) != hipSuccess || hipEventCreate(&stop) != hipSuccess) {
      start = stop = nullptr;
      return;
    }
    (void)hipEventRecord(start, s);
    h->timed.push_back({name, start, stop});
  }
  ~KernelTimer() {
    if (stop) (void)hipEventRecord(stop, s);
  }
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one 32x32->64 multiply per product (v_mad_u64_u32) instead of hi + lo
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0;
    const uint32_t h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
    // three-input xor = one v_bitop3_b32 (LUT 0x96); two v_xor_b32 otherwise
    const uint32_t n0 = __builtin_amdgcn_bitop3_b32(h1, c1, k0, 0x96), n2 = __builtin_amdgcn_bitop3_b32(h0, c3, k1, 0x96);
    c0 = n0;
    c1 = l1;
    c2 = n2;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// ---- the B operand of k_permute_mfma (scoary_mfma.hip): THE definition of its layout, for the two kernels that
// write it (k_mfma_bfrag from label tiles in HBM, the label generator from its rows in LDS) ----
typedef int v4i __attribute__((ext_vector_type(4)));
constexpr int kKSteps = 32;                       // K-steps of 64 isolates: N <= 2048
constexpr int kFragBytes = 1024;                  // one operand fragment: 64 lanes x 16 bytes (32 E2M1 values)
constexpr int kStageBytes = 2 * kKSteps * kFragBytes;   // B of (trait, 64 permutations): [K-step][column tile][lane]

// 8 presence bits -> 8 E2M1 nibbles (bit i -> nibble i = 0b0010 = 1.0): pairs of bits select a byte
// of the pool {0x00, 0x02, 0x20, 0x22} through v_perm_b32
__device__ __forceinline__ uint32_t fp4_of_bits8(uint32_t b) {
  uint32_t y = b | (b << 12);
  y = (y | (y << 6)) & 0x03030303u;
  return __builtin_amdgcn_perm(0u, 0x22200200u, y);
}
__device__ __forceinline__ v4i fp4_of_bits32(uint32_t w) {
  return v4i{(int)fp4_of_bits8(w & 0xffu), (int)fp4_of_bits8((w >> 8) & 0xffu),
             (int)fp4_of_bits8((w >> 16) & 0xffu), (int)fp4_of_bits8(w >> 24)};
}

// A 32 x 32 bit matrix held one row per lane by the 32 lanes of a wavefront half, transposed: bit c of lane i
// becomes bit i of lane c.  Five butterfly stages; stage s swaps the off-diagonal s x s blocks of every 2s x 2s
// block -- a lane takes its partner's word (lane ^ s, ds_swizzle) rotated by s towards the bits it gives away and
// keeps the bits of its own diagonal block.
__device__ __forceinline__ uint32_t bit_transpose32(uint32_t x) {
  const uint32_t lane = threadIdx.x;
#define SCOARY_TRANSPOSE_STAGE(S, M)                                                                     \
  {                                                                                                      \
    const uint32_t p = (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, ((S) << 10) | 0x1f);                \
    const bool up = lane & (S);                                                                          \
    const uint32_t r = __builtin_amdgcn_alignbit(p, p, up ? (S) : 32 - (S)), keep = up ? ~(M) : (M);     \
    x = (x & keep) | (r & ~keep);                                                                        \
  }
  SCOARY_TRANSPOSE_STAGE(16, 0x0000ffffu)
  SCOARY_TRANSPOSE_STAGE(8, 0x00ff00ffu)
  SCOARY_TRANSPOSE_STAGE(4, 0x0f0f0f0fu)
  SCOARY_TRANSPOSE_STAGE(2, 0x33333333u)
  SCOARY_TRANSPOSE_STAGE(1, 0x55555555u)
#undef SCOARY_TRANSPOSE_STAGE
  return x;
}

// Column tile j of stage s of trait t: bfrag[t][s][K-step k][j][lane] x 16 bytes, S stages per trait.  Lane l
// holds permutation 64 s + 32 j + (l & 31), isolates 64 k + 32 (l >> 5) .. + 31.  row_word(row) = the 32
// permutation bits of isolate `row` in this column tile (bit c = permutation 64 s + 32 j + c), zero for rows >= N:
// a wavefront takes 64 rows (lane = isolate) and each of its halves transposes its 32 x 32 bits.  Every one of the
// kKSteps K-steps is written, zeros included (k_permute_mfma masks columns, not rows).  Called by whole
// wavefronts, wavefront `wave` of the `nwaves` that share the work.
template <class RowWord>
__device__ __forceinline__ void mfma_bfrag_emit(v4i* __restrict__ bfrag, int S, int t, int s, int j, int wave,
                                                int nwaves, RowWord row_word) {
  const int lane = threadIdx.x & 63;
  v4i* out = bfrag + ((int64_t)t * S + s) * (kStageBytes / 16) + j * 64 + lane;
  for (int k = wave; k < kKSteps; k += nwaves) out[k * 128] = fp4_of_bits32(bit_transpose32(row_word(k * 64 + lane)));
}

struct CmhSegments {                 // the layout of scoary_cmh's d_scratch (k_cmh_segments)
  uint32_t count, pad[3];
  uint2 seg[1];                      // [count] = ((stratum << 16) | word, mask)
};

// acc += popcount(x) as ONE v_bcnt_u32_b32 (its second operand is the
// accumulator).  Opaque to the optimiser on purpose: left to itself LLVM
// reassociates the accumulate chain into short chains joined by v_add3_u32,
// ~15 % more VALU work in the permutation inner loop.
__device__ __forceinline__ void bcnt_acc(uint32_t& acc, uint32_t x) {
  asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(x));
}

// acc += popcount(a & b) over the four words of a quad: one accumulator, one dependent chain
__device__ __forceinline__ void and_popc(uint32_t& acc, const uint4 a, const uint4 b) {
  bcnt_acc(acc, a.x & b.x);
  bcnt_acc(acc, a.y & b.y);
  bcnt_acc(acc, a.z & b.z);
  bcnt_acc(acc, a.w & b.w);
}


// inclusive Hillis-Steele scan of s[0 .. THREADS) in place by a block of THREADS lanes, s[idx] = op(s[idx],
// s[idx - o]) for o = 1, 2, 4, ...: lane idx (a permutation of the lanes) has written s[idx] and reads the
// results after the return.  Elements without a left neighbour combine with T(0), so op(x, 0) = x must hold.
template <int THREADS, class T, class Op>
__device__ __forceinline__ void block_scan(T* s, int idx, Op op) {
  __syncthreads();
  for (int o = 1; o < THREADS; o <<= 1) {
    const T v = idx >= o ? s[idx - o] : T(0);
    __syncthreads();
    s[idx] = op(s[idx], v);
    __syncthreads();
  }
}

// exclusive prefix sum of off[0 .. M) in place, off[M] = total.  One block walks the array in tiles of
// 1024 with a running carry (once per trait group: 0.5 M entries are ~500 tiles).  Shared by the
// table plans of scoary_minp.hip (S7) and scoary_cmh.hip (S11): CSR offsets from the support sizes.
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

}  // namespace
#endif
