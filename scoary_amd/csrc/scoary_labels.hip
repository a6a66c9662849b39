// scoary_labels.hip -- a8: label permutations (PermuteGTC, scoary/methods.py:1371-1384),
// spec S4 of round 5: a sampler with NO dependence from one isolate to the next.
//
// Rounds 1-4 drew a permutation by sequential selection sampling: N dependent steps per
// permutation, a latency chain that every rank of a gene-sharded run repeated in full (the
// serial fraction of cfg4's strong split).  The law is the contract -- the
// reference's shuffle is unseeded -- so the bits were redefined (the
// CPU checker restates them independently):
//
//   round 0  every valid isolate is MARKED independently with probability q/256.  Thirty-two
//            permutations share eight Philox words per isolate and the 8-bit comparison runs
//            bit-sliced: lane = isolate, bit = permutation, one tile-row dword comes out of a
//            register -- no ballot, no v_writelane transposition;
//   counts   K = marks per permutation: bit-sliced per-lane counters, a butterfly over the
//            wavefront, one LDS atomic per wavefront and permutation;
//   fix-up   lane = permutation: |m - K| uniformly drawn positions are toggled (rejection on
//            non-candidates; Lemire rejection makes the position exactly uniform).  Conditional
//            on K the marked set is uniform among K-subsets, and adding / removing uniformly
//            chosen isolates keeps it uniform -- the result is exactly uniform under ideal
//            random words;
//   output   isolate-major LDS tiles (scoary_perm_generate_tiles), the same tiles together with the E2M1 B
//            fragments of k_permute_mfma (scoary_perm_generate_tiles_bfrag_range: a block's columns are one
//            stage of that kernel, or half of one) or permutation-major bit rows (scoary_perm_generate); the
//            last two through 32 ballots per 64 isolates.
//
// A block = (trait, NB dword columns of 32 permutations); its rows live in LDS until the fix-up is
// done: N * NB * 4 bytes (NB = 1 or 2 by how many blocks the launch has).  Beyond N = 40 000 a
// row keeps only 16 / 8 / ... 1 of the 32 permutations of a dword (more Philox work per label,
// still parallel in N).
//
// One generator, two fix-up drivers.  The block map (label_block), the LDS carve-up (lds_map), round 0
// (bern_word, store_row0), the fix-up pieces (fix_group, toggle4, toggle1, fix_rounds, fix_tail), the output
// (emit_labels) and the host side (launch_block behind launch_labels / launch_labels_strata, which pick the
// instance and carry each kernel's own limit; label_args, tile_shape) exist once.  What the two kernels
// own is how a permutation's surplus |m - K| is found and who places it:
//   k_labels         (spec S4) one plan per trait, K from bit-sliced counters kept during round 0, the fix-up
//                    over all N isolates; rows of fewer than 32 permutations per dword for large N;
//   k_labels_strata  (spec S9) a plan per (trait, stratum), K from a count over the stratum's members, the
//                    fix-up per stratum over its member list, the tails of L strata side by side.
#include "scoary_common.hpp"

namespace {

constexpr uint32_t kDomBernLo = 0x53434F42u;   // "SCOB": words R_0..R_3 of round 0
constexpr uint32_t kDomBernHi = 0x53434F43u;   // "SCOC": words R_4..R_7
constexpr uint32_t kDomFix = 0x53434F44u;      // "SCOD": fix-up position draws
constexpr uint32_t kFixMaxCalls = 1u << 20;    // safety stop of the fix-up loop (the CPU checker has the same bound)
constexpr int kCntPlanes = 10;                 // per-lane bit-sliced mark count: <= 1023 rows per thread
constexpr int kSumPlanes = 16;                 // per-wavefront sum: <= 64 * 1023
constexpr int kMaxRowsPerThread = (1 << kCntPlanes) - 1;
constexpr int kLabelsMaxLds = 160 * 1024;

struct LabelPlan {
  uint32_t m, q;     // marks to place; 8-bit round-0 probability
  bool flip;         // the complement is emitted (npos > nval / 2)
};
__device__ __forceinline__ uint32_t isqrt64(uint64_t v) {
  uint64_t r = 0;
  for (int s = 31; s >= 0; --s) {
    const uint64_t c = r | ((uint64_t)1 << s);
    if (c * c <= v) r = c;
  }
  return (uint32_t)r;
}
// the plan of spec S4 -- wave-uniform integer arithmetic, the same in the CPU checker
__device__ __forceinline__ LabelPlan label_plan(int32_t npos_i, int32_t nval_i) {
  const int64_t npos = npos_i, nval = nval_i;
  LabelPlan p;
  p.flip = 2 * npos > nval;
  const int64_t m = p.flip ? nval - npos : npos;
  p.m = m > 0 ? (uint32_t)m : 0u;
  p.q = 0u;
  if (m > 0 && nval > 0) {
    const uint64_t s = isqrt64((uint64_t)m * (uint64_t)(nval - m) / (uint64_t)nval);
    const uint64_t b = 12u * s * (uint64_t)(nval - 2 * m) / (5u * (uint64_t)nval);
    const uint64_t target = (uint64_t)m > b ? (uint64_t)m - b : 0u;
    p.q = (uint32_t)(256u * target / (uint64_t)nval);
  }
  return p;
}

// Round 0: the marks of isolate i in the 32 permutations of block B (bit b = permutation 32 B + b).
// fold_j (q_j ? x | R_j : x & R_j) from x = 0: leading zero bits of q keep x = 0, so the first
// Philox call is skipped when q's low nibble is zero.
__device__ __forceinline__ uint32_t bern_word(uint32_t i, uint32_t B, uint32_t t, uint32_t q,
                                              uint32_t k0, uint32_t k1) {
  uint32_t x = 0u, r[4];
  if (q == 0u) return 0u;
  if (q & 0xFu) {
    philox4x32_10(i, B, t, kDomBernLo, k0, k1, r);
#pragma unroll
    for (int j = 0; j < 4; ++j) x = ((q >> j) & 1u) ? (x | r[j]) : (x & r[j]);
  }
  philox4x32_10(i, B, t, kDomBernHi, k0, k1, r);
#pragma unroll
  for (int j = 0; j < 4; ++j) x = ((q >> (4 + j)) & 1u) ? (x | r[j]) : (x & r[j]);
  return x;
}

struct LabelArgs {
  const uint32_t* masks;     // vecrows [T][Wp]
  const int32_t* margins;    // [T][2] = (npos, nval)
  int N, Wp;
  int64_t P, perm_base;
  int trait_base;
  uint32_t k0, k1;
  int elt_log2;              // log2 of the permutations of a dword column one block keeps (5: all 32)
  // tiles
  int ntiles, TW;
  int64_t first_flat, nflat; // flat (trait, tile) range of this launch
  uint32_t* out;
  v4i* bfrag;                // tiles + fragments: [trait][stage][K-step][column tile][lane], mfma_bfrag_emit
};

// What a block produces: (trait, NB dword columns of 32 permutations), or with sub-dword rows the bits
// [bit0, bit0 + elt) of one column
template <int NB>
struct LabelBlock {
  int t, bit0;
  uint32_t Bglob;            // Philox block of column 0
  uint32_t* tile_base;       // tiles: row 0, column `col` of the block's tile
  int stage, jcol;           // tiles + fragments: column w is column tile jcol + w of this stage (< 0: none to write)
  uint32_t live[NB];         // permutations of column w that exist, as a mask over the 32 bits of the Philox block
};
// The block map of both kernels.  SUB: rows may keep fewer than 32 permutations of a dword (a.elt_log2 < 5;
// only k_labels has such rows).  false: the block has nothing to do (the padding of a tile launch)
template <int NB, int OUT, bool SUB>
__device__ __forceinline__ bool label_block(const LabelArgs& a, LabelBlock<NB>& b) {
  const int elt_log2 = SUB ? a.elt_log2 : 5;
  const int elt = 1 << elt_log2;                     // permutation bits a row keeps per column
  const int subs = 32 >> elt_log2;                   // blocks that share one dword column
  int64_t lc0 = 0;                                   // tiles: dword column among this launch's permutations
  b.tile_base = nullptr;
  b.stage = -1, b.jcol = 0;
  if constexpr (OUT != 1) {
    // block id -> (flat tile, unit): the units of one tile get ids that are equal mod 8, i.e. run
    // on one XCD (observed placement: block b on XCD b % 8), so the 4 * NB-byte pieces they
    // write into the same tile rows meet in one L2 and leave it as whole lines
    const int units = a.TW * subs / NB;
    const int64_t id = blockIdx.x;
    const int64_t qd = id >> 3;
    const int unit = (int)(qd % units);
    const int64_t fl = (qd / units) * 8 + (id & 7);
    if (fl >= a.nflat) return false;
    const int64_t f = a.first_flat + fl;
    b.t = (int)(f / a.ntiles);
    const int tile = (int)(f % a.ntiles);
    const int col = unit / subs * NB;
    b.bit0 = (unit % subs) * elt;
    lc0 = (int64_t)tile * a.TW + col;
    b.Bglob = (uint32_t)((a.perm_base >> 5) + lc0);
    // (more than one segment means N > 20479, hence TW == kSegTW; below that this is list_tile_dwords)
    b.tile_base = a.out + f * list_tile_dwords_seg(a.N, a.TW) + col;
    if constexpr (OUT == 2) {
      // sixteen-dword tiles of whole dwords (the entry point checks): a stage of 64 permutations is two columns,
      // and the buffer ends at the last stage that holds a permutation
      const int stage = tile * 8 + (col >> 1);
      if ((int64_t)stage * 64 < a.P) b.stage = stage, b.jcol = col & 1;
    }
  } else {
    b.t = blockIdx.y;
    b.Bglob = (uint32_t)((a.perm_base >> 5) + blockIdx.x / subs);
    b.bit0 = (int)(blockIdx.x % subs) * elt;
  }
#pragma unroll
  for (int w = 0; w < NB; ++w) {
    int64_t lo, hi;                                  // bits [lo, hi) of the block exist
    if constexpr (OUT != 1) {
      lo = 0;
      hi = a.P - (lc0 + w) * 32;
    } else {
      const int64_t first = (int64_t)(b.Bglob + w) * 32;
      lo = a.perm_base - first;
      hi = a.perm_base + a.P - first;
    }
    lo = lo < 0 ? 0 : (lo > 32 ? 32 : lo);
    hi = hi < 0 ? 0 : (hi > 32 ? 32 : hi);
    const uint32_t below_hi = hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u);
    const uint32_t below_lo = lo >= 32 ? 0xffffffffu : ((1u << lo) - 1u);
    b.live[w] = hi > lo ? (below_hi & ~below_lo) : 0u;
  }
  return true;
}

// The LDS of a block as dword offsets, read by the kernel and by the host code that sizes its launch: the rows
// xs at 0 (stride_bits per isolate), the validity words vm, then what the kernel keeps besides (own).
// I: int64_t on the host, which sizes the launch for any N a caller may pass; int in the kernels, where a
// launch that fits kLabelsMaxLds keeps N * stride_bits below 2^21
template <class I>
struct LdsMap {
  I vm, own, end;
  __host__ __device__ I bytes() const { return end * 4; }
};
template <class I>
__host__ __device__ inline LdsMap<I> lds_map(I N, int stride_bits, I own_dwords) {
  LdsMap<I> m;
  m.vm = (((N * stride_bits + 31) >> 5) + 3) & ~(I)3;
  m.own = m.vm + ((((N + 31) >> 5) + 3) & ~(I)3);
  m.end = m.own + own_dwords;
  return m;
}
// k_labels keeps the mark counts of its 32 * NB permutations; k_labels_strata the stratum table (16 bytes each)
// and the 16-bit member list
template <class I>
__host__ __device__ inline LdsMap<I> labels_lds(I N, int elt, int NB) { return lds_map<I>(N, elt * NB, 32 * NB); }
template <class I>
__host__ __device__ inline LdsMap<I> strata_lds(I N, int NB, I S) {
  return lds_map<I>(N, 32 * NB, 4 * S + (N + 1) / 2);
}

// Round 0 leaves the marks of isolate `row` in xs: whole dwords, or (sub-dword rows, xs zeroed) OR-ed into place
template <int NB>
__device__ __forceinline__ void store_row0(uint32_t* xs, int row, const uint32_t (&x)[NB], int elt_log2) {
  if (elt_log2 == 5) {
    if constexpr (NB == 2) {
      *reinterpret_cast<uint2*>(xs + (int64_t)row * 2) = make_uint2(x[0], x[1]);
    } else {
      xs[row] = x[0];
    }
  } else if (x[0]) {
    const uint32_t bp = (uint32_t)row << elt_log2;
    atomicOr(&xs[bp >> 5], x[0] << (bp & 31u));
  }
}

// ---- the fix-up: a group of L lanes per permutation ----
// The spec consumes the position draws c = 0, 1, 2, ... of a permutation one after the other; but as long as at
// least as many marks are missing as a batch has draws, EVERY distinct candidate the batch hits is toggled,
// whatever the order -- so lane l of the group takes Philox call base + l (four draws) and the group toggles
// with LDS atomics (the returned old bit says who was first at a position).  A round uses k = min(L, |d| / 4)
// calls, so it can never overshoot; the last < 4 marks are placed by ONE lane, draw by draw (fix_tail).
// A draw is a position in [0, n), exactly uniform by Lemire rejection (reject_below = 2^32 mod n); iso(position)
// is the isolate there, and its bit of this permutation is bit bp = isolate * stride_bits + pidx of xs.
struct FixGroup {
  uint32_t* xs;              // the rows
  const uint32_t* vm;        // the validity words
  uint32_t stride_bits;      // bits of xs per isolate = permutations of the block
  int L, l, pidx;            // lanes per permutation (a power of two), this lane among them, their permutation
  bool in_group, alive;      // tpb > 64 * nperm: the last wavefronts idle; alive: the permutation exists
  uint32_t pi;               // the permutation's global index (Philox counter word 1)
  uint64_t gmask;            // the group's lanes within the wavefront
  uint32_t tglob, k0, k1;    // Philox counter word 2 and key
};
template <int NB>
__device__ __forceinline__ FixGroup fix_group(const LabelArgs& a, const LabelBlock<NB>& b, uint32_t* xs,
                                              const uint32_t* vm, int nperm) {
  const int tid = threadIdx.x, lane = tid & 63;
  FixGroup g;
  g.xs = xs, g.vm = vm, g.stride_bits = (uint32_t)nperm;
  g.L = min(kWave, (int)blockDim.x / nperm);
  g.pidx = tid / g.L, g.l = tid & (g.L - 1);
  g.in_group = g.pidx < nperm;
  const int w = g.pidx >> 5, j = g.pidx & 31;
  g.alive = g.in_group && ((((w & (NB - 1)) ? b.live[NB - 1] : b.live[0]) >> (b.bit0 + j)) & 1u);
  g.pi = (b.Bglob + (uint32_t)w) * 32u + (uint32_t)(b.bit0 + j);
  g.gmask = (g.L == 64 ? ~(uint64_t)0 : (((uint64_t)1 << g.L) - 1)) << (lane & ~(g.L - 1));
  g.tglob = (uint32_t)(a.trait_base + b.t), g.k0 = a.k0, g.k1 = a.k1;
  return g;
}
// Four draws of one Philox call: positions, then the toggles as LDS atomics -- an OR on a marked isolate / an
// AND on an unmarked one changes nothing, so only invalid isolates have to be kept away (add mode), and the
// returned old word says whether THIS lane changed the bit.  The four atomics are independent: issued back to
// back, one wait.  Returns how many bits this lane changed.
template <class Iso>
__device__ __forceinline__ int toggle4(const FixGroup& g, const uint32_t (&rnd)[4], bool add, uint32_t n,
                                       uint32_t reject_below, Iso iso) {
  uint32_t idx[4], bit[4];
  bool ok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint64_t prod = (uint64_t)rnd[u] * (uint64_t)n;
    const uint32_t pos = iso((uint32_t)(prod >> 32));
    const uint32_t bp = pos * g.stride_bits + (uint32_t)g.pidx;
    idx[u] = bp >> 5;
    bit[u] = 1u << (bp & 31u);
    ok[u] = (uint32_t)prod >= reject_below;            // Lemire rejection: no draw otherwise
    if (add) ok[u] = ok[u] && ((g.vm[pos >> 5] >> (pos & 31u)) & 1u);
  }
  uint32_t old[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    old[u] = add ? bit[u] : 0u;                        // "no change" for the draws that are none
    if (ok[u])
      old[u] = add ? __hip_atomic_fetch_or(&g.xs[idx[u]], bit[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                   : __hip_atomic_fetch_and(&g.xs[idx[u]], ~bit[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  int won = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) won += add ? ((old[u] & bit[u]) ? 0 : 1) : ((old[u] & bit[u]) ? 1 : 0);
  return won;
}
// one draw at a time (the last < 4 marks): returns 1 if the bit changed
template <class Iso>
__device__ __forceinline__ int toggle1(const FixGroup& g, uint32_t rnd, bool add, uint32_t n, uint32_t reject_below,
                                       Iso iso) {
  const uint64_t prod = (uint64_t)rnd * (uint64_t)n;
  if ((uint32_t)prod < reject_below) return 0;
  const uint32_t pos = iso((uint32_t)(prod >> 32));
  const uint32_t bp = pos * g.stride_bits + (uint32_t)g.pidx, b1 = 1u << (bp & 31u);
  if (add) {
    if (!((g.vm[pos >> 5] >> (pos & 31u)) & 1u)) return 0;
    return (__hip_atomic_fetch_or(&g.xs[bp >> 5], b1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & b1) ? 0 : 1;
  }
  return (__hip_atomic_fetch_and(&g.xs[bp >> 5], ~b1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & b1) ? 1 : 0;
}
// The batched rounds, group-uniform, while |d| >= 4 (d > 0: marks to add, < 0: to remove); `base` is the next
// Philox call, `ctr_hi` what is OR-ed into the call counter (the stratum, from bit 20).  The safety stop
// kFixMaxCalls ends the loop; CLAMP also keeps a round's calls below it, which the stratified kernel needs
// because the stratum sits right above (the stop is unreachable on consistent input).
template <bool CLAMP, class Iso>
__device__ __forceinline__ void fix_rounds(const FixGroup& g, int& d, uint32_t& base, uint32_t ctr_hi, uint32_t n,
                                           uint32_t reject_below, Iso iso) {
  while ((d >= 4 || d <= -4) && base < kFixMaxCalls) {
    const bool add = d > 0;
    const int need = add ? d : -d;
    int k = min(g.L, need >> 2);
    if constexpr (CLAMP) k = min(k, (int)(kFixMaxCalls - base));
    uint32_t r[4];
    int won = 0;
    if (g.l < k) {
      philox4x32_10(ctr_hi | (base + (uint32_t)g.l), g.pi, g.tglob, kDomFix, g.k0, g.k1, r);
      won = toggle4(g, r, add, n, reject_below, iso);
    }
    // marks toggled by the group in this round
    int got = 0;
#pragma unroll
    for (int bitn = 0; bitn < 3; ++bitn) got += __popcll(__ballot((won >> bitn) & 1) & g.gmask) << bitn;
    d = add ? d - got : d + got;
    base += (uint32_t)k;
  }
}
// The last |d| < 4 marks, in draw order: the work of one lane (the caller says which)
template <class Iso>
__device__ __forceinline__ void fix_tail(const FixGroup& g, int d, uint32_t base, uint32_t ctr_hi, uint32_t n,
                                         uint32_t reject_below, Iso iso) {
  const bool add = d > 0;
  int left = add ? d : -d;
  while (left > 0 && base < kFixMaxCalls) {
    uint32_t r[4];
    philox4x32_10(ctr_hi | base, g.pi, g.tglob, kDomFix, g.k0, g.k1, r);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (left > 0) left -= toggle1(g, r[u], add, n, reject_below, iso);
    ++base;
  }
}

// Output of a block whose rows are final: row_field(row, w) = the labels of isolate `row`, column w
template <int NB, int OUT, class RowField>
__device__ __forceinline__ void emit_labels(const LabelArgs& a, const LabelBlock<NB>& b, RowField row_field) {
  const int tid = threadIdx.x, lane = tid & 63, tpb = blockDim.x, nwaves = tpb >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = a.N, elt = OUT == 2 ? 32 : 1 << a.elt_log2, bit0 = b.bit0;
  uint32_t* tile_base = b.tile_base;
  if constexpr (OUT != 1) {
    const bool seg = a.TW == kSegTW;                  // two-dword tiles: segmented above N = 20479
    auto row_off = [&](int64_t row) -> int64_t { return seg ? list_row_dword(N, row) : row * a.TW; };
    if (elt == 32) {
      for (int row = tid; row < N; row += tpb) {
        uint32_t* dst = tile_base + row_off(row);
        if constexpr (NB == 2) {
          *reinterpret_cast<uint2*>(dst) = make_uint2(row_field(row, 0), row_field(row, 1));
        } else {
          dst[0] = row_field(row, 0);
        }
      }
    } else {                                          // 16 / 8 permutations of the dword: narrow stores
      for (int row = tid; row < N; row += tpb) {
        uint8_t* dst = reinterpret_cast<uint8_t*>(tile_base + row_off(row)) + (bit0 >> 3);
        const uint32_t f = row_field(row, 0);
        if (elt == 16) *reinterpret_cast<uint16_t*>(dst) = (uint16_t)f;
        else *dst = (uint8_t)f;
      }
    }
    // the all-zero row(s) list padding points at: one per segment
    const int nseg = seg ? list_segments(N) : 1;
    if (tid < nseg) {
      const int64_t z = nseg > 1 ? (int64_t)tid * kSegStride + list_seg_rows(N, tid) * kSegTW : row_off(N);
      if (elt == 32) {
#pragma unroll
        for (int w = 0; w < NB; ++w) tile_base[z + w] = 0u;
      } else {
        uint8_t* dst = reinterpret_cast<uint8_t*>(tile_base + z) + (bit0 >> 3);
        if (elt == 16) *reinterpret_cast<uint16_t*>(dst) = 0;
        else *dst = 0;
      }
    }
    if constexpr (OUT == 2) {
      // the same bits once more as the stage's B fragments: the K-steps go round the wavefronts of the block
      if (b.stage >= 0) {
#pragma unroll
        for (int w = 0; w < NB; ++w)
          mfma_bfrag_emit(a.bfrag, (int)((a.P + 63) >> 6), b.t, b.stage, b.jcol + w, wave, nwaves,
                          [&](int row) { return row < N ? row_field(row, w) : 0u; });
      }
    }
  } else {
    static_assert(OUT != 1 || NB == 1, "bit rows: one dword column per block");
    // permutation-major rows: 64 isolates per wavefront step, one ballot per permutation
    const int nchunks = (N + 63) >> 6;
    const int64_t pl = (int64_t)b.Bglob * 32 + bit0 + lane - a.perm_base;   // lane < elt: its permutation
    const bool mine = lane < elt && ((b.live[0] >> (bit0 + (lane & 31))) & 1u);
    uint32_t* prow = a.out + ((int64_t)b.t * a.P + (mine ? pl : 0)) * a.Wp;
    for (int c = wave; c < nchunks; c += nwaves) {
      const int row = c * 64 + lane;
      const uint32_t f = row < N ? row_field(row, 0) : 0u;
      uint32_t lo = 0u, hi = 0u;
      for (int j = 0; j < elt; ++j) {
        const uint64_t m64 = __ballot((f >> j) & 1u);
        if (lane == j) {
          lo = (uint32_t)m64;
          hi = (uint32_t)(m64 >> 32);
        }
      }
      if (mine) *reinterpret_cast<uint2*>(prow + 2 * c) = make_uint2(lo, hi);
    }
    if (mine)
      for (int k = 2 * nchunks + wave; k < a.Wp; k += nwaves) prow[k] = 0u;
  }
}

// tiles + fragments: a block none of whose permutations exists (the columns of the last tile beyond P) has zero
// rows to write, and zero fragments where its stage still holds permutations -- nothing to draw
template <int NB, int OUT>
__device__ __forceinline__ bool emit_dead_block(const LabelArgs& a, const LabelBlock<NB>& b) {
  if constexpr (OUT == 2) {
    uint32_t any = 0u;
#pragma unroll
    for (int w = 0; w < NB; ++w) any |= b.live[w];
    if (any == 0u) {
      emit_labels<NB, OUT>(a, b, [](int, int) { return 0u; });
      return true;
    }
  }
  return false;
}

// NB dword columns per block (NB > 1 only with all 32 permutations per dword); OUT 0: tiles, 1: rows, 2: tiles and
// the B fragments of k_permute_mfma
template <int NB, int OUT>   // NB = 1, 2
__global__ __launch_bounds__(1024) void k_labels(const LabelArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int tid = threadIdx.x, lane = tid & 63, tpb = blockDim.x;
  const int N = a.N;
  constexpr bool SUB = OUT != 2;                    // rows of fewer than 32 permutations: never with fragments
  const int elt_log2 = SUB ? a.elt_log2 : 5;
  const int elt = 1 << elt_log2;                    // permutation bits a row keeps per column
  LabelBlock<NB> blk;
  if (!label_block<NB, OUT, SUB>(a, blk)) return;
  if (emit_dead_block<NB, OUT>(a, blk)) return;
  const int t = blk.t, bit0 = blk.bit0;
  const uint32_t Bglob = blk.Bglob;
  const uint32_t (&live)[NB] = blk.live;
  const uint32_t fieldmask = elt == 32 ? 0xffffffffu : ((1u << elt) - 1u);
  const uint32_t tglob = (uint32_t)(a.trait_base + t);
  const LabelPlan plan = label_plan(__builtin_amdgcn_readfirstlane(a.margins[2 * t]),
                                    __builtin_amdgcn_readfirstlane(a.margins[2 * t + 1]));
  const uint32_t* mrow = a.masks + (int64_t)t * a.Wp;

  // ---- LDS: rows (elt * NB bits per isolate), validity words, mark counts ----
  const LdsMap<int> lm = labels_lds(N, elt, NB);
  uint32_t* xs = lds;
  uint32_t* vm = lds + lm.vm;
  int* kc = reinterpret_cast<int*>(lds + lm.own);
  const int nmw = (N + 31) >> 5;
  for (int k = tid; k < nmw; k += tpb) vm[k] = mrow[k];
  if (tid < 32 * NB) kc[tid] = 0;
  if (elt != 32) {                                   // sub-dword rows are OR-ed into place
    for (int k = tid; k < lm.vm; k += tpb) xs[k] = 0u;   // (with the up to 3 dwords of padding before vm)
    __syncthreads();
  }

  // ---- round 0: lane = isolate ----
  uint32_t cp[NB][kCntPlanes];
#pragma unroll
  for (int w = 0; w < NB; ++w)
#pragma unroll
    for (int k = 0; k < kCntPlanes; ++k) cp[w][k] = 0u;
  const int rows_per_thread = (N + tpb - 1) / tpb;
  const int kpl = 32 - __builtin_clz((unsigned)rows_per_thread | 1u);   // planes a lane's count needs
  for (int row = tid; row < N; row += tpb) {
    const bool valid = (mrow[row >> 5] >> (row & 31)) & 1u;
    uint32_t x[NB];
#pragma unroll
    for (int w = 0; w < NB; ++w) {
      x[w] = 0u;
      if (valid)
        x[w] = ((bern_word((uint32_t)row, Bglob + (uint32_t)w, tglob, plan.q, a.k0, a.k1) & live[w]) >> bit0) &
               fieldmask;
      uint32_t carry = x[w];
#pragma unroll
      for (int k = 0; k < kCntPlanes; ++k)
        if (k < kpl) {
          const uint32_t nc = cp[w][k] & carry;
          cp[w][k] ^= carry;
          carry = nc;
        }
    }
    store_row0<NB>(xs, row, x, elt_log2);
  }
  // ---- marks per permutation: butterfly over the wavefront, then one LDS atomic per wavefront ----
#pragma unroll
  for (int w = 0; w < NB; ++w) {
    uint32_t c[kSumPlanes];
#pragma unroll
    for (int k = 0; k < kSumPlanes; ++k) c[k] = k < kCntPlanes ? cp[w][k] : 0u;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      uint32_t carry = 0u;
#pragma unroll
      for (int k = 0; k < kSumPlanes; ++k)
        if (k < kpl + s + 1) {
          const uint32_t y = (uint32_t)__shfl_xor((int)c[k], 1 << s);
          const uint32_t sum = c[k] ^ y ^ carry;
          carry = (c[k] & y) | (carry & (c[k] | y));
          c[k] = sum;
        }
    }
    if (lane < 32) {
      int K = 0;
#pragma unroll
      for (int k = 0; k < kSumPlanes; ++k) K |= (int)((c[k] >> lane) & 1u) << k;
      // the atomics wait for the barrier below: kc was zeroed by other threads
      cp[w][0] = (uint32_t)K;
    }
  }
  __syncthreads();
  if (lane < 32) {
#pragma unroll
    for (int w = 0; w < NB; ++w)
      if (cp[w][0]) atomicAdd(&kc[w * 32 + lane], (int)cp[w][0]);
  }
  __syncthreads();

  // ---- fix-up over all N isolates: the batched rounds, then the group's first lane places the last marks ----
  {
    const FixGroup g = fix_group<NB>(a, blk, xs, vm, elt * NB);
    int d = g.alive ? (int)plan.m - kc[g.in_group ? g.pidx : 0] : 0;   // > 0: add marks, < 0: remove
    const uint32_t reject_below = (uint32_t)(((uint64_t)1 << 32) % (uint64_t)N);
    const auto isolate = [](uint32_t pos) { return pos; };
    uint32_t base = 0;                                   // next Philox call of this permutation
    fix_rounds<false>(g, d, base, 0u, (uint32_t)N, reject_below, isolate);
    if (g.l == 0) fix_tail(g, d, base, 0u, (uint32_t)N, reject_below, isolate);
  }
  __syncthreads();

  // ---- output ----
  // the labels of row `row`, column w: marks, or their complement among the valid isolates
  auto row_field = [&](int row, int w) -> uint32_t {
    uint32_t f;
    if (elt == 32) {
      f = xs[(int64_t)row * NB + w];
    } else {
      const uint32_t bp = (uint32_t)row << elt_log2;
      f = (xs[bp >> 5] >> (bp & 31u)) & fieldmask;
    }
    if (plan.flip) {
      const bool valid = (vm[row >> 5] >> (row & 31)) & 1u;
      f = valid ? (~f & (live[w] >> bit0) & fieldmask) : 0u;
    }
    return f;
  };
  emit_labels<NB, OUT>(a, blk, row_field);
}

// ---- spec S9: labels shuffled within strata ------------------------------------------------------
// Restricted exchangeability: every stratum s (isolates mem_s[0..n_s), any partition of the isolates the caller
// supplies) keeps its own npos_ts positives, placed uniformly on its nval_ts valid members; the strata are
// independent.  The plan (m, flip, q) is S4's per (trait, stratum), round 0 is S4's bern_word with the
// stratum's q, and the fix-up runs per (permutation, stratum) over the stratum's members with the stratum in
// the Philox counter -- with one stratum this is S4 bit for bit.
constexpr int kMaxStrata = 1024;                // the per-stratum table of a block: 16 bytes each in LDS
constexpr int kStrataMaxIsolates = 20479;       // unsegmented tiles; members are 16-bit in LDS

struct StrataArgs {
  const uint16_t* strata;    // [N] stratum of every isolate
  const int32_t* members;    // [N] isolates by (stratum, index)
  const int32_t* offsets;    // [S + 1] first member of every stratum; offsets[S] = N
  const int32_t* smargins;   // [T][S][2] = (npos_ts, nval_ts)
  int S;
};

// NB dword columns of 32 permutations per block; OUT as for k_labels.  The block shape of k_labels.
template <int NB, int OUT>   // NB = 1, 2
__global__ __launch_bounds__(1024) void k_labels_strata(const LabelArgs a, const StrataArgs sa) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int tid = threadIdx.x, tpb = blockDim.x;
  const int N = a.N, S = sa.S;
  LabelBlock<NB> blk;
  if (!label_block<NB, OUT, false>(a, blk)) return;
  if (emit_dead_block<NB, OUT>(a, blk)) return;
  const int t = blk.t;
  const uint32_t Bglob = blk.Bglob;
  const uint32_t (&live)[NB] = blk.live;
  const uint32_t tglob = (uint32_t)(a.trait_base + t);
  const uint32_t* mrow = a.masks + (int64_t)t * a.Wp;

  // ---- LDS: rows (NB dwords per isolate), validity words, the stratum table, the members ----
  const LdsMap<int> lm = strata_lds(N, NB, S);
  const int nmw = (N + 31) >> 5;
  uint32_t* xs = lds;
  uint32_t* vm = lds + lm.vm;
  uint4* tab = reinterpret_cast<uint4*>(lds + lm.own);    // (m, n_s, 2^32 mod n_s, offset | q << 16 | flip << 24)
  uint16_t* mem = reinterpret_cast<uint16_t*>(tab + S);
  for (int k = tid; k < nmw; k += tpb) vm[k] = mrow[k];
  for (int s = tid; s < S; s += tpb) {
    // (a table that does not partition [0, N) is refused on the host; the clamps keep every index inside)
    const int off = min(max(sa.offsets[s], 0), N);
    const int n = min(max(sa.offsets[s + 1] - off, 0), N - off);
    const int32_t* mg = sa.smargins + ((int64_t)t * S + s) * 2;
    const LabelPlan plan = label_plan(mg[0], mg[1]);
    const uint32_t rej = n > 0 ? (0u - (uint32_t)n) % (uint32_t)n : 0u;        // 2^32 mod n_s
    tab[s] = make_uint4(plan.m, (uint32_t)n, rej, (uint32_t)off | (plan.q << 16) | ((plan.flip ? 1u : 0u) << 24));
  }
  for (int k = tid; k < N; k += tpb) mem[k] = (uint16_t)min(max(sa.members[k], 0), N - 1);
  __syncthreads();
  auto stratum_of = [&](int row) -> uint32_t { return tab[min((int)sa.strata[row], S - 1)].w; };

  // ---- round 0: lane = isolate, q by the isolate's stratum ----
  for (int row = tid; row < N; row += tpb) {
    const bool valid = (vm[row >> 5] >> (row & 31)) & 1u;
    uint32_t x[NB];
#pragma unroll
    for (int w = 0; w < NB; ++w) x[w] = 0u;
    if (valid) {
      const uint32_t q = (stratum_of(row) >> 16) & 0xffu;
#pragma unroll
      for (int w = 0; w < NB; ++w)
        x[w] = bern_word((uint32_t)row, Bglob + (uint32_t)w, tglob, q, a.k0, a.k1) & live[w];
    }
    store_row0<NB>(xs, row, x, 5);
  }
  __syncthreads();

  // ---- fix-up: the group of L lanes of a permutation walks the strata ----
  // Per stratum: K = the permutation's marks among the members (marks sit on valid isolates only), then the
  // batched rounds against mem_s.  The last < 4 marks have to go draw by draw -- one lane's work -- but strata
  // are independent (their members are disjoint), so the group walks L strata, leaves the
  // tail of stratum s0 + l to lane l, and the L tails run side by side: at eight isolates per stratum nearly
  // every stratum is all tail, and one active lane per group would cost a Philox call per stratum and wavefront.
  // The loops over the strata are uniform for the block, the batched rounds for the group.
  {
    const FixGroup g = fix_group<NB>(a, blk, xs, vm, 32 * NB);
    const int L = g.L, l = g.l, j = g.pidx & 31;
    const uint32_t* xw = xs + (g.pidx >> 5);             // the permutation's dword column of the rows
    // position -> isolate of the stratum whose members start at `off`
    const auto member_at = [mem](uint32_t off) {
      return [mem, off](uint32_t pos) -> uint32_t { return mem[off + pos]; };
    };
    for (int s0 = 0; s0 < S; s0 += L) {
      int my_d = 0;                                      // stratum s0 + l: marks its tail has to add (> 0) / remove
      uint32_t my_base = 0;                              // ... and its next Philox call
      const int s1 = min(S, s0 + L);
      for (int s = s0; s < s1; ++s) {
        const uint4 e = tab[s];
        const uint32_t n = e.y, off = e.w & 0xffffu;
        if (n == 0u) continue;
        int K = 0;
        if (g.alive)                                     // bit bp = member * 32 * NB + pidx, by dword and bit
          for (uint32_t k = (uint32_t)l; k < n; k += (uint32_t)L) K += (xw[(uint32_t)mem[off + k] * NB] >> j) & 1u;
        for (int o = 1; o < L; o <<= 1) K += __shfl_xor(K, o);
        int d = g.alive ? (int)e.x - K : 0;              // > 0: add marks, < 0: remove
        uint32_t base = 0;                               // next Philox call of this (permutation, stratum)
        // the stratum in the counter: calls stay below 2^20
        fix_rounds<true>(g, d, base, (uint32_t)s << 20, n, e.z, member_at(off));
        if (l == s - s0) my_d = d, my_base = base;       // |d| < 4 (or the safety stop): the tail
      }
      // the tails of the L strata, lane l in the draw order of stratum s0 + l
      if (my_d != 0) {
        const uint4 e = tab[s0 + l];
        fix_tail(g, my_d, my_base, (uint32_t)(s0 + l) << 20, e.y, e.z, member_at(e.w & 0xffffu));
      }
    }
  }
  __syncthreads();

  // ---- output: marks, or per stratum their complement among the valid isolates ----
  auto row_field = [&](int row, int w) -> uint32_t {
    uint32_t f = xs[(int64_t)row * NB + w];
    if ((stratum_of(row) >> 24) & 1u) {
      const bool valid = (vm[row >> 5] >> (row & 31)) & 1u;
      f = valid ? (~f & live[w]) : 0u;
    }
    return f;
  };
  emit_labels<NB, OUT>(a, blk, row_field);
}

// (npos_ts, nval_ts) of every (trait, stratum): one block per trait, a histogram over the strata in LDS
__global__ __launch_bounds__(256) void k_strata_margins(const uint32_t* __restrict__ labels,
                                                        const uint32_t* __restrict__ masks,
                                                        const uint16_t* __restrict__ strata, int N, int Wp, int S,
                                                        int32_t* __restrict__ out) {
  __shared__ int hist[2 * kMaxStrata];
  const int t = blockIdx.x, tid = threadIdx.x;
  for (int k = tid; k < 2 * S; k += blockDim.x) hist[k] = 0;
  __syncthreads();
  const uint32_t* lrow = labels + (int64_t)t * Wp;
  const uint32_t* mrow = masks + (int64_t)t * Wp;
  for (int row = tid; row < N; row += blockDim.x) {
    const uint32_t valid = (mrow[row >> 5] >> (row & 31)) & 1u;
    if (!valid) continue;
    const int s = min((int)strata[row], S - 1);
    if ((lrow[row >> 5] >> (row & 31)) & 1u) atomicAdd(&hist[2 * s], 1);
    atomicAdd(&hist[2 * s + 1], 1);
  }
  __syncthreads();
  for (int k = tid; k < 2 * S; k += blockDim.x) out[(int64_t)t * 2 * S + k] = hist[k];
}

// ---- launch geometry --------------------------------------------------------------------------
// permutations of a dword column a block keeps: 32 while its rows fit LDS, else 16, 8 (tiles),
// ... 1 (bit rows); 0: N too large
int labels_elt(int64_t N, int min_elt) {
  for (int elt = 32; elt >= min_elt; elt >>= 1)
    if (labels_lds(N, elt, 1).bytes() <= kLabelsMaxLds) return elt;
  return 0;
}
int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}
// threads per block: 256, more when the launch has too few wavefronts for the chip and the rows
// are long (the row loop is what the extra wavefronts share)
int labels_threads(int64_t blocks, int64_t N, int num_cu) {
  int tpb = 256;
  while (tpb < 1024 && blocks * (tpb / 64) < (int64_t)num_cu * 8 && N / tpb >= 4) tpb *= 2;
  // a lane counts its round-0 marks in kCntPlanes bit-sliced planes: at most 1023 rows per thread
  // (N > 261 888 needs 512 threads, N > 523 776 needs 1024; scoary_perm_max_isolates() = 654 848)
  while (tpb < 1024 && (N + tpb - 1) / tpb > kMaxRowsPerThread) tpb *= 2;
  return tpb;
}
// The one launch path of the generator kernels.  optin_bit: the kernel's bit in the handle's record of who may
// use more than 64 KB of LDS; fits / why: the kernel's own limit, and what to say when it or the block size is off
template <class... Args>
int launch_block(scoary_handle h, hipStream_t s, void (*kernel)(Args...), int optin_bit, int64_t lds_bytes,
                 bool fits, const char* why, dim3 grid, int tpb, const Args&... args) {
  if (tpb < 64 || tpb > 1024 || (tpb & (tpb - 1)) || !fits) return fail(h, SCOARY_ERR_SIZE, why);
  const void* fn = reinterpret_cast<const void*>(kernel);
  if (lds_bytes > 64 * 1024 && !(h->labels_lds_optin & optin_bit)) {
    HIP_TRY(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLabelsMaxLds));
    h->labels_lds_optin |= optin_bit;
  }
  hipLaunchKernelGGL(kernel, grid, dim3((unsigned)tpb), (size_t)lds_bytes, s, args...);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}
int launch_labels(scoary_handle h, hipStream_t s, const LabelArgs& a, int NB, int OUT, dim3 grid, int tpb) {
  // the per-lane mark counters would wrap (labels_threads never picks such a geometry)
  const bool fits = (int64_t)tpb * kMaxRowsPerThread >= a.N;
  return launch_block(h, s,
                      OUT == 1 ? k_labels<1, 1>
                               : (OUT == 2 ? (NB == 2 ? k_labels<2, 2> : k_labels<1, 2>)
                                           : (NB == 2 ? k_labels<2, 0> : k_labels<1, 0>)),
                      1 << (NB + 4 * OUT) /* 2, 4 | 32 | 512, 1024 */, labels_lds<int64_t>(a.N, 1 << a.elt_log2, NB).bytes(), fits,
                      "k_labels: more than 1023 isolates per thread (or a block size that is no power of two in "
                      "64..1024)", grid, tpb, a);
}
int launch_labels_strata(scoary_handle h, hipStream_t s, const LabelArgs& a, const StrataArgs& sa, int NB, int OUT,
                         dim3 grid, int tpb) {
  const int64_t lds_bytes = strata_lds<int64_t>(a.N, NB, sa.S).bytes();
  return launch_block(h, s,
                      OUT == 1 ? k_labels_strata<1, 1>
                               : (OUT == 2 ? (NB == 2 ? k_labels_strata<2, 2> : k_labels_strata<1, 2>)
                                           : (NB == 2 ? k_labels_strata<2, 0> : k_labels_strata<1, 0>)),
                      1 << (16 + NB + 4 * OUT), lds_bytes, lds_bytes <= kLabelsMaxLds,
                      "k_labels_strata: rows, members and the stratum table do not fit LDS (or a block size that is "
                      "no power of two in 64..1024)", grid, tpb, a, sa);
}

// What every launch fills of LabelArgs (bit rows are complete with it; tiles add their range from a TileShape)
LabelArgs label_args(const uint32_t* d_masks, const int32_t* d_margins, int64_t N, int64_t P, int64_t perm_base,
                     int64_t trait_base, uint64_t seed, int elt, uint32_t* d_out) {
  LabelArgs a{};
  a.masks = d_masks, a.margins = d_margins, a.N = (int)N, a.Wp = (int)scoary_row_words(N);
  a.P = P, a.perm_base = perm_base, a.trait_base = (int)trait_base;
  a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.elt_log2 = ilog2(elt), a.out = d_out;
  return a;
}

// ---- the checks the entry points share beside check_args / strata_check (scoary_common.hpp) ------
int check_tile_base(scoary_handle h, const char* what, int64_t perm_base) {
  return (perm_base & 31) ? fail(h, SCOARY_ERR_ARG, std::string(what) + ": perm_base must be a multiple of 32")
                          : SCOARY_OK;
}
int check_grid(scoary_handle h, const char* what, int64_t gx) {
  return gx > 0x7fffffffLL ? fail(h, SCOARY_ERR_SIZE, std::string(what) + ": grid too large") : SCOARY_OK;
}

// bit rows: one block per (Philox block touched, sub-dword piece)
int64_t row_blocks(int64_t perm_base, int64_t P, int elt) {
  return (((perm_base + P - 1) >> 5) - (perm_base >> 5) + 1) * (32 / elt);
}

// The launch shape of a tile range.  gx = 0: the range is empty, nothing to launch
struct TileShape {
  int TW, NB, tpb;
  int64_t ntiles, gx;
};
// elt: permutations of a dword a block keeps (0: N too large for the generator); lds(NB): the kernel's LDS map
template <class Lds>
int tile_shape(scoary_handle h, const char* what, int64_t T, int64_t N, int64_t P, int64_t first_tile,
               int64_t n_tiles, int elt, Lds lds, TileShape& ts) {
  ts = TileShape{};
  ts.TW = list_tw(N);
  if (!ts.TW) return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": N too large for LDS tiles");
  const int64_t tile_perms = ts.TW * 32;
  ts.ntiles = (P + tile_perms - 1) / tile_perms;
  if (first_tile + n_tiles > T * ts.ntiles)
    return fail(h, SCOARY_ERR_ARG, std::string(what) + ": tile range past the last (trait, tile)");
  if (n_tiles == 0) return SCOARY_OK;
  if (!elt) return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": N too large for the label generator");
  // dword columns per block: two if that keeps >= 2 blocks per CU in the launch and >= 2 blocks
  // of LDS per CU (wider pieces per tile row, fewer count reductions)
  // (four columns per block were measured too: the fix-up then has two lanes per permutation and
  // k_labels is slower at the headline shape, 0.086 against 0.077 ms)
  ts.NB = (elt == 32 && 2 <= ts.TW && n_tiles * (ts.TW / 2) >= 2 * (int64_t)h->num_cu &&
           lds(2).bytes() <= kLabelsMaxLds / 2) ? 2 : 1;
  const int64_t units = (int64_t)ts.TW * (32 / elt) / ts.NB;
  ts.gx = (n_tiles + 7) / 8 * 8 * units;
  if (int rc = check_grid(h, what, ts.gx)) return rc;
  ts.tpb = labels_threads(n_tiles * units, N, h->num_cu);
  return SCOARY_OK;
}
void tile_args(LabelArgs& a, const TileShape& ts, int64_t first_tile, int64_t n_tiles, void* d_bfrag) {
  a.ntiles = (int)ts.ntiles, a.TW = ts.TW, a.first_flat = first_tile, a.nflat = n_tiles;
  a.bfrag = static_cast<v4i*>(d_bfrag);
}
// tiles + fragments: the shapes whose tiles are cut the way k_permute_mfma's stages are -- sixteen-dword tiles of
// whole dwords, at most kKSteps K-steps of isolates (elt: what labels_elt gives for N)
int check_bfrag_shape(scoary_handle h, const char* what, int64_t N, int elt) {
  return (N > scoary_mfma_max_isolates() || list_tw(N) != 16 || elt != 32)
             ? fail(h, SCOARY_ERR_SIZE, std::string(what) + ": more isolates than scoary_mfma_max_isolates()")
             : SCOARY_OK;
}

}  // namespace

extern "C" {

int64_t scoary_perm_max_isolates(void) {
  int64_t lo = 1, hi = (int64_t)1 << 24;            // largest N with one permutation per row in LDS
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (labels_elt(mid, 1)) lo = mid; else hi = mid - 1;
  }
  return lo;
}

int scoary_perm_generate(scoary_handle h, const uint32_t* d_masks, const int32_t* d_margins,
                         int64_t T, int64_t N, int64_t P, int64_t perm_base, int64_t trait_base,
                         uint64_t seed, uint32_t* d_perms, scoary_stream_t stream) {
  const char* what = "scoary_perm_generate";
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = check_args(h, what, d_masks && d_margins && d_perms && T >= 1 && N >= 1 && P >= 1 && perm_base >= 0 &&
                                       trait_base >= 0))
    return rc;
  if (T > 65535 || trait_base + T > 0x7fffffffLL || perm_base + P > 0xffffffffLL)
    return fail(h, SCOARY_ERR_SIZE, "scoary_perm_generate: T > 65535 or permutation index >= 2^32");
  const int elt = labels_elt(N, 1);
  if (!elt) return fail(h, SCOARY_ERR_SIZE, "scoary_perm_generate: more isolates than scoary_perm_max_isolates()");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LabelArgs a = label_args(d_masks, d_margins, N, P, perm_base, trait_base, seed, elt, d_perms);
  const int64_t gx = row_blocks(perm_base, P, elt);
  if (int rc = check_grid(h, what, gx)) return rc;
  KernelTimer kt(h, s, "k_perm_generate");
  return launch_labels(h, s, a, 1, 1, dim3((unsigned)gx, (unsigned)T), labels_threads(gx * T, N, h->num_cu));
}

extern "C++" {
// the tile-range generator, plain; d_bfrag (`fragments`): the B fragments of the range's stages as well
static int generate_tiles(scoary_handle h, const uint32_t* d_masks, const int32_t* d_margins, int64_t T, int64_t N,
                          int64_t P, int64_t perm_base, int64_t trait_base, uint64_t seed, int64_t first_tile,
                          int64_t n_tiles, uint32_t* d_tiles, bool fragments, void* d_bfrag,
                          scoary_stream_t stream) {
  const char* what = fragments ? "scoary_perm_generate_tiles_bfrag_range" : "scoary_perm_generate_tiles";
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = check_args(h, what, d_masks && d_margins && d_tiles && T >= 1 && N >= 1 && P >= 1 && perm_base >= 0 &&
                                       trait_base >= 0 && first_tile >= 0 && n_tiles >= 0 &&
                                       (d_bfrag || !fragments)))
    return rc;
  if (int rc = check_tile_base(h, what, perm_base)) return rc;
  if (T > 65535 || perm_base + P > 0xffffffffLL)
    return fail(h, SCOARY_ERR_SIZE, "scoary_perm_generate_tiles: T > 65535 or permutation index >= 2^32");
  const int elt = labels_elt(N, 8);
  if (fragments)
    if (int rc = check_bfrag_shape(h, what, N, elt)) return rc;
  TileShape ts;
  if (int rc = tile_shape(h, what, T, N, P, first_tile, n_tiles, elt,
                          [&](int nb) { return labels_lds(N, 32, nb); }, ts))
    return rc;
  if (ts.gx == 0) return SCOARY_OK;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  LabelArgs a = label_args(d_masks, d_margins, N, P, perm_base, trait_base, seed, elt, d_tiles);
  tile_args(a, ts, first_tile, n_tiles, d_bfrag);
  KernelTimer kt(h, s, "k_perm_generate_tiles");   // either output mode: the step's generator
  return launch_labels(h, s, a, ts.NB, fragments ? 2 : 0, dim3((unsigned)ts.gx), ts.tpb);
}
}  // extern "C++"

int scoary_perm_generate_tiles_range(scoary_handle h, const uint32_t* d_masks, const int32_t* d_margins,
                                     int64_t T, int64_t N, int64_t P, int64_t perm_base,
                                     int64_t trait_base, uint64_t seed, int64_t first_tile,
                                     int64_t n_tiles, uint32_t* d_tiles, scoary_stream_t stream) {
  return generate_tiles(h, d_masks, d_margins, T, N, P, perm_base, trait_base, seed, first_tile, n_tiles, d_tiles,
                        false, nullptr, stream);
}

int scoary_perm_generate_tiles_bfrag_range(scoary_handle h, const uint32_t* d_masks, const int32_t* d_margins,
                                           int64_t T, int64_t N, int64_t P, int64_t perm_base,
                                           int64_t trait_base, uint64_t seed, int64_t first_tile,
                                           int64_t n_tiles, uint32_t* d_tiles, void* d_bfrag,
                                           scoary_stream_t stream) {
  return generate_tiles(h, d_masks, d_margins, T, N, P, perm_base, trait_base, seed, first_tile, n_tiles, d_tiles,
                        true, d_bfrag, stream);
}

int scoary_perm_generate_tiles(scoary_handle h, const uint32_t* d_masks, const int32_t* d_margins,
                               int64_t T, int64_t N, int64_t P, int64_t perm_base,
                               int64_t trait_base, uint64_t seed, uint32_t* d_tiles,
                               scoary_stream_t stream) {
  const int TW = list_tw(N);
  const int64_t ntiles = TW && P > 0 ? (P + TW * 32 - 1) / (TW * 32) : 0;
  return scoary_perm_generate_tiles_range(h, d_masks, d_margins, T, N, P, perm_base, trait_base, seed,
                                          0, T * ntiles, d_tiles, stream);
}


// ---- spec S9: within-stratum shuffles ---------------------------------------------------------------
int scoary_perm_max_strata(void) { return kMaxStrata; }
int64_t scoary_perm_strata_max_isolates(void) { return kStrataMaxIsolates; }

int scoary_strata_margins(scoary_handle h, const uint32_t* d_labels, const uint32_t* d_masks,
                          const uint16_t* d_strata, int64_t T, int64_t N, int64_t S, int32_t* d_smargins,
                          scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = strata_check(h, "scoary_strata_margins", d_labels && d_masks && d_strata && d_smargins, T, N, S))
    return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  KernelTimer kt(h, s, "k_strata_margins");
  hipLaunchKernelGGL(k_strata_margins, dim3((unsigned)T), dim3(256), 0, s, d_labels, d_masks, d_strata, (int)N,
                     (int)scoary_row_words(N), (int)S, d_smargins);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_perm_generate_strata(scoary_handle h, const uint32_t* d_masks, const uint16_t* d_strata,
                                const int32_t* d_members, const int32_t* d_offsets, const int32_t* d_smargins,
                                int64_t T, int64_t N, int64_t S, int64_t P, int64_t perm_base, int64_t trait_base,
                                uint64_t seed, uint32_t* d_perms, scoary_stream_t stream) {
  const char* what = "scoary_perm_generate_strata";
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = strata_check(h, what, d_masks && d_strata && d_members && d_offsets && d_smargins && d_perms &&
                                         P >= 1 && perm_base >= 0 && trait_base >= 0, T, N, S))
    return rc;
  if (trait_base + T > 0x7fffffffLL || perm_base + P > 0xffffffffLL)
    return fail(h, SCOARY_ERR_SIZE, "scoary_perm_generate_strata: permutation index >= 2^32");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LabelArgs a = label_args(d_masks, nullptr, N, P, perm_base, trait_base, seed, 32, d_perms);
  const StrataArgs sa{d_strata, d_members, d_offsets, d_smargins, (int)S};
  const int64_t gx = row_blocks(perm_base, P, 32);
  if (int rc = check_grid(h, what, gx)) return rc;
  KernelTimer kt(h, s, "k_perm_generate_strata");
  return launch_labels_strata(h, s, a, sa, 1, 1, dim3((unsigned)gx, (unsigned)T),
                              labels_threads(gx * T, N, h->num_cu));
}

extern "C++" {
// the tile-range generator within strata; d_bfrag (`fragments`): the B fragments of the range's stages as well
static int generate_tiles_strata(scoary_handle h, const uint32_t* d_masks, const uint16_t* d_strata,
                                 const int32_t* d_members, const int32_t* d_offsets, const int32_t* d_smargins,
                                 int64_t T, int64_t N, int64_t S, int64_t P, int64_t perm_base, int64_t trait_base,
                                 uint64_t seed, int64_t first_tile, int64_t n_tiles, uint32_t* d_tiles,
                                 bool fragments, void* d_bfrag, scoary_stream_t stream) {
  const char* what = fragments ? "scoary_perm_generate_tiles_strata_bfrag_range"
                               : "scoary_perm_generate_tiles_strata_range";
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = strata_check(h, what, d_masks && d_strata && d_members && d_offsets && d_smargins && d_tiles &&
                                         P >= 1 && perm_base >= 0 && trait_base >= 0 && first_tile >= 0 &&
                                         n_tiles >= 0 && (d_bfrag || !fragments), T, N, S))
    return rc;
  if (int rc = check_tile_base(h, what, perm_base)) return rc;
  if (trait_base + T > 0x7fffffffLL || perm_base + P > 0xffffffffLL)
    return fail(h, SCOARY_ERR_SIZE, std::string(what) + ": permutation index >= 2^32");
  if (fragments)
    if (int rc = check_bfrag_shape(h, what, N, 32)) return rc;
  TileShape ts;
  if (int rc = tile_shape(h, what, T, N, P, first_tile, n_tiles, 32,
                          [&](int nb) { return strata_lds(N, nb, S); }, ts))
    return rc;
  if (ts.gx == 0) return SCOARY_OK;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  LabelArgs a = label_args(d_masks, nullptr, N, P, perm_base, trait_base, seed, 32, d_tiles);
  tile_args(a, ts, first_tile, n_tiles, d_bfrag);
  const StrataArgs sa{d_strata, d_members, d_offsets, d_smargins, (int)S};
  KernelTimer kt(h, s, "k_perm_generate_tiles_strata");
  return launch_labels_strata(h, s, a, sa, ts.NB, fragments ? 2 : 0, dim3((unsigned)ts.gx), ts.tpb);
}
}  // extern "C++"

int scoary_perm_generate_tiles_strata_range(scoary_handle h, const uint32_t* d_masks, const uint16_t* d_strata,
                                            const int32_t* d_members, const int32_t* d_offsets,
                                            const int32_t* d_smargins, int64_t T, int64_t N, int64_t S, int64_t P,
                                            int64_t perm_base, int64_t trait_base, uint64_t seed,
                                            int64_t first_tile, int64_t n_tiles, uint32_t* d_tiles,
                                            scoary_stream_t stream) {
  return generate_tiles_strata(h, d_masks, d_strata, d_members, d_offsets, d_smargins, T, N, S, P, perm_base,
                               trait_base, seed, first_tile, n_tiles, d_tiles, false, nullptr, stream);
}

int scoary_perm_generate_tiles_strata_bfrag_range(scoary_handle h, const uint32_t* d_masks, const uint16_t* d_strata,
                                                  const int32_t* d_members, const int32_t* d_offsets,
                                                  const int32_t* d_smargins, int64_t T, int64_t N, int64_t S,
                                                  int64_t P, int64_t perm_base, int64_t trait_base, uint64_t seed,
                                                  int64_t first_tile, int64_t n_tiles, uint32_t* d_tiles,
                                                  void* d_bfrag, scoary_stream_t stream) {
  return generate_tiles_strata(h, d_masks, d_strata, d_members, d_offsets, d_smargins, T, N, S, P, perm_base,
                               trait_base, seed, first_tile, n_tiles, d_tiles, true, d_bfrag, stream);
}

}  // extern "C"
