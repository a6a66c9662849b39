// scoary_mfma.hip -- the matrix-core permutation path for long-list genes (N <= 2048).
//
// The list count of the list-driven kernel is a 0/1 GEMM,
//     u[slot][pi] = sum_i minority[slot][i] * label[i][pi],
// exact in fp32, whose cost does not depend on the list length.  k_permute_lists pays 2 LUT ops
// per listed isolate and 32 permutations, so beyond a break-even list length (kMfmaNsPerGene /
// kListNsPerEntry below) the matrix cores are cheaper; scoary_permute_hybrid routes the slots
// [0, k_split) -- the long-list end of the slot order -- here and leaves the rest to the lists.
//
//   k_mfma_panels  (once per data set)  minority rows of the list slots as E2M1 (0 = 0x0, 1.0 = 0x2)
//                                       in 16-byte pieces (32 isolates of a slot), laid out as the A fragments
//                                       of a 32x32x64 fp4 MFMA, 1 KB per slot
//   B fragments    (per label batch)    the labels as E2M1 B fragments, 64 KB per (trait, 64 permutations): the
//                                       SAME draws the list kernel reads.  The label generator writes them next
//                                       to its tile rows, out of the rows it holds in LDS (scoary_labels.hip,
//                                       output mode "tiles + fragments"; the layout is mfma_bfrag_emit's,
//                                       scoary_common.hpp), and scoary_permute_hybrid_bfrag(bfrag_ready = 1)
//                                       takes them as they are;
//   k_mfma_bfrag                        the same fragments from label tiles that come from elsewhere (gathered
//                                       from other ranks, or a caller's own): scoary_permute_hybrid
//   k_permute_mfma                      v_mfma_f32_16x16x128_f8f6f4 on those pieces (the chip holds a higher
//                                       clock on this shape than on 32x32x64: profiles/mfma_16x16.txt); gene
//                                       operand stationary in registers (128 per lane), two wavefronts
//                                       per SIMD half a stage apart in the data and a quarter in time, B
//                                       streamed through a four-slot LDS ring by LDS-DMA, region test on the
//                                       accumulators, 16-bit counts
//                                       into the list path's `partial`
#include "scoary_common.hpp"

// The two measured rates the routing is decided by (scoary_mfma_route): a routed gene costs kMfmaNsPerGene
// whatever its list holds, a listed gene kListNsPerEntry per padded list entry -- break-even list length
// = their ratio (scoary_mfma_breakeven_entries).  Both per 100 000 tests of the gene (cfg3: 10 traits x
// 10 000 permutations), chip-wide, on MI355X: k_permute_mfma + k_mfma_bfrag with every cfg3 gene routed,
// k_permute_lists with none (profiles/mfma_ranges.txt: 57.1-59.4 and 0.179-0.184 in three sessions).  With the
// fragments written by the label generator k_mfma_bfrag is no part of the step (1.0 of the 58); one session of
// that step gave 56.3 and 0.175 (profiles/labels_bfrag.txt), both inside or next to the ranges above: the
// constants stay until more than one session says otherwise (cfg3's split with them: 32 768 slots, as before).
const double kMfmaNsPerGene = 58.0;
const double kListNsPerEntry = 0.18;
// What a block costs beside its stages, in stage-times of its loop (scoary_mfma_geom; least squares over P and
// trait count in profiles/mfma_ranges.txt: 5.7-6.1 and 1.9-2.3 at 2.14-2.19 us per stage): its start and end
// (thresholds, the A panel: 256 KB from HBM, ring fill, epilogue), and every trait it enters after its first (the
// segment's lane reduction and store, the thresholds out of the LDS; both wavefront groups pay it in turn).
const double kMfmaBlockStartStages = 6.0;
const double kMfmaTraitSwitchStages = 2.0;

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

// (kKSteps, kFragBytes, kStageBytes and the E2M1 conversion: scoary_common.hpp, with the B-fragment layout)
constexpr int kBlockGenes = 256;                  // list slots of a block: eight wavefronts x 32
constexpr int kBlockWaves = 8;                    // two per SIMD
constexpr int kHalfBytes = kStageBytes / 2;       // the unit of the LDS ring: 8 K-steps of 128 isolates
constexpr int kKSteps128 = kKSteps / 2;           // K-steps of v_mfma_f32_16x16x128_f8f6f4
constexpr int kKStepBytes = kStageBytes / kKSteps128;   // B of one of them: four 16-column tiles
constexpr int kRingSlots = 4;                     // 128 KB
constexpr int kAhead = kRingSlots - 2;            // a half stage is issued this many ticks before its first read
constexpr int kRingBytes = kRingSlots * kHalfBytes;
constexpr int kDmaPerHalf = kHalfBytes / kBlockWaves / kFragBytes;   // LDS-DMA instructions per wavefront and half stage
constexpr int kThrBytes = 32 * 8;                 // behind the ring: the (lo, hi1) pairs of a wavefront's 32 slots
constexpr int kMfmaLds = kRingBytes + kBlockWaves * kThrBytes;
static_assert(kRingSlots >= 4 && kMfmaLds <= 160 * 1024 && (kAhead - 1) * kDmaPerHalf < 64,
              "a half stage is issued at least two ticks ahead, within the LDS of a CU and the vmcnt field");

// A panels: [wave panel of 64 slots][row tile i][K-step k][lane] x 16 bytes.  Lane l of fragment (i, k)
// holds slot 64 * panel + 32 i + (l & 31), isolates 64 k + 32 (l >> 5) .. + 31: one 32-bit word of the
// gene's tiled row, XOR `flipped` (the MINORITY indicator: the accumulator is the list count u),
// isolates >= N and slots >= G zero.
__global__ __launch_bounds__(256) void k_mfma_panels(const uint32_t* __restrict__ tiled, int64_t Gp, int G, int N,
                                                     const int32_t* __restrict__ order,
                                                     const uint8_t* __restrict__ flipped, int64_t total,
                                                     v4i* __restrict__ panels) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int lane = (int)(idx & 63);
  const int64_t f = idx >> 6;
  const int k = (int)(f & 31), i = (int)((f >> 5) & 1);
  const int64_t slot = (f >> 6) * 64 + i * 32 + (lane & 31);
  const int w = 2 * k + (lane >> 5);              // word of the row: isolates 32 w .. 32 w + 31
  uint32_t bits = 0u;
  if (slot < G && 32 * w < N) {
    const int g = order[slot];
    bits = tiled[((int64_t)(w >> 2) * Gp + g) * 4 + (w & 3)];
    if (flipped[g]) bits = ~bits;
    if (32 * w + 32 > N) bits &= (1u << (N - 32 * w)) - 1u;
  }
  panels[idx] = fp4_of_bits32(bits);
}

// B fragments from label tiles that come from elsewhere (tiles[t][tile][row 0..N][16 dwords], dword j of a row =
// permutations 512 tile + 32 j .. + 31): stage s of trait t is dwords 2 (s % 8) + j of tile s / 8, in the layout of
// mfma_bfrag_emit (scoary_common.hpp).  Rows >= N are zero; permutations >= P hold whatever the tile holds and are
// masked by the kernel.
__global__ __launch_bounds__(256) void k_mfma_bfrag(const uint32_t* __restrict__ tiles, int N, int ntiles,
                                                    int64_t tile_dwords, int S, v4i* __restrict__ bfrag) {
  const int s = blockIdx.x, t = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t* tile = tiles + ((int64_t)t * ntiles + (s >> 3)) * tile_dwords + 2 * (s & 7);
#pragma unroll
  for (int j = 0; j < 2; ++j)
    mfma_bfrag_emit(bfrag, S, t, s, j, wave, 4, [&](int row) { return row < N ? tile[(int64_t)row * 16 + j] : 0u; });
}

// One 16-byte vector per lane, src + 16 * lane -> LDS address lds + 16 * lane, by LDS-DMA: wave-uniform
// base in an SGPR pair, the lane offset in one VGPR, the LDS destination in M0 (handed back as it was).
__device__ __forceinline__ void mfma_dma16(uint32_t lds, uint32_t lane_off, const unsigned char* src) {
  uint32_t m0_saved;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0"
               : "=&s"(m0_saved)
               : "s"(lds), "v"(lane_off), "s"(src)
               : "memory");
}

// The same for one dword per lane: src + lane_off -> LDS address lds + 4 * lane.
__device__ __forceinline__ void mfma_dma4(uint32_t lds, uint32_t lane_off, const unsigned char* src) {
  uint32_t m0_saved;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
               "global_load_lds_dword %2, %3\n\ts_mov_b32 m0, %0"
               : "=&s"(m0_saved)
               : "s"(lds), "v"(lane_off), "s"(src)
               : "memory");
}

// Bijective XCD remap: consecutive work items land on ONE XCD (blocks are dealt to the eight XCDs
// round-robin), so the blocks resident on an XCD at one time share their (trait, permutation range)
// and stream the same B stages out of that XCD's L2.
__device__ __forceinline__ int xcd_item(int orig, int n) {
  const int q = n >> 3, r = n & 7, x = orig & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (orig >> 3);
}

// Block = 256 list slots x one range of the linear stage sequence q = t * S + s (S stages of 64 permutations per
// trait, bfrag's own address order): stages [q0, q0 + ns), q0 = range * L.  A range may start and end inside a
// trait and may hold several traits; the A panel and the ring are set up once per block whatever it holds.  A
// SEGMENT is the part of one trait inside one range: its count goes to partial tile `range - first range that
// meets the trait` (scoary_mfma_geom admits a range length only if every trait meets at most ntiles ranges), and the
// block of the segment with the trait's last stage also writes, behind its loop, the zeros of the tiles behind that
// segment's, so every (trait, tile) cell of a routed slot is written exactly once.  Eight wavefronts, two per SIMD.
// Wavefront w owns 32 slots, row tile w & 1 of wave panel w >> 1, as two row tiles of 16: its A fragments of all
// 16 K-steps of 128 isolates stay in 128 registers, next to the 2 x 4 accumulator tiles of a stage's 64
// permutations (32 registers), minus the interval centre and the half width of its 8 rows and 8 counters (no LDS
// beside the ring, at most 256 registers: two wavefronts per SIMD).
// The accumulators start at minus the centre of the acceptance interval [lo, hi1) of the list count -- the C
// operand of a stage's first K-step -- so "u outside the interval" is one compare, |acc| > half width; the four
// column tiles of a row share one per-lane counter that lives across the stages of a segment, the 16 lanes of a
// row meet once per segment, at its end.
//
// Stagger.  Wavefronts 4..7, the SIMD partners of 0..3, run half a stage behind them in the data AND half a half
// stage apart in time.  A block executes nh + 1 barriers for nh half stages; INTERVAL n is what a wavefront does
// between barrier n and barrier n + 1:
//   early (0..3)  half n whole, fragments 0..31: the barrier stands in front of a half;
//   late  (4..7)  fragments 16..31 of half n - 1, the half boundary WITHOUT a barrier, fragments 0..15 of half n:
//                 the barrier stands in the middle of a half, in front of fragment 16.  Interval 0 holds only
//                 fragments 0..15 of half 0 -- that sets the offset -- and interval nh is the tail, fragments
//                 16..31 of half nh - 1 behind the last barrier, with nothing of the early wavefronts beside it.
// So at a barrier the early wavefronts are between two halves (first fragment reads; every other time the region
// test) while their partners are in mid-half with fragments in the register ring and go on with MFMAs at once; and
// the late wavefronts' own boundary lies beside the early partners' fragments 16..: their fragment ring runs across
// it (fragments 0..2 of half n are read in front of the last MFMAs of half n - 1: half n has been whole since
// barrier n), and their region test, end of segment, threshold traffic and LDS-DMA issue stand there.  What the
// partners still share is the barrier's own skew.  The region test of a stage stands at the boundary behind it, in
// front of the next stage's first MFMA (which takes the centres as C); the range's last one follows the loop.
// Where the tested stage was its trait's last, the same place ends the segment (ragged column count, lane
// reduction, stores, counters to zero) and takes the next trait's centres and half widths out of the LDS.  All of
// it is wave-local.
// The two groups are two instances of one loop body (`run`), chosen by the wave-uniform `late`; they differ in
// where the barrier and the LDS-DMA issue stand.
// Measured and not built in, each within the kernel's run-to-run spread (profiles/r11_mfma_two_wave.txt):
// s_setprio 1 for the late wavefronts; a fifth ring slot (issue three intervals ahead, 160 KB); with it, reading
// the next half's first fragments in front of a barrier both partners took between halves.  Measured against this
// schedule and slower (profiles/mfma_time_stagger.txt): the four pieces of an interval issued one by one among its
// MFMAs instead of together, with the barriers where they were and with this stagger (0.07 and 0.08 ms off the cfg3
// step in the session in which this schedule took 0.10).
//
// Ring.  B moves HBM/L2 -> LDS by LDS-DMA in half stages of 32 KB (8 K-steps), half n into slot
// n % kRingSlots, every wavefront 4 KB of it in kDmaPerHalf pieces.  Halves 0 and 1 are issued in front of the
// loop.  Invariant, for every n:
//   * in front of barrier n a wavefront has issued every piece of the halves 0 .. n + kAhead - 1 and waits with
//     the counted vmcnt(kAhead - 1 halves) until its pieces of half n have landed: barrier n makes half n whole.
//     Every read of half n lies behind barrier n (early: interval n; late: intervals n and n + 1);
//   * the kDmaPerHalf pieces of half n + kAhead = n + 2 are issued in interval n, together: by an early wavefront
//     right behind barrier n, by a late one at its boundary into half n (in interval 0: right behind barrier 0, which
//     is that boundary) -- in both cases in front of the interval's counted wait, which so means what the line above
//     says;
//   * they go into slot (n + 2) % kRingSlots = (n - 2) % kRingSlots.  Half n - 2 is read by the early wavefronts in
//     interval n - 2 and by the late ones in n - 2 and n - 1, the last read retired by the MFMA that uses it: all of
//     it in front of barrier n.  In interval n the halves n - 1 and n are read and n + 1, n + 2 are in flight: four
//     distinct slots, kRingSlots = 4, kAhead = 2.
// Halves past the end re-read the last one into such a slot, which nobody reads any more (the late wavefronts'
// look-ahead reads of "half nh" behind barrier nh find that copy and use nothing of it), so the counts stay the same
// to the end; ns = 1 needs no case of its own.  (tests/test_mfma_ring_schedule.py walks these statements.)
// Stores and the threshold DMA among the ring's LDS-DMAs.  A trait switch inside the loop stores the ended
// segment's counts, and the boundary one stage before it fetches the next trait's thresholds, while halves are in
// flight.  Vector memory operations retire in the order they were issued and the counted wait only bounds how many
// are outstanding, so an operation YOUNGER than the DMAs a wait is there for makes it retire more of the older DMAs,
// never fewer: a store or a fetch can make a wait longer, not early.  The fetch is one more LDS-DMA, issued at the
// boundary into a trait's last stage.  A late wavefront issues it IN FRONT of that boundary's half pieces, so the
// next barrier's counted wait, which leaves only those four outstanding, retires it.  An early wavefront issues it
// behind the pieces of its interval n; the wait in front of barrier n + 1 may leave it outstanding, the one in front
// of barrier n + 2 has the four pieces of interval n + 1 behind it and retires it.  take_thresholds stands one stage
// later, at the boundary into the next stage: for an early wavefront behind barrier n + 2, for a late one behind
// the two barriers it takes in between.  Either way the fetch has landed, with no wait of its own and without
// draining the ring (as a register load it would: the compiler waits vmcnt(0) for one, and measured so a switch
// cost four to seven stages).  It lands in 256 bytes only its own wavefront reads, so no barrier is part of that,
// and the next fetch is issued behind the take.  There is still no ordinary global load inside the loop.
__global__ __launch_bounds__(kBlockWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_permute_mfma(const v4i* __restrict__ panels, const unsigned char* __restrict__ bfrag,
                    const uint2* __restrict__ lcrit, int G, int64_t P, int S, int64_t Q, int L, int nblk_genes,
                    int ntiles, int64_t gs, uint16_t* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int item = xcd_item(blockIdx.x, gridDim.x);
  const int gb = item % nblk_genes, rng = item / nblk_genes;
  const int64_t q0 = (int64_t)rng * L;
  const int ns = (int)min((int64_t)L, Q - q0);
  // (t, s) of the stage the loop is at, and the partial tile of the segment it is in: all wave-uniform
  int t = (int)(q0 / S), s = (int)(q0 % S);
  int jt = rng - (int)((int64_t)t * S / L);
  const int tid = threadIdx.x, lane = tid & 63, quad = lane >> 4, l15 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool late = wave >= kBlockWaves / 2;
  // accumulator register r of row tile i is row 16 i + 4 quad + r of the wavefront's 32 slots
  const int wslot0 = gb * kBlockGenes + wave * 32;  // the wavefront's first slot
  const int rows_mine = min(32, G - wslot0) - 4 * quad;   // a lane's row 16 i + r is a slot < G below this (<= 0: none is)
  v4f negc[2];
  float hw[8];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)lds;
  const uint32_t lane_off = (uint32_t)lane * 16u;
  // Thresholds.  The (lo, hi1) pairs of the wavefront's 32 slots are 256 contiguous bytes of lcrit[tt]: one LDS-DMA
  // of a dword per lane copies them into the wavefront's own 256 bytes behind the ring (slots >= G: the last
  // slot's pair again).  The lane's part of the addresses and conditions goes through an opaque copy, here and in
  // end_segment: they are needed once per trait, and hoisted out of the stage loop they would take registers the
  // loop has not got.
  const int thr_slot0 = min(wslot0, G - 1);
  const uint32_t thr_lds = kRingBytes + (uint32_t)wave * kThrBytes;
  auto fetch_thresholds = [&](int tt) {
    uint32_t l = lane_off;
    asm volatile("" : "+v"(l));
    l >>= 4;
    const uint32_t off = (uint32_t)min((int)(l >> 1), G - 1 - thr_slot0) * 8u + (l & 1u) * 4u;
    mfma_dma4(lds0 + thr_lds, off, reinterpret_cast<const unsigned char*>(lcrit + ((int64_t)tt * G + thr_slot0)));
  };
  // The centres and half widths from the pairs fetch_thresholds brought; the caller has waited for that DMA.  A
  // wavefront reads only what it fetched itself: no barrier is involved.
  auto take_thresholds = [&]() {
    int q4 = 4 * quad, mine = rows_mine;
    asm volatile("" : "+v"(q4), "+v"(mine));
    const uint2* thr = reinterpret_cast<const uint2*>(lds + thr_lds) + q4;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int row = 16 * (r >> 2) + (r & 3);
      const uint2 cr = thr[row];
      negc[r >> 2][r & 3] = -0.5f * (float)((int)cr.x + (int)cr.y - 1);
      hw[r] = row < mine ? 0.5f * (float)((int)cr.y - 1 - (int)cr.x) : 1e30f;   // slots >= G: never counted
    }
    // read and converted here: the next fetch may overwrite the pairs
    asm volatile("" : "+v"(negc[0]), "+v"(negc[1]));
#pragma unroll
    for (int r = 0; r < 8; ++r) asm volatile("" : "+v"(hw[r]));
  };
  // The A fragments out of the panel's 16-byte pieces (32 isolates of one slot): fragment (row tile i, K-step k)
  // of 16 slots x 128 isolates holds in lane l the piece of slot 16 i + (l & 15), isolates 128 k + 32 (l >> 4)
  // .. + 31, which the panel keeps in its K-step 2 k + (l >> 5), lane 16 i + (l & 15) + 32 ((l >> 4) & 1).
  v4i a[2][kKSteps128];
  {
    fetch_thresholds(t);
    const v4i* ap = panels + ((int64_t)gb * kBlockWaves + wave) * (kKSteps * 64) + (quad >> 1) * 64 + (quad & 1) * 32 + l15;
#pragma unroll
    for (int k = 0; k < kKSteps128; ++k)
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i][k] = ap[k * 128 + i * 16];
    // every global load and the first thresholds retired here, before the ring's first LDS-DMA is issued
#pragma unroll
    for (int k = 0; k < kKSteps128; ++k) asm volatile("" : "+v"(a[0][k]), "+v"(a[1][k]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    take_thresholds();
  }

  const unsigned char* bsrc = bfrag + q0 * kStageBytes + wave * (kHalfBytes / kBlockWaves);
  const int nh = 2 * ns;
  auto issue_half = [&](int n) {
    const unsigned char* src = bsrc + (int64_t)min(n, nh - 1) * kHalfBytes;
    const uint32_t dst = lds0 + (uint32_t)(n % kRingSlots) * kHalfBytes + (uint32_t)wave * (kHalfBytes / kBlockWaves);
#pragma unroll
    for (int p = 0; p < kDmaPerHalf; ++p) mfma_dma16(dst + p * kFragBytes, lane_off, src + p * kFragBytes);
  };
#pragma unroll
  for (int n = 0; n < kAhead; ++n) issue_half(n);
  auto barrier = [&]() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kAhead - 1) * kDmaPerHalf) : "memory");
    __builtin_amdgcn_s_barrier();
  };

  uint32_t ex[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) ex[r] = 0u;
  const int ragged = (int)(P - (int64_t)(S - 1) * 64);    // columns of a trait's last stage that exist: 1 .. 64

  v4f acc[2][4];                                    // [row tile][column tile]: column 16 j + (l & 15) of the stage
  auto region_test = [&](int nvalid) {
    if (nvalid < 64) {                              // ragged last stage of a trait: columns >= P do not count --
#pragma unroll
      for (int j = 0; j < 4; ++j) {                 // a NaN is outside no interval
        const bool v = 16 * j + l15 < nvalid;
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r >> 2][j][r & 3] = v ? acc[r >> 2][j][r & 3] : __builtin_nanf("");
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) ex[r] += (uint32_t)(__builtin_fabsf(acc[r >> 2][j][r & 3]) > hw[r]);
  };
  // The end of trait tt's segment in this range: partial[tt][jt][slot] takes its count and the counters start
  // again.  Lanes 0 .. 7 of each group of 16 keep the sum of counter `lane` and store one row each: ONE store
  // instruction, issued iff the wavefront owns a slot < G.  A trait the block enters after this one begins inside
  // the range: tile 0.
  const int jt0 = jt;
  auto end_segment = [&](int tt) {
    uint16_t* out = partial + ((int64_t)tt * ntiles + jt) * gs + wslot0;   // wave-uniform
    int rl = l15, q4 = 4 * quad, mine = rows_mine;
    asm volatile("" : "+v"(rl), "+v"(q4), "+v"(mine));
    uint32_t count = 0u;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      uint32_t v = ex[r];
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
      ex[r] = 0u;
      count = rl == r ? v : count;
    }
    const int row = 16 * (rl >> 2) + (rl & 3);
    if (rl < 8 && row < mine) out[q4 + row] = (uint16_t)count;
    jt = 0;
  };
  // B fragment (K-step k, column tile j) holds in lane l the piece of column 16 j + (l & 15), isolates 128 k +
  // 32 (l >> 4) .. + 31, which the stage keeps in its K-step 2 k + (l >> 5), column tile j >> 1, lane
  // 16 (j & 1) + (l & 15) + 32 ((l >> 4) & 1): every 16 lanes read 256 contiguous bytes.
  const unsigned char* lbase = lds + ((quad >> 1) * 128 + (quad & 1) * 32 + l15) * 16;
  // A half stage is 32 B fragments, f = 4 (K-step) + column tile, two MFMAs each (one per row tile).  Fragment
  // f + kBLead is read in front of the MFMAs of fragment f through a register ring of kBLead + 1: one
  // ds_read_b128 per pair of MFMAs, three pairs ahead of its use.  The scheduling barriers keep the reads where
  // they are written (left alone, the compiler reads each fragment right before its MFMAs).  Measured
  // (profiles/mfma_16x16.txt section 3): whole K-steps read two K-steps ahead, as the 32x32x64 body did, cost
  // 0.13 ms of the cfg3 step against this, leads of 2, 4, 5 and 6 fragments 0.01-0.03 ms.
  constexpr int kBLead = 3, kFrags = 4 * (kKSteps128 / 2);
  // The loop of one wavefront group (see "Stagger" above): the early wavefronts take their barrier in front of a
  // half, the late ones behind its fragment kFrags / 2 - 1, and only that differs between the two instances.
  auto run = [&](auto group) {
    constexpr bool kLate = decltype(group)::value;
    v4i bq[kBLead + 1];
    auto read_b = [&](const unsigned char* buf, int f) {
      bq[f % (kBLead + 1)] =
          *reinterpret_cast<const v4i*>(buf + (f >> 2) * kKStepBytes + ((f >> 1) & 1) * kFragBytes + (f & 1) * 256);
    };
    int rslot = 0;                                  // ring slot of the half this wavefront is reading
    int nx = kAhead;                                // the half it issues next
    const unsigned char* bbuf = lbase;
    if (kLate) {                                    // interval 0: fragments 0 .. 15 of half 0
      barrier();
#pragma unroll
      for (int f = 0; f < kBLead; ++f) read_b(bbuf, f);
    }
    for (int st = 0; st < ns; ++st) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (!kLate) {
          barrier();
          issue_half(nx++);
#pragma unroll
          for (int f = 0; f < kBLead; ++f) read_b(bbuf, f);
        }
        if (h == 0) {
          __builtin_amdgcn_sched_barrier(0);
          if (st > 0) {                             // stage st - 1, never the range's last
            const bool entered = s == 0;            // but the last of trait t - 1
            region_test(entered ? ragged : 64);
            if (entered) {
              end_segment(t - 1);
              take_thresholds();                    // fetched a stage ago: two counted waits lie between
            }
          }
          if (s == S - 1 && st + 1 < ns) fetch_thresholds(t + 1);   // the trait's last stage: the next stage's trait
          __builtin_amdgcn_sched_barrier(0);
        }
        if (kLate) issue_half(nx++);                // at the boundary, behind the fetch, in front of the counted wait
        rslot = rslot == kRingSlots - 1 ? 0 : rslot + 1;
        const unsigned char* nbuf = lbase + rslot * kHalfBytes;
#pragma unroll
        for (int f = 0; f < kFrags; ++f) {
          const int k = h * (kKSteps128 / 2) + (f >> 2), j = f & 3;
          if (kLate && f == kFrags / 2) barrier();
          if (f + kBLead < kFrags) read_b(bbuf, f + kBLead);
          else if (kLate) read_b(nbuf, f + kBLead - kFrags);   // whole since this interval's barrier
          __builtin_amdgcn_sched_barrier(0);
          const v4i x = bq[f % (kBLead + 1)];
          const v8i bb = v8i{x.x, x.y, x.z, x.w, 0, 0, 0, 0};
#pragma unroll
          for (int i = 0; i < 2; ++i)
            // The stage's first K-step takes minus the centre as C: no accumulator set-up.  Scale operands 0 select
            // the instruction without block scales (v_mfma_f32_16x16x128_f8f6f4: every scale 1, half the code
            // bytes): the same counts, and 0.14 ms of the cfg3 step less than the form that reads 0x7f scales from
            // a VGPR.
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                v8i{a[i][k].x, a[i][k].y, a[i][k].z, a[i][k].w, 0, 0, 0, 0}, bb, k == 0 ? negc[i] : acc[i][j], 4, 4, 0,
                0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        bbuf = nbuf;
      }
      if (++s == S) s = 0, ++t;
    }
    if (!kLate) barrier();                          // barrier nh: the late wavefronts' tail is behind it
  };
  if (late) run(std::true_type{});
  else run(std::false_type{});
  const bool trait_done = s == 0;                   // (t, s) is one past the range's last stage
  region_test(trait_done ? ragged : 64);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the ring's last (redundant) transfers land before the LDS is given up
  end_segment(trait_done ? t - 1 : t);

  // The zeros of the tiles behind a trait's last segment, for every trait whose last stage this range held: traits
  // t0 .. t - 1, the first in tile jt0, the others in tile 0 (k_lists_reduce sums every tile of every slot).  Out
  // here they are no traffic among the ring's.
  {
    int rl = l15, q4 = 4 * quad, mine = rows_mine;
    asm volatile("" : "+v"(rl), "+v"(q4), "+v"(mine));
    const int row = 16 * (rl >> 2) + (rl & 3);
    const bool stores = rl < 8 && row < mine;
    const int t0 = (int)(q0 / S);
    for (int tt = t0; tt < t; ++tt) {
      uint16_t* out = partial + (int64_t)tt * ntiles * gs + wslot0 + q4 + row;
      for (int tile = (tt == t0 ? jt0 : 0) + 1; tile < ntiles; ++tile)
        if (stores) out[(int64_t)tile * gs] = 0;
    }
  }
}

}  // namespace

// The range lengths L a launch may use, longest first (one entry per distinct ceil(Q / R)): L <= 1023 keeps a
// segment's count within 16 bits, and every trait meets at most ntiles ranges, so each of its segments has a
// partial tile of its own (P <= 512, one tile: every cut on a trait boundary).  `switches` = the most traits any
// range enters after its first.  L = min(S, 1023) always qualifies.
struct MfmaRange {
  int64_t L, ranges, switches;
};
static std::vector<MfmaRange> mfma_ranges(int64_t T, int64_t P, int64_t ntiles) {
  std::vector<MfmaRange> out;
  const int64_t S = (P + 63) / 64, Q = T * S;
  for (int64_t L = std::min<int64_t>(Q, 1023); L >= 1; --L) {
    const int64_t ranges = (Q + L - 1) / L;
    if ((Q + ranges - 1) / ranges != L) continue;           // not ceil(Q / R) for any R
    // where a trait (a range) starts inside a range (a trait) repeats after at most L traits (S ranges), and the
    // short last range enters no more traits than a whole one that starts where it does
    bool ok = true;
    for (int64_t t = 0; t < std::min(T, L) && ok; ++t) ok = ((t + 1) * S - 1) / L - t * S / L + 1 <= ntiles;
    if (!ok) continue;
    MfmaRange c{L, ranges, 0};
    for (int64_t r = 0; r < std::min(ranges, S); ++r)
      c.switches = std::max(c.switches, (std::min(Q, (r + 1) * L) - 1) / S - r * L / S);
    out.push_back(c);
  }
  return out;
}

// The cheapest of them for `gene_blocks` 256-slot blocks on num_cu CUs, in stage-times of one CU:
//   rounds of blocks over the CUs x (L + kMfmaBlockStartStages + switches x kMfmaTraitSwitchStages).
// The one-trait-per-block shapes (L = S / k) are candidates like any other; on a tie the longest range wins.
static MfmaGeom mfma_pick(const std::vector<MfmaRange>& cands, int num_cu, int64_t gene_blocks, int64_t S,
                          int64_t T) {
  MfmaGeom g{};
  g.stages = S;
  g.Q = T * S;
  g.gene_blocks = gene_blocks;
  for (const MfmaRange& c : cands) {
    const int64_t blocks = gene_blocks * c.ranges;
    const double cost = (double)((blocks + num_cu - 1) / num_cu) *
                        ((double)c.L + kMfmaBlockStartStages + (double)c.switches * kMfmaTraitSwitchStages);
    if (g.L == 0 || cost < g.cost) g.cost = cost, g.ranges = c.ranges, g.L = c.L, g.blocks = blocks;
  }
  return g;
}

MfmaGeom scoary_mfma_geom(int num_cu, int64_t k_split, int64_t T, int64_t P, int64_t ntiles) {
  return mfma_pick(mfma_ranges(T, P, ntiles), num_cu, (k_split + kBlockGenes - 1) / kBlockGenes, (P + 63) / 64, T);
}

int scoary_mfma_launch(scoary_handle h, hipStream_t s, const uint32_t* d_tiles, const void* d_panels, void* d_bfrag,
                       const uint32_t* d_lcrit, uint16_t* d_partial, int64_t k_split, int64_t G, int64_t T,
                       int64_t N, int64_t P, int64_t ntiles, int64_t gs, bool bfrag_ready) {
  const MfmaGeom g = scoary_mfma_geom(h->num_cu, k_split, T, P, ntiles);
  if (g.blocks > 0x7fffffffLL || g.stages > 0x7fffffffLL / 64)
    return fail(h, SCOARY_ERR_SIZE, "scoary_permute_hybrid: grid too large");
  if (!h->mfma_lds_optin) {
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_permute_mfma),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    h->mfma_lds_optin = 1;
  }
  if (!bfrag_ready) {                               // tiles from elsewhere: the generator did not write d_bfrag
    KernelTimer kt(h, s, "k_mfma_bfrag");
    hipLaunchKernelGGL(k_mfma_bfrag, dim3((unsigned)g.stages, (unsigned)T), dim3(256), 0, s, d_tiles, (int)N,
                       (int)ntiles, list_tile_dwords(N, 16), (int)g.stages, static_cast<v4i*>(d_bfrag));
  }
  {
    KernelTimer kt(h, s, "k_permute_mfma");
    hipLaunchKernelGGL(k_permute_mfma, dim3((unsigned)g.blocks), dim3(kBlockWaves * 64), kMfmaLds, s,
                       static_cast<const v4i*>(d_panels), static_cast<const unsigned char*>(d_bfrag),
                       reinterpret_cast<const uint2*>(d_lcrit), (int)G, P, (int)g.stages, g.Q, (int)g.L,
                       (int)g.gene_blocks, (int)ntiles, gs, d_partial);
  }
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

extern "C" {

int64_t scoary_mfma_max_isolates(void) { return kKSteps * 64; }
int64_t scoary_mfma_panels_bytes(int64_t G, int64_t N) {
  if (G < 1 || N < 1 || N > kKSteps * 64) return 0;
  return round_up(G, kBlockGenes) * (2 * kKSteps * 16);
}
int64_t scoary_mfma_bfrag_bytes(int64_t N, int64_t P, int64_t T) {
  if (N < 1 || N > kKSteps * 64 || P < 1 || T < 1) return 0;
  return T * ((P + 63) / 64) * kStageBytes;
}
int64_t scoary_mfma_breakeven_entries(void) { return (int64_t)std::ceil(kMfmaNsPerGene / kListNsPerEntry); }

int scoary_mfma_panels_build(scoary_handle h, const uint32_t* d_tiled, int64_t G, int64_t N, const int32_t* d_order,
                             const uint8_t* d_flipped, void* d_panels, scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (!d_tiled || !d_order || !d_flipped || !d_panels || G < 1 || N < 1)
    return fail(h, SCOARY_ERR_ARG, "scoary_mfma_panels_build: bad argument");
  if (N > kKSteps * 64 || G > 0x7fffffffLL - kBlockGenes)
    return fail(h, SCOARY_ERR_SIZE, "scoary_mfma_panels_build: N > 2048 or G >= 2^31");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t total = scoary_mfma_panels_bytes(G, N) / 16;
  KernelTimer kt(h, s, "k_mfma_panels");
  hipLaunchKernelGGL(k_mfma_panels, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_tiled,
                     scoary_tiled_genes(G), (int)G, (int)N, d_order, d_flipped, total, static_cast<v4i*>(d_panels));
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

int scoary_mfma_plan(int num_cu, int64_t k_split, int64_t T, int64_t P, int64_t* out) {
  if (num_cu < 1 || k_split < 1 || T < 1 || P < 1 || !out) return SCOARY_ERR_ARG;
  const MfmaGeom g = scoary_mfma_geom(num_cu, k_split, T, P, (P + 511) / 512);
  out[0] = g.gene_blocks, out[1] = g.ranges, out[2] = g.L, out[3] = g.blocks;
  return SCOARY_OK;
}

int scoary_set_mfma_route(scoary_handle h, int mode) {
  if (!h) return SCOARY_ERR_ARG;
  if (mode < SCOARY_MFMA_ROUTE_NONE || mode > SCOARY_MFMA_ROUTE_AUTO)
    return fail(h, SCOARY_ERR_ARG, "scoary_set_mfma_route: mode is 0 (none), 1 (all) or 2 (auto)");
  h->mfma_route = mode;
  return SCOARY_OK;
}

// AUTO: the whole number of 256-slot blocks that makes (the cost of its cheapest plan, scoary_mfma_geom) x (time
// of a stage) + (entries left to the lists) x kListNsPerEntry smallest.  Where a round of blocks
// is short against the whole this is the break-even length; the rounds term keeps the split off block counts
// that are a fraction over a multiple of the CU count (cfg3: 106 gene blocks x 10 traits = 4.1 rounds).
int64_t scoary_mfma_route(scoary_handle h, const int64_t* block_start, int64_t G, int64_t T, int64_t N, int64_t P) {
  if (!h || G < 1 || T < 1 || P < 1 || N < 1 || N > kKSteps * 64 || h->mfma_route == SCOARY_MFMA_ROUTE_NONE)
    return 0;
  if (h->mfma_route == SCOARY_MFMA_ROUTE_ALL) return G;
  if (!block_start) return 0;
  const int64_t nb = G / kBlockGenes, total = block_start[(G + kBlockGenes - 1) / kBlockGenes];
  const double tests = (double)T * (double)P / 1e5;
  const double stage_ns = kMfmaNsPerGene * h->num_cu * kBlockGenes * 64 / 1e5;   // one block, one stage
  double best = kListNsPerEntry * (double)total * tests;
  int64_t best_nb = 0;
  const std::vector<MfmaRange> cands = mfma_ranges(T, P, (P + 511) / 512);
  for (int64_t b = 1; b <= nb; ++b) {
    const MfmaGeom g = mfma_pick(cands, h->num_cu, b, (P + 63) / 64, T);
    if (g.blocks < h->num_cu) continue;            // less than one round of blocks over the CUs: lists
    const double cost = g.cost * stage_ns + kListNsPerEntry * (double)(total - block_start[b]) * tests;
    if (cost < best) best = cost, best_nb = b;
  }
  return best_nb * kBlockGenes;
}

}  // extern "C"
