// scoary_rank_shift.hip -- the Hodges-Lehmann shift of the rank-sum test and its distribution-free confidence limits
// (spec S19 of DESIGN.md): order statistics of the K = m (n - m) differences d_ij = fl(x_i - x_j), carrier i minus
// non-carrier j, of every (trait, gene), selected by counting -- the differences are never written anywhere.
//
// The host sorts a trait's valid values once (engine.ranksum_shift_plan): xs = the values ascending, pos = the
// isolate at each sorted position.  A double maps to an order-preserving 64-bit key; the d-th smallest difference is
// the smallest key k with count(value of k) >= d, count(v) = #{(i, j) : d_ij <= v}, found by bisection over the keys
// between the smallest and the largest difference the trait can have.  No candidate list, no tolerance: when the
// bracket is one key wide the key is the answer.
//
//   k_rank_shift   block = one trait's xs in LDS and W wavefronts, a gene per wavefront at a time.  The wavefront
//                  gathers the gene's bits into sorted order (ballot), takes prefix popcounts of them and lists the
//                  sorted positions of the smaller of carriers and non-carriers (the "walked" side).  count(v) is a
//                  sum over the walked side: the lanes take its members in turn, each finds by binary search over xs
//                  -- the predicate fl(x_i - xs[p]) <= v is monotone in p -- where the other side's members begin or
//                  end to count, and the prefix popcounts turn that boundary into their number.  The four order
//                  statistics (lower limit, the two middle ones, upper limit) share the loop: every count narrows
//                  every bracket it can, and brackets that coincide are counted once.
#include "scoary_common.hpp"

namespace {

constexpr int kShiftMaxIsolates = 16320;          // = scoary_ranksum_max_isolates()
constexpr int kShiftMaxWaves = 16;
constexpr int kShiftLdsBytes = 160 * 1024 - 64;   // dynamic LDS of a block (the 64: the kernel's static LDS)

// LDS of a block: xs, then per wavefront the bit words, their exclusive prefix popcounts and the walked positions
__host__ __device__ constexpr int shift_words(int N) { return 2 * ((N + 64) / 64); }         // covers word N >> 5
__host__ __device__ constexpr int shift_xs_bytes(int N) { return (8 * N + 15) / 16 * 16; }
__host__ __device__ constexpr int shift_wave_bytes(int N) {
  return (8 * shift_words(N) + 2 * (N / 2 + 1) + 15) / 16 * 16;
}
// wavefronts of a block: the largest power of two, 16 at the most, whose lists fit next to xs
__host__ __device__ constexpr int shift_waves(int N) {
  int w = kShiftMaxWaves;
  while (w > 1 && shift_xs_bytes(N) + w * shift_wave_bytes(N) > kShiftLdsBytes) w >>= 1;
  return w;
}
static_assert(shift_xs_bytes(kShiftMaxIsolates) + shift_wave_bytes(kShiftMaxIsolates) <= kShiftLdsBytes &&
                  shift_waves(1) == kShiftMaxWaves,
              "a block holds xs and at least one wavefront's lists at every N the rank-sum stage takes");
// a lane's count: at most (8160 / 64 + 1) members x 8160 < 2^21; a wavefront's: at most K
static_assert((int64_t)(kShiftMaxIsolates / 2) * (kShiftMaxIsolates / 2) < (1LL << 27), "K fits 27 bits");

// order-preserving key of a double that is not NaN, and back
__device__ __forceinline__ uint64_t shift_key(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double shift_value(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}
// a value every lane holds alike, in scalar registers
__device__ __forceinline__ uint64_t shift_uniform(uint64_t x) {
  const uint32_t l = __builtin_amdgcn_readfirstlane((uint32_t)x), u = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
  return ((uint64_t)u << 32) | l;
}

// a wavefront's LDS writes before, its LDS reads behind: LDS serves a wavefront's accesses in the order they were
// issued, so this only has to keep the compiler from moving them
__device__ __forceinline__ void shift_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int shift_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return __builtin_amdgcn_readfirstlane(v);
}

// word w of a trait's validity row, isolates >= N cleared
__device__ __forceinline__ uint32_t shift_valid_word(const uint32_t* __restrict__ vrow, int w, int N) {
  uint32_t v = vrow[w];
  if (32 * w + 32 > N) v &= (1u << (N - 32 * w)) - 1u;
  return v;
}

// What the walked member with the value xv adds to count(v).  q = how many sorted positions p < n are on the "low"
// side of the predicate (a prefix: xs ascends and fl is monotone), found in log2(top) + 1 probes of xs.  Carriers
// walked (flip 0): the non-carriers at q and behind count, those whose value is large enough for fl(xv - xs[p]) <= v.
// Non-carriers walked (flip 1): the carriers before q count, those whose value is small enough for
// fl(xs[p] - xv) <= v.
__device__ __forceinline__ int shift_term(const double* xs, const uint32_t* bits, const uint32_t* pre, int n, int top,
                                          bool flip, int nwalk, double xv, double v) {
  int q = 0;
  for (int step = top; step > 0; step >>= 1) {
    const int c = q + step;
    const double y = xs[min(c, n) - 1];
    const double d = flip ? y - xv : xv - y;
    const bool low = flip ? d <= v : !(d <= v);
    if (c <= n && low) q = c;
  }
  const int cc = (int)pre[q >> 5] + __popc(bits[q >> 5] & ((1u << (q & 31)) - 1u));   // carriers before q
  const int cw = flip ? q - cc : cc;                                                 // walked members before q
  return flip ? q - cw : (n - q) - (nwalk - cw);
}

__global__ __launch_bounds__(kShiftMaxWaves * 64) void k_rank_shift(
    const uint32_t* __restrict__ tiled, int64_t Gp, int G, int N, int Wp, int W, const double* __restrict__ xs_all,
    const int32_t* __restrict__ pos_all, const uint32_t* __restrict__ valid, const int32_t* __restrict__ d_m,
    const double* __restrict__ d_var, double zq, double* __restrict__ d_shift, double* __restrict__ d_lower,
    double* __restrict__ d_upper, int64_t* __restrict__ d_ca) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int s_n;
  const int t = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* xs = reinterpret_cast<double*>(lds);
  unsigned char* mine = lds + shift_xs_bytes(N) + wave * shift_wave_bytes(N);
  const int nwa = shift_words(N);
  uint32_t* bits = reinterpret_cast<uint32_t*>(mine);
  uint32_t* pre = bits + nwa;
  uint16_t* walk = reinterpret_cast<uint16_t*>(pre + nwa);         // N / 2 + 1 entries

  const uint32_t* vrow = valid + (int64_t)t * Wp;
  const int nw = (N + 31) / 32;
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int i = tid; i < N; i += blockDim.x) xs[i] = xs_all[(int64_t)t * N + i];
  int cnt = 0;
  for (int w = tid; w < nw; w += blockDim.x) cnt += __popc(shift_valid_word(vrow, w, N));
  if (cnt) atomicAdd(&s_n, cnt);
  __syncthreads();                                 // the block's only barriers: from here on a wavefront is on its own
  const int n = __builtin_amdgcn_readfirstlane(min(s_n, N));
  const int32_t* pos = pos_all + (int64_t)t * N;
  int top = 1;
  while (2 * top <= n) top <<= 1;                  // the largest power of two <= n (1 where n < 2)
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  for (int64_t g64 = (int64_t)blockIdx.x * W + wave; g64 < G; g64 += (int64_t)gridDim.x * W) {
    const int g = (int)g64;
    const int64_t o = (int64_t)t * G + g;
    shift_wave_sync();                             // (the last gene's reads of the lists are behind us)
    // the gene's bits in sorted order, positions >= n clear
    for (int p0 = 0; p0 < 32 * nwa; p0 += 64) {
      const int p = p0 + lane;
      uint32_t bit = 0;
      if (p < n) {
        const int iso = min(max(pos[p], 0), N - 1);               // clamped: a bad plan reads inside the matrix
        bit = (tiled[((int64_t)(iso >> 7) * Gp + g) * 4 + ((iso >> 5) & 3)] >> (iso & 31)) & 1u;
      }
      const uint64_t b = __ballot(bit);
      if (lane == 0) bits[p0 >> 5] = (uint32_t)b, bits[(p0 >> 5) + 1] = (uint32_t)(b >> 32);
    }
    shift_wave_sync();
    int m = 0;                                     // exclusive prefix popcounts, 64 words a round
    for (int w0 = 0; w0 < nwa; w0 += 64) {
      const bool in = w0 + lane < nwa;
      const int c = in ? __popc(bits[w0 + lane]) : 0;
      int x = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
      }
      if (in) pre[w0 + lane] = (uint32_t)(m + x - c);
      m += __shfl(x, 63);
    }
    m = __builtin_amdgcn_readfirstlane(m);
    const double var = d_var[o];
    if (m != d_m[o]) {                             // not the plan of these genes and values
      if (lane == 0) d_shift[o] = nan, d_lower[o] = nan, d_upper[o] = nan, d_ca[o] = 0;
      continue;
    }
    if (!(var > 0.0) || m <= 0 || m >= n) {        // S15's untestable genes
      if (lane == 0) d_shift[o] = 0.0, d_lower[o] = -inf, d_upper[o] = inf, d_ca[o] = 0;
      continue;
    }
    const bool flip = 2 * m > n;                   // walk the smaller side
    const int nwalk = flip ? n - m : m;            // <= n / 2 <= N / 2
    for (int w = lane; 32 * w < n; w += 64) {
      uint32_t word = bits[w];
      int off = (int)pre[w];
      if (flip) {
        word = ~word;
        if (32 * w + 32 > n) word &= (1u << (n - 32 * w)) - 1u;
        off = 32 * w - off;
      }
      while (word) {
        walk[min(off, N / 2)] = (uint16_t)(32 * w + __builtin_ctz(word));
        ++off;
        word &= word - 1u;
      }
    }
    shift_wave_sync();

    const int64_t K = (int64_t)m * (int64_t)(n - m);
    const double half_k = 0.5 * (double)K;
    const double sd = sqrt(var);
    const double zs = zq * sd;
    int64_t ca = (int64_t)shift_uniform((uint64_t)(int64_t)floor(half_k - zs));
    ca = min(ca, K / 2);
    const bool limits = ca >= 1;
    // the ranks wanted, ascending: lower limit, the two middle ones, upper limit (without limits: the middle ones)
    const int64_t r1 = (K - 1) / 2 + 1, r2 = K / 2 + 1;
    const int64_t rk[4] = {limits ? ca : r1, r1, r2, limits ? K + 1 - ca : r2};
    // every difference lies between fl(xs[0] - xs[n-1]) and fl(xs[n-1] - xs[0]): finite keys, count(hi) = K
    const uint64_t lo0 = shift_uniform(shift_key(xs[0] - xs[n - 1])), hi0 = shift_uniform(shift_key(xs[n - 1] - xs[0]));
    uint64_t lo[4] = {lo0, lo0, lo0, lo0}, hi[4] = {hi0, hi0, hi0, hi0};

    for (int it = 0; it < 66; ++it) {              // (a bracket halves every round: 64 rounds at the most)
      bool act[4];
      double v[4];
      uint64_t mid[4];
      bool any = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        mid[k] = lo[k] + ((hi[k] - lo[k]) >> 1);
        v[k] = shift_value(mid[k]);
        act[k] = lo[k] < hi[k] && !(k > 0 && lo[k] == lo[k - 1] && hi[k] == hi[k - 1]);
        any = any || lo[k] < hi[k];
      }
      if (!any) break;
      int c[4] = {0, 0, 0, 0};
      for (int i = lane; i < nwalk; i += 64) {
        const double xv = xs[min((int)walk[i], n - 1)];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (act[k]) c[k] += shift_term(xs, bits, pre, n, top, flip, nwalk, xv, v[k]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!act[k]) continue;
        const int64_t ck = shift_wave_sum(c[k]);
        // count(v) is monotone in the key: the count at mid[k] narrows every bracket that holds mid[k]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (ck >= rk[j]) {
            if (mid[k] < hi[j]) hi[j] = max(mid[k], lo[j]);
          } else {
            if (mid[k] >= lo[j]) lo[j] = min(mid[k] + 1, hi[j]);
          }
        }
      }
    }
    if (lane == 0) {
      double s[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s[k] = shift_value(hi[k]);
        if (s[k] == 0.0) s[k] = 0.0;               // a zero difference is +0.0
      }
      const double sum = s[1] + s[2];
      double sh = sum * 0.5;
      if (sh == 0.0) sh = 0.0;
      d_shift[o] = sh;
      d_lower[o] = limits ? s[0] : -inf;
      d_upper[o] = limits ? s[3] : inf;
      d_ca[o] = ca;
    }
  }
}

}  // namespace

extern "C" {

int64_t scoary_rank_shift_waves(int64_t N) {
  return N >= 1 && N <= kShiftMaxIsolates ? shift_waves((int)N) : 0;
}

int scoary_ranksum_shift(scoary_handle h, const uint32_t* d_tiled, const double* d_xs, const int32_t* d_pos,
                         const uint32_t* d_valid, const int32_t* d_m, const double* d_var, double zq, int64_t G,
                         int64_t T, int64_t N, double* d_shift, double* d_lower, double* d_upper, int64_t* d_ca,
                         scoary_stream_t stream) {
  if (!h) return SCOARY_ERR_ARG;
  if (int rc = check_args(h, "scoary_ranksum_shift",
                          d_tiled && d_xs && d_pos && d_valid && d_m && d_var && d_shift && d_lower && d_upper &&
                              d_ca && zq > 0.0 && zq < 1e300 && G >= 1 && T >= 1 && N >= 1))
    return rc;
  if (N > kShiftMaxIsolates)
    return fail(h, SCOARY_ERR_SIZE, "scoary_ranksum_shift: more isolates than scoary_ranksum_max_isolates()");
  if (T > 65535 || G > 0x7fffffffLL - 256)
    return fail(h, SCOARY_ERR_SIZE, "scoary_ranksum_shift: T > 65535 or G >= 2^31");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int W = shift_waves((int)N);
  const int lds_bytes = shift_xs_bytes((int)N) + W * shift_wave_bytes((int)N);
  // more than 64 KB of dynamic LDS need the opt-in; asked for at every launch, so that the handle keeps no state
  HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rank_shift),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kShiftLdsBytes));
  // a wavefront takes the genes blockIdx.x W + wave, + gridDim.x W, ...: enough blocks for four rounds over the CUs,
  // so that xs is loaded a few times per CU and not once per gene, and no more blocks than there are genes for
  const int64_t per_trait = std::max<int64_t>(1, (4 * (int64_t)h->num_cu + T - 1) / T);
  const int64_t nblk = std::min<int64_t>((G + W - 1) / W, per_trait);
  KernelTimer kt(h, s, "k_rank_shift");
  hipLaunchKernelGGL(k_rank_shift, dim3((unsigned)nblk, (unsigned)T), dim3(W * 64), lds_bytes, s, d_tiled,
                     scoary_tiled_genes(G), (int)G, (int)N, (int)scoary_row_words(N), W, d_xs, d_pos, d_valid, d_m,
                     d_var, zq, d_shift, d_lower, d_upper, d_ca);
  HIP_TRY(h, hipGetLastError());
  return SCOARY_OK;
}

}  // extern "C"
