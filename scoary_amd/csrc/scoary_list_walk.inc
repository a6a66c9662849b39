// scoary_list_walk.inc -- the list walk of the list-driven permutation kernels, included into
// the body of k_permute_lists and k_permute_seglists (scoary_lists.hip): adds the tile rows of
// one wave group's index list into the bit-sliced counter planes c0..c3.
// Expects in scope: LPG, NW, KC (template parameters); cur (Group), ring[4] (the group's first
// four index vectors, already requested), nhalf, nsuper, colb, lane_off; c0..c3[16];
// kVecSub = sub-steps (of 4 entries per gene) one 16-byte index vector feeds -- LPG in
// k_permute_lists (32-bit entries, lane h of a gene's group holds sub-step h's four), 2 in
// k_permute_seglists (eight 16-bit entries per lane) -- and the macro SCOARY_READ4(H, X, E):
// issue the four tile-row reads of sub-step H of vector E into X.
// Textual include on purpose: the counter planes are pinned physical registers and the walk
// is one basic-block chain the scheduler must see whole.
    Rows4 xa, xb;
    auto s4 = [&](const Rows4& x) -> Carry4 {
      Carry4 b;
      b.w[0] = sum4<0>(c0, x.w0);
      b.w[1] = NW > 1 ? sum4<1>(c1, x.w1) : 0u;
      if constexpr (NW > 2) {
        b.w[2] = sum4<2>(c2, x.w2);
        b.w[3] = sum4<3>(c3, x.w3);
      } else {
        b.w[2] = b.w[3] = 0u;
      }
      return b;
    };
#define FA4(PLANE, A, B)                                               \
  Carry4 {                                                             \
    {                                                                  \
      full_add<0, PLANE>(c0[PLANE], (A).w[0], (B).w[0]),               \
          NW > 1 ? full_add<1, PLANE>(c1[PLANE], (A).w[1], (B).w[1]) : 0u, \
          NW > 2 ? full_add<2, PLANE>(c2[PLANE], (A).w[2], (B).w[2]) : 0u, \
          NW > 2 ? full_add<3, PLANE>(c3[PLANE], (A).w[3], (B).w[3]) : 0u  \
    }                                                                  \
  }
    // pieces of 4*LPG entries; the index loads run three pieces ahead in a ring of
    // four vectors (a region of four steps is a multiple of four pieces, so the ring
    // slot of every piece is a compile-time constant).  Reads past the end of the
    // list re-read its last piece (valid rows, never summed).
    int piece = 0;                                   // piece whose vector is ring[piece % 4]
    auto load_piece = [&](int p) -> Ent { return load_from(cur, lane_off, p); };
    SCOARY_READ4(0, xa, ring[0].e);
    // sub-step S of step K (both literals): issue the reads of the next sub-step into
    // `other`, sum `mine`
#define SUBSTEP(K, S, MINE, OTHER)                                          \
  [&]() -> Carry4 {                                                         \
    constexpr int kSub = (K) * 8 + (S);          /* sub-step within the region */ \
    constexpr int kCur = (kSub / kVecSub) % 4;   /* ring slot in use */           \
    constexpr int Hn = (kSub + 1) % kVecSub;                                 \
    if constexpr (Hn == 0) {                     /* piece finished: refill its slot */ \
      ring[kCur] = load_piece(piece + 4);                                    \
      ++piece;                                                               \
      SCOARY_READ4(0, OTHER, ring[(kCur + 1) % 4].e);                         \
    } else {                                                                 \
      SCOARY_READ4(Hn, OTHER, ring[kCur].e);                                  \
    }                                                                        \
    return s4(MINE);                                                         \
  }()
    // Carries are kept pending level by level (weights 4, 8, ..., 64 inside a region of four
    // steps) and only the top one ripples through the upper planes.  kDeep: one more pending
    // level -- regions of eight steps, the two weight-128 carries meet in plane 7 and the
    // ripple starts at plane 8 -- where the four extra VGPRs are available.
    constexpr bool kDeep = LPG == 4;
    constexpr int kRegion = kDeep ? 8 : 4;
    const Carry4 zero = {{0u, 0u, 0u, 0u}};
    for (int sg = 0; sg < nsuper; sg += kRegion) {
#define STEP(K)                                   /* 32 listed isolates */ \
  [&]() -> Carry4 {                                                         \
    const int left = nhalf - 2 * (sg + (K));     /* half-steps left, wave-uniform */ \
    if (left <= 0) return zero;                                             \
    const Carry4 b0 = SUBSTEP(K, 0, xa, xb);                                \
    const Carry4 b1 = SUBSTEP(K, 1, xb, xa);                                \
    const Carry4 d0 = FA4(2, b0, b1);                                       \
    const Carry4 b2 = SUBSTEP(K, 2, xa, xb);                                \
    const Carry4 b3 = SUBSTEP(K, 3, xb, xa);                                \
    const Carry4 d1 = FA4(2, b2, b3);                                       \
    const Carry4 e0 = FA4(3, d0, d1);                                       \
    Carry4 e1 = zero;                                                       \
    if (left > 1) {                              /* the second 16 entries exist */ \
      const Carry4 b4 = SUBSTEP(K, 4, xa, xb);                              \
      const Carry4 b5 = SUBSTEP(K, 5, xb, xa);                              \
      const Carry4 d2 = FA4(2, b4, b5);                                     \
      const Carry4 b6 = SUBSTEP(K, 6, xa, xb);                              \
      const Carry4 b7 = SUBSTEP(K, 7, xb, xa);                              \
      const Carry4 d3 = FA4(2, b6, b7);                                     \
      e1 = FA4(3, d2, d3);                                                  \
    }                                                                       \
    return FA4(4, e0, e1);                       /* weight 32 */            \
  }()
#define QUAD(K0)                                  /* four steps -> carry of weight 128 */ \
  [&]() -> Carry4 {                                                         \
    const Carry4 f0 = STEP(K0), f1 = STEP((K0) + 1);                        \
    const Carry4 g0 = FA4(5, f0, f1);                                       \
    const Carry4 f2 = STEP((K0) + 2), f3 = STEP((K0) + 3);                  \
    const Carry4 g1 = FA4(5, f2, f3);                                       \
    return FA4(6, g0, g1);                                                  \
  }()
      Carry4 carry = QUAD(0);
      if constexpr (kDeep) {
        const Carry4 h1 = sg + 4 < nsuper ? QUAD(4) : zero;
        carry = FA4(7, carry, h1);
      }
#define RIPPLE(K)                                                       \
  if constexpr (K < KC && K >= (kDeep ? 8 : 7)) {                       \
    Carry4 nc = {{c0[K] & carry.w[0], c1[K] & carry.w[1], c2[K] & carry.w[2], c3[K] & carry.w[3]}}; \
    Ctr<0, K>::xor2(c0[K], carry.w[0]);                                 \
    if constexpr (NW > 1) Ctr<1, K>::xor2(c1[K], carry.w[1]);           \
    if constexpr (NW > 2) {                                             \
      Ctr<2, K>::xor2(c2[K], carry.w[2]);                               \
      Ctr<3, K>::xor2(c3[K], carry.w[3]);                               \
    }                                                                   \
    carry = nc;                                                         \
  }
      RIPPLE(7) RIPPLE(8) RIPPLE(9) RIPPLE(10) RIPPLE(11) RIPPLE(12) RIPPLE(13) RIPPLE(14) RIPPLE(15)
#undef RIPPLE
    }
#undef QUAD
#undef STEP
#undef SUBSTEP
#undef FA4
