#pragma once
// vbn_walk_kde.h -- the kde CPD step: distance passes, index search, moment tables (part of
// vbn_walk_impl.h).
#include "vbn_walk_cpd.h"

// ------------------------------------------------------------------------------------------
// kde (kde.py:105-182)
//   points at off_pts: [M][stride] = parents[dp] ++ targets[D]
//   tail: inv_sp, inv_sy, noise_scale, cy, log_n;  aux0 = dp, aux1 = stride
// Weights are taken relative to the kernel's peak (exp(-q/2) <= 1); if every weight of a
// particle underflows the pass is redone relative to the particle's nearest point.
// ------------------------------------------------------------------------------------------
// squared scaled distance to point ``pt`` over the parent dims.  DP >= 0: parent values in
// registers (pv); DP < 0: generic count, parent values re-read from LDS.
template <int DP>
__device__ __forceinline__ float kde_qp(const float* __restrict__ pt, const float (&pv)[4], float inv,
                                        int dp, const vbn_walk_args& A, const vbn_step& st, const Lane& L) {
  float q = 0.f;
  if (DP >= 0) {
#pragma unroll
    for (int i = 0; i < (DP >= 0 ? DP : 0); ++i) {
      const float df = (pv[i] - pt[i]) * inv;
      q = fmaf(df, df, q);
    }
  } else {
    for (int i = 0; i < dp; ++i) {
      const float df = (vread(L, L.ic[st.in_off + i]) - pt[i]) * inv;
      q = fmaf(df, df, q);
    }
  }
  return q;
}

template <int DY>
__device__ __forceinline__ float kde_qy(const float* __restrict__ pty, float x0, float inv, int D,
                                        const vbn_step& st, const Lane& L) {
  if (DY == 1) {
    const float df = (x0 - pty[0]) * inv;
    return df * df;
  }
  float q = 0.f;
  for (int d = 0; d < D; ++d) {
    const float df = (vread(L, st.out_col + d) - pty[d]) * inv;
    q = fmaf(df, df, q);
  }
  return q;
}

// ---- pairwise kernel weights on MFMA ------------------------------------------------------
// The kernel weight of particle n and stored point m is exp(-|x_n - y_m|^2 / (2 s^2)) =
// exp2(-|x'_n - y'_m|^2) with x' = c x, y' = c y, c = sqrt(log2(e) / 2) / s, and
//   -|x' - y'|^2 = sum_k (2 x'_k) y'_k - |y'|^2 - |x'|^2,
// a contraction over K <= 4 features, computed on bf16 MFMAs from exact three-way splits
// (kde_b32_sums below) for the inverse-CDF chunk sums and the log-density sums alike.
// Padding points have |y'|^2 = 1e30 -> weight 0.  The wave's 64 particles are 2 tiles of 32
// (tile t = particles 32t .. 32t+31); D layout: lane l holds points 8j + 4(l>>5) + i (j, i < 4)
// of the block for particle 32t + (l&31).  Bound: v_exp_f32 issue (one exp per pair).  The inverse-CDF scan
// recomputes its chunk's weights with kde_arg_rec, the float32 chain of the same contraction
// (equal to the MFMA sums to f32 rounding; a crossing past the chunk end is clamped, kde_scan).
// the lane's own particle: x'_k and -|x'|^2 exactly as kde_b32_ops computes them
__device__ __forceinline__ float kde_own(const Lane& L, const int (&slots)[4], const float (&scl)[4], int nf,
                                         float (&xv)[4]) {
  float sq = 0.f;
  for (int f = 0; f < nf; ++f) {
    const float v = scl[f] * vread(L, slots[f]);
    xv[f] = v;
    sq = fmaf(v, v, sq);
  }
  return -sq;
}

// VALU form of one pair's argument (a k-ordered fmaf chain), point record r =
// (y'_0 .. y'_{nf-1}, |y'|^2, ..) of the per-point record pack.
__device__ __forceinline__ float kde_arg_rec(const float4 r, float xb0, float xb1, float xb2, float negsq,
                                             int nf) {
  const bool zc = nf <= 2;
  float d = zc ? 0.f : negsq;
  d = fmaf(r.x, xb0, d);
  d = nf > 1 ? fmaf(r.y, xb1, d) : d;
  d = nf > 2 ? fmaf(r.z, xb2, d) : d;
  const float y2 = nf == 1 ? r.y : (nf == 2 ? r.z : r.w);
  d = fmaf(y2, -1.f, d);
  return zc ? fmaf(1.f, negsq, d) : d;
}

// 16-point blocks per chunk: a multiple of 4, so a chunk is a whole number of the MFMA pass's
// KDE_PF = 2 blocks of 32 points (the host pads the packs to KDE_CHUNKS * kde_cb(M) 16-point
// blocks)
__device__ __forceinline__ int kde_cb(int M) {
  const int nblk = (M + 15) >> 4;
  return (((nblk + KDE_CHUNKS - 1) / KDE_CHUNKS) + 3) & ~3;
}

// Point operands are prefetched a whole trip ahead, across chunk boundaries: the packs of a
// 64-node M = 10,000 DAG do not stay in one XCD's 4 MiB L2 while ~4,000 resident waves walk
// different nodes, so most operand loads are served by the Infinity Cache (cfg4: 78 GB of L2
// fills per launch, r04 PMC), ~545+ cycles away.  Measured not to cost time: re-reading only
// the first 32 blocks of every pack (VBN_ABL_L2FIT, L2-resident) ran 202.5 vs 201.0 ms.

#ifdef VBN_ABL_L2FIT
#define KDE_BLK(x) ((x) & 31)        // ablation: every pass re-reads its node's first 32 blocks
#else
#define KDE_BLK(x) (x)
#endif

// Pass-1 sums on v_mfma_f32_32x32x16_bf16 ("bf16x3", round 5): rows = 32 points, columns =
// the 32 particles of tile t (particles 32 t .. 32 t + 31), K = 16 slots (one MFMA, nf = 1) or
// 32 (two chained MFMAs, nf = 2..4).  Every f32 operand is split into three bf16 whose sum is
// it exactly (hi = bf16(v), mid = bf16(v - hi), lo = the 8-bit rest); per feature f the six
// products u_h y_h, u_h y_m, u_m y_h, u_h y_l, u_l y_h, u_m y_m (u = 2x' on the B side, y' on
// the A side, slots 6f .. 6f+5; the omitted ones are < 2^-25 of u y) are exact in f32,
// |y'|^2's three parts (slots 6nf .. +2) meet -1 and 1.0 (6nf+3 .. +5) meets -|x'|^2's three
// parts, so the MFMA's f32 sum from C = 0 is the contraction -|x' - y'|^2 to f32 rounding
// (tests/test_plan.py).  Against round 4's v_mfma_f32_16x16x32_bf16 tiles the wave issues a
// quarter of the MFMAs per pair (one 32x32x16 per 1,024 pairs instead of four 16x16x32, each
// holding the SIMD's vector issue for 8 cycles) and reads 32 instead of 64 bytes per point
// for nf = 1; the 16 exps per lane and MFMA are summed with plain f32 adds (4 accumulators
// per tile; packed f32 adds beside MFMAs cost extra issue cycles, MI355X_MICROARCH.md).
// A = host pack (plan.py _kde_pack_b32) [block of 32][K group g][64 lanes][8]: lane l loads
// point l & 31's slots 16 g + 8 (l >> 5) .. +7 (16 B, 1 KiB per wave, block and K group);
// B = kde_b32_ops; D: lane l holds rows 8 j + 4 (l >> 5) + i (j, i < 4) of column l & 31.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <int KG>
struct KdeB32 {
  bf16x8 b[2][KG];  // tile t: particle 32 t + (lane & 31), slots 16 g + 8 (lane >> 5) .. +7
};

__device__ __forceinline__ void bf16_split3(float v, __bf16 (&p)[3]) {
  p[0] = (__bf16)v;
  const float r1 = v - (float)p[0];
  p[1] = (__bf16)r1;
  p[2] = (__bf16)(r1 - (float)p[1]);
}

// slot k of the B operand: feature splits sp (_BF16_B pattern), -1 x 3, split of -|x'|^2 (zero
// in the factored form: the A side's 1.0 slots then contribute nothing), 0
__device__ __forceinline__ __bf16 kde_bslot(int k, int nf, const __bf16 (&sp)[4][3], const __bf16 (&sx)[3],
                                            bool fform) {
  constexpr int pat[6] = {0, 0, 1, 0, 2, 1};
  const int f = k / 6;
  if (f < nf) return sp[f][pat[k - 6 * f]];
  const int r = k - 6 * nf;
  if (r < 3) return (__bf16)-1.f;
  if (r < 6 && !fform) return sx[r - 3];
  return (__bf16)0.f;
}

// the lane's particle side of tile t; -|x'|^2 exactly as kde_own accumulates it
template <int KG>
__device__ __forceinline__ void kde_b32_ops(const Lane& L, const int (&slots)[4], const float (&scl)[4], int nf,
                                            bool fform, KdeB32<KG>& o) {
  const int h = L.lane >> 5, n = L.lane & 31;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float sq = 0.f;
    __bf16 sp[4][3], sx[3];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const float v = f < nf ? scl[f] * L.vals[slots[f] * WAVE + 32 * t + n] : 0.f;
      if (f < nf) sq = fmaf(v, v, sq);
      bf16_split3(2.f * v, sp[f]);
    }
    bf16_split3(-sq, sx);
#pragma unroll
    for (int g = 0; g < KG; ++g) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const __bf16 v0 = kde_bslot(16 * g + j, nf, sp, sx, fform);
        const __bf16 v1 = kde_bslot(16 * g + 8 + j, nf, sp, sx, fform);
        o.b[t][g][j] = h ? v1 : v0;
      }
    }
  }
}

// Sum over a chunk's 32-point blocks of the lane's tile partials: lane l receives the total of
// particle l (tile l >> 5, column l & 31): one cross-lane move.
__device__ __forceinline__ float kde_reduce_tiles(const float (&s)[2], int lane) {
  const int h = lane >> 5;
  const float k = h ? s[1] : s[0], o = h ? s[0] : s[1];
  return k + __shfl_xor(o, 32);
}

// One tile of one 32-point block: KG chained MFMAs (C = 0)
template <int KG>
__device__ __forceinline__ f32x16 kde_b32_tile(const bf16x8 (&a)[KG], const bf16x8 (&b)[KG]) {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  f32x16 d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], z, 0, 0, 0);
  if constexpr (KG == 2) d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], d, 0, 0, 0);
  return d;
}

// A tile's 16 exps summed into its 4 accumulators (in the order i = 0 .. 15, so the same sums
// whatever the MFMA schedule)
template <int KG>
__device__ __forceinline__ void kde_b32_exps(const f32x16& d, float (&acc)[4]) {
  if constexpr (KG == 1) {
    // f32x2 adds, one v_pk_add_f32 per two exps: 0.69 vs 0.63 of the exp-issue peak with
    // plain adds (profiles/microbench/kde_pass1.hip w1p / w1s); beside the denser chained
    // MFMAs of K = 32 they gain nothing (w2u 0.600 vs w2t 0.597), so that form keeps plain adds
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
      f32x2 p0 = f32x2{acc[0], acc[1]}, p1 = f32x2{acc[2], acc[3]};
      p0 += f32x2{__builtin_amdgcn_exp2f(d[i]), __builtin_amdgcn_exp2f(d[i + 1])};
      p1 += f32x2{__builtin_amdgcn_exp2f(d[i + 2]), __builtin_amdgcn_exp2f(d[i + 3])};
      acc[0] = p0.x; acc[1] = p0.y; acc[2] = p1.x; acc[3] = p1.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i & 3] += __builtin_amdgcn_exp2f(d[i]);
  }
}

// block b's operands (clamped to the pack's last block; pa = pack + lane; PG = the pack's K
// groups per block: the factored form of two features reads group 0 of a K = 32 pack)
template <int KG, int PG>
__device__ __forceinline__ void kde_b32_load(const bf16x8* __restrict__ pa, int b, int blast, bf16x8 (&a)[KG]) {
  const int bb = KDE_BLK(min(b, blast));
#pragma unroll
  for (int g = 0; g < KG; ++g) a[g] = pa[(bb * PG + g) * 64];
}

// In flight across a node's blocks (and its chunks): the operands of the next KDE_PF blocks
// (a ring: block b's set is reloaded with block b + KDE_PF once its last MFMA is issued) and
// the tile-0 result of the next block.  The walk is tile-pipelined: tile i + 1's MFMAs are
// issued before tile i's exps, so no exp waits on its MFMA (microbenchmark w1u 0.707 vs w1p
// 0.690, w2t 0.597 vs w2s 0.588 of the exp-issue peak), with two tile results live as before.
#define KDE_PF 2             // kde_cb keeps every chunk a multiple of 2 blocks of 32 points
template <int KG>
struct KdeTrip {
  bf16x8 x[KDE_PF][KG];
  f32x16 d0;                 // tile 0 of the next block
};

template <int KG, int PG>
__device__ __forceinline__ void kde_b32_prefetch(const bf16x8* __restrict__ pa, int b0, int blast,
                                                 const KdeB32<KG>& o, KdeTrip<KG>& q) {
#pragma unroll
  for (int u = 0; u < KDE_PF; ++u) kde_b32_load<KG, PG>(pa, b0 + u, blast, q.x[u]);
  q.d0 = kde_b32_tile<KG>(q.x[0], o.b[0]);
}

// per-lane tile partial sums of exp2(arg) over 32-point blocks [b0, b1), b1 - b0 a multiple of
// KDE_PF (kde_cb); q holds block b0's tile 0 and the operands of blocks b0, b0 + 1
template <int KG, int PG>
__device__ __forceinline__ void kde_b32_sums(const bf16x8* __restrict__ pa, int b0, int b1, int blast,
                                             const KdeB32<KG>& o, float (&s)[2], KdeTrip<KG>& q) {
  float acc[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[t][i] = 0.f;
  for (int b = b0; b < b1; b += KDE_PF) {
#pragma unroll
    for (int u = 0; u < KDE_PF; ++u) {
      const f32x16 d1 = kde_b32_tile<KG>(q.x[u], o.b[1]);              // block b + u, tile 1
      kde_b32_load<KG, PG>(pa, b + u + KDE_PF, blast, q.x[u]);
      kde_b32_exps<KG>(q.d0, acc[0]);                                   // block b + u, tile 0
      q.d0 = kde_b32_tile<KG>(q.x[(u + 1) % KDE_PF], o.b[0]);           // block b + u + 1, tile 0
      kde_b32_exps<KG>(d1, acc[1]);
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) s[t] += (acc[t][0] + acc[t][1]) + (acc[t][2] + acc[t][3]);
}

// The factored form (round 5).  Sampling needs the chunk sums only up to a per-particle
// factor, so they may be taken of exp2(2 x'.y' - |y'|^2) = 2^{|x'|^2} exp2(-|x' - y'|^2): the
// contraction drops -|x'|^2's three slots and fits K = 16 for two features (6 nf + 3 = 15)
// -- one MFMA per block instead of two chained ones, and the f32x2 adds (w1p, 0.69 vs w2s
// 0.59 of the exp-issue peak).  The particle's sums are then shifted by s = -|x'|^2 relative to
// the full form, and the record scan, the all-underflow rescue and the per-sample / per-query
// pre-passes all work on a' = 2 x'.y' - |y'|^2 minus a shift sigma (0 here, |x'|^2 in the full
// form, the largest a' after a rescue).  Used when every lane of the wave has |x'|^2 <=
// KDE_FFORM_MAX (no overflow: sums <= M 2^{|x'|^2}); otherwise the full form.
#define KDE_FFORM_MAX 96.f

// v_exp_f32 gives 0 for results below 2^-126 (no denormal results), so a sum of M weights whose
// largest lies near 2^-126 has silently lost up to M 2^-126 of its mass while still being > 0
// (measured: a log-density 0.058 too low where the sum was ~2^-123, tests/test_gpu_kde_paths.py).
// Below kde_tiny(M) = M 2^-109 -- where that loss could exceed 2^-17 of the sum -- a sum counts
// as underflowed, exactly like a sum of 0: the rescue / the shifted path takes the particle.
__device__ __forceinline__ float kde_tiny(int M) { return (float)M * 0x1p-109f; }

// Sub-chunks (round 6; VBN_ABL_NOHALVES: A/B without).  A wave's scan lasts as long as its
// slowest lane's, about half a chunk (the max over 64 lanes of the bidirectional walk).  Pass 1
// therefore also keeps KDE_NSUB - 1 prefix sums per chunk (a private array: the LDS rows are
// the occupancy budget -- 32 chunk rows instead cost 16 -> 12 waves per CU and ran slower), at
// block boundaries kde_sub_blocks(cb32, k) (multiples of KDE_PF, about k / KDE_NSUB of the
// chunk), and the scan covers the sub-chunk holding the threshold.  cfg4 plain plan, one box
// (profiles/r06_bench/r06i_ab_sub.txt): 88.86 ms -> 81.82 (halves) / 81.87 (quarters).
#ifndef KDE_NSUB
#define KDE_NSUB 2
#endif
#define KDE_HALF_MIN 16      // 32-point blocks per chunk below which a chunk is scanned whole
__device__ __forceinline__ int kde_sub_blocks(int cb32, int k) {
  return ((cb32 * k) / KDE_NSUB) & ~(KDE_PF - 1);
}

// Pass 1 of a node with nf features over its KDE_CHUNKS chunks: chunk sums -> scr[chunk][lane]
template <int KG, int PG>
__device__ __forceinline__ double kde_pass1(const bf16x8* __restrict__ pa, int cb32, const Lane& L,
                                            const int (&slots)[4], const float (&scl)[4], int nf, bool fform,
                                            float* __restrict__ hs = nullptr) {
  KdeB32<KG> o;
  kde_b32_ops<KG>(L, slots, scl, nf, fform, o);
  const int blast = KDE_CHUNKS * cb32 - 1;
  KdeTrip<KG> q;
  kde_b32_prefetch<KG, PG>(pa, 0, blast, o, q);
  double tot = 0.0;
  for (int ch = 0; ch < KDE_CHUNKS; ++ch) {
    float s[2] = {0.f, 0.f};
    if (hs) {                                         // the sub-chunk prefix sums on the way
      int b = ch * cb32;
#pragma unroll
      for (int k = 1; k < KDE_NSUB; ++k) {
        const int bk = ch * cb32 + kde_sub_blocks(cb32, k);
        kde_b32_sums<KG, PG>(pa, b, bk, blast, o, s, q);
        hs[ch * (KDE_NSUB - 1) + k - 1] = kde_reduce_tiles(s, L.lane);
        b = bk;
      }
      kde_b32_sums<KG, PG>(pa, b, ch * cb32 + cb32, blast, o, s, q);
    } else {
      kde_b32_sums<KG, PG>(pa, ch * cb32, ch * cb32 + cb32, blast, o, s, q);
    }
    const float cs = kde_reduce_tiles(s, L.lane);
    L.scr[ch * WAVE + L.lane] = cs;
    tot += (double)cs;
  }
  return tot;
}

// Sum over all nb32 blocks of a log-density pack (kde_logp_mfma)
template <int KG, int PG>
__device__ __forceinline__ float kde_sum_all(const bf16x8* __restrict__ pa, int nb32, const Lane& L,
                                             const int (&slots)[4], const float (&scl)[4], int nf, bool fform) {
  KdeB32<KG> o;
  kde_b32_ops<KG>(L, slots, scl, nf, fform, o);
  KdeTrip<KG> q;
  kde_b32_prefetch<KG, PG>(pa, 0, nb32 - 1, o, q);
  float s[2] = {0.f, 0.f};
  kde_b32_sums<KG, PG>(pa, 0, nb32, nb32 - 1, o, s, q);
  return kde_reduce_tiles(s, L.lane);
}

// the form of a pack of nf features: K groups read (KG), K groups per block of the pack (PG)
__device__ __forceinline__ float kde_sums_nf(const bf16x8* __restrict__ pa, int nb32, const Lane& L,
                                             const int (&slots)[4], const float (&scl)[4], int nf, bool fform) {
  if (nf == 1) return kde_sum_all<1, 1>(pa, nb32, L, slots, scl, nf, fform);
  if (nf == 2 && fform) return kde_sum_all<1, 2>(pa, nb32, L, slots, scl, nf, fform);
  return kde_sum_all<2, 2>(pa, nb32, L, slots, scl, nf, fform);
}

// Inverse-CDF scan of one chunk [j0, j1) (pass 2).  A lane whose threshold lies in the upper
// half of its chunk scans backwards from the end for the right-hand mass csum - rem: the
// point found is the same (the largest j with cum(j-1) <= rem), and no lane scans more than
// about half a chunk.  Backward lanes walk the reversed record copy forward, so every lane
// reads 4 consecutive records per trip with the next trip's 4 in flight (two named record sets,
// no register rotation) and no per-lane selects.  The weights exp2(arg(r)) (arg includes the
// shift) are summed in scan order (bit-identical running sums to a point-by-point scan); one
// compare per trip -- c > lim, with lim the float below the goal for backward lanes (c >= goal)
// -- and the crossing inside the trip is located after the loop; a crossing past the chunk end
// (rounding) is clamped to the chunk's last point.  rec: records (plan.py _kde_pack
// records=True), rev = reversed copy; M points.  Against round 4's form (selects inside the
// trip, a register rotation of the next records, the shift as a separate subtraction): cfg4
// plan kernel without precompute 143 -> 137 ms; trips of 8 records lost (145 ms,
// profiles/r05_bench/r05d_ab_scan.txt).
// the largest float below x (x finite): the backward scan's c >= goal as c > float_below(goal)
__device__ __forceinline__ float float_below(float x) {
  const int i = __float_as_int(x);
  return x > 0.f ? __int_as_float(i - 1) : (x == 0.f ? -__int_as_float(1) : __int_as_float(i + 1));
}

template <class ARG>
__device__ __forceinline__ int kde_scan(const float4* __restrict__ rec, const float4* __restrict__ rev, int M,
                                        int j0, int j1, float rem, float csum, ARG arg) {
  const bool back = rem > 0.5f * csum;
  const float goal = back ? csum - rem : rem;
  const float lim = back ? float_below(goal) : goal;
  const float4* __restrict__ q = back ? rev + (M - j1) : rec + j0;
  const int n = j1 - j0;
  float cs = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
  int kt = n;                                   // first point of the crossing trip (n: none)
  float4 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
  float4 b0 = q[4], b1 = q[5], b2 = q[6], b3 = q[7];
  for (int k = 0; k < n; k += 8) {
    {
      const float e0 = cs + __builtin_amdgcn_exp2f(arg(a0));
      const float e1 = e0 + __builtin_amdgcn_exp2f(arg(a1));
      const float e2 = e1 + __builtin_amdgcn_exp2f(arg(a2));
      const float e3 = e2 + __builtin_amdgcn_exp2f(arg(a3));
      if (e3 > lim) { c0 = e0; c1 = e1; c2 = e2; c3 = e3; kt = k; break; }
      cs = e3;
    }
    a0 = q[k + 8]; a1 = q[k + 9]; a2 = q[k + 10]; a3 = q[k + 11];
    if (k + 4 >= n) break;
    {
      const float e0 = cs + __builtin_amdgcn_exp2f(arg(b0));
      const float e1 = e0 + __builtin_amdgcn_exp2f(arg(b1));
      const float e2 = e1 + __builtin_amdgcn_exp2f(arg(b2));
      const float e3 = e2 + __builtin_amdgcn_exp2f(arg(b3));
      if (e3 > lim) { c0 = e0; c1 = e1; c2 = e2; c3 = e3; kt = k + 4; break; }
      cs = e3;
    }
    b0 = q[k + 12]; b1 = q[k + 13]; b2 = q[k + 14]; b3 = q[k + 15];
  }
  (void)c3;
  const int v = c0 > lim ? 0 : (c1 > lim ? 1 : (c2 > lim ? 2 : 3));
  const int kh = kt < n ? min(kt + v, n - 1) : n - 1;
  return min(max(back ? j1 - 1 - kh : j0 + kh, 0), M - 1);
}

// One-feature node with a moment table (plan.kde_moment_table, round 6): the index of
// kde.py:172-178 without pass 1's exps.  Around the grid centre u_g nearest u = 2 x', a chunk's
// sum is S_c(u) = sum_k d^k T[g][c][k] with d = u - u_g and
// T[g][c][k] = sum_{j in c} exp2(u_g y'_j - |y'_j|^2) (ln2 y'_j)^k / k! (float64 sums, host);
// the series' remainder is < 3e-8 of every weight (plan.KDE_MT_Z), so the sums equal the
// exp-by-exp ones to f32 rounding, at one 16-byte load and 3 FMAs per chunk.  Per cell the
// table holds the chunks (~M/64 points each), their groups of 8 and the whole point set: the
// threshold u * total, then the group whose running sum passes it, then the chunk inside it
// (<= 8 + 8 sums instead of 64), so the scan that follows covers about M/128 points instead of
// the MFMA pass's M/32; a crossing past the last group or chunk (rounding) takes the last.
// Factored form (shift 0): the caller takes this path only when every lane has fform.  Returns
// -1 for the whole wave when some lane's u is off the grid (or NaN): the MFMA pass then runs.
// Table (blob offset vbn_step.off_kmt, -1 = none): header [u_lo, 1 / delta, delta, n_cells,
// n_chunks, chunk points (int32 bits), 0, 0], rows [n_cells][n_chunks + n_groups + 1] float4 =
// 4 series terms: the chunks, their groups of 8, the whole point set (plan.kde_moment_table).
#define KDE_MT_HEAD 8         // header floats (plan.KDE_MT_HEADER)
#define KDE_MT_GROUP 8        // chunks per group (plan.KDE_MT_GROUP)
__device__ __forceinline__ int kde_index_moments(const float* __restrict__ T, float xb0, float ucat,
                                                 const float4* __restrict__ rec, int M, float& total) {
  const cfloat* H = CP(T);
  const float u_lo = H[0], inv_d = H[1], dlt = H[2];
  const int n_cells = __float_as_int(H[3]), nch = __float_as_int(H[4]), per = __float_as_int(H[5]);
  const float gr = rintf((xb0 - u_lo) * inv_d);          // nearest centre (NaN u: not in range)
  const bool in = gr >= 0.f && gr < (float)n_cells;
  if (!__all(in)) return -1;
  const float d = xb0 - fmaf(gr, dlt, u_lo);             // the centre exactly as the host formed it
  const int ng = (nch + KDE_MT_GROUP - 1) / KDE_MT_GROUP;
  const float4* __restrict__ row = reinterpret_cast<const float4*>(T + KDE_MT_HEAD) + (int)gr * (nch + ng + 1);
  auto poly = [&](const float4 c) { return fmaf(fmaf(fmaf(c.w, d, c.z), d, c.y), d, c.x); };
  total = poly(row[nch + ng]);
  const double thr = (double)ucat * (double)total;
  double cum = 0.0;
  float gs = 0.f;
  int g = ng - 1;
  bool hit = false;
  for (int k = 0; k < ng; ++k) {                        // the group
    gs = poly(row[nch + k]);
    const double nx = cum + (double)gs;
    if (nx > thr) { g = k; hit = true; break; }
    cum = nx;
  }
  if (!hit) cum -= (double)gs;                             // the last group
  const int c1 = min(nch, (g + 1) * KDE_MT_GROUP);
  int ch = c1 - 1;
  float cs = 0.f;
  hit = false;
  for (int c = g * KDE_MT_GROUP; c < c1; ++c) {          // the chunk inside it
    cs = poly(row[c]);
    const double nx = cum + (double)cs;
    if (nx > thr) { ch = c; hit = true; break; }
    cum = nx;
  }
  if (!hit) cum -= (double)cs;                             // the group's last chunk
  const int j0 = min(M, ch * per), j1 = min(M, j0 + per);
  const float4* __restrict__ rev = rec + (((M + 15) >> 4) * 16 + KDE_REC_TAIL);
  return kde_scan(rec, rev, M, j0, j1, (float)(thr - cum), cs,
                  [&](const float4 r) { return fmaf(r.y, -1.f, fmaf(r.x, xb0, -0.f)); });
}

// Two-feature node with a 2-D moment table (plan.kde_moment_table2): pass 1 of kde_index_mfma
// without its exps.  Around the cell centre u_g nearest u = 2 x', d = u - u_g, a chunk's sum is
//   S_c(u) = sum_{a+b<K} d0^a d1^b T[g][c][a,b],
//   T[g][c][a,b] = sum_{j in c} exp2(u_g.y'_j - |y'_j|^2) (ln2 y'_j0)^a (ln2 y'_j1)^b / (a! b!)
// (float64 sums, host); the cell widths keep ln2 |d.y'| <= Z = 0.5, so the remainder after
// total degree K - 1 = 8 is < 8.9e-9 of every weight.  A row is its K (K + 1) / 2 = 45
// coefficients in the order of the nested Horner below (a from K - 1 down, inside it b from
// K - 1 - a down), padded to KDE_MT2_ROW4 float4; per cell the 16 chunk rows of the MFMA pass
// (kde_cb) and, where that pass keeps half sums (KDE_HALF_MIN), the 16 first-half rows
// (kde_sub_blocks(cb32, 1)), so everything after pass 1 is kde_index_mfma's own code.
// Factored form (shift 0).  Table (blob offset step_off_kmt2, -1 = none): header per feature
// [u_lo, 1 / delta, delta, n_cells (int32 bits)], then rows per cell, floats per row, K (int32
// bits), zeros (KDE_MT2_HEAD floats); then [n_cells0 * n_cells1][rows][48] f32.
#define KDE_MT2_HEAD 16       // header floats (plan.KDE_MT2_HEADER)
#define KDE_MT2_K 9           // plan.KDE_MT2_K
#define KDE_MT2_ROW4 12       // float4 per row: 45 coefficients padded to 48 (plan.KDE_MT2_ROW)
struct KdeMt2 {
  const float4* cell;         // the lane's cell: [rows][KDE_MT2_ROW4]
  float d0, d1;
};

__device__ __forceinline__ float kde_mt2_row(const float4* __restrict__ row, float d0, float d1) {
  // the row is streamed: float4 i is loaded when the Horner reaches coefficient 4 i, so a few
  // float4 are live at a time, not the row's 12
  float4 v = row[0];
  int i = 0;
  auto next = [&]() {
    const int k = i & 3;
    if (i && !k) v = row[i >> 2];
    ++i;
    return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w));
  };
  float s = next();                                  // a = K - 1: the one coefficient b = 0
#pragma unroll
  for (int a = KDE_MT2_K - 2; a >= 0; --a) {
    float p = next();                                // b = K - 1 - a
#pragma unroll
    for (int b = KDE_MT2_K - 2 - a; b >= 0; --b) p = fmaf(p, d1, next());
    s = fmaf(s, d0, p);
  }
  return s;
}

__device__ __noinline__ float kde_mt2_row_call(const float4* __restrict__ row, float d0, float d1) {
  return kde_mt2_row(row, d0, d1);
}

// The 16 chunk sums of the lane's cell -> scr[chunk][lane], their float64 total -> tot.  False
// for the whole wave (nothing to rely on in scr) when some lane's u is off the grid or NaN.
__device__ __forceinline__ bool kde_index_moments2(const float* __restrict__ T, float u0, float u1, const Lane& L,
                                                   bool halves, double& tot, KdeMt2& m) {
  const cfloat* H = CP(T);
  const float g0 = rintf((u0 - H[0]) * H[1]), g1 = rintf((u1 - H[4]) * H[5]);   // NaN u: not in range
  const int n0 = __float_as_int(H[3]), n1 = __float_as_int(H[7]);
  const bool in = g0 >= 0.f && g0 < (float)n0 && g1 >= 0.f && g1 < (float)n1;
  if (!__all(in)) return false;
  m.d0 = u0 - fmaf(g0, H[2], H[0]);                  // the centres exactly as the host formed them
  m.d1 = u1 - fmaf(g1, H[6], H[4]);
  const int rows = halves ? 2 * KDE_CHUNKS : KDE_CHUNKS;
  m.cell = reinterpret_cast<const float4*>(T + KDE_MT2_HEAD) + ((int)g0 * n1 + (int)g1) * (rows * KDE_MT2_ROW4);
  double t = 0.0;
#pragma unroll 1
  for (int ch = 0; ch < KDE_CHUNKS; ++ch) {
    const float cs = kde_mt2_row(m.cell + ch * KDE_MT2_ROW4, m.d0, m.d1);
    L.scr[ch * WAVE + L.lane] = cs;
    t += (double)cs;
  }
  tot = t;
  return true;
}

// Latent non-root KDE node, parent dims 1..3: index ~ softmax_j log K_p (kde.py:172-178).
// Pass 1 (MFMA): per-chunk weight sums -> scr[chunk][lane]; pass 2 (VALU replica): locate the
// chunk holding u * total, scan it.  All-underflow particles (every weight 0) redo the sums on
// VALU relative to their largest weight.
// lsp (out): ln sum_j K_p(x, y_j) -- the node's own log-density denominator (kde.py:141-146), from
// pass 1's total, ln(tot) + (sigma - |x'|^2) ln 2 in every form (factored, full, rescued,
// precomputed, moment table); NaN when pass 1 gave no positive total
__device__ __forceinline__ int kde_index_mfma(const vbn_walk_args& A, const vbn_step& st, const Lane& L,
                                              float ucat, float c_p, float& lsp) {
  const int M = st.k, nf = st.aux0, lane = L.lane;
  const int cb = kde_cb(M);
  int slots[4] = {0, 0, 0, 0};
  float scl[4] = {c_p, c_p, c_p, c_p};
  for (int f = 0; f < nf; ++f) slots[f] = L.ic[st.in_off + f];
  double tot = 0.0;
  float xv[4] = {0.f, 0.f, 0.f, 0.f};
  const float negsq = kde_own(L, slots, scl, nf, xv);
  const bool pre = (st.flags & VBN_F_PRECOMP) != 0;
  // per-point records (4 weight-0 rows before the first point), then the reversed copy
  const float4* __restrict__ rec = reinterpret_cast<const float4*>(L.P + st.off_kr) + 4;
  if (nf == 1 && st.off_kmt >= 0 && !(st.flags & (VBN_F_PRECOMP | VBN_F_PRE_OUT)) &&
      __all(-negsq <= KDE_FFORM_MAX)) {               // a one-feature node with a moment table
    float mtot = 0.f;
    const int idx = kde_index_moments(L.P + st.off_kmt, 2.f * xv[0], ucat, rec, M, mtot);
    if (idx >= 0) {                                   // the whole wave took it
      if (mtot > 0.f) lsp = __logf(mtot) + negsq * VBN_LN2_F;   // factored form (sigma 0)
      wave_sync();
      return idx;
    }
  }
  float shift = 0.f;                                  // sigma: the sums are of exp2(a' - sigma)
  // pass 1 also keeps each chunk's first-half sum (a private array, kde_sub_blocks), so the
  // scan covers the half holding the threshold: at most a quarter chunk instead of a half
  bool halves = false;
  // a two-feature node with a moment table: pass 1's chunk sums from the table (factored form,
  // sigma 0) when every lane is on its grid; the located chunk's half sum is then one more row.
  // A wave whose total is not safely positive somewhere runs the MFMA pass and its rescue.
  bool tab2 = false;
  KdeMt2 mt2 = {nullptr, 0.f, 0.f};
  if (nf == 2 && step_off_kmt2(st) >= 0 && !(st.flags & (VBN_F_PRECOMP | VBN_F_PRE_OUT)) &&
      __all(-negsq <= KDE_FFORM_MAX)) {
#ifndef VBN_ABL_NOHALVES
    const bool h2 = KDE_NSUB == 2 && (cb >> 1) >= KDE_HALF_MIN;   // the table's half rows are halves
#else
    const bool h2 = false;
#endif
    double t2 = 0.0;
    if (kde_index_moments2(L.P + step_off_kmt2(st), 2.f * xv[0], 2.f * xv[1], L, (cb >> 1) >= KDE_HALF_MIN, t2, mt2) &&
        __all(t2 >= (double)kde_tiny(M))) {
      tab2 = true;
      halves = h2;
      tot = t2;
    }
  }
#ifndef VBN_ABL_NOHALVES
  float hs[KDE_CHUNKS * (KDE_NSUB - 1)];
#endif
  if (pre) {                                          // pass 1 of this sample / query, pre-pass
    if (st.flags & VBN_F_PRECOMP_Q) {
      const cfloat* q = precomp_qrow(A, st, L);
      for (int ch = 0; ch < KDE_CHUNKS; ++ch) {
        const float cs = q[ch];
        L.scr[ch * WAVE + lane] = cs;
        tot += (double)cs;
      }
      shift = q[KDE_CHUNKS];
    } else {
      const float* __restrict__ q = precomp_row(A, st, L);
      for (int ch = 0; ch < KDE_CHUNKS; ++ch) {
        const float cs = q[ch];
        L.scr[ch * WAVE + lane] = cs;
        tot += (double)cs;
      }
      shift = q[KDE_CHUNKS];
    }
  } else if (!tab2)
#ifdef VBN_ABL_NOP1
  if (true) {
    for (int ch = 0; ch < KDE_CHUNKS; ++ch) { L.scr[ch * WAVE + lane] = 1.f; tot += 1.0; }
  } else
#endif
  {
    const bf16x8* __restrict__ pa = reinterpret_cast<const bf16x8*>(L.P + st.off_kq) + lane;
    const bool fform = __all(-negsq <= KDE_FFORM_MAX);
    shift = fform ? 0.f : -negsq;
#ifndef VBN_ABL_NOHALVES
    // chunks of >= KDE_HALF_MIN 32-point blocks only: shorter chunks scan little, and the
    // sums' 64 B of scratch per particle then cost fabric traffic for no time (cfg5, M = 4096:
    // 8 blocks per chunk, 58.9 ms either way, 27 vs 7 GB per launch)
    float* hsp = ((st.flags & VBN_F_PRE_OUT) || (cb >> 1) < KDE_HALF_MIN) ? nullptr : hs;
    halves = hsp != nullptr;
#else
    float* hsp = nullptr;
#endif
    if (nf == 1)
      tot = kde_pass1<1, 1>(pa, cb >> 1, L, slots, scl, nf, fform, hsp);
    else if (nf == 2 && fform)
      tot = kde_pass1<1, 2>(pa, cb >> 1, L, slots, scl, nf, fform, hsp);
    else
      tot = kde_pass1<2, 2>(pa, cb >> 1, L, slots, scl, nf, fform, hsp);
  }
  const int nfr = nf;                                 // replica form of the pass-1 elements
  const float xb0 = 2.f * xv[0], xb1 = 2.f * xv[1], xb2 = 2.f * xv[2];
  if (!pre && !(tot >= (double)kde_tiny(M))) {       // the weights underflowed (or NaN parent)
    halves = false;
    float amax = -INFINITY;
    for (int j = 0; j < M; ++j) amax = fmaxf(amax, kde_arg_rec(rec[j], xb0, xb1, xb2, 0.f, nfr));
    shift = amax;
    tot = 0.0;
    for (int ch = 0; ch < KDE_CHUNKS; ++ch) {
      const int j0 = min(M, ch * cb * 16), j1 = min(M, j0 + cb * 16);
      float cs = 0.f;
      for (int j = j0; j < j1; ++j)
        cs += __builtin_amdgcn_exp2f(kde_arg_rec(rec[j], xb0, xb1, xb2, 0.f, nfr) - shift);
      L.scr[ch * WAVE + lane] = cs;
      tot += (double)cs;
    }
  }
  if (tot > 0.0) lsp = __logf((float)tot) + (shift + negsq) * VBN_LN2_F;
  if (st.flags & VBN_F_PRE_OUT) {                    // pre-pass: pass 1's result is the output
    for (int c = 0; c < KDE_CHUNKS; ++c) vwrite(L, st.out_col + c, L.scr[c * WAVE + lane]);
    vwrite(L, st.out_col + KDE_CHUNKS, shift);
    wave_sync();
    return -1;
  }
  const double thr = (double)ucat * tot;
  double cum = 0.0;
  int ch = KDE_CHUNKS - 1;
  for (int c2 = 0; c2 < KDE_CHUNKS; ++c2) {
    const double nx = cum + (double)L.scr[c2 * WAVE + lane];
    if (nx > thr) { ch = c2; break; }
    cum = nx;
  }
  const int j0 = min(M, ch * cb * 16), j1 = min(M, j0 + cb * 16);
#ifdef VBN_ABL_NOSCAN
  wave_sync();
  return min(j0, M - 1);
#endif
  float rem = (float)(thr - cum);
  float csum = L.scr[ch * WAVE + lane];
  int jlo = j0, jhi = j1;
#ifndef VBN_ABL_NOHALVES
  if (halves) {                                       // the sub-chunk holding thr
    const double rd = thr - cum;
    float plo = 0.f, phi = csum;
    int klo = 0, khi = KDE_NSUB;
#pragma unroll
    for (int k = 1; k < KDE_NSUB; ++k) {
      const float pk = tab2 ? kde_mt2_row_call(mt2.cell + (KDE_CHUNKS + ch) * KDE_MT2_ROW4, mt2.d0, mt2.d1)
                            : hs[ch * (KDE_NSUB - 1) + k - 1];
      if (rd >= (double)pk) { klo = k; plo = pk; }
      else if (khi == KDE_NSUB) { khi = k; phi = pk; }
    }
    const int cb32 = cb >> 1;
    jlo = klo ? min(M, j0 + 32 * kde_sub_blocks(cb32, klo)) : j0;
    jhi = khi < KDE_NSUB ? min(M, j0 + 32 * kde_sub_blocks(cb32, khi)) : j1;
    rem = (float)(rd - (double)plo);
    csum = phi - plo;
  }
#endif
  const float4* __restrict__ rev = rec + (((M + 15) >> 4) * 16 + KDE_REC_TAIL);
  int idx;
  // the replica chain a' = 2 x'.y' - |y'|^2 per feature count, compile-time (kde_arg_rec with
  // no -|x'|^2 term: sigma carries it in the full form)
  // (the shift enters the chain as its addend: -0 in the factored form, so the same values)
  const float nsh = -shift;
  if (nfr == 1)
    idx = kde_scan(rec, rev, M, jlo, jhi, rem, csum,
                   [&](const float4 r) { return fmaf(r.y, -1.f, fmaf(r.x, xb0, nsh)); });
  else if (nfr == 2)
    idx = kde_scan(rec, rev, M, jlo, jhi, rem, csum, [&](const float4 r) {
      return fmaf(r.z, -1.f, fmaf(r.y, xb1, fmaf(r.x, xb0, nsh)));
    });
  else
    idx = kde_scan(rec, rev, M, jlo, jhi, rem, csum, [&](const float4 r) {
      return fmaf(r.w, -1.f, fmaf(r.z, xb2, fmaf(r.y, xb1, fmaf(r.x, xb0, nsh))));
    });
  wave_sync();
  return idx;
}

// log p(x | parents) of a KDE node on MFMA (kde.py:114-146):
//   root:     LSE_j log K_y - log M
//   non-root: LSE_j (log K_p + log K_y) - LSE_j log K_p
// pack kq (parent features) and kqy (parent ++ target features, scales c_p / c_y).  Returns
// false (nothing added) when a sum underflows (kde_tiny); the caller then takes the shifted VALU path.
__device__ __forceinline__ bool kde_logp_mfma(const vbn_step& st, const Lane& L, bool root, float c_p,
                                              float c_y, float cy, float log_n, float& lp, float lsp) {
  const int M = st.k, dp = st.aux0, D = st.out_dim, lane = L.lane;
  // the blocks holding points (a whole number of KDE_PF blocks), not the chunk-padded pack: the
  // blocks past them hold only weight-0 padding, whose +0 terms leave every sum unchanged
  const int nb32 = min((KDE_CHUNKS * kde_cb(M)) >> 1, (((M + 31) >> 5) + KDE_PF - 1) / KDE_PF * KDE_PF);
  int slots[4] = {0, 0, 0, 0};
  float scl[4] = {c_p, c_p, c_p, c_p};
  for (int f = 0; f < dp; ++f) slots[f] = L.ic[st.in_off + f];
  for (int d = 0; d < D; ++d) { slots[dp + d] = st.out_col + d; scl[dp + d] = c_y; }
  const int ny = dp + D;
  // factored sums (kde_pass1) when no lane's |x'|^2 can overflow them: ln of a full-form sum =
  // ln(factored sum) - |x'|^2 ln 2
  float xv[4];
  const float sq_y = -kde_own(L, slots, scl, ny, xv);
  const float sq_p = root ? 0.f : -kde_own(L, slots, scl, dp, xv);
  const bool fform = __all(sq_y <= KDE_FFORM_MAX);
  const bf16x8* __restrict__ pay = reinterpret_cast<const bf16x8*>(L.P + st.off_kqy) + lane;
  const float sy = kde_sums_nf(pay, nb32, L, slots, scl, ny, fform);
  constexpr float LN2 = 0.69314718055994531f;
#ifndef VBN_ABL_NOLSP
  // a sampled node's denominator is its own pass 1's total (kde_index_mfma lsp): every lane of
  // the wave has it, so the parent-feature pass is not run again (cfg4's target: M exps per
  // particle)
  if (!root && __all(lsp == lsp)) {
    wave_sync();
    if (!(sy >= kde_tiny(M))) return false;
    lp += ((__logf(sy) - (fform ? sq_y * LN2 : 0.f)) - lsp) + cy;
    return true;
  }
#endif
  float sp = 1.f;
  if (!root) {
    const bf16x8* __restrict__ pa = reinterpret_cast<const bf16x8*>(L.P + st.off_kq) + lane;
    sp = kde_sums_nf(pa, nb32, L, slots, scl, dp, fform);
  }
  wave_sync();
  if (!(sy >= kde_tiny(M)) || !(sp >= kde_tiny(M))) return false;
  const float corr = fform ? (root ? sq_y : sq_y - sq_p) * LN2 : 0.f;
  lp += root ? ((__logf(sy) - corr) + cy - log_n) : (((__logf(sy) - __logf(sp)) - corr) + cy);
  return true;
}

// ---- pairwise kernel weights on VALU (alternative path, VBN_F_KDE_VALU) ---------------------
// -|x' - y'|^2 with packed f32 VALU (v_pk_add / v_pk_mul / v_pk_fma on two points per lane),
// points wave-uniform from scalar loads.  Measured on MI355X (cfg4, 64-node KDE, M = 10k,
// 4096 x 1024 particles): 253 ms per walk vs 245 ms with the MFMA distance tile (and 266 ms
// with the scalar loads software-pipelined), so the MFMA tile is the default.
// Pack kv (plan.py _kde_pack_valu): [KDE_CHUNKS * csz / 8][NF][8] fp32, padding points
// y' = 1e15 (weight 0).  Chunk ch = points [ch * csz, (ch + 1) * csz).
__device__ __forceinline__ int kde_csz(int M) { return (((M + KDE_CHUNKS - 1) / KDE_CHUNKS) + 7) & ~7; }

// -|x' - y'|^2 of one point record r = (y'_0, y'_1, y'_2, .); same operations, same order as
// the packed pass (bit-identical per element)
template <int NF>
__device__ __forceinline__ float kde_arg_valu(const float (&xv)[4], const float4 r) {
#pragma clang fp contract(off)
  const float d0 = xv[0] - r.x;
  float a = d0 * d0;
  if (NF > 1) { const float d1 = xv[1] - r.y; a = fmaf(d1, d1, a); }
  if (NF > 2) { const float d2 = xv[2] - r.z; a = fmaf(d2, d2, a); }
  return -a;
}

template <int NF>
__device__ __forceinline__ int kde_index_valu(const vbn_walk_args& A, const vbn_step& st, const Lane& L,
                                              float ucat, float c_p) {
#pragma clang fp contract(off)
  const float* __restrict__ kv = L.P + st.off_kv;
  const int M = st.k, lane = L.lane, csz = kde_csz(M);
  float xv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int f = 0; f < NF; ++f) xv[f] = c_p * vread(L, L.ic[st.in_off + f]);
  f32x2 xp[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) xp[f] = f32x2{xv[f], xv[f]};
  double tot = 0.0;
  for (int ch = 0; ch < KDE_CHUNKS; ++ch) {
    const float* __restrict__ blk = kv + (int64_t)(ch * (csz >> 3)) * (NF * 8);
    f32x2 acc = f32x2{0.f, 0.f};
    for (int b = 0; b < (csz >> 3); ++b, blk += NF * 8) {
#pragma unroll
      for (int i = 0; i < 8; i += 2) {
        const f32x2 d0 = xp[0] - f32x2{blk[i], blk[i + 1]};
        f32x2 a = d0 * d0;
        if (NF > 1) {
          const f32x2 d1 = xp[1] - f32x2{blk[8 + i], blk[8 + i + 1]};
          a = __builtin_elementwise_fma(d1, d1, a);
        }
        if (NF > 2) {
          const f32x2 d2 = xp[2] - f32x2{blk[16 + i], blk[16 + i + 1]};
          a = __builtin_elementwise_fma(d2, d2, a);
        }
        acc += f32x2{__builtin_amdgcn_exp2f(-a.x), __builtin_amdgcn_exp2f(-a.y)};
      }
    }
    const float cs = acc.x + acc.y;
    L.scr[ch * WAVE + lane] = cs;
    tot += (double)cs;
  }
  // per-point records (4 weight-0 rows before the first point), then the reversed copy
  const float4* __restrict__ rec = reinterpret_cast<const float4*>(L.P + st.off_kr) + 4;
  float shift = 0.f;
  if (!(tot >= (double)kde_tiny(M))) {               // the weights underflowed (or NaN parent)
    float amax = -INFINITY;
    for (int j = 0; j < M; ++j) amax = fmaxf(amax, kde_arg_valu<NF>(xv, rec[j]));
    shift = amax;
    tot = 0.0;
    for (int ch = 0; ch < KDE_CHUNKS; ++ch) {
      const int j0 = min(M, ch * csz), j1 = min(M, j0 + csz);
      float cs = 0.f;
      for (int j = j0; j < j1; ++j) cs += __builtin_amdgcn_exp2f(kde_arg_valu<NF>(xv, rec[j]) - shift);
      L.scr[ch * WAVE + lane] = cs;
      tot += (double)cs;
    }
  }
  const double thr = (double)ucat * tot;
  double cum = 0.0;
  int ch = KDE_CHUNKS - 1;
  for (int c2 = 0; c2 < KDE_CHUNKS; ++c2) {
    const double nx = cum + (double)L.scr[c2 * WAVE + lane];
    if (nx > thr) { ch = c2; break; }
    cum = nx;
  }
  const int j0 = min(M, ch * csz), j1 = min(M, j0 + csz);
  const float rem = (float)(thr - cum);
  const float csum = L.scr[ch * WAVE + lane];
  const float4* __restrict__ rev = rec + (((M + 15) >> 4) * 16 + KDE_REC_TAIL);
  const int idx = kde_scan(rec, rev, M, j0, j1, rem, csum,
                           [&](const float4 r) { return kde_arg_valu<NF>(xv, r) - shift; });
  wave_sync();
  return idx;
}

template <int DP, int DY>
__device__ __forceinline__ void step_kde_t(const vbn_walk_args& A, const vbn_step& st, const Lane& L, float& lp) {
#pragma clang fp contract(off)
  const float* __restrict__ P = L.P;
  const float* __restrict__ pts = P + st.off_pts;
  const int M = st.k, dp = DP >= 0 ? DP : st.aux0, stride = st.aux1, D = DY > 0 ? DY : st.out_dim;
  const cfloat* t = CP(P + st.off_tail);
  const float inv_sp = t[0], inv_sy = t[1], noise_scale = t[2], cy = t[3], log_n = t[4];
  const float c_p = t[5], c_y = t[6];
  const bool root = (st.flags & VBN_F_ROOT) != 0;
  const int lane = L.lane;
  float pv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < (DP > 0 ? DP : 0); ++i) pv[i] = vread(L, L.ic[st.in_off + i]);

  float lsp = __int_as_float(0x7fc00000);            // the sampling pass's ln sum_j K_p (NaN: none)
  if (st.role == VBN_ROLE_LATENT) {
    const float ucat = draw_uniforms(A, st, 0, L).x;
    int idx;
    if (root) {
      idx = min((int)(ucat * (float)M), M - 1);             // randint(0, M)
    } else if (st.off_kv >= 0 && (st.flags & VBN_F_KDE_VALU)) {
      idx = st.aux0 == 1 ? kde_index_valu<1>(A, st, L, ucat, c_p)
          : (st.aux0 == 2 ? kde_index_valu<2>(A, st, L, ucat, c_p) : kde_index_valu<3>(A, st, L, ucat, c_p));
    } else if (st.off_kq >= 0) {
      idx = kde_index_mfma(A, st, L, ucat, c_p, lsp);
      if (st.flags & VBN_F_PRE_OUT) return;            // pre-pass: sums written, no sample
    } else {
      // pass 1: per-chunk weight sums -> scr[chunk][lane]
      const int csz = (M + KDE_CHUNKS - 1) / KDE_CHUNKS;
      double tot = 0.0;
      float qmin = INFINITY;
      for (int ch = 0; ch < KDE_CHUNKS; ++ch) {
        const int j0 = ch * csz, j1 = min(M, j0 + csz);
        float cs = 0.f;
        for (int j = j0; j < j1; ++j) {
          const float q = kde_qp<DP>(pts + (int64_t)j * stride, pv, inv_sp, dp, A, st, L);
          qmin = fminf(qmin, q);
          cs += __expf(-0.5f * q);
        }
        L.scr[ch * WAVE + lane] = cs;
        tot += (double)cs;
      }
      float shift = 0.f;
      if (!(tot >= (double)kde_tiny(M))) {               // the weights underflowed
        shift = qmin;
        tot = 0.0;
        for (int ch = 0; ch < KDE_CHUNKS; ++ch) {
          const int j0 = ch * csz, j1 = min(M, j0 + csz);
          float cs = 0.f;
          for (int j = j0; j < j1; ++j)
            cs += __expf(-0.5f * (kde_qp<DP>(pts + (int64_t)j * stride, pv, inv_sp, dp, A, st, L) - shift));
          L.scr[ch * WAVE + lane] = cs;
          tot += (double)cs;
        }
      }
      // pass 2: locate the chunk, then scan inside it (per-lane chunk; vector loads)
      const double thr = (double)ucat * tot;
      double cum = 0.0;
      int ch = KDE_CHUNKS - 1;
      for (int c2 = 0; c2 < KDE_CHUNKS; ++c2) {
        const double nx = cum + (double)L.scr[c2 * WAVE + lane];
        if (nx > thr) { ch = c2; break; }
        cum = nx;
      }
      const int j0 = ch * csz, j1 = min(M, j0 + csz);
      const float rem = (float)(thr - cum);
      float cs = 0.f;
      idx = max(j1 - 1, 0);
      for (int j = j0; j < j1; ++j) {
        cs += __expf(-0.5f * (kde_qp<DP>(pts + (int64_t)j * stride, pv, inv_sp, dp, A, st, L) - shift));
        if (cs > rem) { idx = j; break; }
      }
      wave_sync();
    }
    for (int d = 0; d < D; ++d) {
      const float sel = pts[(int64_t)idx * stride + dp + d];
      vwrite(L, st.out_col + d, sel + draw_normal(A, st, d, L) * noise_scale);
    }
  } else {
    for (int d = 0; d < D; ++d) vwrite(L, st.out_col + d, node_fixed(A, st, d, L));
  }

  if ((st.flags & VBN_F_LOGP) && st.off_kqy >= 0 && (root || st.off_kq >= 0)) {
    wave_sync();
    if (kde_logp_mfma(st, L, root, c_p, c_y, cy, log_n, lp, lsp)) return;
  }
  if (st.flags & VBN_F_LOGP) {
    const float x0 = NODE_X(0);
    float sy = 0.f, sp = 0.f, qymin = INFINITY, qpmin = INFINITY, qsmin = INFINITY;
    for (int j = 0; j < M; ++j) {
      const float* pt = pts + (int64_t)j * stride;
      const float qy = kde_qy<DY>(pt + dp, x0, inv_sy, D, st, L);
      if (root) {
        sy += __expf(-0.5f * qy);
        qymin = fminf(qymin, qy);
      } else {
        const float qp = kde_qp<DP>(pt, pv, inv_sp, dp, A, st, L);
        sp += __expf(-0.5f * qp);
        sy += __expf(-0.5f * (qp + qy));
        qpmin = fminf(qpmin, qp);
        qsmin = fminf(qsmin, qp + qy);
      }
    }
    float sh_y = 0.f, sh_p = 0.f;
    if (!(sy >= kde_tiny(M)) || (!root && !(sp >= kde_tiny(M)))) {   // underflow: re-sum relative to the minimum
      sh_y = root ? qymin : qsmin;
      sh_p = qpmin;
      sy = 0.f;
      sp = 0.f;
      for (int j = 0; j < M; ++j) {
        const float* pt = pts + (int64_t)j * stride;
        const float qy = kde_qy<DY>(pt + dp, x0, inv_sy, D, st, L);
        if (root) {
          sy += __expf(-0.5f * (qy - sh_y));
        } else {
          const float qp = kde_qp<DP>(pt, pv, inv_sp, dp, A, st, L);
          sp += __expf(-0.5f * (qp - sh_p));
          sy += __expf(-0.5f * (qp + qy - sh_y));
        }
      }
    }
    const float ls_y = logf(sy) - 0.5f * sh_y;
    if (root) {
      lp += ls_y + cy - log_n;
    } else {
      const float ls_p = logf(sp) - 0.5f * sh_p;
      lp += (ls_y - ls_p) + cy;
    }
  }
}

__device__ __forceinline__ void step_kde(const vbn_walk_args& A, const vbn_step& st, const Lane& L, float& lp) {
  if (st.out_dim == 1) {
    switch (st.aux0) {
      case 0: step_kde_t<0, 1>(A, st, L, lp); return;
      case 1: step_kde_t<1, 1>(A, st, L, lp); return;
      case 2: step_kde_t<2, 1>(A, st, L, lp); return;
      case 3: step_kde_t<3, 1>(A, st, L, lp); return;
      default: break;
    }
  }
  step_kde_t<-1, -1>(A, st, L, lp);
}
