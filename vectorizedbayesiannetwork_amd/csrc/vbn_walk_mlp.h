#pragma once
// vbn_walk_mlp.h -- the NN CPDs' MLP: layers 1 and 2, the heads, mlp_forward, mlp_generic, run_mlp
// (part of vbn_walk_impl.h).
#include "vbn_walk_common.h"

// ------------------------------------------------------------------------------------------
// MLP (in -> 32 -> 32 -> n_out) for the wave's 64 particles; head outputs to scr[j][lane].
//
// Two 32-particle groups per wave (g = 0: particles 0-31, g = 1: 32-63).  Both hidden layers
// run with the hidden unit on M and the particle on N; both accumulators start from the layer's
// bias (register r of lane half h = b[row(r, h)], four 16-byte loads, exact f32).
//   layer 1: K = n_in on v_mfma_f32_32x32x2_f32, A = W1 fragments, B = z of the lane's particle
//   layer 2: K = 32 on v_mfma_f32_32x32x16_f16 as a 3-pass split product: x = hi + lo with
//            hi = f16(x), lo = f16(x - hi) for both operands; A_lo.B_hi + A_hi.B_lo + A_hi.B_hi
//            accumulated in f32 (relative error ~2^-22 per product, i.e. fp32-level) at 1/5
//            of the f32-MFMA time.  The layer-1 accumulator IS the B operand: register 8s+j
//            of lane half h holds hidden row 16s + 8(j>>2) + 4h + (j&3), and the host packs
//            W2 in that k order.  If any |h| > 32768 (f16 range) the wave takes the exact
//            f32 chain (v_mfma_f32_32x32x2_f32, k-step s pairs rows (row(s,0), row(s,1))).
//   head   : 16 v_permlane32_swap transpose the layer-2 accumulators so lane l holds all 32
//            hidden units of particle l; the head then runs on VALU with wave-uniform weights.
//
// Parameter blocks (packed by vectorizedbayesiannetwork_amd/plan.py):
//   off_std : mean_x[n_in], 1/std_x[n_in]                            (gaussian_nn only)
//   off_w1  : [t][64]  lane l: W1z[l&31][2t + (l>>5)],  W1z = [W1 | 0] (even width)
//   off_b2  : [layer 2][group 2][half 2][16] = b[row(r, h)] (accumulator init; the two group
//             copies are identical)
//   off_w2  : [q 4][lane 64][4], step s = 4q+e: W2[l&31][row(s, l>>5)]   (exact f32 fallback)
//   off_w2h : [4][lane 64][8 f16]: hi(s=0), hi(s=1), lo(s=0), lo(s=1);
//             element j of lane l: W2[l&31][16s + 8(j>>2) + 4(l>>5) + (j&3)]
//   off_w3  : [n_out][32] = W3[j][row(r,0)] (r<16) ++ W3[j][row(r,1)]
//   off_b3  : [n_out]
// with row(r, h) = (r&3) + 8(r>>2) + 4h, the 32x32 accumulator row of register r, half h.
// ------------------------------------------------------------------------------------------

// layer-1 B operand of k-step t for group g: z[2t + half] of particle (c + 32 g); the
// column beyond n_in (odd n_in) is 0.
// The operands of both lane halves are read with wave-uniform addresses (scalar loads) and
// selected per lane: a per-lane address would make them vector loads, whose vmcnt wait also
// waits for the next step's weight-block DMA.
template <bool STD, int NIN>
__device__ __forceinline__ float l1_operand(const vbn_walk_args& A, const vbn_step& st, const Lane& L,
                                            int t, int g) {
  const int half = L.lane >> 5;
  const int nin = NIN > 0 ? NIN : st.n_in;
  const int kk = 2 * t + half;
  const int ke = min(2 * t, nin - 1), ko = min(2 * t + 1, nin - 1);
  const int se = CI(L.ic)[st.in_off + ke], so = CI(L.ic)[st.in_off + ko];
  const int slot = half ? so : se;
  float z = L.vals[slot * WAVE + (L.lane & 31) + 32 * g];
  if (STD) {
    const cfloat* sp = CP(L.P) + st.off_std;
    const float me = sp[ke], mo = sp[ko], ie = sp[nin + ke], io = sp[nin + ko];
    z = (z - (half ? mo : me)) * (half ? io : ie);
  }
  return kk < nin ? z : 0.0f;
}

// Layer-1 accumulator init of group g = bias rows of the lane half (register r of half h =
// b1[row(r, h)]), from the staged weight block (LDS) or, on the exact fallback, the blob.
__device__ __forceinline__ f32x16 load_acc16(const float* __restrict__ src) {
  const float4* q4 = reinterpret_cast<const float4*>(src);
  f32x16 a;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = q4[q];
    a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
  }
  return a;
}

// layer-2 bias as the accumulator's initial value of group g (exact f32 fallback path)
__device__ __forceinline__ f32x16 layer2_init(const vbn_step& st, const Lane& L, int g) {
  const float4* bacc = reinterpret_cast<const float4*>(L.P + st.off_b2 + 64 + 32 * g + 16 * (L.lane >> 5));
  f32x16 b;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = bacc[q];
    b[4 * q] = v.x; b[4 * q + 1] = v.y; b[4 * q + 2] = v.z; b[4 * q + 3] = v.w;
  }
  return b;
}

// y - f32(half h of packed f16 pair ph), exact: one v_fma_mix_f32 (reads the f16 in place),
// selected by the compiler from fma(f32(h), m, y) with m = -1 held opaque in an SGPR (a literal
// -1 folds the fma into a subtraction, which gfx950 selects as cvt + sub).  Not inline asm: an
// asm v_fma_mix is invisible to the hazard recognizer, which then does not pad its VGPR write
// against an in-flight MFMA reading or writing that register -- the cause of round 3's
// hipcc / hiprtc divergence of the split-f16 heads (the two compiles scheduled it differently).
__device__ __forceinline__ float neg_one_sgpr() {
  float m = -1.0f;
  asm("" : "+s"(m));     // not volatile: CSE'd / hoisted like any pure value
  return m;
}
__device__ __forceinline__ float sub_f16_lo(float y, f16x2 ph) {
  return __builtin_fmaf((float)ph[0], neg_one_sgpr(), y);
}
__device__ __forceinline__ float sub_f16_hi(float y, f16x2 ph) {
  return __builtin_fmaf((float)ph[1], neg_one_sgpr(), y);
}

// Layer 2 of one group on the split-f16 path from the activations y (|y| <= 32768 checked by
// the caller): y = hi + lo with hi = f16(y), lo = f16(y - hi); A_lo.B_hi + A_hi.B_lo + A_hi.B_hi
// on v_mfma_f32_32x32x16_f16 (f32 accumulate).  B operand: register 8s+j of lane half h holds
// hidden row 16s + 8(j>>2) + 4h + (j&3).
__device__ __forceinline__ f32x16 layer2_split(const uint4 (&w2h)[4], const f32x16& binit, const float (&y)[16]) {
#ifdef VBN_ABL_NOL2
  f32x16 r = binit;
  for (int i = 0; i < 16; ++i) r[i] += y[i];
  return r;
#endif
  f16x8 bh[2], bl[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const float y0 = y[8 * s2 + j], y1 = y[8 * s2 + j + 1];
      const f16x2 ph = __builtin_convertvector((f32x2){y0, y1}, f16x2);
#ifdef VBN_ABL_NOSPLIT
      const f16x2 pl = ph;
#else
      const f16x2 pl = __builtin_convertvector((f32x2){sub_f16_lo(y0, ph), sub_f16_hi(y1, ph)}, f16x2);
#endif
      bh[s2][j] = ph[0];
      bh[s2][j + 1] = ph[1];
      bl[s2][j] = pl[0];
      bl[s2][j + 1] = pl[1];
    }
  }
  f32x16 b = binit;
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const f16x8 ah = __builtin_bit_cast(f16x8, w2h[s2]);
    const f16x8 al = __builtin_bit_cast(f16x8, w2h[2 + s2]);
#ifndef VBN_ABL_NOSPLIT
    b = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[s2], b, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[s2], b, 0, 0, 0);
#endif
    b = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[s2], b, 0, 0, 0);
  }
  return b;
}

// Layer 2 of one group from the raw layer-1 pre-activations z with the ReLU folded into the
// f16 split (the caller guarantees z < 2048): hi = f16 of z rounded toward zero, so the
// residual z - hi lies in [0, 1) for z >= 0 and in (-1, 0] for z < 0; one v_fma_mix_f32 with
// the clamp bit ([0, 1]) then gives relu(z) - relu(hi) exactly, and one v_pk_max_f16 per pair
// gives relu(hi): hi + lo = relu(z) to f16 x f16 precision, 5 VALU per pair of activations
// instead of 6 (two ReLU maxes, two conversions, two residuals).
__device__ __forceinline__ f32x16 layer2_split_relu(const uint4 (&w2h)[4], const f32x16& binit,
                                                    const float (&z)[16]) {
  f16x8 bh[2], bl[2];
  const f16x2 zero2 = {(_Float16)0.f, (_Float16)0.f};
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const float z0 = z[8 * s2 + j], z1 = z[8 * s2 + j + 1];
      const f16x2 pr = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(z0, z1));
      const float r0 = __builtin_amdgcn_fmed3f(sub_f16_lo(z0, pr), 0.f, 1.f);
      const float r1 = __builtin_amdgcn_fmed3f(sub_f16_hi(z1, pr), 0.f, 1.f);
      const f16x2 pl = __builtin_convertvector((f32x2){r0, r1}, f16x2);
      const f16x2 ph = __builtin_elementwise_max(pr, zero2);
      bh[s2][j] = ph[0];
      bh[s2][j + 1] = ph[1];
      bl[s2][j] = pl[0];
      bl[s2][j + 1] = pl[1];
    }
  }
  f32x16 b = binit;
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const f16x8 ah = __builtin_bit_cast(f16x8, w2h[s2]);
    const f16x8 al = __builtin_bit_cast(f16x8, w2h[2 + s2]);
    b = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[s2], b, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[s2], b, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[s2], b, 0, 0, 0);
  }
  return b;
}

// Layer 2 of one group from the activations y, exact f32 chain (K = 32 as 16
// v_mfma_f32_32x32x2_f32 steps)
__device__ __forceinline__ f32x16 layer2_exact(const vbn_step& st, const Lane& L, int g, const float (&y)[16]) {
  const float4* w2p = reinterpret_cast<const float4*>(L.P + st.off_w2);
  f32x16 b = layer2_init(st, L, g);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = w2p[q * WAVE + L.lane];
    b = __builtin_amdgcn_mfma_f32_32x32x2f32(v.x, y[4 * q + 0], b, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_32x32x2f32(v.y, y[4 * q + 1], b, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_32x32x2f32(v.z, y[4 * q + 2], b, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_32x32x2f32(v.w, y[4 * q + 3], b, 0, 0, 0);
  }
  return b;
}

// Head outputs two at a time (both outputs' weights in flight together; w3/b3 (weight block)
// and scr (head scratch) are distinct LDS rows, so the reads need not wait for the writes).
__device__ __forceinline__ float head_dot(const float4 (&w)[4], const float (&y0)[16], const float (&y1)[16],
                                          float b, bool nan_in) {
  float a0 = 0.f, c0 = 0.f, a1 = 0.f, c1 = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    a0 = fmaf(w[q].x, y0[4 * q], a0);
    c0 = fmaf(w[q].y, y0[4 * q + 1], c0);
    a1 = fmaf(w[q].x, y1[4 * q], a1);
    c1 = fmaf(w[q].y, y1[4 * q + 1], c1);
    a0 = fmaf(w[q].z, y0[4 * q + 2], a0);
    c0 = fmaf(w[q].w, y0[4 * q + 3], c0);
    a1 = fmaf(w[q].z, y1[4 * q + 2], a1);
    c1 = fmaf(w[q].w, y1[4 * q + 3], c1);
  }
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(a0 + c0), __float_as_uint(a1 + c1), false, false);
  const float o = (__uint_as_float(sw[0]) + __uint_as_float(sw[1])) + b;
  return nan_in ? __int_as_float(0x7fc00000) : o;
}

__device__ __forceinline__ void head_outputs(const float* __restrict__ w3, const float* __restrict__ b3,
                                             float* __restrict__ scr, int nout, const float (&y0)[16],
                                             const float (&y1)[16], bool nan_in) {
#pragma clang loop unroll(disable)
  for (int j = 0; j < nout; j += 2) {
    const bool two = j + 1 < nout;
    const float4* wa = reinterpret_cast<const float4*>(w3 + 32 * j);
    const float4* wb = reinterpret_cast<const float4*>(w3 + 32 * (two ? j + 1 : j));
    const float4 va[4] = {wa[0], wa[1], wa[2], wa[3]};
    const float4 vb[4] = {wb[0], wb[1], wb[2], wb[3]};
    const float ba = b3[j], bb = b3[two ? j + 1 : j];
    scr[j * WAVE] = head_dot(va, y0, y1, ba, nan_in);
    if (two) scr[(j + 1) * WAVE] = head_dot(vb, y0, y1, bb, nan_in);
  }
}

// Head on VALU in the accumulator layout (no transpose): lane half h holds hidden rows
// row(r, h) of its particle, so per output j the half's 16 products use per-lane weights
// W3[j][row(r, h)] (the pack's [n_out][32] rows hold 16 per half), in two independent chains
// per group; one v_permlane32_swap per output then adds the two halves (group 0 | group 1 ->
// lane l = particle l).  W = the step's weight block (W3 at off_w3, b3 at off_b3, relative to
// wblk_off); outputs to scr[j][lane].
template <int ACT>
__device__ __forceinline__ void mlp_head(const vbn_step& st, const Lane& L, const float* __restrict__ W,
                                         const f32x16& h0, const f32x16& h1, bool nan_in) {
  const int lane = L.lane;
#ifdef VBN_ABL_NOHEAD
  for (int j = 0; j < st.n_out; ++j) L.scr[j * WAVE + lane] = h0[j] + h1[j + 1];
  wave_sync();
  return;
#endif
  float y0[16], y1[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    y0[r] = act_fn<ACT>(h0[r]);
    y1[r] = act_fn<ACT>(h1[r]);
  }
  head_outputs(W + (st.off_w3 - st.wblk_off) + 16 * (lane >> 5), W + (st.off_b3 - st.wblk_off),
               L.scr + lane, st.n_out, y0, y1, nan_in);
  wave_sync();
}

// Layer 1 of group g (v_mfma_f32_32x32x2_f32, K = n_in, bias rows as the accumulator init)
// and its activation.  W = weight block base (LDS: staged block; global: blob + wblk_off), so
// W1 sits at W[t * 64 + lane] and the biases at W + (off_b2 - wblk_off).  ``pre`` runs between
// the fragment reads and the first MFMA (group 0: the step's draws).  Returns a wave-uniform
// flag: CHK = 0 (fast path) -- some layer-1 operand lies beyond the node's bound zlim
// (step_zlim: within it no activation can leave the f16 split range, plan._pack_mlp), one
// compare per MFMA operand instead of one max per activation; CHK = 1 -- some activation
// leaves the split range |y| <= 32768 (NaN with the sign bit clear counts as out of range).
template <int ACT, bool STD, int NIN, int CHK = 0, bool RAW = false, typename F>
__device__ __forceinline__ bool mlp_l1_act(const vbn_walk_args& A, const vbn_step& st, const Lane& L,
                                           const float* __restrict__ W, int g, float (&y)[16], F&& pre) {
  const int lane = L.lane;
  f32x16 a = load_acc16(W + (st.off_b2 - st.wblk_off) + 32 * g + 16 * (lane >> 5));
  const float zlim = step_zlim(st);
  bool out = false;
  if (NIN > 0) {
    float w1[(NIN + 1) / 2 > 0 ? (NIN + 1) / 2 : 1];
#pragma unroll
    for (int t = 0; t < (NIN + 1) / 2; ++t) w1[t] = W[t * WAVE + lane];
    pre();
#pragma unroll
    for (int t = 0; t < (NIN + 1) / 2; ++t) {
      const float op = l1_operand<STD, NIN>(A, st, L, t, g);
      if (CHK == 0) out |= !(fabsf(op) <= zlim);
      a = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[t], op, a, 0, 0, 0);
    }
  } else {
    pre();
    const int t1 = (st.n_in + 1) >> 1;
    for (int t = 0; t < t1; ++t) {
      const float op = l1_operand<STD, NIN>(A, st, L, t, g);
      if (CHK == 0) out |= !(fabsf(op) <= zlim);
      a = __builtin_amdgcn_mfma_f32_32x32x2f32(W[t * WAVE + lane], op, a, 0, 0, 0);
    }
  }
  int big = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    y[r] = RAW ? a[r] : act_fn<ACT>(a[r]);                // RAW: relu folded into the split
    if (CHK == 1) big = max(big, __float_as_int(y[r]));   // activations are >= -1: the positive side
  }
  // split range: relu nodes (layer2_split_relu) z < 2048, others |act(z)| <= 32768
  return CHK == 1 ? __any(big > (ACT == VBN_ACT_RELU ? 0x44ffffff : 0x47000000)) : __any(out);
}

// Head outputs with a compile-time count (NOUT > 0): straight-line code, so the scheduler can
// place it beside the other group's layer-2 MFMAs (same operations as head_outputs).
template <int NOUT>
__device__ __forceinline__ void head_outputs_n(const float* __restrict__ w3, const float* __restrict__ b3,
                                               float* __restrict__ scr, const float (&y0)[16],
                                               const float (&y1)[16], bool nan_in) {
#pragma unroll
  for (int j = 0; j < NOUT; ++j) {
    const float4* wa = reinterpret_cast<const float4*>(w3 + 32 * j);
    const float4 va[4] = {wa[0], wa[1], wa[2], wa[3]};
    scr[j * WAVE] = head_dot(va, y0, y1, b3[j], nan_in);
  }
}

// Wide heads (VBN_F_HEAD_MFMA: mdn, softmax_nn; 8..32 outputs) on the split-f16 MFMA like
// layer 2: the layer-2 activations are already in the B-operand layout, W3 is packed as layer
// 2's A fragments (output rows padded to 32) and the bias is the accumulator init, so the head
// is 6 MFMAs and one f16 split per group instead of 16 FMAs per output per group.  Lane half h
// of group g then holds outputs row(r, h) of particle (lane & 31) + 32 g, stored to the head
// rows.  Activations beyond the split range, or a NaN parent input, take the VALU head.
__host__ __device__ constexpr bool head_on_mfma(int flags) {
#ifdef VBN_ABL_NOHEADMFMA      // A/B only: every head on VALU (outputs within an ulp, not bitwise)
  return false;
#else
  return (flags & VBN_F_HEAD_MFMA) != 0 && (flags & VBN_F_F32L2) == 0;
#endif
}

template <int ACT, bool MIR>
__device__ __forceinline__ void head_mfma(const vbn_step& st, const Lane& L, const float* __restrict__ W,
                                          const f32x16& h0, const f32x16& h1, bool nan_in) {
  const int lane = L.lane;
  float y0[16], y1[16];
  int big = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    y0[r] = act_fn<ACT>(h0[r]);
    y1[r] = MIR ? y0[r] : act_fn<ACT>(h1[r]);
    big = max(big, max(__float_as_int(y0[r]), __float_as_int(y1[r])));   // positive side only
  }
  if (__any(big > 0x47000000 || nan_in)) {         // rare: the VALU head
    mlp_head<ACT>(st, L, W, h0, h1, nan_in);
    return;
  }
  const float* __restrict__ F = L.P + step_off_w3h(st);
  const uint4* w3h = reinterpret_cast<const uint4*>(F);
  const uint4 wq[4] = {w3h[lane], w3h[WAVE + lane], w3h[2 * WAVE + lane], w3h[3 * WAVE + lane]};
  const f32x16 bi = load_acc16(F + 1024 + 16 * (lane >> 5));
  const f32x16 o0 = layer2_split(wq, bi, y0);
  const f32x16 o1 = MIR ? o0 : layer2_split(wq, bi, y1);
  const int h = lane >> 5, n = lane & 31;
  float* __restrict__ scr = L.scr;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
    if (row < st.n_out) {
      scr[row * WAVE + n] = o0[r];
      scr[row * WAVE + n + 32] = o1[r];
    }
  }
  wave_sync();
}

// One NN node for the wave's 64 particles from the LDS-staged weight block.  Group 0 (layer 1,
// layer 2 split-f16 on MFMA), group 1, the head on both -- one basic block: the f16 range
// check only ORs a wave-uniform flag, and the rare exact path (an activation beyond the split
// range, or VBN_F_F32L2) re-runs the node on the exact f32 chain after the head and overwrites
// its outputs.  Without branches between them, the compiler can issue group 1's layer-1 /
// split VALU work and group 0's head in the shadow of the other group's MFMAs.  ``pre`` (the
// step's draws) runs after group 0's fragment reads are issued.
template <int ACT, bool STD, int NIN, bool MIR, int NOUT, typename F>
__device__ __forceinline__ void mlp_forward(const vbn_walk_args& A, const vbn_step& st, const Lane& L, F&& pre) {
  const int lane = L.lane;
  const int nin = NIN > 0 ? NIN : st.n_in;
  const float* __restrict__ W = L.wb;
  const uint4* w2h = reinterpret_cast<const uint4*>(W + (st.off_w2h - st.wblk_off));
  const float* b2 = W + (st.off_b2 - st.wblk_off) + 64 + 16 * (lane >> 5);
  bool nan_in = false;                            // torch keeps NaN through Linear/act
  for (int d = 0; d < nin; ++d) {
    const float v = L.vals[L.ic[st.in_off + d] * WAVE + lane];
    nan_in |= (v != v);
  }
  f32x16 h0, h1;
  bool beyond;                                    // some layer-1 operand beyond the node's bound
  {
#ifdef VBN_ABL_NOFUSE      // A/B only: relu then the plain split (same outputs to f32 rounding)
    constexpr bool FUSE = false;
#else
    constexpr bool FUSE = ACT == VBN_ACT_RELU;    // relu folded into the f16 split
#endif
    float y[16];
    beyond = mlp_l1_act<ACT, STD, NIN, 0, FUSE>(A, st, L, W, 0, y, pre);
    const uint4 wq[4] = {w2h[lane], w2h[WAVE + lane], w2h[2 * WAVE + lane], w2h[3 * WAVE + lane]};
    h0 = FUSE ? layer2_split_relu(wq, load_acc16(b2), y) : layer2_split(wq, load_acc16(b2), y);
    if constexpr (MIR) {
      h1 = h0;                                    // group 1 = group 0's particles
    } else {
      float y1[16];
      beyond |= mlp_l1_act<ACT, STD, NIN, 0, FUSE>(A, st, L, W, 1, y1, [] {});
      h1 = FUSE ? layer2_split_relu(wq, load_acc16(b2 + 32), y1) : layer2_split(wq, load_acc16(b2 + 32), y1);
    }
  }
  if constexpr (NOUT > 0) {
    float y0[16], y1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      y0[r] = act_fn<ACT>(h0[r]);
      y1[r] = act_fn<ACT>(h1[r]);
    }
    head_outputs_n<NOUT>(W + (st.off_w3 - st.wblk_off) + 16 * (lane >> 5), W + (st.off_b3 - st.wblk_off),
                         L.scr + lane, y0, y1, nan_in);
    wave_sync();
  } else if (head_on_mfma(st.flags)) {
    head_mfma<ACT, MIR>(st, L, W, h0, h1, nan_in);
  } else {
    mlp_head<ACT>(st, L, W, h0, h1, nan_in);
  }
  // rare: an operand beyond the bound -- check the activations themselves (recomputed from the
  // blob: the same values); beyond the split range, the exact f32 chain overwrites the outputs
#ifdef VBN_ABL_NOEXACT   // measurement only: no exact-path branch (wrong when it is needed)
  if (false) {
#else
  if (beyond || (st.flags & VBN_F_F32L2)) {
#endif
    const float* __restrict__ Wg = L.P + st.wblk_off;
    bool big = (st.flags & VBN_F_F32L2) != 0;
    if (!big) {
      float y[16];
      big = mlp_l1_act<ACT, STD, NIN, 1>(A, st, L, Wg, 0, y, [] {});
      if constexpr (!MIR) big |= mlp_l1_act<ACT, STD, NIN, 1>(A, st, L, Wg, 1, y, [] {});
    }
    if (big) {                                    // the exact f32 chain, outputs overwritten
      float y[16];
      mlp_l1_act<ACT, STD, NIN>(A, st, L, Wg, 0, y, [] {});
      h0 = layer2_exact(st, L, 0, y);
      if constexpr (MIR) {
        h1 = h0;
      } else {
        mlp_l1_act<ACT, STD, NIN>(A, st, L, Wg, 1, y, [] {});
        h1 = layer2_exact(st, L, 1, y);
      }
      mlp_head<ACT>(st, L, W, h0, h1, nan_in);
    }
  }
}

// Non-relu activations (kind-set bit 5) take the generic fan-in loop only: a compile-time fan-in
// per activation multiplied the inlined MLP copies of those kind sets by 4 (their objects took
// ~40 min each to build); relu -- the reference default and every benchmark DAG -- keeps them.
template <int ACT, bool STD, bool MIR, int NOUT, typename F>
__device__ __forceinline__ void mlp_nin(const vbn_walk_args& A, const vbn_step& st, const Lane& L, F&& pre) {
  if constexpr (ACT != VBN_ACT_RELU) {
    mlp_forward<ACT, STD, 0, MIR, NOUT>(A, st, L, pre);
  } else {
  switch (st.n_in) {
    case 1: mlp_forward<ACT, STD, 1, MIR, NOUT>(A, st, L, pre); break;
    case 2: mlp_forward<ACT, STD, 2, MIR, NOUT>(A, st, L, pre); break;
    case 3: mlp_forward<ACT, STD, 3, MIR, NOUT>(A, st, L, pre); break;
    default: mlp_forward<ACT, STD, 0, MIR, NOUT>(A, st, L, pre); break;
  }
  }
}

// ------------------------------------------------------------------------------------------
// Generic MLP (any hidden_dims, reference gaussian_nn.py:16-34 _build_mlp; VBN_F_MLP_GENERIC):
// every layer -- input layer, hidden layers, head -- as exact f32 v_mfma_f32_32x32x2_f32 tiles
// of 32 units x 32 particles, K in steps of 2, activations ping-ponged through the wave's LDS
// scratch rows (layer input row k of particle n at buf[k][n]; conflict-free: lane halves read
// rows 2t and 2t + 1).  Out of line so the (32, 32) hot path keeps its registers.
//   off_w2 (step) -> layer table int32 [1 + 4 L]: L, then per layer (in, out, off_w, off_b);
//   off_w : [ceil(out/32)][ceil(in/2)][64]  lane l: W[32 blk + (l & 31)][2 t + (l >> 5)] (0-padded)
//   off_b : [ceil(out/32)][2][16]           b[32 blk + row(r, h)] (accumulator init, 0-padded)
// Scratch rows: [0, n_out) the head's outputs (what the CPD epilogues read), then two buffers
// of max(hidden) rows (plan.py sizes max_out = n_out + 2 max(hidden)).
// ------------------------------------------------------------------------------------------
template <int ACT, bool STD>
__device__ __attribute__((noinline)) void mlp_generic(const vbn_walk_args& A, const vbn_step& st, const Lane& L) {
  const int lane = L.lane, h = lane >> 5, col = lane & 31;
  const cint* tab = CI(L.P + st.off_w2);
  const int nl = tab[0];
  int hmax = 1;
  for (int li = 0; li + 1 < nl; ++li) hmax = max(hmax, tab[2 + 4 * li]);
  float* buf0 = L.scr + st.n_out * WAVE;
  float* buf1 = buf0 + hmax * WAVE;
  bool nan_in = false;                            // torch keeps NaN through Linear / activation
  for (int d = 0; d < st.n_in; ++d) {
    const float v = L.vals[L.ic[st.in_off + d] * WAVE + lane];
    nan_in |= (v != v);
  }
  for (int li = 0; li < nl; ++li) {
    const int in = tab[1 + 4 * li], out = tab[2 + 4 * li];
    const float* __restrict__ W = L.P + tab[3 + 4 * li];
    const float* __restrict__ Bs = L.P + tab[4 + 4 * li];
    const bool last = li + 1 == nl;
    const float* src = (li & 1) ? buf0 : buf1;    // layer li >= 1 reads what li - 1 wrote
    float* dst = last ? L.scr : ((li & 1) ? buf1 : buf0);
    const int nblk = (out + 31) >> 5, t1 = (in + 1) >> 1;
    for (int blk = 0; blk < nblk; ++blk) {
      for (int g = 0; g < 2; ++g) {
        f32x16 a = load_acc16(Bs + blk * 32 + 16 * h);
        for (int t = 0; t < t1; ++t) {
          const float w = W[(blk * t1 + t) * WAVE + lane];
          float x;
          if (li == 0) {
            x = l1_operand<STD, 0>(A, st, L, t, g);
          } else {
            const int k = 2 * t + h;
            x = k < in ? src[k * WAVE + col + 32 * g] : 0.f;
          }
          a = __builtin_amdgcn_mfma_f32_32x32x2f32(w, x, a, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * blk + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (row < out) dst[row * WAVE + col + 32 * g] = last ? a[r] : act_fn<ACT>(a[r]);
        }
      }
    }
    wave_sync();
  }
  if (nan_in)
    for (int j = 0; j < st.n_out; ++j) L.scr[j * WAVE + lane] = __int_as_float(0x7fc00000);
  wave_sync();
}

template <unsigned KM>
__device__ __forceinline__ void run_mlp_generic(const vbn_walk_args& A, const vbn_step& st, const Lane& L) {
  const bool sd = (st.flags & VBN_F_STANDARDIZE) != 0;
  if (!(KM & VBN_KM_NONRELU) || st.act == VBN_ACT_RELU) {
    if (sd) mlp_generic<VBN_ACT_RELU, true>(A, st, L); else mlp_generic<VBN_ACT_RELU, false>(A, st, L);
    return;
  }
  if constexpr ((KM & VBN_KM_NONRELU) != 0) {
    switch (st.act * 2 + (sd ? 1 : 0)) {
      case 2: mlp_generic<VBN_ACT_TANH, false>(A, st, L); break;
      case 3: mlp_generic<VBN_ACT_TANH, true>(A, st, L); break;
      case 4: mlp_generic<VBN_ACT_GELU, false>(A, st, L); break;
      case 5: mlp_generic<VBN_ACT_GELU, true>(A, st, L); break;
      case 6: mlp_generic<VBN_ACT_ELU, false>(A, st, L); break;
      default: mlp_generic<VBN_ACT_ELU, true>(A, st, L); break;
    }
  }
}

// KM bit 5: some NN CPD uses a non-relu activation; bit 6: half-wave instantiation.  ``pre``:
// the step's draws (see mlp_forward).  NOUT > 0: the caller's head width is a compile-time
// constant (gaussian_nn with D = 1: loc, scale).
template <unsigned KM, int NOUT = 0, typename F>
__device__ __forceinline__ void run_mlp(const vbn_walk_args& A, const vbn_step& st, const Lane& L, F&& pre) {
  constexpr bool MIR = (KM & VBN_KM_HALFWAVE) != 0;   // half-wave instantiation
  if (st.flags & VBN_F_PRECOMP) {                  // parents = shared root draws / evidence: this
    pre();                                         // sample's / query's head outputs, pre-pass
    if (st.flags & VBN_F_PRECOMP_Q) {
      const cfloat* q = precomp_qrow(A, st, L);
      for (int j = 0; j < st.n_out; ++j) L.scr[j * WAVE + L.lane] = q[j];
    } else {
      const float* __restrict__ q = precomp_row(A, st, L);
      for (int j = 0; j < st.n_out; ++j) L.scr[j * WAVE + L.lane] = q[j];
    }
    wave_sync();
    return;
  }
  if constexpr ((KM & VBN_KM_GENERIC_MLP) != 0) {     // kind-set bit 9: plans with generic MLPs
    if (st.flags & VBN_F_MLP_GENERIC) {            // hidden_dims other than (32, 32)
      pre();
      run_mlp_generic<KM>(A, st, L);
      return;
    }
  }
  const bool sd = (st.flags & VBN_F_STANDARDIZE) != 0;
  if (!(KM & VBN_KM_NONRELU) || st.act == VBN_ACT_RELU) {
    if (sd) mlp_nin<VBN_ACT_RELU, true, MIR, NOUT>(A, st, L, pre);
    else mlp_nin<VBN_ACT_RELU, false, MIR, NOUT>(A, st, L, pre);
    return;
  }
  if constexpr ((KM & VBN_KM_NONRELU) != 0) {
    switch (st.act * 2 + (sd ? 1 : 0)) {
      case 2: mlp_nin<VBN_ACT_TANH, false, MIR, NOUT>(A, st, L, pre); break;
      case 3: mlp_nin<VBN_ACT_TANH, true, MIR, NOUT>(A, st, L, pre); break;
      case 4: mlp_nin<VBN_ACT_GELU, false, MIR, NOUT>(A, st, L, pre); break;
      case 5: mlp_nin<VBN_ACT_GELU, true, MIR, NOUT>(A, st, L, pre); break;
      case 6: mlp_nin<VBN_ACT_ELU, false, MIR, NOUT>(A, st, L, pre); break;
      default: mlp_nin<VBN_ACT_ELU, true, MIR, NOUT>(A, st, L, pre); break;
    }
  }
}
