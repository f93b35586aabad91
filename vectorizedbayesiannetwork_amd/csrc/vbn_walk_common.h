#pragma once
// vbn_walk_common.h -- gfx950 (MI355X) particle walks, the part every walk kernel shares: the
// vbn_step accessors, wave and activation helpers, the Philox / Box-Muller draws, the Lane
// state, slot / evidence / pre-pass reads and the LDS staging constants.  Included on its own by
// vbn_table_walk.hip; the NN / KDE walk takes it through vbn_walk_impl.h.
//
// One wave64 owns 64 particles (lane == particle in every per-particle stage).  The wave
// walks the plan's topological steps; each node's value lives in LDS (vals[slot][64]), so
// the [B,S,sum(D)] particle tensor of the reference never touches HBM: only evidence in,
// pdf/log-weights and the target slice out.
//
// NN CPDs (gaussian_nn, mdn, softmax_nn; MLP in->32->32->out): the 32x32 hidden layer runs
// on MFMA (v_mfma_f32_32x32x2_f32, exact f32) with the hidden unit on the M axis and the
// particle on the N axis, two 32-particle groups per wave.  Layer 1 (K = #parents <= few)
// is computed on VALU directly in the MFMA B-operand layout, the head on VALU from the
// accumulator layout, combined across lane halves with one v_permlane32_swap per output.
//
// Reference ops replaced (file:line in Giovannibriglia/VectorizedBayesianNetwork):
//   topo loop            vbn/inference/monte_carlo_marginalization.py:60-91,
//                        importance_sampling.py:56-80, likelihood_weighting.py:41-71,
//                        vbn/sampling/ancestral.py:26-40
//   gaussian_nn          vbn/cpds/gaussian_nn.py:215-288
//   linear_gaussian      vbn/cpds/linear_gaussian.py:163-217
//   mdn                  vbn/cpds/mdn.py:185-272
//   kde                  vbn/cpds/kde.py:105-182
//   softmax_nn           vbn/cpds/softmax_nn.py:581-759
//   softmax + ESS        importance_sampling.py:82-84, likelihood_weighting.py:75-80
#ifndef __HIPCC_RTC__               // hiprtc (plan-specialised walks) brings its own runtime
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#endif

#include "vbn_hip_types.h"

#ifndef INFINITY
#define INFINITY __builtin_inff()
#endif

#define WAVE 64
#define KDE_CHUNKS 16
#define KDE_REC_TAIL 16  // weight-0 record rows after the last point (plan.py KDE_REC_TAIL)
#define LOG_2PI_F 1.8378770664093453f

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// The three vbn_step words that mean something else on another step kind, by the name that
// fits the reader (include/vbn_hip_types.h).
// NN steps: the layer-1 operand bound zlim (plan._pack_mlp), float bits in off_kq
__device__ __forceinline__ float step_zlim(const vbn_step& st) { return __int_as_float(st.off_kq); }
// NN steps with VBN_F_HEAD_MFMA: blob offset of the split-f16 head fragments, in off_kqy
__host__ __device__ constexpr int32_t step_off_w3h(const vbn_step& st) { return st.off_kqy; }
// kde steps: blob offset of the two-feature moment table (plan.kde_moment_table2), -1 = none, in
// off_w1 (an NN field; the packer writes it on every kde step)
__host__ __device__ constexpr int32_t step_off_kmt2(const vbn_step& st) { return st.off_w1; }

// ------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ void wave_sync() {
  // LDS ops of one wave are issued in order; this only stops the compiler from moving
  // LDS accesses of different lanes across the hand-off point.
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __builtin_amdgcn_wave_barrier();
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// relu as one v_max_i32 on the float's bits (negative floats are negative ints; -0 -> +0).
// fmaxf would add a canonicalising v_max(x, x) in IEEE mode, inline asm would hide the
// MFMA->VALU read hazard from the compiler.  NaN parents are handled by the caller.
__device__ __forceinline__ float relu_nan(float x) { return __int_as_float(max(__float_as_int(x), 0)); }

template <int ACT>
__device__ __forceinline__ float act_fn(float x) {
  if (ACT == VBN_ACT_RELU) return relu_nan(x);
  if (ACT == VBN_ACT_TANH) return tanhf(x);
  if (ACT == VBN_ACT_GELU) return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
  return x > 0.f ? x : expm1f(x);  // ELU(alpha=1)
}

// Hardware transcendentals without the library's denormal / correctly-rounded fix-ups: the
// natural log as v_log_f32 (log2) x ln 2 and the reciprocal as v_rcp_f32 (each ~1 ulp).  Only
// for arguments that are normal floats by construction (the callers say why): __logf /
// __fdividef / sqrtf lower to ~12-instruction sequences that handle denormal inputs, which
// was ~10 % of the cfg2 walk's VALU stream (softplus and Box-Muller once per node).
#define VBN_LN2_F 0.69314718055994530942f
__device__ __forceinline__ float log_hw(float x) { return __builtin_amdgcn_logf(x) * VBN_LN2_F; }

// F.softplus(beta=1, threshold=20) (reference cpds/utils.py:6-7) with hardware exp/log:
// log1p(e) as Kahan's log(u) * e / (u - 1) (u - 1 is exact) for x >= -5 (u in [1, 2^29]:
// normal), a 4-term series below (relative error < 1e-9 there).
__device__ __forceinline__ float softplus_t(float x) {
#ifdef VBN_ABL_NOSOFTPLUS
  return x;
#endif
  if (x > 20.f) return x;
  const float e = __expf(x);
  if (x < -5.f) return e * (1.f - e * (0.5f - e * (0.33333334f - e * 0.25f)));
  const float u = 1.0f + e;
  return log_hw(u) * (e * __builtin_amdgcn_rcpf(u - 1.0f));   // u - 1 >= e^-5: normal
}

// Philox-2x32-10 counter-based RNG (Random123): counter (c0, c1), 32-bit key; one
// v_mad_u64_u32 and one three-input XOR (gfx950 v_bitop3_b32, truth table 0x96) per round.
__device__ __forceinline__ uint2 philox2x32(uint2 c, uint32_t k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p = (uint64_t)0xD256D193u * c.x;
    c = make_uint2(__builtin_amdgcn_bitop3_b32((uint32_t)(p >> 32), k, c.y, 0x96), (uint32_t)p);
    k += 0x9E3779B9u;
  }
  return c;
}

__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }

// r = sqrt(-2 ln u1) with u1 in [2^-24, 1] (normal) on v_log_f32 / v_sqrt_f32 (-2 ln u1 in
// [0, 33.3]: normal or 0)
__device__ __forceinline__ float bm_radius(float u1) {
  return __builtin_amdgcn_sqrtf(-2.0f * log_hw(u1));
}

__device__ __forceinline__ float box_muller(uint32_t a, uint32_t b) {
  const float u1 = (float)((a >> 8) + 1u) * (1.0f / 16777216.0f);  // (0,1]
  const float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
  return bm_radius(u1) * __builtin_amdgcn_cosf(u2);                 // cos(2*pi*u2)
}

struct Lane {
  const float* P;        // parameter blob (from a __restrict__ kernel argument)
  const int32_t* ic;     // parent column slots (from a __restrict__ kernel argument)
  float* vals;   // LDS [n_slots][64]
  float* scr;    // LDS [max_out][64]
  const float* wb;  // LDS: this step's weight block (wblk, staged one step ahead by the workgroup)
  int lane;
  int64_t p;     // particle (clamped)
  int64_t b;     // query (Gibbs: chain)
  int s;         // sample (Gibbs: candidate)
  int iter;      // Gibbs sweep (0 for every other walk)
  bool valid;    // particle index inside the batch
  bool mirror;   // half-wave launch: lanes 32-63 mirror lanes 0-31 (kind-set bit 6)
  bool lean;     // no injected draws, no segment state, not Gibbs (kind-set bit 7): the
                 // kernel sets these from KM, so every inlined check on them folds away
  bool noiseless;  // no injected draws (lean, or kind-set bit 8: production Gibbs)
  bool wq;       // every lane of the wave is in the same query (S a multiple of the wave's particles)
  mutable float bm_spare;  // lean walks: the r sin half of a VBN_F_BM_FIRST step's Box-Muller pair
};

// Draws of node ``st``, dimension d, for this particle.  Stream 0 gives a standard normal
// (Box-Muller on both words), stream 1 two uniforms: the categorical / index choice and the
// within-bin uniform, stream 2 the Gibbs chain choice (one per chain and sweep).  Counter =
// (sample, query ^ seed_hi), key = seed_lo + stream id, where the query key is 0 for draws
// shared by all queries (root nodes in MCM/LW/ancestral, Q5).  Stream id = offset[8] |
// node[14] | dim[8] | stream[2]: disjoint for every (node, dim, stream) the host admits
// (PackedModel: < 16384 nodes, < 256 dims per node).
// With injected noise (parity tests) slot 0 = categorical uniform, slot 1 = normal / uniform.
#define RNG_NORMAL 0
#define RNG_UNIFORM 1
#define RNG_SELECT 2
__device__ __forceinline__ uint2 rng_words(const vbn_walk_args& A, const vbn_step& st, int d, int stream,
                                           const Lane& L) {
  const uint32_t qkey = (st.flags & VBN_F_SHARED) ? 0u : (uint32_t)(A.q_base + L.b + 1);
  const uint32_t sid = ((uint32_t)(A.offset & 0xffu) << 24) | ((uint32_t)st.node_id << 10) |
                       ((uint32_t)d << 2) | (uint32_t)stream;
  const uint32_t ctr = (uint32_t)L.s + (uint32_t)L.iter * (uint32_t)A.n_samples;
  return philox2x32(make_uint2(ctr, qkey ^ (uint32_t)(A.seed >> 32)), (uint32_t)A.seed + sid);
}

__device__ __forceinline__ int64_t noise_index(const vbn_walk_args& A, const vbn_step& st, int d, int slot,
                                               const Lane& L) {
  const int64_t bq = A.noise_b == 1 ? 0 : L.b;
  const int64_t stride_slot = (int64_t)A.noise_b * A.n_samples * A.dmax;
  const int64_t stride_iter = (int64_t)A.n_noise * 2 * stride_slot;       // Gibbs sweeps
  return (int64_t)L.iter * stride_iter + ((int64_t)st.noise_idx * 2 + slot) * stride_slot +
         (bq * A.n_samples + L.s) * A.dmax + d;
}

__device__ __forceinline__ float draw_normal(const vbn_walk_args& A, const vbn_step& st, int d, const Lane& L) {
  if (!L.noiseless && A.noise) return A.noise[noise_index(A, st, d, 1, L)];
#ifdef VBN_ABL_NORNG
  return 0.5f;
#endif
  // lean walks pair the dim-0 normals of consecutive one-dimensional gaussian steps (host flags,
  // plan.py _pair_normals): the first step's Philox pair gives r cos(2 pi u2) to itself and
  // r sin(2 pi u2) -- an independent N(0, 1) -- to the second, halving Philox + log + sqrt
  if (L.lean && d == 0 && (st.flags & VBN_F_BM_SECOND)) return L.bm_spare;
  const uint2 w = rng_words(A, st, d, RNG_NORMAL, L);
  if (L.lean && d == 0 && (st.flags & VBN_F_BM_FIRST)) {
    const float u1 = (float)((w.x >> 8) + 1u) * (1.0f / 16777216.0f);
    const float u2 = (float)(w.y >> 8) * (1.0f / 16777216.0f);
    const float r = bm_radius(u1);
    L.bm_spare = r * __builtin_amdgcn_sinf(u2);
    return r * __builtin_amdgcn_cosf(u2);
  }
  return box_muller(w.x, w.y);
}

// (categorical uniform, within-bin uniform)
__device__ __forceinline__ float2 draw_uniforms(const vbn_walk_args& A, const vbn_step& st, int d, const Lane& L) {
  if (!L.noiseless && A.noise)
    return make_float2(A.noise[noise_index(A, st, d, 0, L)], A.noise[noise_index(A, st, d, 1, L)]);
  const uint2 w = rng_words(A, st, d, RNG_UNIFORM, L);
  return make_float2(u01(w.x), u01(w.y));
}

// Read-only buffers (parameter blob, slot lists, evidence) seen through the constant address
// space: wave-uniform reads become scalar loads (s_load, lgkmcnt) instead of vector loads.
typedef __attribute__((address_space(4))) const float cfloat;
typedef __attribute__((address_space(4))) const int32_t cint;
#define CP(p) ((cfloat*)(p))
#define CI(p) ((cint*)(p))

__device__ __forceinline__ float vread(const Lane& L, int slot) { return L.vals[slot * WAVE + L.lane]; }
__device__ __forceinline__ void vwrite(const Lane& L, int slot, float v) { L.vals[slot * WAVE + L.lane] = v; }

__device__ __forceinline__ float fixed_value(const vbn_walk_args& A, const vbn_step& st, int d,
                                             const Lane& L) {
  if (!A.fixed_per_particle && L.wq) {               // one query per wave: a scalar load
    const int64_t b = ((int64_t)__builtin_amdgcn_readfirstlane((int)(L.b >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)L.b);
    return CP(A.fixed)[b * A.fixed_ld + st.fixed_col + d];
  }
  const int64_t row = A.fixed_per_particle ? L.p : L.b;
  return A.fixed[row * A.fixed_ld + st.fixed_col + d];
}

// likelihood weighting's clamp_evidence (_core.py:112-114) on the value read, for steps with
// VBN_F_CLAMP_EV: the unclamped fixed buffer of importance sampling serves its fallback as is
__device__ __forceinline__ float fixed_read(const vbn_walk_args& A, const vbn_step& st, int d, const Lane& L) {
  const float v = fixed_value(A, st, d, L);
  if (st.flags & VBN_F_CLAMP_EV) return v != v ? 0.f : fminf(fmaxf(v, -1e6f), 1e6f);
  return v;
}

// VBN_F_PRECOMP: this sample's row of the node's pre-pass quantities (state_flags 4: state =
// the one-query pre-pass walk's out_x [S][stride]; aux2 = first column | stride << 16)
__device__ __forceinline__ const float* precomp_row(const vbn_walk_args& A, const vbn_step& st, const Lane& L) {
  const int col = st.aux2 & 0xffff, stride = (int)((unsigned)st.aux2 >> 16);
  return A.state + (int64_t)L.s * stride + col;
}

// VBN_F_PRECOMP | VBN_F_PRECOMP_Q: this query's row of the per-query pre-pass quantities
// (precomp_q [B][stride]); one query per wave (host: n_samples % 64 == 0), so the row address is
// wave-uniform and its reads are scalar loads
__device__ __forceinline__ const cfloat* precomp_qrow(const vbn_walk_args& A, const vbn_step& st, const Lane& L) {
  const int col = st.aux2 & 0xffff, stride = (int)((unsigned)st.aux2 >> 16);
  const int64_t b = ((int64_t)__builtin_amdgcn_readfirstlane((int)(L.b >> 32)) << 32) |
                    (uint32_t)__builtin_amdgcn_readfirstlane((int)L.b);
  return CP(A.precomp_q) + b * stride + col;
}

// value of a fixed node: from the fixed buffer, or (VBN_F_KEEP, Gibbs) the slot's current value
__device__ __forceinline__ float node_fixed(const vbn_walk_args& A, const vbn_step& st, int d,
                                            const Lane& L) {
  return (!L.lean && (st.flags & VBN_F_KEEP)) ? vread(L, st.out_col + d) : fixed_read(A, st, d, L);
}

// LDS staging (the walk kernels' weight blocks, the table walk's tables)
typedef __attribute__((address_space(3))) void lds_void;
#define WBLK_CHUNK 256   // floats per global_load_lds_dwordx4 wave instruction (64 lanes x 16 B)
