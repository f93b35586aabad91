#pragma once
// vbn_walk_kernel.h -- the walk itself: Gibbs roles, walk_step, weight-block staging, the fused
// posterior-summary epilogue, vbn_walk_kernel and the list of instantiated kind sets (part of
// vbn_walk_impl.h).
#include "vbn_walk_kde.h"

// ------------------------------------------------------------------------------------------
// Gibbs sweep steps (gibbs.py:40-87): lanes 8c .. 8c+7 hold chain c's 8 candidates
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void gibbs_select(const vbn_walk_args& A, const vbn_step& st, Lane& L, float lp) {
  const int lane = L.lane, g0 = lane & ~7;
  float m = fmaxf(lp, __shfl_xor(lp, 1));
  m = fmaxf(m, __shfl_xor(m, 2));
  m = fmaxf(m, __shfl_xor(m, 4));
  const float e = __expf(lp - m);                       // softmax(log_score, 1) (79)
  float se = e + __shfl_xor(e, 1);
  se += __shfl_xor(se, 2);
  se += __shfl_xor(se, 4);
  float pk[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) pk[k] = __shfl(e, g0 + k) / se;
  // one uniform per chain (candidate lane 0's draw), multinomial(weights, 1) (80); without
  // injected noise it comes from the node's own SELECT stream, which no candidate draw uses
  const int s_keep = L.s;
  L.s = 0;
  const float u = (!L.noiseless && A.noise) ? draw_uniforms(A, st, 0, L).x : u01(rng_words(A, st, 0, RNG_SELECT, L).x);
  L.s = s_keep;
  const int idx = inv_cdf(8, u, [&](int k) { return pk[k]; });
  for (int d = 0; d < st.out_dim; ++d) {
    const float v = __shfl(vread(L, st.out_col + d), g0 + idx);
    wave_sync();
    vwrite(L, st.out_col + d, v);                        // chosen candidate (81-82)
  }
}

__device__ __forceinline__ void gibbs_collect(const vbn_walk_args& A, const vbn_step& st, const Lane& L) {
  const int it = L.iter, burn = A.gibbs_burn_in, thin = max(A.gibbs_thin, 1);
  if (it < burn || (it - burn) % thin != 0 || L.s != 0 || !L.valid || (L.mirror && L.lane >= 32)) return;  // 83-87
  const int n_collect = (A.gibbs_iters - burn + thin - 1) / thin;
  const int k = (it - burn) / thin;
  for (int d = 0; d < st.out_dim; ++d)
    A.out_x[(L.b * n_collect + k) * A.n_out_cols + d] = vread(L, st.out_col + d);
}

// ------------------------------------------------------------------------------------------
// the walk
// ------------------------------------------------------------------------------------------
// One step of the walk for the wave's 64 particles.
// KM: bit0 gaussian_nn, bit1 linear_gaussian, bit2 mdn, bit3 kde, bit4 softmax_nn,
// bit5 non-relu activations, bit9 the out-of-line steps (generic MLPs, rff_gaussian).  Each
// instantiation only carries the code (and registers) of the CPD kinds a plan uses.
template <unsigned KM>
__device__ __forceinline__ void walk_step(const vbn_walk_args& A, const vbn_step& st, Lane& L, float& lp) {
  if (st.role == VBN_ROLE_SKIP) return;
  if (!L.lean && (st.flags & VBN_F_LPRESET)) lp = 0.f;
  if (!L.lean && st.role == VBN_ROLE_SELECT) {        // Gibbs roles: not in lean walks
    gibbs_select(A, st, L, lp);
    wave_sync();
    return;
  }
  if (!L.lean && st.role == VBN_ROLE_COLLECT) {
    gibbs_collect(A, st, L);
    return;
  }
  if ((st.flags & VBN_F_PRE_OUT) && st.kind != VBN_KIND_KDE) {   // shared-sample pre-pass: the
    if constexpr ((KM & VBN_KM_NN_KINDS) != 0) {                      // NN CPD's head outputs
      if (st.kind == VBN_KIND_GAUSSIAN_NN && st.out_dim == 1) run_mlp<KM, 2>(A, st, L, [] {});
      else run_mlp<KM>(A, st, L, [] {});
      for (int j = 0; j < st.n_out; ++j) vwrite(L, st.out_col + j, L.scr[j * WAVE + L.lane]);
    }
    wave_sync();
    return;
  }
  if (st.role == VBN_ROLE_FIXED && !(st.flags & VBN_F_LOGP)) {   // evidence / do: value only
    for (int d = 0; d < st.out_dim; ++d) vwrite(L, st.out_col + d, node_fixed(A, st, d, L));
    wave_sync();
    return;
  }
  // rff_gaussian runs out of line in the kind sets with bit 9 only (its plans set the bit, as
  // generic-MLP plans do).  It is tested here and not as a case of the switch below, whose
  // default is softmax_nn: a sixth case changed the code of every other instantiation
  if constexpr ((KM & VBN_KM_GENERIC_MLP) != 0) {
    if (st.kind == VBN_KIND_RFF_GAUSSIAN) {
      step_rff_gaussian<KM>(A, st, L, lp);
      wave_sync();
      return;
    }
  }
  switch (st.kind) {
    case VBN_KIND_GAUSSIAN_NN: if constexpr ((KM & 1) != 0) step_gaussian_nn<KM>(A, st, L, lp); break;
    case VBN_KIND_LINEAR_GAUSSIAN: if constexpr ((KM & 2) != 0) step_linear_gaussian(A, st, L, lp); break;
    case VBN_KIND_MDN: if constexpr ((KM & 4) != 0) step_mdn<KM>(A, st, L, lp); break;
    case VBN_KIND_KDE: if constexpr ((KM & 8) != 0) step_kde(A, st, L, lp); break;
    default: if constexpr ((KM & 16) != 0) step_softmax_nn<KM>(A, st, L, lp); break;
  }
  wave_sync();
}

// Staged walks (kind sets of gaussian_nn / linear_gaussian only): NN weight blocks are DMA'd
// into LDS one step ahead and shared by the 4 waves of a workgroup, one barrier per step.
// Measured on MI355X (walk ms, staged vs direct): cfg2 1.22 vs 1.35; with mdn/softmax_nn heads
// (cfg3) 4.43 vs 4.26 and with KDE nodes (cfg5) 186 vs 166 (per-wave work varies by node, the
// barrier waits for the slowest wave) -- those kind sets read the blob straight (L1/L2).
#ifndef VBN_STAGE
#define VBN_STAGE 1
#endif
__host__ __device__ constexpr bool staged_kinds(unsigned km) {
  return VBN_STAGE && (km & VBN_KM_UNSTAGED_KINDS) == 0;
}
#define WG_MAX_WAVES 4

// Stage step j's NN weight block into LDS weight buffer ``buf``: the workgroup's waves split
// its 1-KiB chunks, one global_load_lds_dwordx4 each (no VGPRs; completion is waited for by
// step_barrier before the step that reads it).
__device__ __forceinline__ void stage_block(const vbn_walk_args& A, const vbn_step* __restrict__ steps,
                                            const float* __restrict__ params, float* wbuf, int j, int buf,
                                            int wave, int nw, int lane) {
  const int off = steps[j].wblk_off, len = steps[j].wblk_len;
  if (len <= 0) return;
  float* dst = wbuf + buf * A.wbuf_floats;
  for (int c = wave; c * WBLK_CHUNK < len; c += nw)
    __builtin_amdgcn_global_load_lds((const void*)(params + off + c * WBLK_CHUNK + lane * 4),
                                     (lds_void*)(dst + c * WBLK_CHUNK), 16, 0, 0);
}

// first step >= j that runs an MLP (has a weight block), or -1
__device__ __forceinline__ int first_mlp(const vbn_step* __restrict__ steps, int j, int n) {
  for (; j < n; ++j)
    if (CI(steps)[j * (int)(sizeof(vbn_step) / 4) + (int)(__builtin_offsetof(vbn_step, wblk_len) / 4)] > 0) return j;
  return -1;
}

// start of an MLP step: this wave's LDS-DMA of the step's block has landed, every wave of the
// workgroup is done with the buffer the next MLP step's prefetch overwrites
__device__ __forceinline__ void step_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef VBN_ABL_NOBAR
  return;
#endif
  __syncthreads();
}

// (ABI v13) Posterior-summary partials of VBN._posterior_stats (vbn.py:495-503) fused into an
// MCM walk's epilogue: the wave's 64 particles all belong to query L.b (n_samples % 64 == 0), so
// it reduces their weights w = pdf (nan / inf -> 0, clamped >= 0) and target values in float64
// with xor butterflies (every lane ends with the same sums) and lane 0 writes one row of
// vbn_walk_args.stats_part: [W, Q, per output column: m_w, M2_w, m_u, M2_u] (two-pass inside the
// wave: the mean first, then the centred second moment around it).  A zero-weight wave keeps
// m_w = sum w x (0, or NaN when a sample is NaN as in the reference's 0 * NaN).
// vbn_hip_posterior_stats_merge combines a query's S / 64 rows.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ void stats_partials(const vbn_walk_args& A, const Lane& L, float pdf) {
  const int D = A.n_out_cols;
  const double w = (pdf != pdf || pdf == INFINITY || pdf == -INFINITY) ? 0.0 : (double)fmaxf(pdf, 0.f);
  const double W = wave_sum_f64(w), Q = wave_sum_f64(w * w);
  const int stride = 2 + 4 * D;
  double* row = A.stats_part + ((int64_t)L.b * (A.n_samples >> 6) + (L.s >> 6)) * stride;
  if (L.lane == 0) {
    row[0] = W;
    row[1] = Q;
  }
  for (int d = 0; d < D; ++d) {
    const double x = (double)vread(L, A.out_cols[d]);
    const double sx = wave_sum_f64(w * x);
    const double mw = W > 0.0 ? sx / W : sx;
    const double cw = x - mw;
    const double m2w = wave_sum_f64(w * (cw * cw));
    const double mu = wave_sum_f64(x) * (1.0 / 64.0);
    const double cu = x - mu;
    const double m2u = wave_sum_f64(cu * cu);
    if (L.lane == 0) {
      row[2 + 4 * d] = mw;
      row[3 + 4 * d] = m2w;
      row[4 + 4 * d] = mu;
      row[5 + 4 * d] = m2u;
    }
  }
}

// The walk.  A workgroup = nw (1, 2 or 4; blockDim.x / 64) waves, each owning 64 consecutive
// particles with its own LDS value slots; the waves walk the same step table in lockstep (one
// barrier per step) and share two LDS weight buffers: while step i runs on buffer i & 1, step
// i + 1's MLP weights are DMA'd into the other one (one memory latency per step, hidden
// behind the step's compute, and one copy per workgroup instead of per wave).
#ifndef VBN_WPE
#define VBN_WPE 4
#endif
template <unsigned KM>
__global__ void __launch_bounds__(WG_MAX_WAVES * WAVE) __attribute__((amdgpu_waves_per_eu(VBN_WPE)))
vbn_walk_kernel(const vbn_walk_args A, const float* __restrict__ params, const vbn_step* __restrict__ steps,
                const int32_t* __restrict__ in_cols) {
  if (A.run_if && *A.run_if == 0) return;            // predicated launch, not needed (uniform)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int per_wave = (A.n_slots + (A.max_out > 0 ? A.max_out : 1)) * WAVE;
  float* wbuf = smem + nw * per_wave;
  Lane L;
  L.P = params;
  L.ic = in_cols;
  L.lane = threadIdx.x & (WAVE - 1);
  L.vals = smem + wave * per_wave;
  L.scr = L.vals + A.n_slots * WAVE;
  L.wb = wbuf;
  const int64_t total = A.n_queries * (int64_t)A.n_samples;
  // half-wave launches (wave_particles 32): lane l and l + 32 carry the same particle, so
  // every draw and value agrees; only the lower half writes, the MLPs run group 0 only
  L.mirror = (KM & VBN_KM_HALFWAVE) != 0;            // host: wave_particles == 32
  L.lean = (KM & VBN_KM_LEAN) != 0;                  // host: no noise, no state, not Gibbs
  L.noiseless = (KM & (VBN_KM_LEAN | VBN_KM_NOISELESS)) != 0;   // host: no injected draws
  L.bm_spare = 0.f;
  const int wp = L.mirror ? 32 : WAVE;
  L.wq = A.mode != VBN_MODE_GIBBS && (A.n_samples & (wp - 1)) == 0;
  const int64_t p_raw = ((int64_t)blockIdx.x * nw + wave) * wp + (L.lane & (wp - 1));
  const bool valid = p_raw < total;
  L.p = valid ? p_raw : total - 1;
  L.b = L.p / A.n_samples;
  L.s = (int)(L.p - L.b * A.n_samples);
  L.iter = 0;
  L.valid = valid;

  float lp = 0.f;
  if (!L.lean && A.state && (A.state_flags & 1)) {  // resume a segmented walk
    for (int c = 0; c < A.n_slots; ++c) vwrite(L, c, A.state[(int64_t)c * total + L.p]);
    lp = A.state[(int64_t)A.n_slots * total + L.p];
    wave_sync();
  }
  const int iters = (!L.lean && A.mode == VBN_MODE_GIBBS) ? A.gibbs_iters : 1;
  if constexpr (staged_kinds(KM)) {
  // Only MLP steps (wblk_len > 0) touch the weight buffers, so only they synchronise: MLP step
  // k waits for its block (DMA'd during MLP step k - 1), then, once every wave is past that
  // barrier (so done with the other buffer), DMAs MLP step k + 1's block into it.  The DMA
  // overlaps MLP step k and every root / evidence step up to k + 1.
  int par = 0;
  int nxt = first_mlp(steps, 0, A.n_steps);
  if (nxt >= 0) stage_block(A, steps, params, wbuf, nxt, 0, wave, nw, L.lane);
  for (int it = 0; it < iters; ++it) {
    L.iter = it;
    for (int i = 0; i < A.n_steps; ++i) {
      if (i == nxt) {
        step_barrier();
        nxt = first_mlp(steps, i + 1, A.n_steps);
        if (nxt < 0 && it + 1 < iters) nxt = first_mlp(steps, 0, A.n_steps);   // next sweep
        if (nxt >= 0) stage_block(A, steps, params, wbuf, nxt, par ^ 1, wave, nw, L.lane);
        L.wb = wbuf + par * A.wbuf_floats;
        par ^= 1;
      }
      walk_step<KM>(A, steps[i], L, lp);
    }
  }
  } else {
  (void)wbuf;
  for (int it = 0; it < iters; ++it) {
    L.iter = it;
    for (int i = 0; i < A.n_steps; ++i) {
      const vbn_step st = steps[i];
      L.wb = params + st.wblk_off;
      walk_step<KM>(A, st, L, lp);
    }
  }
  }
  if (!valid || (L.mirror && L.lane >= 32)) return;
  if (A.mode == VBN_MODE_GIBBS) return;                  // outputs written by COLLECT steps
  if (!L.lean && A.state && (A.state_flags & 2)) {
    for (int c = 0; c < A.n_slots; ++c) A.state[(int64_t)c * total + L.p] = vread(L, c);
    A.state[(int64_t)A.n_slots * total + L.p] = lp;
  }
  if (A.out_lp && A.mode != VBN_MODE_SAMPLE) A.out_lp[L.p] = (A.mode == VBN_MODE_MCM) ? __expf(lp) : lp;
  if (A.out_x) {
    for (int k = 0; k < A.n_out_cols; ++k)
      A.out_x[L.p * A.n_out_cols + k] = vread(L, A.out_cols[k]);
  }
  if (A.stats_part && A.mode == VBN_MODE_MCM && L.wq && !L.mirror) stats_partials(A, L, __expf(lp));
}

// Instantiated kind sets: bits 0-4 the CPD kinds walked, bit 5 non-relu activations, bit 6 the
// half-wave (mirror) launch (include/vbn_hip.h wave_particles = 32), bit 7 the lean walk (no
// injected draws, no segment state, not Gibbs: the production MCM / IS / LW / ancestral path;
// measured cfg2 1.215 -> 1.19 ms, SGPR spills 35 -> 0), bit 8 no injected draws (with bit 6: the
// production half-wave Gibbs sweeps; SGPR spills 34 -> 9), bit 9 the out-of-line steps (plans
// with an NN CPD of hidden_dims other than (32, 32) or with an rff_gaussian node: only with the
// all-kinds set 63, so the out-of-line mlp_generic / rff_loc calls never touch the hot
// instantiations' registers).  Each is compiled in its
// own object from walk_inst.hip (Makefile KIND_SETS must list the same values).
#define VBN_WALK_KIND_SETS(X) \
  X(1) X(2) X(3) X(4) X(8) X(16) X(20) X(23) X(31) X(63) \
  X(65) X(66) X(67) X(68) X(72) X(80) X(84) X(87) X(95) X(127) \
  X(129) X(130) X(131) X(132) X(136) X(144) X(148) X(151) X(159) X(191) \
  X(321) X(322) X(323) X(324) X(328) X(336) X(340) X(343) X(351) X(383) \
  X(575) X(639) X(703) X(895)
#define VBN_LAUNCHER_(K) vbn_launch_walk_km##K
#define VBN_LAUNCHER(K) VBN_LAUNCHER_(K)
