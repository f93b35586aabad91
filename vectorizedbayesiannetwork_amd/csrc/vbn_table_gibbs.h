#pragma once
// vbn_table_gibbs.h -- gfx950 (MI355X) Gibbs sweeps for networks whose every CPD is a
// categorical_table (reference vbn/sampling/gibbs.py:36-87 over vbn/cpds/categorical_table.py
// sample / log_prob), launched by vbn_hip_table_walk with mode GIBBS.  Part of
// vbn_table_walk.hip, which defines TW_WAVES and TW_ROW_VEC before it includes this header.
//
// Lane = (chain, candidate): lanes 8c .. 8c+7 of a wave64 hold chain c's 8 candidates (the
// convention of gibbs_select in vbn_walk_kernel.h, so the start state and the injected draws keep
// their layouts), 8 chains per wave, TW_WAVES waves per workgroup, every sweep in one launch.
// A node's state is its class INDEX per output dim in the lane's own column of the LDS slots
// idx[slot][64]: between SELECT steps the 8 lanes of a chain hold the same column, a LATENT step
// puts one candidate in each.  A lane reads no other lane's column, so the sweep loop has no LDS
// hand-off and no barrier; the only cross-lane traffic is SELECT's, in registers.
//
// The sweep table is plan.build_gibbs_plan's, per latent node:
//   LATENT (F_LPRESET)       q from the chain's current parent indices, one inverse-CDF draw per
//                            output dim on the off_w1 row (the table walk's rule: the smallest k
//                            with cdf[k] > u cdf[C-1], else C - 1), candidate index into the
//                            lane's column, score = sum_d off_pts row[k_d]
//   FIXED + KEEP + LOGP      one per child: the child's index from its slot (evidence and do nodes
//                            hold theirs from the start state), q from the parents' slots -- the
//                            updated node's holds this lane's candidate --, score += log-prob
//   SELECT                   softmax over the chain's 8 scores, one uniform per chain, inverse
//                            CDF over the 8 weights, the chosen candidate's indices to all 8 lanes
// and one COLLECT at the end: at collected sweeps the chain's lane 0 writes the target's class
// VALUES (off_w3[k]) to out_x[(chain * n_collect + j) * out_dim + d].
//
// Every term is one row gather from the blob plan._pack_table packs, staged into LDS once per
// workgroup when tw_shape allows (the blob is then read from LDS in every one of the sweeps),
// gathered from global / L2 otherwise: the same floats, the same arithmetic, identical outputs.
// Every class, configuration and blob index is clamped as in the table walk; lanes past the
// last chain clamp to the last chain and write nothing.

// parent configuration of step st from this lane's column of the slots
__device__ __forceinline__ int tg_config(const vbn_walk_args& A, const vbn_step& st, const float* __restrict__ params,
                                         const int32_t* __restrict__ in_cols, const int* idx, int lane, int P) {
  const cint* hdr = CI(params) + st.off_tail;
  int q = 0;
  for (int j = 0; j < st.n_in; ++j) {
    const int slot = min(max(CI(in_cols)[st.in_off + j], 0), A.n_slots - 1);
    const int stride = hdr[2 * j], card = hdr[2 * j + 1];
    q += min(max(idx[slot * WAVE + lane], 0), card - 1) * stride;
  }
  return min(max(q, 0), P - 1);
}

// the table walk's inverse-CDF pick on one row: the count of entries of cdf[0 .. C-2] that are <= thr
__device__ __forceinline__ int tg_pick(const float* cdf, float u, int C, int Cp) {
  const float thr = u * cdf[C - 1];
  int k = 0;
  if (Cp <= TW_ROW_VEC) {
    for (int c4 = 0; c4 < Cp; c4 += 4) {
      const float4 v = *reinterpret_cast<const float4*>(cdf + c4);
      k += (c4 + 0 < C - 1 && v.x <= thr) + (c4 + 1 < C - 1 && v.y <= thr) + (c4 + 2 < C - 1 && v.z <= thr) +
           (c4 + 3 < C - 1 && v.w <= thr);
    }
  } else {
    int lo = 0, hi = C - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] <= thr) lo = mid + 1; else hi = mid;
    }
    k = lo;
  }
  return min(max(k, 0), C - 1);
}

// SELECT (gibbs.py:79-82) for the 8 lanes of a chain: returns the chosen candidate (0..7), the
// same in all 8.  The weights' running sums are an 8-lane prefix scan in registers; every lane
// compares its own sum with u x total and the first lane that passes is read off the wave's
// ballot, so the pick costs no loop over the candidates.
__device__ __forceinline__ int tg_select(float score, float u, int lane) {
  const int c = lane & 7, g0 = lane & ~7;
  float m = fmaxf(score, __shfl_xor(score, 1));
  m = fmaxf(m, __shfl_xor(m, 2));
  m = fmaxf(m, __shfl_xor(m, 4));
  float cum = __expf(score - m);                       // softmax(log_score, 1) up to its total
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    const float below = __shfl_up(cum, o, 8);
    cum += c >= o ? below : 0.f;
  }
  const float thr = u * __shfl(cum, g0 + 7);           // multinomial(weights, 1): u x total
  const unsigned long long hits = __ballot(c < 7 && cum > thr);
  const unsigned mine = (unsigned)(hits >> g0) & 0x7fu;
  return mine ? __builtin_ctz(mine) : 7;
}

template <bool STAGED>
__global__ void __launch_bounds__(TW_WAVES* WAVE)
vbn_table_gibbs_kernel(const vbn_walk_args A, const float* __restrict__ params, const vbn_step* __restrict__ steps,
                       const int32_t* __restrict__ in_cols, const int blob_floats) {
  if (A.run_if && *A.run_if == 0) return;            // predicated launch, not needed (uniform)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & (WAVE - 1);
  const float* T = params;
  int* idx = reinterpret_cast<int*>(smem) + wave * A.n_slots * WAVE;
  if (STAGED) {
    // the whole blob once per workgroup, as in the table walk: 1-KiB chunks split over the waves
    for (int c = wave; c * WBLK_CHUNK < blob_floats; c += nw)
      __builtin_amdgcn_global_load_lds((const void*)(params + c * WBLK_CHUNK + lane * 4),
                                       (lds_void*)(smem + c * WBLK_CHUNK), 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    T = smem;
    idx = reinterpret_cast<int*>(smem + blob_floats) + wave * A.n_slots * WAVE;
  }
  const int t_max = blob_floats - 1;
  Lane L;
  L.P = params;
  L.ic = in_cols;
  L.lane = lane;
  L.vals = smem;
  L.scr = smem;
  L.wb = params;
  L.mirror = false;
  L.lean = false;
  L.noiseless = A.noise == nullptr;
  L.bm_spare = 0.f;
  const int64_t total = A.n_queries * (int64_t)A.n_samples;     // n_samples = 8 candidates
  const int64_t p_raw = ((int64_t)blockIdx.x * nw + wave) * WAVE + lane;
  const bool valid = p_raw < total;                   // whole chains: total is a multiple of 8
  L.p = valid ? p_raw : total - 1;
  L.b = L.p / A.n_samples;
  L.s = (int)(L.p - L.b * A.n_samples);
  L.iter = 0;
  L.valid = valid;
  L.wq = false;

  // the start state: one ancestral table walk's class indices, every candidate lane the chain's
  for (int c = 0; c < A.n_slots; ++c) idx[c * WAVE + lane] = __float_as_int(A.state[(int64_t)c * total + L.p]);

  const int burn = A.gibbs_burn_in, thin = max(A.gibbs_thin, 1);
  const int n_collect = (A.gibbs_iters - burn + thin - 1) / thin;
  float score = 0.f;
  for (int it = 0; it < A.gibbs_iters; ++it) {
    L.iter = it;
    for (int i = 0; i < A.n_steps; ++i) {
      const vbn_step st = steps[i];                    // wave-uniform: scalar loads
      if (st.kind != VBN_KIND_CATEGORICAL_TABLE || st.role == VBN_ROLE_SKIP) continue;
      const int C = max(st.k, 1), P = max(st.aux0, 1), Cp = max(st.aux1, C), D = st.out_dim;
      if (st.role == VBN_ROLE_SELECT) {
        // one uniform per chain: candidate lane 0's draw, computed alike by the chain's 8 lanes
        const int s_keep = L.s;
        L.s = 0;
        const float u = A.noise ? A.noise[noise_index(A, st, 0, 0, L)] : u01(rng_words(A, st, 0, RNG_SELECT, L).x);
        L.s = s_keep;
        const int src = (lane & ~7) + tg_select(score, u, lane);
        for (int d = 0; d < D; ++d) {
          int* cell = idx + min(max(st.out_col + d, 0), A.n_slots - 1) * WAVE + lane;
          *cell = __shfl(*cell, src);
        }
        continue;
      }
      if (st.role == VBN_ROLE_COLLECT) {
        if (it < burn || (it - burn) % thin != 0 || L.s != 0 || !valid) continue;
        const int j = (it - burn) / thin;
        for (int d = 0; d < D; ++d) {
          const int k = min(max(idx[min(max(st.out_col + d, 0), A.n_slots - 1) * WAVE + lane], 0), C - 1);
          A.out_x[(L.b * n_collect + j) * A.n_out_cols + d] = T[min(max(st.off_w3 + d * Cp + k, 0), t_max)];
        }
        continue;
      }
      const bool latent = st.role == VBN_ROLE_LATENT;
      // a FIXED row of a sweep scores the child's current index; any other FIXED row does nothing
      if (!latent && (st.role != VBN_ROLE_FIXED || (st.flags & (VBN_F_KEEP | VBN_F_LOGP)) != (VBN_F_KEEP | VBN_F_LOGP)))
        continue;
      if (st.flags & VBN_F_LPRESET) score = 0.f;
      const int q = tg_config(A, st, params, in_cols, idx, lane, P);
      for (int d = 0; d < D; ++d) {
        const int row = (d * P + q) * Cp;
        int* cell = idx + min(max(st.out_col + d, 0), A.n_slots - 1) * WAVE + lane;
        int k;
        if (latent) {
          const float u = A.noise ? A.noise[noise_index(A, st, d, 0, L)] : u01(rng_words(A, st, d, RNG_UNIFORM, L).x);
          k = tg_pick(T + min(max(st.off_w1 + row, 0), t_max - Cp + 1), u, C, Cp);
          *cell = k;
        } else {
          k = min(max(*cell, 0), C - 1);
        }
        if (st.flags & VBN_F_LOGP) score += T[min(max(st.off_pts + row + k, 0), t_max)];
      }
    }
  }
}
