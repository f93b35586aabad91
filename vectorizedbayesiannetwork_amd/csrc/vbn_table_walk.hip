// vbn_table_walk.hip — gfx950 (MI355X) particle walk for networks whose every CPD is a
// categorical_table (reference vbn/cpds/categorical_table.py:359-417: _logits_from_parents,
// sample, log_prob), and its C-ABI entry vbn_hip_table_walk (include/vbn_hip.h).
//
// Lane = particle, wave64, as in vbn_walk_kernel.h; the step table, roles, flags, modes, evidence
// buffer, injected draws and Philox keying are the walk's (rng_words / u01 of that header).  A
// node's state is its class INDEX per output dim, kept in LDS slots idx[slot][64] (rows are
// lane-contiguous: no bank conflicts; a lane only ever reads its own column, so the steps need no
// hand-off between lanes).  Everything the reference computes per call from the count table is
// precomputed by the host packer (plan.py _pack_table) into rows of Cp = C rounded up to 4
// floats, one per (output dim d, parent configuration q):
//
//   off_pts  log-prob rows    log_softmax(log(clamp(counts / sum)))                [D][P][Cp]
//   off_w1   inverse-CDF rows cumsum(softmax(logits)), float64 sums rounded once   [D][P][Cp]
//   off_w2   probability rows softmax(logits) (role PARAMS)                        [D][P][Cp]
//   off_w3   class values                                                          [D][Cp]
//   off_b3   valid classes per dim (int32 bits)                                    [D]
//   off_tail per parent column (stride, cardinality) (int32 bits)                  [n_in][2]
//   k = C, aux0 = P (parent configurations), aux1 = Cp
//
// Per step: q = sum_j idx_j stride_j, one row gather, then LATENT: the smallest k with
// cdf[k] > u cdf[C-1] (else C - 1), u = stream RNG_UNIFORM word 0 (or injected slot 0);
// FIXED: the evidence value's index by a search over the node's sorted class values;
// LOGP: one read of the log-prob row; PARAMS: the probability row into the node's slots.
//
// Every class and configuration index is clamped into its table before it is used, so no
// evidence tensor or parent state can make the kernel read outside the blob (the host refuses
// out-of-support values first; one that arrives anyway walks as class 0 with lp = NaN).
//
// Tables small enough (tw_shape below) are staged once per workgroup into LDS with
// global_load_lds_dwordx4 and gathered from there; larger blobs are gathered from global / L2.
// Both paths read the same floats and run the same arithmetic: identical outputs.
#include "vbn_hip.h"
#include "vbn_walk_common.h"

#include <stdlib.h>

#define TW_WAVES 4
#define TW_ROW_VEC 8       // rows of at most this many floats: every entry compared (float4 loads)

template <bool STAGED>
__global__ void __launch_bounds__(TW_WAVES* WAVE)
vbn_table_walk_kernel(const vbn_walk_args A, const float* __restrict__ params, const vbn_step* __restrict__ steps,
                      const int32_t* __restrict__ in_cols, const int blob_floats) {
  if (A.run_if && *A.run_if == 0) return;            // predicated launch, not needed (uniform)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & (WAVE - 1);
  const float* T = params;
  int* idx = reinterpret_cast<int*>(smem) + wave * A.n_slots * WAVE;
  if (STAGED) {
    // the whole table blob, once per workgroup: 1-KiB chunks split over the waves, one
    // global_load_lds_dwordx4 each (blob_floats is a multiple of the chunk, plan.py PackedModel)
    for (int c = wave; c * WBLK_CHUNK < blob_floats; c += nw)
      __builtin_amdgcn_global_load_lds((const void*)(params + c * WBLK_CHUNK + lane * 4),
                                       (lds_void*)(smem + c * WBLK_CHUNK), 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    T = smem;
    idx = reinterpret_cast<int*>(smem + blob_floats) + wave * A.n_slots * WAVE;
  }
  // last float a gather may touch: offsets come from the host packer, the clamps below only keep
  // a corrupt step table inside the blob
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
  const int64_t total = A.n_queries * (int64_t)A.n_samples;
  const int64_t p_raw = ((int64_t)blockIdx.x * nw + wave) * WAVE + lane;
  const bool valid = p_raw < total;
  L.p = valid ? p_raw : total - 1;
  L.b = L.p / A.n_samples;
  L.s = (int)(L.p - L.b * A.n_samples);
  L.iter = 0;
  L.valid = valid;
  L.wq = (A.n_samples & (WAVE - 1)) == 0;             // one query per wave: scalar evidence loads

  float lp = 0.f;
  for (int i = 0; i < A.n_steps; ++i) {
    const vbn_step st = steps[i];                    // wave-uniform: scalar loads
    if (st.kind != VBN_KIND_CATEGORICAL_TABLE || st.role == VBN_ROLE_SKIP) continue;
    const int C = max(st.k, 1), P = max(st.aux0, 1), Cp = max(st.aux1, C), D = st.out_dim;
    const bool reads = st.role != VBN_ROLE_FIXED || (st.flags & VBN_F_LOGP);
    int q = 0;
    if (reads) {
      const cint* hdr = CI(params) + st.off_tail;
      for (int j = 0; j < st.n_in; ++j) {
        const int slot = min(max(CI(in_cols)[st.in_off + j], 0), A.n_slots - 1);
        const int stride = hdr[2 * j], card = hdr[2 * j + 1];
        const int k = min(max(idx[slot * WAVE + lane], 0), card - 1);
        q += k * stride;
      }
      q = min(max(q, 0), P - 1);
    }
    float node_lp = 0.f;
    for (int d = 0; d < D; ++d) {
      const int row = (d * P + q) * Cp;
      if (st.role == VBN_ROLE_PARAMS) {
        const float* pr = T + min(max(st.off_w2 + row, 0), t_max - Cp + 1);
        for (int c = 0; c < C; ++c)
          idx[min(max(st.out_col + d * C + c, 0), A.n_slots - 1) * WAVE + lane] = __float_as_int(pr[c]);
        continue;
      }
      int k = 0;
      bool bad = false;
      if (st.role == VBN_ROLE_LATENT) {
        const float u = A.noise ? A.noise[noise_index(A, st, d, 0, L)] : u01(rng_words(A, st, d, RNG_UNIFORM, L).x);
        const float* cdf = T + min(max(st.off_w1 + row, 0), t_max - Cp + 1);
        const float thr = u * cdf[C - 1];
        if (Cp <= TW_ROW_VEC) {
          // short rows: one or two 16-byte loads, every entry below C - 1 compared
          for (int c4 = 0; c4 < Cp; c4 += 4) {
            const float4 v = *reinterpret_cast<const float4*>(cdf + c4);
            k += (c4 + 0 < C - 1 && v.x <= thr) + (c4 + 1 < C - 1 && v.y <= thr) + (c4 + 2 < C - 1 && v.z <= thr) +
                 (c4 + 3 < C - 1 && v.w <= thr);
          }
        } else {
          // longer rows: the first entry above thr among cdf[0 .. C-2] by bisection (the row is
          // non-decreasing, so this is the count of entries <= thr)
          int lo = 0, hi = C - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] <= thr) lo = mid + 1; else hi = mid;
          }
          k = lo;
        }
      } else {                                        // FIXED: the value's index among the class values
        const float v = fixed_read(A, st, d, L);
        const float* cv = T + min(max(st.off_w3 + d * Cp, 0), t_max - Cp + 1);
        const int nv = min(max(CI(params)[st.off_b3 + d], 1), C);
        int lo = 0, hi = nv;                          // lower bound of v in cv[0 .. nv)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (cv[mid] < v) lo = mid + 1; else hi = mid;
        }
        bad = !(lo < nv && cv[min(lo, nv - 1)] == v);
        k = bad ? 0 : lo;
      }
      k = min(max(k, 0), C - 1);
      idx[min(max(st.out_col + d, 0), A.n_slots - 1) * WAVE + lane] = k;
      if (st.flags & VBN_F_LOGP) {
        const float l = T[min(max(st.off_pts + row + k, 0), t_max)];
        node_lp += bad ? __int_as_float(0x7fc00000) : l;
      }
    }
    if (st.flags & VBN_F_LOGP) lp += node_lp;
  }
  if (!valid) return;
  if (A.out_lp && A.mode != VBN_MODE_SAMPLE) A.out_lp[L.p] = (A.mode == VBN_MODE_MCM) ? __expf(lp) : lp;
  if (A.out_x) {
    // out_cols = [slot per column] ++ [blob offset of the column's class values, or -1 for a
    // PARAMS column, whose slot holds the probability's bits]
    for (int c = 0; c < A.n_out_cols; ++c) {
      const int slot = min(max(CI(A.out_cols)[c], 0), A.n_slots - 1);
      const int cvo = CI(A.out_cols)[A.n_out_cols + c];
      const int k = idx[slot * WAVE + lane];
      A.out_x[L.p * A.n_out_cols + c] = cvo < 0 ? __int_as_float(k) : T[min(max(cvo + k, 0), t_max)];
    }
  }
}

// ------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------
int vbn_fail(int code, const char* msg);              // vbn_walk.hip (sets vbn_hip_last_error)

// Staging budget.  The kernel needs 40 (staged) / 42 (global) VGPRs and no scratch (make
// table-resources), which leaves the full 8 waves per SIMD, i.e. 8 workgroups of 4 waves per CU,
// so LDS is what limits residency.  A plan stages its tables when that keeps as many workgroups
// resident per CU (160 KiB) as the unstaged launch would have, and the workgroup stays within
// the 64 KiB a launch may ask for without an opt-in attribute.  Staging at the price of
// residency loses: 4096 x 1024 particles, 4 classes, walk ms global vs staged -- 24 nodes (25 KiB
// of tables, 4 instead of 8 workgroups per CU) 0.43 vs 0.47, 40 nodes (42 KiB, 2 instead of 8)
// 0.70 vs 1.26.  VBN_TABLE_GLOBAL=1 (read at every call) forces the global path.
#define TW_LDS_CU (160 * 1024)
#define TW_LDS_WG_MAX (64 * 1024)
#define TW_WG_PER_CU 8

struct tw_launch {
  int nw;            // waves per workgroup
  bool stage;        // tables staged into LDS
  size_t lds;
};

static int tw_check(const vbn_walk_args* a) {
  if (!a || (!a->steps && a->n_steps > 0) || a->n_steps < 0 || !a->params || a->n_samples <= 0 ||
      a->n_queries <= 0 || a->n_slots <= 0 || !a->in_cols)
    return vbn_fail(VBN_E_ARGS, "vbn_hip_table_walk: bad arguments");
  if (a->kind_mask != VBN_KM_TABLE)
    return vbn_fail(VBN_E_ARGS, "vbn_hip_table_walk: only plans whose every step is a categorical_table "
                                "(kind_mask 1024)");
  if (a->state || a->state_flags || a->precomp_q || a->stats_part || a->wave_particles == 32 ||
      (a->mode != VBN_MODE_MCM && a->mode != VBN_MODE_WEIGHTED && a->mode != VBN_MODE_SAMPLE))
    return vbn_fail(VBN_E_ARGS, "vbn_hip_table_walk: segment state, precomputed quantities, fused statistics, "
                                "half waves and Gibbs sweeps are not implemented for table walks");
  if (a->out_x && (!a->out_cols || a->n_out_cols <= 0))
    return vbn_fail(VBN_E_ARGS, "vbn_hip_table_walk: out_x without out_cols");
  if (a->wbuf_floats <= 0 || (a->wbuf_floats % WBLK_CHUNK) != 0)
    return vbn_fail(VBN_E_ARGS, "vbn_hip_table_walk: wbuf_floats must be the blob length in floats, a positive "
                                "multiple of 256");
  if (a->noise && (a->dmax <= 0 || (a->noise_b != 1 && a->noise_b != a->n_queries)))
    return vbn_fail(VBN_E_ARGS, "vbn_hip_table_walk: bad injected-draw shape");
  return 0;
}

static int tw_shape(const vbn_walk_args* a, tw_launch* out) {
  const int64_t per_wave = (int64_t)a->n_slots * WAVE * (int64_t)sizeof(int32_t);
  const int64_t tab_bytes = (int64_t)a->wbuf_floats * (int64_t)sizeof(float);
  int nw = TW_WAVES;
  while (nw > 1 && nw * per_wave > TW_LDS_WG_MAX) nw >>= 1;
  if (nw * per_wave > TW_LDS_WG_MAX)
    return vbn_fail(VBN_E_LDS, "vbn_hip_table_walk: plan needs more than 64 KiB of LDS per wave");
  const int64_t plain = nw * per_wave, staged = plain + tab_bytes;
  const char* env = getenv("VBN_TABLE_GLOBAL");
  const bool force_global = env && env[0] && env[0] != '0';
  // A/B only: VBN_TABLE_STAGE=1 stages whenever the workgroup fits, whatever the occupancy
  const char* env_s = getenv("VBN_TABLE_STAGE");
  const bool force_stage = env_s && env_s[0] && env_s[0] != '0';
  out->nw = nw;
  out->stage = !force_global && nw == TW_WAVES && staged <= TW_LDS_WG_MAX &&
               (force_stage || std::min<int64_t>(TW_WG_PER_CU, TW_LDS_CU / staged) ==
                                   std::min<int64_t>(TW_WG_PER_CU, TW_LDS_CU / plain));
  out->lds = (size_t)(out->stage ? staged : plain);
  return 0;
}

extern "C" int vbn_hip_table_walk(const vbn_walk_args* a, void* stream) {
  int rc = tw_check(a);
  if (rc) return rc;
  tw_launch w;
  rc = tw_shape(a, &w);
  if (rc) return rc;
  const int64_t total = a->n_queries * (int64_t)a->n_samples;
  const int64_t blocks = (total + (int64_t)WAVE * w.nw - 1) / ((int64_t)WAVE * w.nw);
  if (blocks > 0x7fffffffLL) return vbn_fail(VBN_E_ARGS, "vbn_hip_table_walk: too many particles for one launch");
  hipStream_t st = (hipStream_t)stream;
  if (w.stage)
    hipLaunchKernelGGL(vbn_table_walk_kernel<true>, dim3((unsigned)blocks), dim3(WAVE * w.nw), w.lds, st, *a,
                       a->params, a->steps, a->in_cols, a->wbuf_floats);
  else
    hipLaunchKernelGGL(vbn_table_walk_kernel<false>, dim3((unsigned)blocks), dim3(WAVE * w.nw), w.lds, st, *a,
                       a->params, a->steps, a->in_cols, a->wbuf_floats);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return vbn_fail((int)e, hipGetErrorString(e));
  return 0;
}

extern "C" int vbn_hip_table_walk_staged(const vbn_walk_args* a) {
  int rc = tw_check(a);
  if (rc) return -rc;
  tw_launch w;
  rc = tw_shape(a, &w);
  return rc ? -rc : (w.stage ? 1 : 0);
}
