#pragma once
// vbn_table_embed.h -- the categorical_embedded_softmax step of the discrete walk
// (vbn_table_walk.hip, its EMBED instantiation; reference vbn/cpds/categorical_embedded_softmax.py:
// 306-329 _embed_parents / _logits_from_parents, 469-511 sample / log_prob).
//
// The reference gathers one embedding row per parent column, concatenates them, runs an MLP
// (embedding_dim * n_in -> hidden_dims -> D * C) and samples from the softmax of the logits with
// the classes it never saw filled with -1e9.  Roots have no network: the host packs their masked
// logits as one-configuration categorical_table rows (plan.py _pack_embed), so only nodes with
// parents arrive here.
//
// Layer 1 is linear in the concatenated embeddings, W1 concat(e_1 .. e_n) = sum_j W1_j emb_j[idx_j],
// so the host contracts every (parent column j, class c) into a row T_j[c] = W1_j emb_j[c] of H1
// floats (float64 sums rounded once).  Neither the embedding tables nor W1 reach the device:
// layer 1 is n_in row gathers and adds on top of b1.  Without a hidden layer T_j[c] is the logit
// contribution itself.
//
// Work split: lane = particle as in the table walk, but the MLP runs with the hidden unit on the M
// axis and the particle on the N axis of v_mfma_f32_32x32x2_f32, one 32-particle group g after the
// other (g = 0: particles 0-31, g = 1: 32-63).  In that orientation lane l = 32 h + n holds, for
// particle 32 g + n, the 16 rows row(r, h) = 8 (r / 4) + 4 h + r % 4 of every 32-row block -- both
// as the accumulator of a layer and as the B operand of the next one: k-step s of a block pairs
// the rows (row(s, 0), row(s, 1)), which is the order the host packs the A operands in.  So
//   * layer 1 gathers, per parent column, exactly the 16-float half rows [blk][h][16] of
//     T_j[idx_j] this lane will feed (the parent's class index is read from the LDS column of
//     particle 32 g + n: the indices already live there, no cross-lane exchange is needed);
//   * the activation runs in registers, and a layer's output feeds the next MFMA from registers;
//   * weights are A operands read from global / L2, identical for every wave.
// Widths are zero-padded to 32-row blocks at pack time (act(0) = 0 for all four activations); a
// hidden layer holds at most EMBED_NB blocks per lane (the model loader refuses wider ones).
//
// The logits land in the wave's LDS scratch rows [D C][64]; after a wave-level hand-off every lane
// reads its own particle's column and finishes on VALU: valid classes first (the loader checks
// that), masked ones carry exp(-1e9 - max) = 0 exactly, so the row max / sum of exps run over the
// valid classes only.  LOGP reads logit[k] - max - log(sum), PARAMS writes exp(logit - max) / sum
// (0 for masked classes), LATENT picks the smallest k with cdf[k] > u sum among the valid classes
// (else the last valid one) on the table walk's uniform, FIXED maps the value to its index by the
// same search as tables.
//
// Step fields (plan.py _pack_embed): k = C, aux1 = Cp, off_w3 class values [D][Cp], off_b3 valid
// classes per dim (as tables); n_out = D C; aux0 = 32-row blocks of the layer-1 output; off_w1 =
// b1 as accumulator init [aux0][2][16]; off_tail = per parent column (offset of T_j, cardinality),
// T_j = [card][aux0][2][16]; off_w2 = the table of the layers after the first, int32
// [L, (in blocks, out blocks, off_w, off_b) x L]: off_w [out blk][in blk][16 s][64 lanes] =
// W[32 ob + (l & 31)][32 ib + row(s, l >> 5)], off_b [out blk][2][16].
#include "vbn_walk_common.h"

#define EMBED_NB 2               // 32-row blocks per hidden layer a lane keeps in registers (width <= 64)
#define EMBED_MAX_LAYERS 16      // layers after the first (the blob ends in 256 floats of slack)

// offset of a block of len floats kept inside the blob (offsets come from the host packer; this
// only keeps a corrupt step table from reading outside)
__device__ __forceinline__ int embed_off(int off, int len, int blob_floats) {
  return min(max(off, 0), max(blob_floats - len, 0));
}

__device__ __forceinline__ f32x16 embed_load16(const float* __restrict__ src) {
  const float4* q4 = reinterpret_cast<const float4*>(src);
  f32x16 a;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = q4[q];
    a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
  }
  return a;
}

template <int ACT>
__device__ __forceinline__ void embed_act(f32x16 (&hr)[EMBED_NB]) {
#pragma unroll
  for (int b = 0; b < EMBED_NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) hr[b][r] = act_fn<ACT>(hr[b][r]);
}

// accumulator rows of lane half h to the scratch column of particle pcol
__device__ __forceinline__ void embed_store(float* scr, const f32x16& a, int blk, int h, int pcol, int n_out) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = 32 * blk + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (row < n_out) scr[row * WAVE + pcol] = a[r];
  }
}

// Logits of the wave's 64 particles into scr[row][particle], rows [0, n_out).
__device__ __forceinline__ void embed_logits(const vbn_walk_args& A, const vbn_step& st,
                                             const float* __restrict__ P, const int32_t* __restrict__ in_cols,
                                             const int* idx, float* scr, int lane, int n_out, int blob_floats) {
  const int h = lane >> 5, col = lane & 31;
  const int nb1 = max(st.aux0, 1), rowlen = nb1 * 32;
  const cint* hdr = CI(P) + embed_off(st.off_tail, 2 * max(st.n_in, 1), blob_floats);
  const cint* tab = CI(P) + embed_off(st.off_w2, 1 + 4 * EMBED_MAX_LAYERS, blob_floats);
  const int nl = min(max(tab[0], 0), EMBED_MAX_LAYERS);
  const float* b1 = P + embed_off(st.off_w1, rowlen, blob_floats);
  for (int g = 0; g < 2; ++g) {
    const int pcol = col + 32 * g;
    if (nl == 0) {
      // no hidden layer: b + sum_j T_j[idx_j] are the logits, one block at a time
      for (int blk = 0; blk < min(nb1, (n_out + 31) >> 5); ++blk) {
        f32x16 a = embed_load16(b1 + blk * 32 + 16 * h);
        for (int j = 0; j < st.n_in; ++j) {
          const int slot = min(max(CI(in_cols)[st.in_off + j], 0), A.n_slots - 1);
          const int card = max(hdr[2 * j + 1], 1);
          const int k = min(max(idx[slot * WAVE + pcol], 0), card - 1);
          a += embed_load16(P + embed_off(hdr[2 * j] + k * rowlen, rowlen, blob_floats) + blk * 32 + 16 * h);
        }
        embed_store(scr, a, blk, h, pcol, n_out);
      }
      continue;
    }
    f32x16 hr[EMBED_NB];
#pragma unroll
    for (int b = 0; b < EMBED_NB; ++b) {
      hr[b] = embed_load16(b1 + min(b, nb1 - 1) * 32 + 16 * h);
      if (b >= nb1) hr[b] = (f32x16)(0.f);
    }
    for (int j = 0; j < st.n_in; ++j) {
      const int slot = min(max(CI(in_cols)[st.in_off + j], 0), A.n_slots - 1);
      const int card = max(hdr[2 * j + 1], 1);
      const int k = min(max(idx[slot * WAVE + pcol], 0), card - 1);
      const float* row = P + embed_off(hdr[2 * j] + k * rowlen, rowlen, blob_floats) + 16 * h;
#pragma unroll
      for (int b = 0; b < EMBED_NB; ++b)
        if (b < nb1) hr[b] += embed_load16(row + b * 32);
    }
    for (int li = 0; li < nl; ++li) {
      switch (st.act) {
        case VBN_ACT_RELU: embed_act<VBN_ACT_RELU>(hr); break;
        case VBN_ACT_TANH: embed_act<VBN_ACT_TANH>(hr); break;
        case VBN_ACT_GELU: embed_act<VBN_ACT_GELU>(hr); break;
        default: embed_act<VBN_ACT_ELU>(hr); break;
      }
      const int nbi = min(max(tab[1 + 4 * li], 1), EMBED_NB);
      const int nbo = min(max(tab[2 + 4 * li], 1), li + 1 == nl ? (n_out + 31) >> 5 : EMBED_NB);
      const float* __restrict__ W = P + embed_off(tab[3 + 4 * li], nbo * nbi * 16 * WAVE, blob_floats) + lane;
      const float* __restrict__ Bs = P + embed_off(tab[4 + 4 * li], nbo * 32, blob_floats) + 16 * h;
      if (li + 1 == nl) {
        // the logits: any number of output blocks, each straight to the scratch rows
        for (int ob = 0; ob < nbo; ++ob) {
          f32x16 a = embed_load16(Bs + ob * 32);
#pragma unroll
          for (int ib = 0; ib < EMBED_NB; ++ib)
            if (ib < nbi) {
#pragma unroll
              for (int s = 0; s < 16; ++s)
                a = __builtin_amdgcn_mfma_f32_32x32x2f32(W[((ob * nbi + ib) * 16 + s) * WAVE], hr[ib][s], a, 0, 0, 0);
            }
          embed_store(scr, a, ob, h, pcol, n_out);
        }
      } else {
        f32x16 o[EMBED_NB];
#pragma unroll
        for (int ob = 0; ob < EMBED_NB; ++ob) {
          o[ob] = (f32x16)(0.f);
          if (ob < nbo) {
            o[ob] = embed_load16(Bs + ob * 32);
#pragma unroll
            for (int ib = 0; ib < EMBED_NB; ++ib)
              if (ib < nbi) {
#pragma unroll
                for (int s = 0; s < 16; ++s)
                  o[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(W[((ob * nbi + ib) * 16 + s) * WAVE], hr[ib][s], o[ob],
                                                               0, 0, 0);
              }
          }
        }
#pragma unroll
        for (int b = 0; b < EMBED_NB; ++b) hr[b] = o[b];
      }
    }
  }
}

// One categorical_embedded_softmax step for the lane's particle; returns the node's log-prob
// (0 without VBN_F_LOGP).  idx: the wave's class-index slots, scr: its logit scratch rows.
__device__ __forceinline__ float embed_step(const vbn_walk_args& A, const vbn_step& st, const float* __restrict__ P,
                                            const int32_t* __restrict__ in_cols, int* idx, float* scr,
                                            const Lane& L, int blob_floats) {
  const int lane = L.lane, t_max = blob_floats - 1;
  const int C = max(st.k, 1), Cp = max(st.aux1, C), D = st.out_dim;
  const int n_out = max(min(min(st.n_out, D * C), A.max_out), 1);
  const bool reads = st.role != VBN_ROLE_FIXED || (st.flags & VBN_F_LOGP);
  if (reads) {
    wave_sync();                                     // the other lanes' class indices and last reads of scr
    embed_logits(A, st, P, in_cols, idx, scr, lane, n_out, blob_floats);
    wave_sync();                                     // logits written by other lanes
  }
  float node_lp = 0.f;
  for (int d = 0; d < D; ++d) {
    const int nv = min(max(CI(P)[st.off_b3 + d], 1), C);
    int k = 0;
    bool bad = false;
    float m = -INFINITY, sum = 0.f;
    if (reads) {
      for (int c = 0; c < nv; ++c) m = fmaxf(m, scr[min(d * C + c, n_out - 1) * WAVE + lane]);
      for (int c = 0; c < nv; ++c) sum += expf(scr[min(d * C + c, n_out - 1) * WAVE + lane] - m);
    }
    if (st.role == VBN_ROLE_PARAMS) {
      const float inv = 1.0f / sum;
      for (int c = 0; c < C; ++c) {
        const float p = c < nv ? expf(scr[min(d * C + c, n_out - 1) * WAVE + lane] - m) * inv : 0.f;
        idx[min(max(st.out_col + d * C + c, 0), A.n_slots - 1) * WAVE + lane] = __float_as_int(p);
      }
      continue;
    }
    if (st.role == VBN_ROLE_LATENT) {
      const float u = A.noise ? A.noise[noise_index(A, st, d, 0, L)] : u01(rng_words(A, st, d, RNG_UNIFORM, L).x);
      const float thr = u * sum;
      float run = 0.f;
      for (int c = 0; c < nv - 1; ++c) {
        run += expf(scr[min(d * C + c, n_out - 1) * WAVE + lane] - m);
        k += run <= thr;
      }
    } else {                                          // FIXED: the value's index among the class values
      const float v = fixed_read(A, st, d, L);
      const float* cv = P + min(max(st.off_w3 + d * Cp, 0), t_max - Cp + 1);
      int lo = 0, hi = nv;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cv[mid] < v) lo = mid + 1; else hi = mid;
      }
      bad = !(lo < nv && cv[min(lo, nv - 1)] == v);
      k = bad ? 0 : lo;
    }
    k = min(max(k, 0), nv - 1);
    idx[min(max(st.out_col + d, 0), A.n_slots - 1) * WAVE + lane] = k;
    if (st.flags & VBN_F_LOGP) {
      const float l = scr[min(d * C + k, n_out - 1) * WAVE + lane] - m - logf(sum);
      node_lp += bad ? __int_as_float(0x7fc00000) : l;
    }
  }
  return node_lp;
}
