#pragma once
// vbn_walk_cpd.h -- the parametric CPD steps: gaussian_nn, linear_gaussian, mdn, softmax_nn and
// their inverse-CDF search; rff_gaussian has a header of its own, included here (part of
// vbn_walk_impl.h).
#include "vbn_walk_mlp.h"
#include "vbn_walk_rff.h"

// value of node dim d for this particle: fresh draw result or fixed input
#define NODE_X(d) (vread(L, st.out_col + (d)))

// ------------------------------------------------------------------------------------------
// gaussian_nn (gaussian_nn.py:215-288)
//   tail (non-root): std_y[D], mean_y[D], min_scale
//   tail (root)    : loc[D], scale[D], log_scale[D]
// ------------------------------------------------------------------------------------------
template <unsigned KM>
__device__ __forceinline__ void step_gaussian_nn(const vbn_walk_args& A, const vbn_step& st, const Lane& L, float& lp) {
#pragma clang fp contract(off)
  const float* __restrict__ P = L.P;
  const int D = st.out_dim;
  const bool latent = st.role == VBN_ROLE_LATENT;
  const bool want_lp = (st.flags & VBN_F_LOGP) != 0;
  const cfloat* t = CP(P + st.off_tail);
  if (st.flags & VBN_F_ROOT) {
    for (int d = 0; d < D; ++d) {
      const float loc = t[d], scale = t[D + d];
      if (st.role == VBN_ROLE_PARAMS) {
        vwrite(L, st.out_col + d, loc);
        vwrite(L, st.out_col + D + d, scale);
        continue;
      }
      float x;
      if (latent) {
        x = draw_normal(A, st, d, L) * scale + loc;  // torch.normal(loc, scale)
        vwrite(L, st.out_col + d, x);
      } else {
        x = node_fixed(A, st, d, L);
        vwrite(L, st.out_col + d, x);
      }
      if (want_lp) {                                 // Normal.log_prob (gaussian_nn.py:276-279)
        const float diff = x - loc;
        lp += -(diff * diff) / (2.0f * (scale * scale)) - t[2 * D + d] - 0.91893853320467274178f;
      }
    }
    return;
  }
  float eps0 = 0.f;                                 // dim-0 draw, issued beside the weight loads
  auto pre = [&]() { if (latent) eps0 = draw_normal(A, st, 0, L); };
  if (D == 1) run_mlp<KM, 2>(A, st, L, pre);        // head = (loc, raw scale): straight-line
  else run_mlp<KM>(A, st, L, pre);
  const float min_scale = t[2 * D];
  float acc = 0.f;
  for (int d = 0; d < D; ++d) {
    const float o_loc = L.scr[d * WAVE + L.lane];
    const float o_sc = L.scr[(D + d) * WAVE + L.lane];
    const float sy = t[d], my = t[D + d];
    const float loc = o_loc * sy + my;
    const float scale = (softplus_t(o_sc) + min_scale) * sy;
    if (st.role == VBN_ROLE_PARAMS) {
      vwrite(L, st.out_col + d, loc);
      vwrite(L, st.out_col + D + d, scale);
      continue;
    }
    float x;
    if (latent) {
      x = loc + (d == 0 ? eps0 : draw_normal(A, st, d, L)) * scale;
    } else {
      x = node_fixed(A, st, d, L);
    }
    vwrite(L, st.out_col + d, x);
    if (want_lp) {
      const float diff = x - loc;
      acc += (diff * diff) / (scale * scale) + 2.0f * log_hw(scale) + LOG_2PI_F;   // scale >= min_scale std_y
    }
  }
  if (want_lp) lp += -0.5f * acc;
}

// ------------------------------------------------------------------------------------------
// linear_gaussian (linear_gaussian.py:163-217)
//   tail: W[D][n_in] (W[:, d] of the reference's [n_in, D]), bias[D], scale[D], log_scale[D]
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void step_linear_gaussian(const vbn_walk_args& A, const vbn_step& st, const Lane& L, float& lp) {
#pragma clang fp contract(off)
  const float* __restrict__ P = L.P;
  const int D = st.out_dim, nin = st.n_in;
  const cfloat* t = CP(P + st.off_tail);
  const cfloat* W = t;
  const cfloat* bias = t + D * nin;
  const cfloat* scale = bias + D;
  const cfloat* log_scale = scale + D;
  const bool latent = st.role == VBN_ROLE_LATENT;
  float acc = 0.f;
  for (int d = 0; d < D; ++d) {
    float mu = 0.f;
    for (int i = 0; i < nin; ++i) mu = fmaf(vread(L, L.ic[st.in_off + i]), W[d * nin + i], mu);
    const float loc = (nin > 0) ? mu + bias[d] : bias[d];
    if (st.role == VBN_ROLE_PARAMS) {
      vwrite(L, st.out_col + d, loc);
      vwrite(L, st.out_col + D + d, scale[d]);
      continue;
    }
    float x;
    if (latent) {
      x = loc + draw_normal(A, st, d, L) * scale[d];
    } else {
      x = node_fixed(A, st, d, L);
    }
    vwrite(L, st.out_col + d, x);
    if (st.flags & VBN_F_LOGP) {
      const float diff = x - loc;
      acc += (diff * diff) / (scale[d] * scale[d]) + 2.0f * log_scale[d] + LOG_2PI_F;
    }
  }
  if (st.flags & VBN_F_LOGP) lp += -0.5f * acc;
}

// ------------------------------------------------------------------------------------------
// categorical inverse-CDF: smallest k with cumsum(p)[k] > u * sum(p)
// ------------------------------------------------------------------------------------------
// Without an early exit: the first crossing is kept by selects, so a wave whose lanes cross at
// different k runs one straight pass instead of a divergent loop (the divergent form held the
// mdn / softmax_nn epilogues' values live across exec-mask joins: cfg3 spilled 46 VGPRs)
template <typename F>
__device__ __forceinline__ int inv_cdf(int K, float u, F prob) {
  float tot = 0.f;
  for (int k = 0; k < K; ++k) tot += prob(k);
  const float thr = u * tot;
  float cum = 0.f;
  int idx = K - 1;
  bool found = false;
  for (int k = 0; k < K - 1; ++k) {
    cum += prob(k);
    const bool hit = !found && cum > thr;
    idx = hit ? k : idx;
    found |= hit;
  }
  return idx;
}

// ------------------------------------------------------------------------------------------
// mdn (mdn.py:185-272)
//   non-root: scr = [logits K][comp k: loc D, raw_scale D];  tail: min_scale
//   root    : tail = pi[K], log_pi[K], loc[K*D], scale[K*D], log_scale[K*D], var[K*D],
//             softmax(logits)[K] (unclamped, for the PARAMS role)
// ------------------------------------------------------------------------------------------
template <unsigned KM>
__device__ __forceinline__ void step_mdn(const vbn_walk_args& A, const vbn_step& st, const Lane& L, float& lp) {
#pragma clang fp contract(off)
  const float* __restrict__ P = L.P;
  const int D = st.out_dim, K = st.k;
  const cfloat* t = CP(P + st.off_tail);
  const bool root = (st.flags & VBN_F_ROOT) != 0;
  const bool latent = st.role == VBN_ROLE_LATENT;
  const bool want_lp = (st.flags & VBN_F_LOGP) != 0;
  const int lane = L.lane;
  float* scr = L.scr;
  float min_scale = 0.f, lmax = 0.f, lsum = 1.f, psum = 1.f;
  float u0 = 0.f, eps0 = 0.f;                       // component choice + dim-0 normal
  auto draws = [&]() {
    if (latent) {
      u0 = draw_uniforms(A, st, 0, L).x;
      eps0 = draw_normal(A, st, 0, L);
    }
  };
  // pi = softmax(logits).clamp_min(1e-5); pi /= sum (mdn.py:227-228), computed once per
  // particle into the logit rows (the inverse CDF and the log-prob read pi_k repeatedly).
  // The two normalisations multiply by one reciprocal each (within an ulp of the reference's
  // divisions; cfg3 walk -1.8 %); each exp is computed once and kept in its row
  auto make_pi = [&]() {
    lmax = -INFINITY;
    for (int k = 0; k < K; ++k) lmax = fmaxf(lmax, scr[k * WAVE + lane]);
    lsum = 0.f;
    for (int k = 0; k < K; ++k) {
      const float e = __expf(scr[k * WAVE + lane] - lmax);
      scr[k * WAVE + lane] = e;
      lsum += e;
    }
    psum = 0.f;
    const float rl = __builtin_amdgcn_rcpf(lsum);     // lsum >= 1
    for (int k = 0; k < K; ++k) {
      const float p = fmaxf(scr[k * WAVE + lane] * rl, 1e-5f);
      scr[k * WAVE + lane] = p;
      psum += p;
    }
    psum = fmaxf(psum, 1e-12f);
    const float rp = 1.0f / psum;
    for (int k = 0; k < K; ++k) scr[k * WAVE + lane] = scr[k * WAVE + lane] * rp;
  };
  if (root) draws();
  if (!root) run_mlp<KM>(A, st, L, draws);
  if (st.role == VBN_ROLE_PARAMS) {
    // mixture parameters (CPDHandle.conditional, cpd_handle.py:72-88): softmax(logits) [K]
    // (no clamp), loc [K][D], scale [K][D]; root: the host's softmax / loc / scale constants
    if (root) {
      for (int k = 0; k < K; ++k) vwrite(L, st.out_col + k, t[2 * K + 4 * K * D + k]);
      for (int j = 0; j < K * D; ++j) {
        vwrite(L, st.out_col + K + j, t[2 * K + j]);
        vwrite(L, st.out_col + K + K * D + j, t[2 * K + K * D + j]);
      }
      return;
    }
    const float ms = t[0];
    float mx = -INFINITY, se = 0.f;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, scr[k * WAVE + lane]);
    for (int k = 0; k < K; ++k) se += __expf(scr[k * WAVE + lane] - mx);
    for (int k = 0; k < K; ++k) vwrite(L, st.out_col + k, __expf(scr[k * WAVE + lane] - mx) / se);
    for (int k = 0; k < K; ++k)
      for (int d = 0; d < D; ++d) {
        vwrite(L, st.out_col + K + k * D + d, scr[(K + k * 2 * D + d) * WAVE + lane]);
        vwrite(L, st.out_col + K + K * D + k * D + d,
               softplus_t(scr[(K + k * 2 * D + D + d) * WAVE + lane]) + ms);
      }
    return;
  }
  if (!root) {
    min_scale = t[0];
    make_pi();
  }
  auto pi_k = [&](int k) -> float { return root ? t[k] : scr[k * WAVE + lane]; };
  auto loc_kd = [&](int k, int d) -> float {
    return root ? t[2 * K + k * D + d] : scr[(K + k * 2 * D + d) * WAVE + lane];
  };
  auto scale_kd = [&](int k, int d) -> float {
    return root ? t[2 * K + K * D + k * D + d]
                : softplus_t(scr[(K + k * 2 * D + D + d) * WAVE + lane]) + min_scale;
  };
  if (latent) {
    const int idx = inv_cdf(K, u0, pi_k);
    for (int d = 0; d < D; ++d)
      vwrite(L, st.out_col + d, loc_kd(idx, d) + (d == 0 ? eps0 : draw_normal(A, st, d, L)) * scale_kd(idx, d));
  } else {
    for (int d = 0; d < D; ++d) vwrite(L, st.out_col + d, node_fixed(A, st, d, L));
  }
  if (want_lp) {
    // logsumexp_k(log pi_k + log N_k(x))  (mdn.py:263-272), online form
    float m = -INFINITY, se = 0.f;
    for (int k = 0; k < K; ++k) {
      float acc = 0.f;
      for (int d = 0; d < D; ++d) {
        const float x = NODE_X(d);
        float ls, var;
        if (root) {
          ls = t[2 * K + 2 * K * D + k * D + d];
          var = t[2 * K + 3 * K * D + k * D + d];
        } else {
          ls = log_hw(scale_kd(k, d));                 // scale >= min_scale
          var = __expf(2.0f * ls);
        }
        const float diff = x - loc_kd(k, d);
        acc += (diff * diff) / var + 2.0f * ls + LOG_2PI_F;
      }
      const float lpi = root ? t[K + k] : log_hw(pi_k(k));   // pi >= 1e-5 / sum
      const float term = lpi + (-0.5f * acc);
      if (term == -INFINITY) continue;
      if (term > m) {
        se = se * __expf(m - term) + 1.0f;
        m = term;
      } else {
        se += __expf(term - m);
      }
    }
    lp += (m == -INFINITY) ? m : m + log_hw(se);          // se >= 1
  }
}

// ------------------------------------------------------------------------------------------
// softmax_nn (softmax_nn.py:581-759)
//   scr (non-root) = logits[D][C];  root logits table at off_pts ([D][C], already log_softmax'd)
//   tail: edges[D][C+1], sample_values[D][C], class_values[D][C], within_scale, min_bw, min_bw2
//   aux0 = within-bin mode, aux1 = discrete-dim bit mask
// ------------------------------------------------------------------------------------------
template <unsigned KM>
__device__ __forceinline__ void step_softmax_nn(const vbn_walk_args& A, const vbn_step& st, const Lane& L, float& lp) {
#pragma clang fp contract(off)
  const float* __restrict__ P = L.P;
  const int D = st.out_dim, C = st.k;
  const cfloat* t = CP(P + st.off_tail);
  const cfloat* edges = t;
  const cfloat* svals = t + D * (C + 1);
  const cfloat* cvals = svals + D * C;
  const float wscale = cvals[D * C + 0];
  const float min_bw = cvals[D * C + 1];
  const float min_bw2 = cvals[D * C + 2];
  const bool root = (st.flags & VBN_F_ROOT) != 0;
  const bool latent = st.role == VBN_ROLE_LATENT;
  const bool clip = (st.flags & VBN_F_CLIP) != 0;
  const int mode = st.aux0;
  const int lane = L.lane;
  float2 uu0 = make_float2(0.f, 0.f);               // dim-0 uniforms
  auto draws = [&]() { if (latent) uu0 = draw_uniforms(A, st, 0, L); };
  if (root) draws(); else run_mlp<KM>(A, st, L, draws);
  float lp_acc = 0.f;
  for (int d = 0; d < D; ++d) {
    auto logit = [&](int c) -> float {
      return root ? P[st.off_pts + d * C + c] : L.scr[(d * C + c) * WAVE + lane];
    };
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, logit(c));
    float se = 0.f;
    // a latent non-root step without a log-prob reads the logits only here: each exp is
    // computed once and kept in its row for the class probabilities below (same values)
    const bool keep_e = latent && !root && !(st.flags & VBN_F_LOGP);
    if (keep_e) {
      for (int c = 0; c < C; ++c) {
        const float e = __expf(logit(c) - m);
        L.scr[(d * C + c) * WAVE + lane] = e;
        se += e;
      }
    } else {
      for (int c = 0; c < C; ++c) se += __expf(logit(c) - m);
    }
    if (st.role == VBN_ROLE_PARAMS) {   // softmax(logits) per dim: [D][C] (RB target: D = 1)
      for (int c = 0; c < C; ++c) vwrite(L, st.out_col + d * C + c, __expf(logit(c) - m) / se);
      continue;
    }
    const bool disc = (st.aux1 >> d) & 1;
    const cfloat* e = edges + d * (C + 1);
    float x;
    int idx;
    if (latent) {
      const float2 uu = d == 0 ? uu0 : draw_uniforms(A, st, d, L);
      if (keep_e) {
        // the logits are not read again: the class probabilities replace the kept exps
        // (the inverse CDF reads each twice; same operations, so the same values); one
        // reciprocal of the sum instead of C divisions
        const float rse = __builtin_amdgcn_rcpf(se);  // se >= 1
        for (int c = 0; c < C; ++c) L.scr[(d * C + c) * WAVE + lane] = L.scr[(d * C + c) * WAVE + lane] * rse;
        idx = inv_cdf(C, uu.x, [&](int c) { return L.scr[(d * C + c) * WAVE + lane]; });
      } else {
        const float rse = __builtin_amdgcn_rcpf(se);  // se >= 1
        idx = inv_cdf(C, uu.x, [&](int c) { return __expf(logit(c) - m) * rse; });
      }
      const float left = e[idx];
      const float right = e[idx + 1 < C ? idx + 1 : C];
      const float width = fmaxf(right - left, min_bw);
      const float center = 0.5f * (left + right);
      if (disc) {
        x = svals[d * C + idx];
      } else {
        float cont;
        if (mode == VBN_WITHIN_UNIFORM) {
          cont = left + uu.y * width;
        } else if (mode == VBN_WITHIN_TRIANGULAR) {
          // only the chosen side's root (the same operations on the same values)
          const bool lo = uu.y < 0.5f;
          const float r = sqrtf(fmaxf((lo ? uu.y : 1.0f - uu.y) * 0.5f, 0.0f));
          cont = lo ? left + width * r : right - width * r;
        } else {
          cont = center + draw_normal(A, st, d, L) * fmaxf(wscale * width, min_bw);
        }
        if (clip) cont = fminf(fmaxf(cont, left), right);
        x = cont;
      }
    } else {
      x = node_fixed(A, st, d, L);
    }
    vwrite(L, st.out_col + d, x);
    if (st.flags & VBN_F_LOGP) {
      // bin: count(x >= edges) - 1 clamped (bit-exact); discrete: first exact class match
      int bin;
      if (disc) {
        bin = 0;
        for (int c = C - 1; c >= 0; --c)
          if (x == cvals[d * C + c]) bin = c;
      } else {
        int cnt = 0;
        for (int c = 0; c <= C; ++c) cnt += (x >= e[c]) ? 1 : 0;
        bin = min(max(cnt - 1, 0), C - 1);
      }
      const float log_bin = logit(bin) - m - log_hw(se);
      float lw = 0.f;
      if (!disc) {
        const float left = e[bin];
        const float right = e[bin + 1 < C ? bin + 1 : C];
        const float width = fmaxf(right - left, min_bw);
        const float center = 0.5f * (left + right);
        const float xu = clip ? fminf(fmaxf(x, left), right) : x;
        const bool inside = (x >= left) && (x <= right);
        if (mode == VBN_WITHIN_UNIFORM) {
          lw = -log_hw(width);
          if (!clip && !inside) lw = -INFINITY;
        } else if (mode == VBN_WITHIN_TRIANGULAR) {
          const float dl = fmaxf(width * (center - left), min_bw2);
          const float dr = fmaxf(width * (right - center), min_bw2);
          float pdf = (xu <= center) ? 2.0f * (xu - left) / dl : 2.0f * (right - xu) / dr;
          pdf = fmaxf(pdf, 0.0f);
          lw = log_hw(fmaxf(pdf, 1e-12f));
          if (!clip && !inside) lw = -INFINITY;
        } else {
          const float sigma = fmaxf(wscale * width, min_bw);
          const float diff = xu - center;
          lw = -(diff * diff) / (2.0f * (sigma * sigma)) - log_hw(sigma) - 0.91893853320467274178f;
        }
      }
      lp_acc += log_bin + lw;
    }
  }
  if (st.flags & VBN_F_LOGP) lp += lp_acc;
}
