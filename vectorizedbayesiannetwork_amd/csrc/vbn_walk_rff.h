#pragma once
// vbn_walk_rff.h -- the rff_gaussian step: a random Fourier feature regressor with a fixed
// noise scale (part of vbn_walk_impl.h, included from vbn_walk_cpd.h).
#include "vbn_walk_mlp.h"

// ------------------------------------------------------------------------------------------
// rff_gaussian (rff_gaussian.py:131-146, 183-211, 257-291)
//   feats = sqrt(2 / F) cos(((x - mean_x) / std_x) W^T + b),  loc = (feats coef + bias) std_y + mean_y,
//   scale = sqrt(clamp(_var, min_scale^2)) per output dim;  root: loc = mean_y, no features.
// Parameter blocks (plan.py _pack_rff; st.k = F):
//   off_std : mean_x[n_in], 1 / std_x[n_in]                       (l1_operand<true, 0>)
//   off_w1  : [ceil(F/32)][ceil(n_in/2)][64]  lane l: W[32 blk + (l & 31)][2 t + (l >> 5)] (0-padded),
//             the A fragments of v_mfma_f32_32x32x2_f32 as in mlp_generic
//   off_b2  : [ceil(F/32)][2][16]  b[32 blk + row(r, h)]          (accumulator init, 0-padded)
//   off_w3  : [ceil(F/32)][2][D][16]  coef[32 blk + row(r, h)][d] (0-padded): the 16 feature rows
//             a lane half holds after the MFMA, contiguous per output dim
//   off_tail: bias[D], std_y[D], mean_y[D], scale[D], log_scale[D]
// Per block of 32 features the projections of both 32-particle groups come out of the MFMA in
// registers (register r of lane half h = feature 32 blk + row(r, h) of particle (lane & 31) +
// 32 g); their cosines, the products with the lane's coef rows and the per-lane partial sums stay
// in registers, and one cross-half exchange per output dim after the last block gives each lane
// the total of its own particle.  No feature goes to LDS; the D totals (loc) go to the step's D
// scratch rows, where the inlined epilogue (draw / fixed value / log-prob, as linear_gaussian's)
// reads them.  The feature pass is out of line (noinline, as mlp_generic is) so the hot
// instantiations keep their registers; it holds no draw and no evidence read: those stay with the
// caller, whose kernel arguments are known to be wave-uniform.
//
// Ridge 1e-6 on 256 features leaves |coef| in the thousands with sum |coef| ~ 1e5, so an error of
// 1e-7 per feature is visible in loc.  Everything after the float32 projection therefore runs in
// float64, whose FMA issues at the float32 rate on gfx950: the argument reduction (quarter
// turns: t = 2 p / pi, n = rint(t), r = (t - n) pi / 2), degree-4 polynomials in r^2 for
// (cos r - 1) / r^2 and (sin r / r - 1) / r^2 on [-pi/4, pi/4] (Chebyshev interpolants; |error|
// of cos < 2e-10 for |p| <= 1e5, 6e-9 at 1e7), the products with coef and their sum; loc is
// rounded to float32 once.
// What is left is the projection's own float32 rounding, which the reference has too.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double rff_cos(float p) {
  const double t = (double)p * 0.63661977236758134308;      // quarter turns
  const double q = __builtin_rint(t);
  const double r = (t - q) * 1.57079632679489661923;        // |r| <= pi / 4
  const int n = (int)q;
  const double z = r * r;
  double c = __builtin_fma(z, 0x1.9a6f61ba84cd1p-16, -0x1.6c0e094760935p-10);
  c = __builtin_fma(z, c, 0x1.55554cbcb64efp-5);
  c = __builtin_fma(z, c, -0x1.fffffffab3706p-2);
  c = __builtin_fma(z, c, 1.0);
  double s = __builtin_fma(z, 0x1.6dbe298d6e8f6p-19, -0x1.a013a80f1c1f1p-13);
  s = __builtin_fma(z, s, 0x1.11110defa052ep-7);
  s = __builtin_fma(z, s, -0x1.555555545e496p-3);
  s = __builtin_fma(z * r, s, r);
  const double v = (n & 1) ? s : c;                         // cos(n pi / 2 + r)
  return ((n + 1) & 2) ? -v : v;
}

// DT = output dims per pass over the features (1 for the usual D = 1; wider nodes take
// ceil(D / 2) passes of 2).  Writes loc[d] of the lane's particle to scr[d][lane].
template <bool MIR, int DT>
__device__ __attribute__((noinline)) void rff_loc(const vbn_walk_args& A, const vbn_step& st, const Lane& L) {
  const int lane = L.lane, h = lane >> 5;
  const int D = st.out_dim, F = st.k, nin = st.n_in;
  const cfloat* tl = CP(L.P + st.off_tail);
  const cfloat* bias = tl;
  const cfloat* std_y = tl + D;
  const cfloat* mean_y = tl + 2 * D;
  bool nan_in = false;                             // torch keeps NaN through the projection and cos
  for (int i = 0; i < nin; ++i) {
    const float v = L.vals[L.ic[st.in_off + i] * WAVE + lane];
    nan_in |= (v != v);
  }
  const int nblk = (F + 31) >> 5, t1 = (nin + 1) >> 1;
  const double fscale = __builtin_sqrt(2.0 / (double)(F > 0 ? F : 1));
  const float* __restrict__ W = L.P + st.off_w1;
  for (int d0 = 0; d0 < D; d0 += DT) {
    double part[2][DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) part[0][j] = part[1][j] = 0.0;
    for (int blk = 0; blk < nblk; ++blk) {
      const f32x16 b = load_acc16(L.P + st.off_b2 + blk * 32 + 16 * h);
      f32x16 a0 = b, a1 = b;
      for (int t = 0; t < t1; ++t) {
        const float w = W[(blk * t1 + t) * WAVE + lane];
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w, l1_operand<true, 0>(A, st, L, t, 0), a0, 0, 0, 0);
        if constexpr (!MIR)
          a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w, l1_operand<true, 0>(A, st, L, t, 1), a1, 0, 0, 0);
      }
      const float* cf = L.P + st.off_w3 + (blk * 2 + h) * D * 16;
      f32x16 cj[DT];
#pragma unroll
      for (int j = 0; j < DT; ++j) cj[j] = load_acc16(cf + min(d0 + j, D - 1) * 16);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const double c0 = rff_cos(a0[r]);
        const double c1 = MIR ? 0.0 : rff_cos(a1[r]);
#pragma unroll
        for (int j = 0; j < DT; ++j) {
          const double cw = (double)cj[j][r];
          part[0][j] = __builtin_fma(c0, cw, part[0][j]);
          if constexpr (!MIR) part[1][j] = __builtin_fma(c1, cw, part[1][j]);
        }
      }
    }
    // lane l = particle l: its own half's partial of its group (group h; half-wave launches:
    // group 0 on both halves) + the other half's partial of that group
#pragma unroll
    for (int j = 0; j < DT; ++j) {
      const double mine = MIR ? part[0][j] : (h ? part[1][j] : part[0][j]);
      const double send = MIR ? part[0][j] : (h ? part[0][j] : part[1][j]);
      const double tot = mine + __shfl_xor(send, 32);
      const int d = d0 + j;
      if (d < D) {
        const double loc = __builtin_fma(__builtin_fma(tot, fscale, (double)bias[d]), (double)std_y[d], (double)mean_y[d]);
        L.scr[d * WAVE + lane] = nan_in ? __int_as_float(0x7fc00000) : (float)loc;
      }
    }
  }
  wave_sync();
}

// tail: bias[D], std_y[D], mean_y[D], scale[D], log_scale[D]; root: loc = mean_y, no features
template <unsigned KM>
__device__ __forceinline__ void step_rff_gaussian(const vbn_walk_args& A, const vbn_step& st, const Lane& L,
                                                  float& lp) {
#pragma clang fp contract(off)
  constexpr bool MIR = (KM & VBN_KM_HALFWAVE) != 0;
  const int D = st.out_dim;
  const cfloat* tl = CP(L.P + st.off_tail);
  const cfloat* mean_y = tl + 2 * D;
  const cfloat* scale = tl + 3 * D;
  const cfloat* log_scale = tl + 4 * D;
  const bool root = (st.flags & VBN_F_ROOT) != 0;
  const bool latent = st.role == VBN_ROLE_LATENT;
  if (!root) {
    if (D == 1) rff_loc<MIR, 1>(A, st, L); else rff_loc<MIR, 2>(A, st, L);
  }
  float acc = 0.f;
  for (int d = 0; d < D; ++d) {
    const float loc = root ? mean_y[d] : L.scr[d * WAVE + L.lane];
    const float sc = scale[d];
    if (st.role == VBN_ROLE_PARAMS) {
      vwrite(L, st.out_col + d, loc);
      vwrite(L, st.out_col + D + d, sc);
      continue;
    }
    float x;
    if (latent) {
      x = loc + draw_normal(A, st, d, L) * sc;
    } else {
      x = node_fixed(A, st, d, L);
    }
    vwrite(L, st.out_col + d, x);
    if (st.flags & VBN_F_LOGP) {
      const float diff = x - loc;
      acc += (diff * diff) / (sc * sc) + 2.0f * log_scale[d] + LOG_2PI_F;
    }
  }
  if (st.flags & VBN_F_LOGP) lp += -0.5f * acc;
}
