// KL training of CMCD: the discrete adjoint of ControlledLangevinSDELoss.simulate(train=True) (losses/oc.py:666-755, drift eq/sdes.py:101-110)
// in ONE launch.  The reference's step j evaluates the control and the annealed drift at both ends of the step,
//     x_{j+1} = x_j + (b_j + g u_j) dt_j + g db_j ,   cost_j = (b_j + b_{j+1})/g + u_j - u_{j+1} ,   rnd += 0.5 |cost_j|^2 dt_j + <cost_j, db_j>
// with u_j = ctrl(t_j, x_j), b_j = clip(0.5 g^2 (tau_j s_pi(x_j) + (1 - tau_j) s_prior(x_j)), +-clip), tau_j = t_j / T: the value at evaluation
// point j serves step j - 1 (as its second evaluation) and step j (as its first), so point j collects cotangents from both steps.  With the
// states x_0 .. x_N constants (the step-loop kernel made them), c_j = w_b (cost_j dt_j + db_j) for 0 <= j < N, c_{-1} = c_N = 0, dt_N = 0:
//     Lambda_{N+1} = w_b grad(-log pi~)(x_N)                                       (lam_in)
//     for j = N .. 0:   ubar_j = g dt_j Lambda_{j+1} + c_j - c_{j-1}              cotangent of u_j
//                       v_j    = dt_j Lambda_{j+1} + (c_j + c_{j-1}) / g          cotangent of b_j
//                       Lambda_j = Lambda_{j+1} + J_u(t_j, x_j)^T ubar_j + 0.5 g^2 (tau_j H_pi(x_j) + (1 - tau_j) H_prior) (mask_j * v_j)
// mask_j: where the unclipped drift lies within +-clip (bounds included, NaN nowhere: torch.clip's backward); H_prior = -1/var on the diagonal;
// H_pi: gmm_hvp / phi4_hvp, and ZERO for CADJ_EXT targets -- their score comes from autograd without a graph (distr/base.py:146-154: logistic
// regression), so back-propagation sees a constant, in the drift and in a ScoreCtrl alike.  J_u^T is vjp_tile (the net under its clip mask) plus,
// for a ScoreCtrl (models/reparam.py:63-117), scale s_theta(t_j) H_pi under the score clip's mask unless detach_score; both H_pi products are one
// call on the summed input.  The costs are an INPUT (`cbar`, per unit weight: one batched forward pass on the host side); the kernel scales
// them by w_b, and a particle the loss filtered out (w_b = 0) contributes exactly nothing even where its cost is not finite.
// One wave owns 16 particles and walks j = N .. 0 with Lambda in registers; only x and Lambda are live across the drift net, the target score
// is evaluated after it.  The per-row arrays of vjp_tile (row = j B + b, N + 1 row blocks) carry the parameter gradients as in sdeng_kl_adjoint.
#pragma once
#include "grad_kernel.hpp"

struct CmcdAdjArgs {
  VjpArgs v;               // x = the states x_0 .. x_N as [(N + 1) * B, d] rows, v.N = N + 1 evaluation points; cot / gx / u_out unused
  const float* coef;       // [N + 1][SDENG_NCOEF], the CMCD table of the step loop: [0] t_j, [2] dt_j, [4] t_j/T, [5] 1 - t_j/T, [6], [7] the same at t_{j+1}
  const float* cbar;       // [N][B][d] cost_j dt_j + db_j
  const float* w;          // [B] d loss / d rnd_b
  const float* lam_in;     // [B, d]
  float* lam_out;          // [B, d] Lambda_0, or nullptr
  int steps;               // N
  int ntiles_b;            // ceil(B / 16)
  DistDev target;          // CADJ_GMM: k_dist_tables tables; CADJ_PHI4: the lattice constants
  const float* prior_tab;  // diagonal Gauss prior: [2][dpad] (mean, 1/var); nullptr: isotropic
  float iso_loc, inv_iso_var;
  float g, clip;           // ControlledLangevinSDE.diff_coeff, .clip_score (<= 0: none)
  int has_score;           // ScoreCtrl (else ClippedCtrl)
  const float* stheta;     // [N + 1] clipped s_theta(t_j), or nullptr (no score model: 1)
  float scale_score, clip_score;
  int score_detached;
  float* dst;              // [(N + 1) * B] <ubar, scale clip(score)>: the cotangent of s_theta(t_j), per particle (ScoreCtrl)
  const float* score_ext;  // CADJ_EXT: [(N + 1) * B, d] target score of every row
};

enum { CADJ_GMM = 1, CADJ_PHI4 = 2, CADJ_EXT = 3 };  // target kind (the numbering of ADJ_*)
// ubar_j = g dt_j Lambda + c_j - c_{j-1}: one expression for the net's cotangent and for the score part of a ScoreCtrl
SD_INLINE float cmcd_ubar(float gdt, float lam, float cj, float cm) { return __builtin_fmaf(gdt, lam, cj - cm); }
// Four waves per workgroup, one per SIMD: a wave may then hold 512 registers (256 VGPRs + 256 AGPRs of the unified file), and what does not
// fit 256 VGPRs at d > 64 -- x, Lambda, the state gradient and the mixture's Hessian-vector product beside the drift net's activations -- is
// parked in AGPRs instead of scratch memory.  Training batches are 512 .. 4 096 particles = 32 .. 256 tiles, at most one tile per workgroup:
// the other waves of a workgroup only help to stage the weights, so a second wave per SIMD would buy nothing here.
#define CADJ_WAVES 4
#define CADJ_THREADS (CADJ_WAVES * 64)
template <int NT, int TGT>
__global__ void __launch_bounds__(CADJ_THREADS, 1) k_cmcd_kl_adjoint(const CmcdAdjArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const VjpArgs& v = a.v;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NF = sd_off_wout(NT);
  vjp_stage_weights(v, lds, NF, tid, CADJ_THREADS);
  const float* lds_t = lds + NF;
  const float* bias = v.wpack + sd_off_bias(NT);
  const NetScale ns = load_net_scale(bias, NT);
  const int p = lane & 15, g = lane >> 4;
  float* trash = v.trash + tid * 4;
  const float hg2 = 0.5f * (a.g * a.g), inv_g = 1.0f / a.g;
  const bool clip_b = a.clip > 0.0f, clip_s = a.clip_score > 0.0f;
  for (int tile = blockIdx.x + gridDim.x * wave; tile < a.ntiles_b; tile += gridDim.x * CADJ_WAVES) {
    const uint32_t b = static_cast<uint32_t>(tile) * 16u + p;
    const bool live = b < static_cast<uint32_t>(v.B);
    const float wb = live ? a.w[b] : 0.0f;
    const bool weighted = wb != 0.0f;
    f32x4 lam[NT];
    load_rows<NT>(a.lam_in, b, v.d, live, g, lam);
    for (int j = a.steps; j >= 0; --j) {
      const bool last = j == a.steps, first = j == 0;
      const float* cf = a.coef + static_cast<size_t>(last ? j - 1 : j) * SDENG_NCOEF;
      const float dt = last ? 0.0f : cf[2];
      const float tau = last ? cf[6] : cf[4], omt = last ? cf[7] : cf[5];
      const float gdt = a.g * dt;
      const uint32_t row = static_cast<uint32_t>(j) * static_cast<uint32_t>(v.B) + b;
      const uint32_t row_m = row - static_cast<uint32_t>(v.B);  // c_{j-1}; never read at j = 0
      const bool live_c = live && weighted && !last, live_m = live && weighted && !first;
      f32x4 x[NT], gx[NT];
      load_rows<NT>(v.x, row, v.d, live, g, x);
      vjp_tile<NT, true>(v, lds, lds_t, bias, ns, trash, row, live, v.temb + static_cast<size_t>(j) * SD_H, lane, x, true, false,
                         [&](int t, const f32x4&) __attribute__((always_inline)) {
                           const f32x4 cj = load_quad(a.cbar, row, v.d, live_c, t, g), cm = load_quad(a.cbar, row_m, v.d, live_m, t, g);
                           f32x4 c;
#pragma unroll
                           for (int r = 0; r < 4; ++r) c[r] = cmcd_ubar(gdt, lam[t][r], wb * cj[r], wb * cm[r]);
                           return c;
                         },
                         gx);
      // ---- the annealed drift's part, and the score part of a ScoreCtrl: target score, masks, ONE Hessian-vector product of the target ----
      f32x4 sr[NT];
      asm volatile("" ::: "memory");
      if constexpr (TGT == CADJ_GMM) gmm_score<NT>(x, a.target.tab, a.target.consts, 4, a.target.k, a.target.p0, g, sr);
      else if constexpr (TGT == CADJ_PHI4) phi4_score<NT>(x, a.target, v.d, g, lane, sr);
      else {
#pragma unroll
        for (int t = 0; t < NT; ++t) sr[t] = load_quad(a.score_ext, row, v.d, live, t, g);
      }
      const float gain_st = a.has_score ? a.scale_score * (a.stheta ? a.stheta[j] : 1.0f) : 0.0f;
      const bool hess_ctrl = a.has_score && TGT != CADJ_EXT && !a.score_detached;
      const float w_pi = hg2 * tau, w_prior = hg2 * omt;
      f32x4 hin[TGT != CADJ_EXT ? NT : 1];
      float ds = 0.0f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4 cj = load_quad(a.cbar, row, v.d, live_c, t, g), cm = load_quad(a.cbar, row_m, v.d, live_m, t, g);
        f32x4 pm = {0.0f, 0.0f, 0.0f, 0.0f}, piv;
        if (a.prior_tab) {
          pm = load_tile4(a.prior_tab, t, g);
          piv = load_tile4(a.prior_tab + 16 * NT, t, g);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool fl = feat_live<NT>(t, r, 4 * g, v.d);
            pm[r] = fl ? a.iso_loc : 0.0f;
            piv[r] = fl ? a.inv_iso_var : 0.0f;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ps = -((x[t][r] - pm[r]) * piv[r]);
          float bu = sr[t][r] * tau + ps * omt;  // the step loop's own order of operations (cmcd_eval): the mask must see its drift
          bu = bu * hg2;
          const bool pass_b = !clip_b || __builtin_fabsf(bu) <= a.clip;
          const float cjw = wb * cj[r], cmw = wb * cm[r];
          float vv = __builtin_fmaf(dt, lam[t][r], (cjw + cmw) * inv_g);
          vv = pass_b ? vv : 0.0f;
          gx[t][r] = __builtin_fmaf(-(w_prior * piv[r]), vv, gx[t][r]);
          float hterm = w_pi * vv;
          if (a.has_score) {
            const float ub = cmcd_ubar(gdt, lam[t][r], cjw, cmw);  // cotangent of the whole control (before the net's clip mask)
            ds = __builtin_fmaf(ub, clip_s ? clampf(sr[t][r], a.clip_score) : sr[t][r], ds);
            const bool pass_s = !clip_s || __builtin_fabsf(sr[t][r]) <= a.clip_score;
            if (hess_ctrl && pass_s) hterm = __builtin_fmaf(gain_st, ub, hterm);
          }
          if constexpr (TGT != CADJ_EXT) hin[t][r] = hterm;
        }
      }
      if (a.has_score) {
        ds = group_sum(ds) * a.scale_score;
        if (live && g == 0) a.dst[row] = ds;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) lam[t] = lam[t] + gx[t];
      if constexpr (TGT != CADJ_EXT) {
        f32x4 hv[NT];
        asm volatile("" ::: "memory");
        if constexpr (TGT == CADJ_GMM) gmm_hvp<NT>(x, a.target.tab, a.target.consts, 4, a.target.k, a.target.p0, g, hin, hv);
        else phi4_hvp<NT>(x, a.target, v.d, g, lane, hin, hv);
#pragma unroll
        for (int t = 0; t < NT; ++t) lam[t] = lam[t] + hv[t];
      }
    }
    if (a.lam_out) store_rows<NT>(a.lam_out, trash, b, v.d, live, g, lam);
  }
}

template <int NT, int TGT>
static int launch_cmcd_kl_adjoint(const void* p, hipStream_t stream) {
  const CmcdAdjArgs& a = *static_cast<const CmcdAdjArgs*>(p);
  return sd_launch_kernel(k_cmcd_kl_adjoint<NT, TGT>, sd_grid(a.ntiles_b), CADJ_THREADS, static_cast<size_t>(2 * sd_off_wout(NT)) * sizeof(float), stream, a);
}
