// The RDS step loop over an energy-based (tilted-potential) reference in ONE launch: sdeng_tilted_simulate.
// EIReferenceSDELoss / DDPMLikeReferenceSDELoss / EMReferenceSDELoss.simulate (losses/oc.py:218-296, :444-510, :584-651) with
// reference_ctrl = net(t, x) of a GMMTitledPotential / GaussTiltedPotential (solver/oc.py:577-592, ref_type 'nn'), where the reference
// takes one autograd pass through the 6 x 128 net per step.  The shape is k_tilted_moves' (tilted_moves_inst.hip): one wave owns a
// 16-row tile of particles, 1 to 8 waves per workgroup walk the layers in lock-step through ONE 64 KiB image buffer, the step loop sits
// inside the round loop, N is uniform, idle waves and pad rows meet every barrier of every step.  Per step:
//   a. the reference score at (t_k, x_k): the phases of tilted_kernel.hpp (tl_prior, tl_forward, tl_backward) -- this file holds no
//      walk of its own, the score is sdeng_tilted_eval's at the same row, bit for bit.  Every row of a step shares the step's time, so the
//      EBM's time embedding is a per-step quantity: a table [N][128] made once per launch by k_tilted_rds_times through tl_time_embed
//      (three stagings fewer per step), read back in the lane's register order as the accumulator of the input layer;
//   b. the control u = clip(FourierMLP_4x64(t_k, x_k)): mlp_hidden_scaled and the output tiles of sim_device.hpp over the image k_pack_images
//      makes, staged through the same buffer -- input and hidden layers, then (d > 64, where the image is 96 KiB) the output layer;
//   c. the noise of Philox stream 0 in the step loop's counter layout, or the caller's;
//   d. update and running cost in the statement order of k_simulate's tail (sim_kernel.hpp).
// The state stays in global rows (L2-resident: every lane re-reads only what it wrote itself): x_k is row k of the trajectory and
// x_{k+1} row k + 1, or two ping-pong rows of the workspace; the running cost is a register scalar.  Row and lane indices are re-made
// per phase and per step (tlm_fresh) so that no address is held across the step loop.
// Stagings per step: 12 of the net + 2 per component of a full-covariance prior + 1 (d <= 64) or 2 of the drift net.
#include "tilted_rds.hpp"

SD_INLINE uint32_t tlm_fresh(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

// 2 KiB blocks of the drift-net image (sim_common.hpp): input and hidden layers, then the output layer.  The whole image fits the 64 KiB
// buffer up to four feature tiles (32 blocks at NT = 4); above, the two pieces are staged one after the other (32 + 16 blocks at NT = 8).
constexpr int tlr_hidden_blocks(int NT) { return sd_off_wout(NT) / SD_BLOCK_FLOATS; }
constexpr int tlr_out_blocks(int NT) { return sd_image_blocks(NT, SD_HT); }
constexpr bool tlr_one_image(int NT) { return sd_lds_weight_floats(NT) <= TL_SLOT; }

// mlp_out_tiles (sim_device.hpp) with the output layer's blocks at `wout`: behind the hidden layers of a whole image, or at the head of the
// buffer when the layer is staged alone
template <int OT>
SD_INLINE void tlr_out_tiles(const HidSplit& hs, const float* wout, const float* bias, int t0, int lane, f32x4 (&u)[OT], float inv_out) {
  const int g = lane >> 4;
  f32x4 mx[OT];
#pragma unroll
  for (int o = 0; o < OT; ++o) {
    u[o] = load_tile4(bias + 192, t0 + o, g);  // b_out (times the layer's scale)
    mx[o] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  dense_pre<2, OT>(hs.h, hs.l, u, mx, reinterpret_cast<const f16x8*>(wout + t0 * sd_image_floats(1, SD_HT)), lane);
  fold_lo<OT>(u, mx);
  unscale_tiles<OT>(u, inv_out);
}

template <int NT>
__global__ void __launch_bounds__(512, 2) k_tilted_rds(const TiltedArgs a, const TiltedRdsArgs rn) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  static_assert(sd_off_wout(NT) <= TL_SLOT && sd_image_floats(NT, SD_HT) <= TL_SLOT, "each staged piece of the drift net fits the image buffer");
  const int tid = threadIdx.x, lane0 = tid & 63, threads = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = threads >> 6;
  const int p = lane0 & 15, g0 = lane0 >> 4;
  float* trash = a.trash + tid * 4;
  float* slot = a.hbuf + static_cast<size_t>(blockIdx.x * nw + wave) * TL_HBUF_FLOATS;
  const int per_round = gridDim.x * nw;
  const int rounds = (a.ntiles + per_round - 1) / per_round;
  const size_t Md = static_cast<size_t>(a.M) * a.d;
  const bool lin = rn.form == SDENG_FORM_LIN;
  const float* bias = rn.wpack + sd_off_bias(NT);
  constexpr bool one_image = tlr_one_image(NT);
  const float* wout = one_image ? lds + sd_off_wout(NT) : lds;

  for (int round = 0; round < rounds; ++round) {
    const int tile = (round * gridDim.x + blockIdx.x) * nw + wave;
    const bool active = tile < a.ntiles;  // wave-uniform; an idle wave still helps staging and meets every barrier
    const uint32_t row0 = static_cast<uint32_t>(active ? tile : 0) * 16u + p;
    const bool live = active && row0 < static_cast<uint32_t>(a.M);
    const auto rowf = [&]() __attribute__((always_inline)) { return tlm_fresh(row0); };
    const uint32_t pidx = static_cast<uint32_t>(rn.particle0 + row0);
    float rnd = 0.0f;

    if (active && rn.xs_out) {  // row 0 of the trajectory: x0
      const uint32_t row = rowf();
#pragma unroll
      for (int t = 0; t < NT; ++t) store_quad(rn.xs_out, trash, row, a.d, live, t, g0, load_quad(rn.x_in, row, a.d, live, t, g0));
    }

    for (int k = 0; k < rn.N; ++k) {
      const int g = static_cast<int>(tlm_fresh(static_cast<uint32_t>(g0))), lane = static_cast<int>(tlm_fresh(static_cast<uint32_t>(lane0)));
      // x_k and x_{k+1}: rows of the trajectory, or the caller's x0 and then the two ping-pong rows
      const float* xk = rn.xs_out ? rn.xs_out + static_cast<size_t>(k) * Md : (k == 0 ? rn.x_in : rn.ping + static_cast<size_t>(k & 1) * Md);
      float* xn = rn.xs_out ? rn.xs_out + static_cast<size_t>(k + 1) * Md : rn.ping + static_cast<size_t>((k + 1) & 1) * Md;
      float* sc = rn.ref_out ? rn.ref_out + static_cast<size_t>(k) * Md : rn.score;
      const TlTile w = {lds, tid, threads, lane, g, active, live, xk, sc, slot, trash};

      // ---- a. reference score at (t_k, x_k) into the score rows: the walk of k_tilted_eval ----
      asm volatile("" ::: "memory");  // the state rows were written by the step before: real re-reads
      {
        const float* ti = a.tinfo + static_cast<size_t>(k) * TL_TINFO;
        const float s_t = ti[1], sig_t = ti[2], s_l = ti[3], sig_l = ti[4];
        const float f = a.use_st ? s_t : 1.0f;
        const float* te = rn.te_tab + static_cast<size_t>(k) * TL_H;
        const auto acc_in = [&](f32x4 (&h)[TL_HT]) __attribute__((always_inline)) {  // the input layer's accumulator: the step's time embedding
#pragma unroll
          for (int t = 0; t < TL_HT; ++t) h[t] = load_tile4(te, t, g);
        };
        tl_prior<NT>(a, w, rowf, s_l, sig_l, true);
        tl_forward<NT>(a, w, rowf, s_t, sig_t, f, acc_in, true, true, TlNoRows{});
        tl_backward<NT>(a, w, rowf, s_t, sig_t, f, true, TlNoRows{});
      }

      // ---- b. control: FourierMLP_4x64 under ClippedCtrl (models/mlp.py:135-143, models/reparam.py:33-43) ----
      asm volatile("" ::: "memory");
      const NetScale ns = load_net_scale(bias, NT);
      tl_stage(lds, rn.wpack, tlr_hidden_blocks(NT) + (one_image ? tlr_out_blocks(NT) : 0), tid, threads);
      HidSplit hs;
      if (active) {
        const uint32_t row = rowf();
        f32x4 x[NT], hid[SD_HT];
#pragma unroll
        for (int t = 0; t < NT; ++t) x[t] = load_quad(xk, row, a.d, live, t, g);
        // (the walk above puts the state through unguarded split-f16 products: no range-safe twin here either, scaled weights are
        // un-scaled layer by layer as in the step loops over matrix-pipe references)
        mlp_hidden_scaled<NT>(x, hid, lds, bias, rn.temb + static_cast<size_t>(k) * SD_H, lane, ns);
        hs = split_hidden(hid);
      }
      if (!one_image) tl_stage(lds, rn.wpack + sd_off_wout(NT), tlr_out_blocks(NT), tid, threads);

      // ---- c., d. per pair of output tiles: out_layer -> clip -> cost -> noise -> integrator -> Ito term (k_simulate's tail) ----
      if (active) {
        asm volatile("" ::: "memory");
        const uint32_t row = rowf();
        const float* cf = rn.coef + static_cast<size_t>(k) * SDENG_NCOEF;
        const float c1 = cf[1], c2 = cf[2], c3 = cf[3], c4 = cf[4], c5 = cf[5], c6 = cf[6];
        const float e1 = __builtin_fmaf(c4, c1, 1.0f), e2 = c4 * c2, e3 = c4 * c3, e4 = c2 * c5;  // EM update
        float su2 = 0.0f, suz = 0.0f;
        auto out_group = [&](auto otc, int t0) __attribute__((always_inline)) {
          constexpr int OT = decltype(otc)::value;
          f32x4 u[OT];
          tlr_out_tiles<OT>(hs, wout, bias, t0, lane, u, ns.inv_out);
          if (rn.clip_model > 0.0f) {
            float umax = absmax_tile(u[0]);
#pragma unroll
            for (int o = 1; o < OT; ++o) umax = absmax_tile(umax, u[o]);
            if (__builtin_amdgcn_ballot_w64(!(umax <= rn.clip_model)) != 0) {
#pragma unroll
              for (int o = 0; o < OT; ++o)
#pragma unroll
                for (int r = 0; r < 4; ++r) u[o][r] = clampf(u[o][r], rn.clip_model);
            }
          }
#pragma unroll
          for (int o = 0; o < OT; ++o) {
            const int t = t0 + o;
#pragma unroll
            for (int r = 0; r < 4; ++r) su2 = __builtin_fmaf(u[o][r], u[o][r], su2);
            f32x4 z;
            if (rn.noise_in) z = load_quad(rn.noise_in + static_cast<size_t>(k) * Md, row, a.d, live, t, g);
            else z = philox_normal4(pidx, static_cast<uint32_t>(k), static_cast<uint32_t>(4 * t + g), 0u, rn.seed_lo, rn.seed_hi);
            const f32x4 rq = load_quad(sc, row, a.d, live, t, g), xv = load_quad(xk, row, a.d, live, t, g);
            f32x4 xo;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float uv = u[o][r];
              if (lin) {  // eq/sdes.py:535-538: ret = c1*x + c2*(ref + u); ret += c3*z
                xo[r] = __builtin_fmaf(c3, z[r], __builtin_fmaf(c2, rq[r] + uv, c1 * xv[r]));
              } else {    // losses/oc.py:277-284
                xo[r] = __builtin_fmaf(e4, z[r], __builtin_fmaf(e2, uv, __builtin_fmaf(e3, rq[r], e1 * xv[r])));
              }
              suz = __builtin_fmaf(uv, z[r], suz);
            }
            store_quad(xn, trash, row, a.d, live, t, g, xo);
            if (k == rn.N - 1) store_quad(rn.x_out, trash, row, a.d, live, t, g, xo);
          }
        };
#pragma unroll
        for (int t0 = 0; t0 < NT; t0 += 2) {
          if (t0 + 1 < NT) out_group(std::integral_constant<int, 2>{}, t0);
          else out_group(std::integral_constant<int, 1>{}, t0);
        }
        // running cost 0.5*omega*|u|^2 (losses/oc.py:493) or 0.5*|u|^2*dt (:274); per-step constant; stochastic integral (:284, :499)
        su2 = group_sum(su2);
        rnd += lin ? c4 * su2 : (0.5f * su2) * c4;
        rnd += c6;
        if (rn.flags & SDENG_FLAG_ITO) {
          suz = group_sum(suz);
          rnd += c5 * suz;
        }
      }
    }
    if (live && g0 == 0) rn.rnd_out[row0] = rnd;
  }
}

// The EBM's time embedding at the N step times: lane (p, g) of wave j holds step 16 j + p.  tl_time_embed is per row, so the 128 channels
// of a step are the bits k_tilted_eval computes in place for a row at that time.
__global__ void __launch_bounds__(64) k_tilted_rds_times(const TiltedArgs a, float* te_tab) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x, p = lane & 15, g = lane >> 4;
  const int step = blockIdx.x * 16 + p;
  const bool live = step < a.N;
  const TlTile w = {lds, lane, 64, lane, g, true, live, nullptr, nullptr, nullptr, nullptr};
  f32x4 h[TL_HT];
  tl_time_embed(a, w, a.tinfo[static_cast<size_t>(live ? step : 0) * TL_TINFO], h);
  if (live) {
#pragma unroll
    for (int t = 0; t < TL_HT; ++t) *reinterpret_cast<f32x4*>(te_tab + static_cast<size_t>(step) * TL_H + 16 * t + 4 * g) = h[t];
  }
}

int sd_launch_tilted_rds_times(const TiltedArgs& a, float* te_tab, hipStream_t s) {
  return sd_launch_kernel(k_tilted_rds_times, (a.N + 15) / 16, 64, static_cast<size_t>(TL_SLOT) * sizeof(float), s, a, te_tab);
}

int sd_launch_tilted_rds(const TiltedArgs& a, const TiltedRdsArgs& r, int NT, int grid, int waves, hipStream_t s) {
  return tl_dispatch_nt(NT, [&](auto nt) {
    return sd_launch_kernel(k_tilted_rds<decltype(nt)::value>, grid, waves * 64, static_cast<size_t>(TL_SLOT) * sizeof(float), s, a, r);
  });
}
