// All Langevin moves of a sampler level over an energy-based (tilted-potential) reference in ONE launch: sdeng_tilted_moves.
// mala_step / ula_step / heuristics_step_size of additions/mcmc.py (their scalar rules: langevin_rules.hpp, shared with k_chain_moves of
// prep_kernels.hip), with the density of k_tilted_eval (tilted_kernel.hpp) at every proposal.  k_chain_moves cannot take that density as a
// per-thread hook: it is a workgroup-cooperative walk over staged 64 KiB images with barriers.  So the ownership is k_tilted_eval's -- one
// wave owns a 16-row tile of chains, 1 to 8 waves per workgroup walk the layers in lock-step -- and the move loop sits inside the round loop:
// n_moves is uniform, idle waves and pad rows meet every barrier of every move.  The walk is k_tilted_eval's own: the phases of
// tilted_kernel.hpp (tl_prior, tl_time_embed, tl_forward, tl_backward), called with what differs here:
//   * the time embedding depends only on the row's time: computed once per chain before the move loop, kept as layer 5 of the wave's
//     slot (the accumulator the input layer starts from) -- three stagings fewer per move;
//   * the state is evaluated at the proposal rows of the workspace and the score lands in the workspace's proposal-gradient rows; the chain
//     state stays in the caller's x / grad arrays (L2-resident, re-read per phase: every lane re-reads only what it wrote itself) and is
//     overwritten where the move is accepted.  lp, step, acc and the accept bit are per-row scalars, equal in the four lanes of a row
//     (group_sum's two exchanges add the same pairs in every lane).
// What keeps the move loop in 256 registers: the row index re-made per phase and the lane's indices re-made per move (tlm_fresh), and the
// times re-read per move.
#include "langevin_rules.hpp"
#include "tilted_kernel.hpp"

// The row index as a value the compiler cannot see through: the rows of a chain are the same in every move, so the addresses of every
// quad of x / grad / proposal / noise / samples would be hoisted out of the move loop and held (eight registers per tile and array at a
// d that is no multiple of four) -- and spilled.  Recomputed per phase they cost a few integer instructions.
SD_INLINE uint32_t tlm_fresh(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <int NT>
__global__ void __launch_bounds__(512, 2) k_tilted_moves(const TiltedArgs a, const TiltedMovesArgs mv) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane0 = tid & 63, threads = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = threads >> 6;
  const int p = lane0 & 15, g0 = lane0 >> 4;
  float* trash = a.trash + tid * 4;
  float* slot = a.hbuf + static_cast<size_t>(blockIdx.x * nw + wave) * TLM_HBUF_FLOATS;
  const int per_round = gridDim.x * nw;
  const int rounds = (a.ntiles + per_round - 1) / per_round;
  const size_t Md = static_cast<size_t>(a.M) * a.d;
  const bool ula = mv.ula != 0;
  const float log_target = mv.target_acc > 0.0f ? logf(mv.target_acc) : 0.0f;

  for (int round = 0; round < rounds; ++round) {
    const int tile = (round * gridDim.x + blockIdx.x) * nw + wave;
    const bool active = tile < a.ntiles;  // wave-uniform; an idle wave still helps staging and meets every barrier
    const uint32_t row0 = static_cast<uint32_t>(active ? tile : 0) * 16u + p;
    const bool live = active && row0 < static_cast<uint32_t>(a.M);
    const int kt = live ? static_cast<int>(row0 / static_cast<uint32_t>(a.B)) : 0;
    const float* ti = a.tinfo + static_cast<size_t>(kt) * TL_TINFO;
    const auto rowf = [&]() __attribute__((always_inline)) { return tlm_fresh(row0); };

    // ---- time embedding, once per chain: (b_in + e) 2^e_in, the accumulator the input layer of every move starts from ----
    {
      const TlTile w = {lds, tid, threads, lane0, g0, active, live, mv.prop, mv.gprop, slot, trash};
      f32x4 h[TL_HT];
      tl_time_embed(a, w, ti[0], h);
      if (active) tl_store_h(slot, 5, lane0, h);
    }

    float lp = live ? mv.lp[row0] : 0.0f, step = live ? mv.step[row0] : 0.0f, acc = 0.0f, last = 1.0f;
    const uint32_t cidx = static_cast<uint32_t>(mv.chain0 + row0);

    for (int m = 0; m < mv.K; ++m) {
      // (the lane's indices likewise: the addresses of the constants' quads and of the slot's layers are the same in every move)
      const int g = static_cast<int>(tlm_fresh(static_cast<uint32_t>(g0))), lane = static_cast<int>(tlm_fresh(static_cast<uint32_t>(lane0)));
      // the walk evaluates the proposal rows and leaves the score at the proposal in the proposal-gradient rows
      const TlTile w = {lds, tid, threads, lane, g, active, live, mv.prop, mv.gprop, slot, trash};
      // ---- proposal: sample_multivariate_normal_diag(mean = y + h grad, variance = 2 h)  (mcmc.py:19-21, :97-99) ----
      if (active) {
        const uint32_t row = rowf();
        const float sd = sqrtf(2.0f * step);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          f32x4 zq;
          if (mv.z) zq = load_quad(mv.z + static_cast<size_t>(m) * Md, row, a.d, live, t, g);
          else zq = philox_normal4(cidx, static_cast<uint32_t>(m), static_cast<uint32_t>(4 * t + g), 8u, mv.seed_lo, mv.seed_hi);
          const f32x4 xv = load_quad(mv.x, row, a.d, live, t, g), gv = load_quad(mv.grad, row, a.d, live, t, g);
          f32x4 pr;
#pragma unroll
          for (int r = 0; r < 4; ++r) pr[r] = sd * zq[r] + (xv[r] + step * gv[r]);
          store_quad(mv.prop, trash, row, a.d, live, t, g, pr);
        }
      }

      // ---- the tilted density and score at (t_row, proposal): the walk of k_tilted_eval ----
      asm volatile("" ::: "memory");  // the times are re-read per move: five registers fewer across the move loop
      const float s_t = ti[1], sig_t = ti[2], s_l = ti[3], sig_l = ti[4];
      const float f = a.use_st ? s_t : 1.0f;
      const auto acc_in = [&](f32x4 (&h)[TL_HT]) __attribute__((always_inline)) {  // the input layer's accumulator: the kept time embedding
#pragma unroll
        for (int t = 0; t < TL_HT; ++t) h[t] = tl_load_h(slot, 5, t, lane);
      };
      const float prior_lp = tl_prior<NT>(a, w, rowf, s_l, sig_l, true);
      const float base_lp = tl_forward<NT>(a, w, rowf, s_t, sig_t, f, acc_in, true, true, TlNoRows{});
      const float lp_p = prior_lp + f * base_lp;
      tl_backward<NT>(a, w, rowf, s_t, sig_t, f, true, TlNoRows{});

      // ---- accept, step size, outputs: the Langevin instantiation of k_chain_moves (prep_kernels.hip) ----
      if (active) {
        asm volatile("" ::: "memory");
        const uint32_t row = rowf();
        float log_acc = 0.0f;
        if (!ula) {
          // log q(prop | y) and log q(y | prop), unnormalised: -0.5 sum (samples - mean)^2 / variance  (mcmc.py:24-31)
          float qf = 0.0f, qb = 0.0f;
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const f32x4 xv = load_quad(mv.x, row, a.d, live, t, g), gv = load_quad(mv.grad, row, a.d, live, t, g);
            const f32x4 pv = load_quad(mv.prop, row, a.d, live, t, g), gp = load_quad(mv.gprop, row, a.d, live, t, g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float df = pv[r] - (xv[r] + step * gv[r]);
              const float db = xv[r] - (pv[r] + step * gp[r]);
              qf += df * df;
              qb += db * db;
            }
          }
          qf = group_sum(qf);
          qb = group_sum(qb);
          log_acc = mala_log_acc(lp_p, lp, qf, qb, step);
        }
        bool accept = true;
        if (!ula) {
          float uu;
          if (mv.u) {
            uu = live ? mv.u[static_cast<size_t>(m) * a.M + row] : 1.0f;
          } else {
            uint32_t r4[4];
            philox4x32_10(cidx, 0u, static_cast<uint32_t>(m), 9u, mv.seed_lo, mv.seed_hi, r4);
            uu = u01(r4[0]);
          }
          accept = mh_accept(uu, log_acc);
        }
        const bool keep = m >= mv.keep_from;
        const bool take = live && accept;
        if (take) lp = lp_p;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 pv = load_quad(mv.prop, row, a.d, live, t, g), gp = load_quad(mv.gprop, row, a.d, live, t, g);
          const f32x4 xv = load_quad(mv.x, row, a.d, live, t, g);
          store_quad(mv.x, trash, row, a.d, take, t, g, pv);
          store_quad(mv.grad, trash, row, a.d, take, t, g, gp);
          if (keep && mv.samples)
            store_quad(mv.samples + static_cast<size_t>(m - mv.keep_from) * Md, trash, row, a.d, live, t, g, take ? pv : xv);
        }
        if (!ula && mv.target_acc > 0.0f) step = mh_adapt_step(step, log_acc, log_target);
        if (!ula) last = mh_acc_prob(log_acc);
        if (keep && !ula) acc += last;
      }
    }
    if (live && g0 == 0) {
      mv.lp[row0] = lp;
      mv.step[row0] = step;
      if (mv.acc_sum) mv.acc_sum[row0] = acc;
      if (mv.acc_last) mv.acc_last[row0] = last;
    }
  }
}

int sd_launch_tilted_moves(const TiltedArgs& a, const TiltedMovesArgs& mv, int NT, int grid, int waves, hipStream_t s) {
  return tl_dispatch_nt(NT, [&](auto nt) {
    return sd_launch_kernel(k_tilted_moves<decltype(nt)::value>, grid, waves * 64, static_cast<size_t>(TL_SLOT) * sizeof(float), s, a, mv);
  });
}
