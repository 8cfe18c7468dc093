// All Langevin moves of a sampler level over an energy-based (tilted-potential) reference in ONE launch: sdeng_tilted_moves.
// mala_step / ula_step / heuristics_step_size of additions/mcmc.py as k_chain_moves applies them (prep_kernels.hip), with the density of
// k_tilted_eval (tilted_kernel.hpp) at every proposal.  k_chain_moves cannot take that density as a per-thread hook: it is a
// workgroup-cooperative walk over staged 64 KiB images with barriers.  So the ownership is k_tilted_eval's -- one wave owns a 16-row tile of
// chains, 1 to 8 waves per workgroup walk the layers in lock-step -- and the move loop sits inside the round loop: n_moves is uniform, idle
// waves and pad rows meet every barrier of every move.  The walk is written again from k_tilted_eval's building blocks (tl_stage, tl_mm,
// row_normalise, ...) statement by statement, so k_tilted_eval itself is untouched; what differs:
//   * the time embedding depends only on the row's time: computed once per chain before the move loop, kept as layer 5 of the wave's
//     slot (the accumulator the input layer starts from) -- three stagings fewer per move;
//   * the state is evaluated at the proposal rows of the workspace and the score lands in the workspace's proposal-gradient rows; the chain
//     state stays in the caller's x / grad arrays (L2-resident, re-read per phase: every lane re-reads only what it wrote itself) and is
//     overwritten where the move is accepted.  lp, step, acc and the accept bit are per-row scalars, equal in the four lanes of a row
//     (group_sum's two exchanges add the same pairs in every lane).
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
  const int tid = threadIdx.x, lane = tid & 63, lane0 = lane, threads = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = threads >> 6;
  const int p = lane & 15, g = lane >> 4, g0 = g;
  constexpr int KBD = (NT + 1) / 2;
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  const float* cs = a.consts;
  const float* sc = cs + TL_C_SCALE;
  const float* inv = cs + TL_C_INV;
  float* trash = a.trash + tid * 4;
  float* slot = a.hbuf + static_cast<size_t>(blockIdx.x * nw + wave) * TLM_HBUF_FLOATS;
  const float* X = mv.prop;  // the walk evaluates the proposal ...
  float* G = mv.gprop;       // ... and leaves the score at it here
  const int per_round = gridDim.x * nw;
  const int rounds = (a.ntiles + per_round - 1) / per_round;
  const size_t Md = static_cast<size_t>(a.M) * a.d;
  const bool ula = mv.ula != 0;
  const float log_target = mv.target_acc > 0.0f ? logf(mv.target_acc) : 0.0f;
  auto img = [&](int i) { return a.pack + static_cast<size_t>(i) * TL_SLOT; };

  for (int round = 0; round < rounds; ++round) {
    const int tile = (round * gridDim.x + blockIdx.x) * nw + wave;
    const bool active = tile < a.ntiles;  // wave-uniform; an idle wave still helps staging and meets every barrier
    const uint32_t row0 = static_cast<uint32_t>(active ? tile : 0) * 16u + p;
    const bool live = active && row0 < static_cast<uint32_t>(a.M);
    const int kt = live ? static_cast<int>(row0 / static_cast<uint32_t>(a.B)) : 0;
    const float* ti = a.tinfo + static_cast<size_t>(kt) * TL_TINFO;

    // ---- time embedding, once per chain: (b_in + e) 2^e_in, the accumulator the input layer of every move starts from ----
    {
      const float tt = ti[0];
      f32x4 act[TL_HT], h[TL_HT];
      tl_stage(lds, img(TL_TE1S), TL_HT * TL_KBH, tid, threads);
      if (active) {
        f32x4 e[TL_HT];
#pragma unroll
        for (int t = 0; t < TL_HT; ++t) {
          const f32x4 co = load_tile4(cs + TL_C_COEFF, t, g), ph = load_tile4(cs + TL_C_PHASE, t, g);
#pragma unroll
          for (int r = 0; r < 4; ++r) e[t][r] = sinf(co[r] * tt + ph[r]);
        }
        tl_bias<TL_HT>(h, cs + TL_C_BTE1, g);
        tl_mm<TL_HT, TL_HT>(e, h, lds, lane);
      }
      tl_stage(lds, img(TL_TE1C), TL_HT * TL_KBH, tid, threads);
      if (active) {
        f32x4 e[TL_HT];
#pragma unroll
        for (int t = 0; t < TL_HT; ++t) {
          const f32x4 co = load_tile4(cs + TL_C_COEFF, t, g), ph = load_tile4(cs + TL_C_PHASE, t, g);
#pragma unroll
          for (int r = 0; r < 4; ++r) e[t][r] = cosf(co[r] * tt + ph[r]);
        }
        tl_mm<TL_HT, TL_HT>(e, h, lds, lane);
#pragma unroll
        for (int t = 0; t < TL_HT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) act[t][r] = gelu_fast(h[t][r] * inv[TL_TE1S]);
      }
      tl_stage(lds, img(TL_TE2), TL_HT * TL_KBH, tid, threads);
      if (active) {
        f32x4 te[TL_HT];
        tl_bias<TL_HT>(te, cs + TL_C_BTE2, g);
        tl_mm<TL_HT, TL_HT>(act, te, lds, lane);
        const float it = inv[TL_TE2], si = sc[TL_WIN];
#pragma unroll
        for (int t = 0; t < TL_HT; ++t) {
          const f32x4 b = load_tile4(cs + TL_C_BIN, t, g);
#pragma unroll
          for (int r = 0; r < 4; ++r) h[t][r] = __builtin_fmaf(te[t][r] * it, si, b[r]);
        }
        tl_store_h(slot, 5, lane, h);
      }
    }

    float lp = live ? mv.lp[row0] : 0.0f, step = live ? mv.step[row0] : 0.0f, acc = 0.0f, last = 1.0f;
    const uint32_t cidx = static_cast<uint32_t>(mv.chain0 + row0);

    for (int m = 0; m < mv.K; ++m) {
      // (the lane's indices likewise: the addresses of the constants' quads and of the slot's layers are the same in every move)
      const int g = static_cast<int>(tlm_fresh(static_cast<uint32_t>(g0))), lane = static_cast<int>(tlm_fresh(static_cast<uint32_t>(lane0)));
      // ---- proposal: sample_multivariate_normal_diag(mean = y + h grad, variance = 2 h)  (mcmc.py:19-21, :97-99) ----
      if (active) {
        const uint32_t row = tlm_fresh(row0);
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
      auto scaled_input = [&](f32x4 (&xs)[NT], f32x4 (&rci)[NT]) __attribute__((always_inline)) {
        asm volatile("" ::: "memory");  // a real re-read (see k_tilted_eval)
        const uint32_t row = tlm_fresh(row0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 xv = load_quad(X, row, a.d, live, t, g);
          const f32x4 mg = load_tile4(cs + TL_C_MEANG, t, g), vg = load_tile4(cs + TL_C_VARG, t, g);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float ci = s_t * sqrtf(vg[r] + sig_t);
            const bool ok = feat_lt(t, r, 4 * g, a.d);
            rci[t][r] = ok ? 1.0f / ci : 0.0f;
            xs[t][r] = ok ? (xv[r] - s_t * mg[r]) / ci : 0.0f;
          }
        }
      };
      // prior: the mixture noised to t' (online softmax over the components)
      float lp_p = 0.0f;
      {
        float m_run = -INFINITY, l_run = 0.0f;
        f32x4 pg[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) pg[t] = zero;
        const float s2 = s_l * s_l;
        const float c_norm = 0.9189385332046727f * static_cast<float>(a.d);  // 0.5 d log(2 pi)
        for (int k = 0; k < a.K; ++k) {
          const uint32_t row = tlm_fresh(row0);
          const float* mk = cs + TL_C_MEANS + 128 * k;
          const float* vk = cs + TL_C_VARS + 128 * k;
          f32x4 q[NT];
          float maha = 0.0f, logdet = 0.0f;
          if (!a.full) {
            if (active) {
#pragma unroll
              for (int t = 0; t < NT; ++t) {
                const f32x4 xv = load_quad(X, row, a.d, live, t, g);
                const f32x4 mm = load_tile4(mk, t, g), vv = load_tile4(vk, t, g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const bool ok = feat_lt(t, r, 4 * g, a.d);
                  const float var = s2 * (vv[r] + sig_l), z = xv[r] - s_l * mm[r];
                  q[t][r] = ok ? z / var : 0.0f;
                  maha = __builtin_fmaf(ok ? z : 0.0f, q[t][r], maha);
                  logdet += ok ? logf(var) : 0.0f;
                }
              }
            }
          } else {
            tl_stage(lds, img(TL_EIG + 2 * k), NT * KBD, tid, threads);  // P^T
            if (active) {
              f32x4 z[NT], y[NT];
#pragma unroll
              for (int t = 0; t < NT; ++t) {
                const f32x4 xv = load_quad(X, row, a.d, live, t, g);
                const f32x4 mm = load_tile4(mk, t, g);
#pragma unroll
                for (int r = 0; r < 4; ++r) z[t][r] = feat_lt(t, r, 4 * g, a.d) ? xv[r] - s_l * mm[r] : 0.0f;
                y[t] = zero;
              }
              const float sg = row_normalise<NT>(z), back = inv[TL_EIG + 2 * k] / sg;
              tl_mm<NT, NT, true>(z, y, lds, lane, sg);
#pragma unroll
              for (int t = 0; t < NT; ++t) {
                const f32x4 dv = load_tile4(vk, t, g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const bool ok = feat_lt(t, r, 4 * g, a.d);
                  const float var = s2 * (dv[r] + sig_l), yv = y[t][r] * back;
                  q[t][r] = ok ? yv / var : 0.0f;
                  maha = __builtin_fmaf(ok ? yv : 0.0f, q[t][r], maha);
                  logdet += ok ? logf(var) : 0.0f;
                }
              }
            }
            tl_stage(lds, img(TL_EIG + 2 * k + 1), NT * KBD, tid, threads);  // P
            if (active) {
              f32x4 pq[NT];
#pragma unroll
              for (int t = 0; t < NT; ++t) pq[t] = zero;
              const float sg = row_normalise<NT>(q), back = inv[TL_EIG + 2 * k + 1] / sg;
              tl_mm<NT, NT, true>(q, pq, lds, lane, sg);
#pragma unroll
              for (int t = 0; t < NT; ++t) q[t] = pq[t] * back;
            }
          }
          if (active) {
            maha = group_sum(maha);
            logdet = group_sum(logdet);
            const float lpk = cs[TL_C_LOGW + k] - (c_norm + 0.5f * (logdet + maha));
            const float m_new = fmaxf(m_run, lpk);
            const float so = exp_nonpos(m_run - m_new), pk = exp_nonpos(lpk - m_new);
            l_run = l_run * so + pk;
            m_run = m_new;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
              for (int r = 0; r < 4; ++r) pg[t][r] = __builtin_fmaf(pk, -q[t][r], pg[t][r] * so);
          }
        }
        if (active) {
          lp_p = m_run + logf(l_run);
          const float il = 1.0f / l_run;
          const uint32_t row = tlm_fresh(row0);
#pragma unroll
          for (int t = 0; t < NT; ++t) store_quad(G, trash, row, a.d, live, t, g, pg[t] * il);
        }
      }
      {
        f32x4 act[TL_HT], h[TL_HT];
        // input layer, from the kept time embedding
        tl_stage(lds, img(TL_WIN), TL_HT * KBD, tid, threads);
        if (active) {
          f32x4 xs[NT], rci[NT];
          scaled_input(xs, rci);
#pragma unroll
          for (int t = 0; t < TL_HT; ++t) h[t] = tl_load_h(slot, 5, t, lane);
          tl_mm<NT, TL_HT>(xs, h, lds, lane);
#pragma unroll
          for (int t = 0; t < TL_HT; ++t) {
            h[t] = h[t] * inv[TL_WIN];
#pragma unroll
            for (int r = 0; r < 4; ++r) act[t][r] = gelu_fast(h[t][r]);
          }
          tl_store_h(slot, 0, lane, h);
        }
        // four hidden layers
        for (int l = 0; l < 4; ++l) {
          tl_stage(lds, img(TL_WH + l), TL_HT * TL_KBH, tid, threads);
          if (active) {
            tl_bias<TL_HT>(h, cs + TL_C_BH + 128 * l, g);
            tl_mm<TL_HT, TL_HT>(act, h, lds, lane);
            const float iv = inv[TL_WH + l];
#pragma unroll
            for (int t = 0; t < TL_HT; ++t) {
              h[t] = h[t] * iv;
#pragma unroll
              for (int r = 0; r < 4; ++r) act[t][r] = gelu_fast(h[t][r]);
            }
            tl_store_h(slot, l + 1, lane, h);
          }
        }
        // output layer, tilt 'dot': base_lp = -<v, xs>, and the -v / c_i half of base_grad
        tl_stage(lds, img(TL_WOUT), NT * TL_KBH, tid, threads);
        if (active) {
          f32x4 xs[NT], rci[NT], v[NT];
          scaled_input(xs, rci);
          tl_bias<NT>(v, cs + TL_C_BOUT, g);
          tl_mm<TL_HT, NT>(act, v, lds, lane);
          float dot = 0.0f;
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            v[t] = v[t] * inv[TL_WOUT];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              dot = __builtin_fmaf(v[t][r], xs[t][r], dot);
              v[t][r] *= rci[t][r];
            }
          }
          const float base_lp = -group_sum(dot);
          lp_p = lp_p + f * base_lp;
          tl_grad_axpy<NT>(G, trash, tlm_fresh(row0), a.d, live, g, -f, v);
        }
      }
      // backward: J^T xs, the other half of base_grad
      {
        f32x4 dh[TL_HT], gacc[TL_HT];
        tl_stage(lds, img(TL_WOUT_T), TL_HT * KBD, tid, threads);
        if (active) {
          f32x4 xs[NT], rci[NT];
          scaled_input(xs, rci);
          const float sg = row_normalise<NT>(xs), back = inv[TL_WOUT_T] / sg;
#pragma unroll
          for (int t = 0; t < TL_HT; ++t) gacc[t] = zero;
          tl_mm<NT, TL_HT, true>(xs, gacc, lds, lane, sg);
#pragma unroll
          for (int t = 0; t < TL_HT; ++t) {
            const f32x4 hv = tl_load_h(slot, 4, t, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) dh[t][r] = (gacc[t][r] * back) * gelu_grad(hv[r]);
          }
        }
        for (int l = 3; l >= 0; --l) {
          tl_stage(lds, img(TL_WH_T + l), TL_HT * TL_KBH, tid, threads);  // transpose of hidden layer l
          if (active) {
            const float sg = row_normalise<TL_HT>(dh), back = inv[TL_WH_T + l] / sg;
#pragma unroll
            for (int t = 0; t < TL_HT; ++t) gacc[t] = zero;
            tl_mm<TL_HT, TL_HT, true>(dh, gacc, lds, lane, sg);
#pragma unroll
            for (int t = 0; t < TL_HT; ++t) {
              const f32x4 hv = tl_load_h(slot, l, t, lane);
#pragma unroll
              for (int r = 0; r < 4; ++r) dh[t][r] = (gacc[t][r] * back) * gelu_grad(hv[r]);
            }
          }
        }
        tl_stage(lds, img(TL_WIN_T), NT * TL_KBH, tid, threads);
        if (active) {
          f32x4 xs[NT], rci[NT], jx[NT];
          scaled_input(xs, rci);
          const float sg = row_normalise<TL_HT>(dh), back = inv[TL_WIN_T] / sg;
#pragma unroll
          for (int t = 0; t < NT; ++t) jx[t] = zero;
          tl_mm<TL_HT, NT, true>(dh, jx, lds, lane, sg);
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) jx[t][r] = (jx[t][r] * back) * rci[t][r];
          tl_grad_axpy<NT>(G, trash, tlm_fresh(row0), a.d, live, g, -f, jx);
        }
      }

      // ---- accept, step size, outputs: the Langevin instantiation of k_chain_moves (prep_kernels.hip), statement by statement ----
      if (active) {
        asm volatile("" ::: "memory");
        const uint32_t row = tlm_fresh(row0);
        float log_acc = 0.0f;
        if (!ula) {
          // log q(prop | y) and log q(y | prop), unnormalised: -0.5 sum (samples - mean)^2 / variance  (mcmc.py:24-31)
          float qf = 0.0f, qb = 0.0f;
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const f32x4 xv = load_quad(mv.x, row, a.d, live, t, g), gv = load_quad(mv.grad, row, a.d, live, t, g);
            const f32x4 pv = load_quad(X, row, a.d, live, t, g), gp = load_quad(G, row, a.d, live, t, g);
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
          const float var = 2.0f * step;
          const float joint_prop = lp_p - (-0.5f * qf) / var, joint_orig = lp - (-0.5f * qb) / var;
          log_acc = joint_prop - joint_orig;
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
          accept = logf(uu) < log_acc;  // a NaN log-density at the proposal: NaN log_acc, rejected -- the chain keeps its finite state
        }
        const bool keep = m >= mv.keep_from;
        const bool take = live && accept;
        if (take) lp = lp_p;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 pv = load_quad(X, row, a.d, live, t, g), gp = load_quad(G, row, a.d, live, t, g);
          const f32x4 xv = load_quad(mv.x, row, a.d, live, t, g);
          store_quad(mv.x, trash, row, a.d, take, t, g, pv);
          store_quad(mv.grad, trash, row, a.d, take, t, g, gp);
          if (keep && mv.samples)
            store_quad(mv.samples + static_cast<size_t>(m - mv.keep_from) * Md, trash, row, a.d, live, t, g, take ? pv : xv);
        }
        if (!ula && mv.target_acc > 0.0f) {  // heuristics_step_size (mcmc.py:55-74), per chain
          if (log_acc - log_target > 0.04879016416943205f) step = step * 1.01f;        // log1p(0.05)
          if (log_target - log_acc > 0.05129329438755058f) step = step / 1.01f;        // -log1p(-0.05)
        }
        if (!ula) last = expf(fminf(0.0f, log_acc));
        if (keep && !ula) acc += last;
      }
    }
    if (live && g == 0) {
      mv.lp[row0] = lp;
      mv.step[row0] = step;
      if (mv.acc_sum) mv.acc_sum[row0] = acc;
      if (mv.acc_last) mv.acc_last[row0] = last;
    }
  }
}

template <int NT>
static int launch_tilted_moves(const TiltedArgs& a, const TiltedMovesArgs& mv, int grid, int waves, hipStream_t stream) {
  return sd_launch_kernel(k_tilted_moves<NT>, grid, waves * 64, static_cast<size_t>(TL_SLOT) * sizeof(float), stream, a, mv);
}

int sd_launch_tilted_moves(const TiltedArgs& a, const TiltedMovesArgs& mv, int NT, int grid, int waves, hipStream_t s) {
  switch (NT) {
    case 1: return launch_tilted_moves<1>(a, mv, grid, waves, s);
    case 2: return launch_tilted_moves<2>(a, mv, grid, waves, s);
    case 3: return launch_tilted_moves<3>(a, mv, grid, waves, s);
    case 4: return launch_tilted_moves<4>(a, mv, grid, waves, s);
    case 5: return launch_tilted_moves<5>(a, mv, grid, waves, s);
    case 6: return launch_tilted_moves<6>(a, mv, grid, waves, s);
    case 7: return launch_tilted_moves<7>(a, mv, grid, waves, s);
    case 8: return launch_tilted_moves<8>(a, mv, grid, waves, s);
  }
  return static_cast<int>(hipErrorInvalidValue);
}
