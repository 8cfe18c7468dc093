// Energy-based (tilted-potential) references in ONE launch: log-density and score of GMMTitledPotential / GaussTiltedPotential
// (models/reparam.py:277-606) around FourierMLP(num_layers=6, channels=128, GELU) (models/mlp.py:57-143) over M = N * B (time, state)
// rows, row r at time r / B -- the layout of VjpArgs (grad_kernel.hpp) and of replica exchange's levels x chains.  Per row:
//
//   xs   = (x - s mean_gauss) / c_i,  c_i = s sqrt(var_gauss + sigma^2)                        scaling_input        reparam.py:420-424
//   e    = W_t2 gelu(W_t1 [sin(w t + phi) | cos(w t + phi)] + b_t1) + b_t2                      TimeEmbed.forward    mlp.py:85-96
//   h0   = W_in xs + b_in + e ;  h_l = W_l gelu(h_{l-1}) + b_l (l = 1..4) ;  v = W_out gelu(h4) + b_out               mlp.py:135-143
//   base_lp   = -<v, xs>                                                                        tilt 'dot'           reparam.py:428-430
//   base_grad = -(v + J^T xs) / c_i,  J^T xs = W_in^T (gelu'(h0) . W_1^T (gelu'(h1) . ... W_out^T xs))               (compute_gradx, :463-465)
//   prior     = log-density and score of the mixture noised to t' = max(t, t_limit), weights renormalised            :376-418, sdes.py:208-307
//   log_prob  = prior_lp + f base_lp ;  grad = prior_grad + f base_grad,  f = s(t) with use_s_t_scaling, else 1      :457-476
//
// One wave = 16 rows in the register layout of sim_common.hpp; every product is a split-f16 MFMA chain (dense<> of sim_device.hpp, in
// chunks of four output tiles).  The hidden width is 128 = 8 tiles, so one layer image is 64 KiB: the forward and transposed images of
// the net (and the eigenvector images of a full-covariance prior) cannot share the CU's 160 KiB.  Layout chosen: the workgroup walks the
// layers in lock-step and stages ONE image at a time into a 64 KiB LDS buffer (two barriers per layer); its waves -- 1 to 8, as many
// as keep every CU busy -- each own a 16-row tile.  The pre-activations h0..h4 that the backward pass needs (160 registers per lane)
// go to a per-wave slot of the workspace in the lane's own register order (coalesced 16-byte stores) and come back layer by layer.
// Range: the cotangents of the backward pass and the operands of the prior's eigenvector products are scaled per row by a power of two
// (row_normalise, grad_kernel.hpp) and scaled back: exact.  The scaled state xs and the activations of the net are NOT guarded: beyond
// 65 504 the f16 split gives inf / NaN where fp32 GEMMs would stay finite.
#pragma once
#include <type_traits>
#include "grad_kernel.hpp"

#define TL_H 128            // channels of the EBM's net
#define TL_HT 8             // channel tiles
#define TL_KBH 4            // 32-channel K-blocks
#define TL_SLOT sd_image_floats(TL_HT, TL_HT)  // floats of one image slot (a [128 x 128] image): 64 KiB
#define TL_KMAX 16
// image slots: forward net, transposed net, then per mixture component P^T and P
enum { TL_TE1S = 0, TL_TE1C, TL_TE2, TL_WIN, TL_WH, TL_WOUT = TL_WH + 4, TL_WOUT_T, TL_WH_T, TL_WIN_T = TL_WH_T + 4, TL_EIG, TL_NIMG = TL_EIG + 2 * TL_KMAX };
// constants block behind the images (floats)
enum {
  TL_C_COEFF = 0, TL_C_PHASE = 128, TL_C_BTE1 = 256, TL_C_BTE2 = 384, TL_C_BIN = 512, TL_C_BH = 640, TL_C_BOUT = 1152, TL_C_MEANG = 1280,
  TL_C_VARG = 1408, TL_C_SCALE = 1536, TL_C_INV = 1600, TL_C_LOGW = 1664, TL_C_MEANS = 1680, TL_C_VARS = TL_C_MEANS + TL_KMAX * 128,
  TL_C_TOTAL = TL_C_VARS + TL_KMAX * 128
};
#define TL_TINFO 5          // per time: t, s(t), sigma_sq(t), s(t'), sigma_sq(t')
#define TL_HBUF_FLOATS (5 * TL_HT * 64 * 4)  // per-wave slot of pre-activations: 40 KiB

struct TiltedArgs {
  int M, B, d, N, K, full, use_st, ntiles;
  const float* x;       // [M, d]
  const float* tinfo;   // [N][TL_TINFO]
  const float* pack;    // image slots [..][TL_SLOT]
  const float* consts;  // TL_C_*
  float* hbuf;          // [grid * waves][TL_HBUF_FLOATS], or nullptr (no gradient)
  float* log_prob;      // [M] or nullptr
  float* grad;          // [M, d] or nullptr
  float* trash;         // [512 * 4]
};
// per-row arrays of the training instantiation (TRAIN), row-major, row r as in TiltedArgs: everything the weight gradients of
// E_r = -prior_lp_r + f_r <v_r, xs_r> need (sdeng_tilted_vjp, include/sdeng.h); the outer products are the caller's
struct TiltedRows {
  float* a[5];          // [M, 128] gelu(h_l), l = 0..4
  float* d[5];          // [M, 128] f_r dh_l: dh_l the cotangent of h_l under <v, xs> (the backward pass of J^T xs)
  float* xs;            // [M, d] the scaled state
  float* dv;            // [M, d] f_r xs, the cotangent of v
};

// the constants block: time-embedding frequencies, the Gaussian of the input scaling and the mixture prior, padded (k_tilted_consts)
struct TiltedConstArgs {
  float* consts;
  const float *coeff, *phase, *mean_gauss, *var_gauss, *weights, *means, *vars;
  int d, K;
};
// Langevin moves over the tilted density (k_tilted_moves, tilted_moves_inst.hip): the chain state next to the TiltedArgs of the net.
// The caller's x / grad hold the current state and are updated in place on acceptance; prop / gprop are the proposal and the score at it.
#define TLM_HBUF_FLOATS (6 * TL_HT * 64 * 4)  // per-wave slot: the five pre-activations and, as layer 5, the time embedding's accumulator: 48 KiB
struct TiltedMovesArgs {
  float *x, *grad;      // [M, d]
  float *lp, *step;     // [M]
  float *prop, *gprop;  // [M, d] workspace
  const float* z;       // [K, M, d] or nullptr: Philox stream 8
  const float* u;       // [K, M] or nullptr: Philox stream 9
  float* samples;       // [K - keep_from, M, d] or nullptr
  float *acc_sum, *acc_last;  // [M] or nullptr
  int K, keep_from, ula;
  float target_acc;
  uint32_t seed_lo, seed_hi;
  long long chain0;
};
int sd_launch_tilted_consts(const TiltedConstArgs& a, hipStream_t s);
int sd_launch_tilted_moves(const TiltedArgs& a, const TiltedMovesArgs& mv, int NT, int grid, int waves, hipStream_t s);
int sd_launch_tilted(const TiltedArgs& a, int NT, int grid, int waves, hipStream_t s);
int sd_launch_tilted_train(const TiltedArgs& a, const TiltedRows& rows, int NT, int grid, int waves, hipStream_t s);
inline int sd_tilted_waves(int ntiles) {  // waves per workgroup: as many as still leave a workgroup for every CU
  int w = 1;
  while (w < 8 && ntiles / (2 * w) >= 256) w *= 2;
  return w;
}
inline int sd_tilted_grid(int ntiles, int waves) {
  const int g = (ntiles + waves - 1) / waves;
  return g > 512 ? 512 : (g < 1 ? 1 : g);  // two 64 KiB workgroups fit a CU; more tiles than that: further rounds
}

#ifdef __HIPCC__
// out += W in, four output tiles at a time (dense<> of all eight at once would hold 64 registers of A operands); the body is dense<>'s
template <int NTI, int TO, int C0, int TC, bool SCALED>
SD_INLINE void tl_mm_chunk(const f32x4 (&in)[NTI], f32x4 (&out)[TO], const f16x8* w8, int lane, float sg) {
  constexpr int KB = (NTI + 1) / 2;
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 mx[TC];
#pragma unroll
  for (int to = 0; to < TC; ++to) mx[to] = zero;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    f16x8 xh, xl;
    if constexpr (SCALED) {
      if (2 * kb + 1 < NTI) split8(in[2 * kb] * sg, in[2 * kb + 1 < NTI ? 2 * kb + 1 : 0] * sg, xh, xl);
      else split8_half(in[2 * kb] * sg, xh, xl);
    } else {
      if (2 * kb + 1 < NTI) split8(in[2 * kb], in[2 * kb + 1 < NTI ? 2 * kb + 1 : 0], xh, xl);
      else split8_half(in[2 * kb], xh, xl);
    }
    f16x8 ah[TC], al[TC];
#pragma unroll
    for (int to = 0; to < TC; ++to) {
      ah[to] = w8[(((C0 + to) * KB + kb) * 2 + 0) * 64 + lane];
      al[to] = w8[(((C0 + to) * KB + kb) * 2 + 1) * 64 + lane];
    }
#pragma unroll
    for (int to = 0; to < TC; ++to) out[C0 + to] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[to], xh, out[C0 + to], 0, 0, 0);
#pragma unroll
    for (int to = 0; to < TC; ++to) mx[to] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[to], xl, mx[to], 0, 0, 0);
#pragma unroll
    for (int to = 0; to < TC; ++to) mx[to] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[to], xh, mx[to], 0, 0, 0);
  }
#pragma unroll
  for (int to = 0; to < TC; ++to)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[C0 + to][r] = __builtin_fmaf(mx[to][r], SD_LO_INV, out[C0 + to][r]);
  __builtin_amdgcn_sched_barrier(0);
}
template <int NTI, int TO, bool SCALED = false>
SD_INLINE void tl_mm(const f32x4 (&in)[NTI], f32x4 (&out)[TO], const float* w, int lane, float sg = 1.0f) {
  const f16x8* w8 = reinterpret_cast<const f16x8*>(w);
  tl_mm_chunk<NTI, TO, 0, (TO < 4 ? TO : 4), SCALED>(in, out, w8, lane, sg);
  if constexpr (TO > 4) tl_mm_chunk<NTI, TO, 4, TO - 4, SCALED>(in, out, w8, lane, sg);
}

SD_INLINE void tl_stage(float* lds, const float* src, int nblocks, int tid, int threads) {
  __syncthreads();  // every wave is done with the image that is there
  const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
  f32x4* d4 = reinterpret_cast<f32x4*>(lds);
  for (int i = tid; i < nblocks * 128; i += threads) d4[i] = s4[i];
  __syncthreads();
}

template <int T>
SD_INLINE void tl_bias(f32x4 (&v)[T], const float* b, int g) {
#pragma unroll
  for (int t = 0; t < T; ++t) v[t] = load_tile4(b, t, g);
}
SD_INLINE void tl_store_h(float* slot, int layer, int lane, const f32x4 (&v)[TL_HT]) {
#pragma unroll
  for (int t = 0; t < TL_HT; ++t) *reinterpret_cast<f32x4*>(slot + ((layer * TL_HT + t) * 64 + lane) * 4) = v[t];
}
SD_INLINE f32x4 tl_load_h(const float* slot, int layer, int t, int lane) {
  return *reinterpret_cast<const f32x4*>(slot + ((layer * TL_HT + t) * 64 + lane) * 4);
}

// one [M][128] array of the training mode, in the layout of store_h (grad_kernel.hpp): this lane's four channels of every tile in one
// 16-byte store; a pad row (row >= M, or the rows of an idle wave) goes to the lane's dump slot.  `c` scales (the f_r of the cotangents).
SD_INLINE void tl_store_row(float* dst, float* trash, uint32_t row, bool live, int g, const f32x4 (&v)[TL_HT]) {
#pragma unroll
  for (int t = 0; t < TL_HT; ++t) *reinterpret_cast<f32x4*>(live ? dst + static_cast<size_t>(row) * TL_H + 16 * t + 4 * g : trash) = v[t];
}
SD_INLINE void tl_store_row(float* dst, float* trash, uint32_t row, bool live, int g, const f32x4 (&v)[TL_HT], float c) {
#pragma unroll
  for (int t = 0; t < TL_HT; ++t) *reinterpret_cast<f32x4*>(live ? dst + static_cast<size_t>(row) * TL_H + 16 * t + 4 * g : trash) = v[t] * c;
}

// grad[row] += c * v on the live features (the running sum of the score lives in the output array between the phases of the kernel:
// every lane re-reads only what it wrote itself)
template <int NT>
SD_INLINE void tl_grad_axpy(float* grad, float* trash, uint32_t row, int d, bool live, int g, float c, const f32x4 (&v)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x4 o = load_quad(grad, row, d, live, t, g);
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = o[r] + c * v[t][r];
    store_quad(grad, trash, row, d, live, t, g, o);
  }
}

// ---- The walk of one 16-row tile, phase by phase.  k_tilted_eval<NT, TRAIN> below, k_tilted_moves<NT> (tilted_moves_inst.hip) and
// k_tilted_rds<NT> (tilted_rds_inst.hip) call these four phases and hold no walk of their own, so the order of the floating-point statements inside a phase is shared: with
// -ffp-contract=off the same statements give the same bits, and the state a move kernel carries is the evaluation at that state.
// Every tl_stage is met by every wave of the workgroup, idle waves (`active` false) and pad rows included: the conditions around a
// staging are uniform over the workgroup, the conditions on `active` are around the arithmetic only.
// What differs between the callers comes in as arguments and always-inline callables: `rowf()` gives the lane's row (the move kernel
// re-makes it per phase, tlm_fresh), `hook` takes the per-layer rows of the training mode.
struct TlTile {         // a wave and its tile
  float* lds;           // the workgroup's 64 KiB image buffer
  int tid, threads, lane, g;
  bool active, live;    // the wave has a tile (wave-uniform); the lane's row is below M
  const float* x;       // [M, d] the rows the walk evaluates
  float* grad;          // [M, d] the rows the score is summed up in (touched only by a phase that is asked for the score)
  float* slot;          // the wave's slot of pre-activations
  float* trash;         // the lane's dump slot
};
SD_INLINE const float* tl_img(const TiltedArgs& a, int i) { return a.pack + static_cast<size_t>(i) * TL_SLOT; }

struct TlNoRows {       // the hook of the evaluation and of the moves: nothing
  template <class Row>
  SD_INLINE void act(const TlTile&, int, Row, const f32x4 (&)[TL_HT]) const {}
  template <class Row>
  SD_INLINE void cot(const TlTile&, int, Row, const f32x4 (&)[TL_HT], float) const {}
  template <int NT, class Row>
  SD_INLINE void input(const TlTile&, Row, const f32x4 (&)[NT], float) const {}
};
struct TlTrainRows {    // the hook of the training mode: the per-row arrays of TiltedRows
  const TiltedRows& rw;
  int d;
  template <class Row>
  SD_INLINE void act(const TlTile& w, int l, Row rowf, const f32x4 (&v)[TL_HT]) const {
    tl_store_row(rw.a[l], w.trash, rowf(), w.live, w.g, v);
  }
  template <class Row>
  SD_INLINE void cot(const TlTile& w, int l, Row rowf, const f32x4 (&dh)[TL_HT], float f) const {
    tl_store_row(rw.d[l], w.trash, rowf(), w.live, w.g, dh, f);
  }
  template <int NT, class Row>
  SD_INLINE void input(const TlTile& w, Row rowf, const f32x4 (&xs)[NT], float f) const {
    const uint32_t row = rowf();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      store_quad(rw.xs, w.trash, row, d, w.live, t, w.g, xs[t]);
      store_quad(rw.dv, w.trash, row, d, w.live, t, w.g, xs[t] * f);
    }
  }
};

// xs and 1 / c_i of this lane's features, from x (re-read where needed: cheaper than 64 live registers)
template <int NT, class Row>
SD_INLINE void tl_scaled_input(const TiltedArgs& a, const TlTile& w, Row rowf, float s_t, float sig_t, f32x4 (&xs)[NT], f32x4 (&rci)[NT]) {
  asm volatile("" ::: "memory");  // a real re-read: merged with the earlier ones, the compiler keeps xs and 1 / c_i live (and spills them)
  const uint32_t row = rowf();
  const float* cs = a.consts;
  const int g = w.g;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const f32x4 xv = load_quad(w.x, row, a.d, w.live, t, g);
    const f32x4 mg = load_tile4(cs + TL_C_MEANG, t, g), vg = load_tile4(cs + TL_C_VARG, t, g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ci = s_t * sqrtf(vg[r] + sig_t);
      const bool ok = feat_lt(t, r, 4 * g, a.d);
      rci[t][r] = ok ? 1.0f / ci : 0.0f;
      xs[t][r] = ok ? (xv[r] - s_t * mg[r]) / ci : 0.0f;
    }
  }
}

// prior: the log-density of the mixture noised to t' (online softmax over the components; diagonal or eigen-form covariances) and, with
// `want_grad` (uniform), its score into w.grad
template <int NT, class Row>
SD_INLINE float tl_prior(const TiltedArgs& a, const TlTile& w, Row rowf, float s_l, float sig_l, bool want_grad) {
  constexpr int KBD = (NT + 1) / 2;
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  const float* cs = a.consts;
  const float* inv = cs + TL_C_INV;
  float* lds = w.lds;
  const int tid = w.tid, threads = w.threads, lane = w.lane, g = w.g;
  const bool active = w.active, live = w.live;
  float prior_lp = 0.0f;
  float m_run = -INFINITY, l_run = 0.0f;
  f32x4 pg[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) pg[t] = zero;
  const float s2 = s_l * s_l;
  const float c_norm = 0.9189385332046727f * static_cast<float>(a.d);  // 0.5 d log(2 pi)
  for (int k = 0; k < a.K; ++k) {
    const uint32_t row = rowf();
    const float* mk = cs + TL_C_MEANS + 128 * k;
    const float* vk = cs + TL_C_VARS + 128 * k;
    f32x4 q[NT];
    float maha = 0.0f, logdet = 0.0f;
    if (!a.full) {
      if (active) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 xv = load_quad(w.x, row, a.d, live, t, g);
          const f32x4 m = load_tile4(mk, t, g), vv = load_tile4(vk, t, g);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool ok = feat_lt(t, r, 4 * g, a.d);
            const float var = s2 * (vv[r] + sig_l), z = xv[r] - s_l * m[r];
            q[t][r] = ok ? z / var : 0.0f;
            maha = __builtin_fmaf(ok ? z : 0.0f, q[t][r], maha);
            logdet += ok ? logf(var) : 0.0f;
          }
        }
      }
    } else {
      tl_stage(lds, tl_img(a, TL_EIG + 2 * k), NT * KBD, tid, threads);  // P^T
      if (active) {
        f32x4 z[NT], y[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 xv = load_quad(w.x, row, a.d, live, t, g);
          const f32x4 m = load_tile4(mk, t, g);
#pragma unroll
          for (int r = 0; r < 4; ++r) z[t][r] = feat_lt(t, r, 4 * g, a.d) ? xv[r] - s_l * m[r] : 0.0f;
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
      if (want_grad) {
        tl_stage(lds, tl_img(a, TL_EIG + 2 * k + 1), NT * KBD, tid, threads);  // P
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
    }
    if (active) {
      maha = group_sum(maha);
      logdet = group_sum(logdet);
      const float lp = cs[TL_C_LOGW + k] - (c_norm + 0.5f * (logdet + maha));
      const float m_new = fmaxf(m_run, lp);
      const float so = exp_nonpos(m_run - m_new), pk = exp_nonpos(lp - m_new);
      l_run = l_run * so + pk;
      m_run = m_new;
      if (want_grad) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) pg[t][r] = __builtin_fmaf(pk, -q[t][r], pg[t][r] * so);
      }
    }
  }
  if (active) {
    prior_lp = m_run + logf(l_run);
    if (want_grad) {
      const float il = 1.0f / l_run;
      const uint32_t row = rowf();
#pragma unroll
      for (int t = 0; t < NT; ++t) store_quad(w.grad, w.trash, row, a.d, live, t, g, pg[t] * il);
    }
  }
  return prior_lp;
}

// time embedding at the row's time tt (per row: a tile may span several times): h = (b_in + e) 2^e_in, the accumulator the input layer
// starts from
SD_INLINE void tl_time_embed(const TiltedArgs& a, const TlTile& w, float tt, f32x4 (&h)[TL_HT]) {
  const float* cs = a.consts;
  const float* sc = cs + TL_C_SCALE;
  const float* inv = cs + TL_C_INV;
  float* lds = w.lds;
  const int tid = w.tid, threads = w.threads, lane = w.lane, g = w.g;
  const bool active = w.active;
  f32x4 act[TL_HT];
  tl_stage(lds, tl_img(a, TL_TE1S), TL_HT * TL_KBH, tid, threads);
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
  tl_stage(lds, tl_img(a, TL_TE1C), TL_HT * TL_KBH, tid, threads);
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
  tl_stage(lds, tl_img(a, TL_TE2), TL_HT * TL_KBH, tid, threads);
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
  }
}

// input layer from the accumulator that `acc(h)` fills, four hidden layers, output layer with the tilt 'dot': returns base_lp = -<v, xs>
// and, with `want_grad`, adds the -f v / c_i half of the score to w.grad.  `keep_h`: the pre-activations go to the wave's slot.
template <int NT, class Row, class Acc, class Hook>
SD_INLINE float tl_forward(const TiltedArgs& a, const TlTile& w, Row rowf, float s_t, float sig_t, float f, Acc acc, bool keep_h, bool want_grad,
                           const Hook& hook) {
  constexpr int KBD = (NT + 1) / 2;
  const float* cs = a.consts;
  const float* inv = cs + TL_C_INV;
  float* lds = w.lds;
  const int tid = w.tid, threads = w.threads, lane = w.lane, g = w.g;
  const bool active = w.active;
  f32x4 act[TL_HT], h[TL_HT];
  float base_lp = 0.0f;
  // ---- input layer ----
  tl_stage(lds, tl_img(a, TL_WIN), TL_HT * KBD, tid, threads);
  if (active) {
    f32x4 xs[NT], rci[NT];
    tl_scaled_input<NT>(a, w, rowf, s_t, sig_t, xs, rci);
    acc(h);
    tl_mm<NT, TL_HT>(xs, h, lds, lane);
#pragma unroll
    for (int t = 0; t < TL_HT; ++t) {
      h[t] = h[t] * inv[TL_WIN];
#pragma unroll
      for (int r = 0; r < 4; ++r) act[t][r] = gelu_fast(h[t][r]);
    }
    if (keep_h) tl_store_h(w.slot, 0, lane, h);
    hook.act(w, 0, rowf, act);
  }
  // ---- four hidden layers ----
  for (int l = 0; l < 4; ++l) {
    tl_stage(lds, tl_img(a, TL_WH + l), TL_HT * TL_KBH, tid, threads);
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
      if (keep_h) tl_store_h(w.slot, l + 1, lane, h);
      hook.act(w, l + 1, rowf, act);
    }
  }
  // ---- output layer, tilt 'dot': base_lp = -<v, xs>, and the -v / c_i half of base_grad ----
  tl_stage(lds, tl_img(a, TL_WOUT), NT * TL_KBH, tid, threads);
  if (active) {
    f32x4 xs[NT], rci[NT], v[NT];
    tl_scaled_input<NT>(a, w, rowf, s_t, sig_t, xs, rci);
    hook.template input<NT>(w, rowf, xs, f);
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
    base_lp = -group_sum(dot);
    if (want_grad) tl_grad_axpy<NT>(w.grad, w.trash, rowf(), a.d, w.live, g, -f, v);
  }
  return base_lp;
}

// backward: J^T xs through the transposed images, from the pre-activations in the wave's slot; with `last` (uniform) the input layer's
// product runs and the other half of the score, -f J^T xs / c_i, is added to w.grad
template <int NT, class Row, class Hook>
SD_INLINE void tl_backward(const TiltedArgs& a, const TlTile& w, Row rowf, float s_t, float sig_t, float f, bool last, const Hook& hook) {
  constexpr int KBD = (NT + 1) / 2;
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  const float* inv = a.consts + TL_C_INV;
  float* lds = w.lds;
  const int tid = w.tid, threads = w.threads, lane = w.lane;
  const bool active = w.active;
  f32x4 dh[TL_HT], gacc[TL_HT];
  tl_stage(lds, tl_img(a, TL_WOUT_T), TL_HT * KBD, tid, threads);
  if (active) {
    f32x4 xs[NT], rci[NT];
    tl_scaled_input<NT>(a, w, rowf, s_t, sig_t, xs, rci);
    const float sg = row_normalise<NT>(xs), back = inv[TL_WOUT_T] / sg;
#pragma unroll
    for (int t = 0; t < TL_HT; ++t) gacc[t] = zero;
    tl_mm<NT, TL_HT, true>(xs, gacc, lds, lane, sg);
#pragma unroll
    for (int t = 0; t < TL_HT; ++t) {
      const f32x4 hv = tl_load_h(w.slot, 4, t, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[t][r] = (gacc[t][r] * back) * gelu_grad(hv[r]);
    }
    hook.cot(w, 4, rowf, dh, f);
  }
  for (int l = 3; l >= 0; --l) {
    tl_stage(lds, tl_img(a, TL_WH_T + l), TL_HT * TL_KBH, tid, threads);  // transpose of hidden layer l
    if (active) {
      const float sg = row_normalise<TL_HT>(dh), back = inv[TL_WH_T + l] / sg;
#pragma unroll
      for (int t = 0; t < TL_HT; ++t) gacc[t] = zero;
      tl_mm<TL_HT, TL_HT, true>(dh, gacc, lds, lane, sg);
#pragma unroll
      for (int t = 0; t < TL_HT; ++t) {
        const f32x4 hv = tl_load_h(w.slot, l, t, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) dh[t][r] = (gacc[t][r] * back) * gelu_grad(hv[r]);
      }
      hook.cot(w, l, rowf, dh, f);  // l = 0 included: the input layer's cotangent
    }
  }
  if (last) tl_stage(lds, tl_img(a, TL_WIN_T), NT * TL_KBH, tid, threads);
  if (active && last) {
    f32x4 xs[NT], rci[NT], jx[NT];
    tl_scaled_input<NT>(a, w, rowf, s_t, sig_t, xs, rci);
    const float sg = row_normalise<TL_HT>(dh), back = inv[TL_WIN_T] / sg;
#pragma unroll
    for (int t = 0; t < NT; ++t) jx[t] = zero;
    tl_mm<TL_HT, NT, true>(dh, jx, lds, lane, sg);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) jx[t][r] = (jx[t][r] * back) * rci[t][r];
    tl_grad_axpy<NT>(w.grad, w.trash, rowf(), a.d, w.live, w.g, -f, jx);
  }
}

// TRAIN: the same walk, and the per-row arrays of TiltedRows on the way (the backward pass then runs whether or not a.grad is asked for)
template <int NT, bool TRAIN>
__global__ void __launch_bounds__(512, 2) k_tilted_eval(const TiltedArgs a, const TiltedRows rw) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, threads = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = threads >> 6;
  const int p = lane & 15, g = lane >> 4;
  float* trash = a.trash + tid * 4;
  float* slot = a.hbuf ? a.hbuf + static_cast<size_t>(blockIdx.x * nw + wave) * TL_HBUF_FLOATS : nullptr;
  const bool want_grad = a.grad != nullptr;  // uniform
  const bool want_bwd = TRAIN || want_grad;  // the pre-activations are kept and the backward pass runs
  const int per_round = gridDim.x * nw;
  const int rounds = (a.ntiles + per_round - 1) / per_round;
  const auto hook = [&]() {
    if constexpr (TRAIN) return TlTrainRows{rw, a.d};
    else return TlNoRows{};
  }();

  for (int round = 0; round < rounds; ++round) {
    const int tile = (round * gridDim.x + blockIdx.x) * nw + wave;
    const bool active = tile < a.ntiles;  // wave-uniform; an idle wave still helps staging and meets every barrier
    const uint32_t row = static_cast<uint32_t>(active ? tile : 0) * 16u + p;
    const bool live = active && row < static_cast<uint32_t>(a.M);
    const int kt = live ? static_cast<int>(row / static_cast<uint32_t>(a.B)) : 0;
    const float* ti = a.tinfo + static_cast<size_t>(kt) * TL_TINFO;
    const float tt = ti[0], s_t = ti[1], sig_t = ti[2], s_l = ti[3], sig_l = ti[4];
    const float f = a.use_st ? s_t : 1.0f;
    const TlTile w = {lds, tid, threads, lane, g, active, live, a.x, a.grad, slot, trash};
    const auto rowf = [&]() __attribute__((always_inline)) { return row; };

    const float prior_lp = tl_prior<NT>(a, w, rowf, s_l, sig_l, want_grad);
    f32x4 te[TL_HT];
    tl_time_embed(a, w, tt, te);
    const auto acc = [&](f32x4 (&h)[TL_HT]) __attribute__((always_inline)) {  // the input layer's accumulator: computed in place
#pragma unroll
      for (int t = 0; t < TL_HT; ++t) h[t] = te[t];
    };
    const float base_lp = tl_forward<NT>(a, w, rowf, s_t, sig_t, f, acc, want_bwd, want_grad, hook);
    if (a.log_prob && live && g == 0) a.log_prob[row] = prior_lp + f * base_lp;
    if (want_bwd) tl_backward<NT>(a, w, rowf, s_t, sig_t, f, !TRAIN || want_grad, hook);
  }
}

// the run-time tile count -> the instance: f(std::integral_constant<int, NT>) for NT = 1 .. 8
template <class F>
static int tl_dispatch_nt(int NT, F f) {
  switch (NT) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    case 7: return f(std::integral_constant<int, 7>());
    case 8: return f(std::integral_constant<int, 8>());
  }
  return static_cast<int>(hipErrorInvalidValue);
}
template <bool TRAIN>
static int launch_tilted(const TiltedArgs& a, const TiltedRows& rows, int NT, int grid, int waves, hipStream_t stream) {
  return tl_dispatch_nt(NT, [&](auto nt) {
    return sd_launch_kernel(k_tilted_eval<decltype(nt)::value, TRAIN>, grid, waves * 64, static_cast<size_t>(TL_SLOT) * sizeof(float), stream, a, rows);
  });
}
#endif
