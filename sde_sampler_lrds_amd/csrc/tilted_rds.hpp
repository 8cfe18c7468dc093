// The RDS step loop over an energy-based (tilted-potential) reference in ONE launch (k_tilted_rds, tilted_rds_inst.hip): the run next to the
// TiltedArgs of the reference's net.  TiltedArgs carries M = B particles, N = the steps and tinfo [N][TL_TINFO] at the step times; its x,
// log_prob and grad stay null -- the state and the score at it are rows of the arrays below.
#pragma once
#include "tilted_kernel.hpp"

struct TiltedRdsArgs {
  int form;               // SDENG_FORM_LIN / SDENG_FORM_EM
  unsigned flags;         // SDENG_FLAG_ITO
  int N;
  const float* coef;      // [N][SDENG_NCOEF]
  const float* wpack;     // packed drift-net image (sim_common.hpp), biases and layer scales behind it
  const float* temb;      // [N][64] time embedding of the drift net, per step
  const float* te_tab;    // [N][128] the EBM's time embedding per step: (b_in + e) 2^e_in, the accumulator its input layer starts from
  float clip_model;
  uint32_t seed_lo, seed_hi;
  long long particle0;
  const float* x_in;      // [B, d]
  const float* noise_in;  // [N, B, d] or nullptr: Philox stream 0
  float* x_out;           // [B, d]
  float* rnd_out;         // [B]
  float* xs_out;          // [N + 1, B, d] or nullptr
  float* ref_out;         // [N, B, d] or nullptr: the reference score at (t_k, x_k) of every step
  float* ping;            // [2][B, d] workspace: the state rows of a run without a trajectory
  float* score;           // [B, d] workspace: the reference score of the step (without ref_out)
};
// te_tab of all N steps: one wave per 16 step times through tl_time_embed (the EBM's time embedding depends on the step alone)
int sd_launch_tilted_rds_times(const TiltedArgs& a, float* te_tab, hipStream_t s);
int sd_launch_tilted_rds(const TiltedArgs& a, const TiltedRdsArgs& r, int NT, int grid, int waves, hipStream_t s);
