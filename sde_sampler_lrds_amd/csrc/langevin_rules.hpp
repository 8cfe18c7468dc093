// The scalar rules of a Metropolis-adjusted move -- mala_step / heuristics_step_size of additions/mcmc.py -- written once for the kernels that
// run all moves of a level in one launch: k_chain_moves (prep_kernels.hip, a thread per chain) and k_tilted_moves (tilted_moves_inst.hip, a
// quad of lanes per row).  The per-feature sums qf / qb and the Philox streams of the noise are the kernels' own: their layouts differ.
#pragma once
#include "sim_device.hpp"

// log acceptance ratio of a Langevin proposal from qf = sum (prop - (y + h grad(y)))^2 and qb = sum (y - (prop + h grad(prop)))^2:
// log q, unnormalised, is -0.5 sum (samples - mean)^2 / variance with variance 2 h  (mcmc.py:24-31, :100-108)
SD_INLINE float mala_log_acc(float lp_p, float lp, float qf, float qb, float step) {
  const float var = 2.0f * step;
  const float joint_prop = lp_p - (-0.5f * qf) / var, joint_orig = lp - (-0.5f * qb) / var;
  return joint_prop - joint_orig;
}
// the accept test on a uniform.  A NaN log_acc (a NaN log-density at the proposal) compares false: rejected, the chain keeps its state
SD_INLINE bool mh_accept(float uu, float log_acc) { return logf(uu) < log_acc; }
// heuristics_step_size (mcmc.py:55-74), per chain; log_target = log(target acceptance)
SD_INLINE float mh_adapt_step(float step, float log_acc, float log_target) {
  if (log_acc - log_target > 0.04879016416943205f) step = step * 1.01f;        // log1p(0.05)
  if (log_target - log_acc > 0.05129329438755058f) step = step / 1.01f;        // -log1p(-0.05)
  return step;
}
// the acceptance probability of the move, as the averages of the samplers report it
SD_INLINE float mh_acc_prob(float log_acc) { return expf(fminf(0.0f, log_acc)); }
