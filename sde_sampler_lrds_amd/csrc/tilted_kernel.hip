// Tilted-potential (EBM) reference evaluation: the constants kernel and the eight evaluation instances of k_tilted_eval
// (tilted_kernel.hpp); the eight training instances are in tilted_train_inst.hip, a unit of their own so that the two halves build in parallel.
#include "tilted_kernel.hpp"

// The constants of the mixture and of the time embedding behind the image slots (TL_C_*); the images themselves, their scales and the
// biases are jobs of k_pack_images (prep_kernels.hip).
__global__ void __launch_bounds__(256) k_tilted_consts(const TiltedConstArgs a) {
  const int tid = threadIdx.x;
  float* cs = a.consts;
  for (int i = tid; i < 128; i += 256) {
    cs[TL_C_COEFF + i] = a.coeff[i];
    cs[TL_C_PHASE + i] = a.phase[i];
    cs[TL_C_MEANG + i] = i < a.d ? a.mean_gauss[i] : 0.0f;
    cs[TL_C_VARG + i] = i < a.d ? a.var_gauss[i] : 0.0f;
  }
  for (int i = tid; i < TL_KMAX * 128; i += 256) {
    const int k = i >> 7, f = i & 127;
    const bool ok = k < a.K && f < a.d;
    cs[TL_C_MEANS + i] = ok ? a.means[k * a.d + f] : 0.0f;
    cs[TL_C_VARS + i] = ok ? a.vars[k * a.d + f] : 1.0f;
  }
  if (tid == 0) {  // weights_t /= weights_t.sum(), then log (models/reparam.py:384, :397)
    float sum = 0.0f;
    for (int k = 0; k < a.K; ++k) sum += a.weights[k];
    for (int k = 0; k < TL_KMAX; ++k) cs[TL_C_LOGW + k] = k < a.K ? logf(a.weights[k] / sum) : -INFINITY;
  }
}

int sd_launch_tilted_consts(const TiltedConstArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_tilted_consts, dim3(1), dim3(256), 0, s, a);
  return static_cast<int>(hipGetLastError());
}

int sd_launch_tilted(const TiltedArgs& a, int NT, int grid, int waves, hipStream_t s) {
  const TiltedRows none = {};
  return launch_tilted<false>(a, none, NT, grid, waves, s);
}
