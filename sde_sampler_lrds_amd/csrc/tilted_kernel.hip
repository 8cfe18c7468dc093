// Tilted-potential (EBM) reference evaluation: the weight packer and the eight evaluation instances of k_tilted_eval
// (tilted_kernel.hpp); the eight training instances are in tilted_train_inst.hip, a unit of their own so that the two halves build in parallel.
#include "tilted_kernel.hpp"

// One block per job: the matrix's power-of-two scale (the rule of k_weight_scales, prep_kernels.hip: a largest entry outside
// [2^-10, 2^14) is normalised to [1, 2)), its split-f16 image in the (to, kb, part, lane, 8 halves) order of k_pack_mlp -- of the matrix
// or, with `transpose`, of its transpose -- and its bias times the scale.  The last block fills the constants of the mixture.
__global__ void __launch_bounds__(256) k_tilted_pack(const TiltedPackArgs a) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  if (blockIdx.x == a.njobs) {
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
    return;
  }
  const TiltedPackJob& j = a.job[blockIdx.x];
  float m = 0.0f;
  for (int i = tid; i < j.scale_n; i += 256) {
    const float v = __builtin_fabsf(j.scale_src[i]);
    m = (v <= 3.0e38f) ? fmaxf(m, v) : m;
  }
  red[tid] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  const float mx = red[0];
  int e = 0;
  if (mx > 0.0f && (mx < 9.765625e-4f || mx >= 16384.0f)) {
    int ex;
    frexpf(mx, &ex);
    e = 1 - ex;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
  }
  const float scale = ldexpf(1.0f, e);
  if (tid == 0) {
    a.consts[TL_C_SCALE + j.slot] = scale;
    a.consts[TL_C_INV + j.slot] = ldexpf(1.0f, -e);
  }
  const int TO = (j.n_out + 15) / 16, KB = (j.n_in + 31) / 32;
  _Float16* img = reinterpret_cast<_Float16*>(a.pack + static_cast<size_t>(j.slot) * TL_SLOT);
  for (int idx = tid; idx < TO * KB * 1024; idx += 256) {
    const int jj = idx & 7, lane = (idx >> 3) & 63, part = (idx >> 9) & 1, blk = idx >> 10;
    const int kb = blk % KB, to = blk / KB;
    const int o = 16 * to + (lane & 15);
    const int i = 16 * (2 * kb + (jj >> 2)) + 4 * (lane >> 4) + (jj & 3);
    float w = 0.0f;
    if (o < j.n_out && i < j.n_in)
      w = (j.transpose ? j.src[static_cast<size_t>(i) * j.ld + j.col0 + o] : j.src[static_cast<size_t>(o) * j.ld + j.col0 + i]) * scale;
    const _Float16 hi = static_cast<_Float16>(w);
    img[idx] = part == 0 ? hi : static_cast<_Float16>((w - static_cast<float>(hi)) * 2048.0f);
  }
  if (j.bias_off >= 0)
    for (int i = tid; i < 128; i += 256) a.consts[j.bias_off + i] = i < j.n_out ? j.bias[i] * scale : 0.0f;
}

int sd_launch_tilted_pack(const TiltedPackArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_tilted_pack, dim3(a.njobs + 1), dim3(256), 0, s, a);
  return static_cast<int>(hipGetLastError());
}

int sd_launch_tilted(const TiltedArgs& a, int NT, int grid, int waves, hipStream_t s) {
  const TiltedRows none = {};
  return launch_tilted<false>(a, none, NT, grid, waves, s);
}
