#include "cmcd_kernel.hpp"
#include "prep_kernels.hpp"
// (the k_simulate_cmcd instantiations live in gen/cmcd_<tiles>.hip, one translation unit per tile count)

// augmented design matrix Xa = [X | 1] (n rows, dw + 1 columns) -> logits image [row tiles][KB(NT)] and grad image
// [NT][row K-blocks] (cmcd_kernel.hpp), zero outside the data; labels padded with zeros
__global__ void k_logreg_images(const float* X, const float* y, int n, int dw, int NT, float* image, float* y_pad) {
  const int KB = sd_kb(NT), RKB = sd_lr_row_kb(n);
  const int n_logit = sd_lr_logit_floats(NT, n) * 2, n_grad = sd_lr_grad_floats(NT, n) * 2;
  _Float16* img = reinterpret_cast<_Float16*>(image);
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n_logit + n_grad; idx += gridDim.x * blockDim.x) {
    const bool logit = idx < n_logit;
    const SdImageCoord c = logit ? sd_image_coord(idx, KB) : sd_image_coord(idx - n_logit, RKB);
    const int row = logit ? c.o : c.i, col = logit ? c.i : c.o;
    float v = 0.0f;
    if (row < n) v = (col < dw) ? X[static_cast<size_t>(row) * dw + col] : (col == dw ? 1.0f : 0.0f);
    img[idx] = sd_split_part(v, c.part);
    if (idx < 32 * RKB) y_pad[idx] = (idx < n) ? y[idx] : 0.0f;
  }
}
int sd_launch_logreg_images(const float* X, const float* y, int n, int dw, int NT, float* image, float* y_pad, hipStream_t s) {
  hipLaunchKernelGGL(k_logreg_images, dim3(96), dim3(256), 0, s, X, y, n, dw, NT, image, y_pad);
  return static_cast<int>(hipGetLastError());
}
