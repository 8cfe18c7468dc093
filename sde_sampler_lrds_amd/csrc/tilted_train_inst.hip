// The eight training instances of k_tilted_eval (tilted_kernel.hpp, TRAIN = true): sdeng_tilted_vjp.
#include "tilted_kernel.hpp"

int sd_launch_tilted_train(const TiltedArgs& a, const TiltedRows& rows, int NT, int grid, int waves, hipStream_t s) {
  return launch_tilted<true>(a, rows, NT, grid, waves, s);
}
