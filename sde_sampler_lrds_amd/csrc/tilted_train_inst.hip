// The eight training instances of k_tilted_eval (tilted_kernel.hpp, TRAIN = true): sdeng_tilted_vjp.
#include "tilted_kernel.hpp"

int sd_launch_tilted_train(const TiltedArgs& a, const TiltedRows& rows, int NT, int grid, int waves, hipStream_t s) {
  switch (NT) {
    case 1: return launch_tilted<1, true>(a, rows, grid, waves, s);
    case 2: return launch_tilted<2, true>(a, rows, grid, waves, s);
    case 3: return launch_tilted<3, true>(a, rows, grid, waves, s);
    case 4: return launch_tilted<4, true>(a, rows, grid, waves, s);
    case 5: return launch_tilted<5, true>(a, rows, grid, waves, s);
    case 6: return launch_tilted<6, true>(a, rows, grid, waves, s);
    case 7: return launch_tilted<7, true>(a, rows, grid, waves, s);
    case 8: return launch_tilted<8, true>(a, rows, grid, waves, s);
  }
  return static_cast<int>(hipErrorInvalidValue);
}
