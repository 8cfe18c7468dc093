// The split-f16 A-operand image: the one format every matrix product of this library reads its left operand from (drift-net and
// tilted-net weights, precision matrices, design matrices, mixture means).  Host and device.
//
// The GEMMs run on the f16 matrix pipe as a two-piece split (sim_device.hpp, dense_f16x2): every value v is stored as
//   hi = f16(v)   and   lo = f16((v - hi) * 2^11)          (v - hi is exact in fp32; v ~ hi + lo * 2^-11 carries 22+ bits)
// A matrix [n_out x n_in] is cut into blocks, one per (16-output tile `to`, 32-input K-block `kb`), stored in the order
//   (to, kb, part, lane, 8 halves):  part 0 = hi, part 1 = lo;  64 lanes x 8 halves x 2 bytes = 1 KiB per part, 2 KiB = 512 floats per block.
// Half j of lane l in block (to, kb) is the element
//   (o, i) = (16 to + (l & 15), 16 (2 kb + j/4) + 4 (l >> 4) + j%4)
// -- K-block kb covers input tiles 2kb and 2kb + 1 in the register order of the wave tile (sim_common.hpp) -- and 0 outside the matrix.
//
// Power-of-two prescale: the split carries fp32's bits only while |v| sits in f16's NORMAL range, so a matrix whose largest finite entry
// is below 2^-10 (the reference initialises the last layer at ~1e-7, models/utils.py:7-22: f16-subnormal) or at / above 2^14 is stored as
// W * 2^e with max |W| 2^e in [1, 2), its bias as b * 2^e, and the product is multiplied by 2^-e (exact).  Matrices in range keep e = 0.
#pragma once
#include <hip/hip_runtime.h>

#define SD_LO_SCALE 2048.0f          // 2^11 of the lo part
#define SD_LO_INV 4.8828125e-04f
constexpr int SD_BLOCK_FLOATS = 512;       // one block, hi and lo parts
constexpr int SD_BLOCK_HALVES = 2 * SD_BLOCK_FLOATS;
constexpr int SD_PART_BYTES = 2 * SD_BLOCK_FLOATS;  // one part (hi or lo) of a block

__host__ __device__ constexpr int sd_kb(int tiles) { return (tiles + 1) / 2; }  // 32-input K-blocks covering `tiles` tiles of 16
// image of a matrix with out_tiles tiles of outputs and in_tiles tiles of inputs (sd_image_floats(1, in_tiles): one output tile's blocks)
__host__ __device__ constexpr int sd_image_blocks(int out_tiles, int in_tiles) { return out_tiles * sd_kb(in_tiles); }
__host__ __device__ constexpr int sd_image_floats(int out_tiles, int in_tiles) { return out_tiles * sd_kb(in_tiles) * SD_BLOCK_FLOATS; }
__host__ __device__ constexpr int sd_image_bytes(int out_tiles, int in_tiles) { return sd_image_floats(out_tiles, in_tiles) * 4; }
// the same for an image whose input side is counted in K-blocks
__host__ __device__ constexpr int sd_blocks_floats(int out_tiles, int k_blocks) { return out_tiles * k_blocks * SD_BLOCK_FLOATS; }

// Full-covariance mixture reference: a component's precision image [NT x NT] is staged in sd_full_pieces(NT) pieces of whole output tiles.
__host__ __device__ constexpr int sd_full_pieces(int NT) { return NT > 4 ? 2 : 1; }
__host__ __device__ constexpr int sd_full_piece_floats(int NT) { return sd_image_floats(NT / sd_full_pieces(NT), NT); }
// Shared-variance mixture on the matrix pipe, kt = ceil(K / 16) component tiles: per step the logit image [kt x NT], then the mean image [NT x kt].
__host__ __device__ constexpr int sd_mm_logit_floats(int kt, int NT) { return sd_image_floats(kt, NT); }
__host__ __device__ constexpr int sd_mm_mean_floats(int kt, int NT) { return sd_image_floats(NT, kt); }

// half index inside an image with KB K-blocks per output tile -> part and element
struct SdImageCoord {
  int part, o, i;
};
__host__ __device__ inline SdImageCoord sd_image_coord(int half, int KB) {
  const int j = half & 7, lane = (half >> 3) & 63, blk = half >> 10;
  const int kb = blk % KB, to = blk / KB;
  return {(half >> 9) & 1, 16 * to + (lane & 15), 16 * (2 * kb + (j >> 2)) + 4 * (lane >> 4) + (j & 3)};
}
// one part of the split of v
__host__ __device__ inline _Float16 sd_split_part(float v, int part) {
  const _Float16 hi = static_cast<_Float16>(v);
  return part == 0 ? hi : static_cast<_Float16>((v - static_cast<float>(hi)) * SD_LO_SCALE);
}
// |v| as it counts towards a matrix's largest entry: non-finite entries do not decide the scale (they poison the result either way)
__host__ __device__ inline float sd_scale_maxabs(float m, float v) {
  const float av = __builtin_fabsf(v);
  return (av <= 3.0e38f) ? fmaxf(m, av) : m;
}
// the scale rule: largest finite |entry| -> e.  Outside [2^-10, 2^14) the largest entry is normalised to [1, 2), |e| <= 100.
__host__ __device__ inline int sd_scale_exponent(float mx) {
  int e = 0;
  if (mx > 0.0f && (mx < 9.765625e-4f || mx >= 16384.0f)) {
    int ex;
    frexpf(mx, &ex);  // mx = f * 2^ex, f in [0.5, 1)
    e = 1 - ex;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
  }
  return e;
}
