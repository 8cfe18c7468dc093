// Shared device/host definitions of the MI355X (gfx950) simulate engine.
//
// Wave-tile layout used by every kernel in this directory
// --------------------------------------------------------
// One wavefront (64 lanes) owns a tile of 16 particles.  Lane l holds particle p = l & 15 and the feature
// group g = l >> 4.  A [16 particles x 16 features] block of state lives in ONE f32x4 register group per lane:
// register r of lane (p,g) is feature
//
//        feat(t, r, g) = 16 t + 4 g + r                 t = feature tile, r = 0..3
//
// which is exactly the C/D layout of the 16x16 MFMAs (v_mfma_f32_16x16x32_f16 here) when the product is computed as Y^T = W * X^T
// (rows = output features, columns = particles).  Because an MFMA's summation index may be permuted as long
// as both operands agree, that same register group is directly the B operand of the next layer (k-step r of
// tile t <-> feature feat(t,r,g)), so the whole [d -> 64 -> 64 -> 64 -> d] drift net runs out of registers with
// no cross-lane traffic; the A operands (weights) are pre-permuted once into an LDS image by k_pack_images.
//
// Why 16-particle tiles (an earlier build used 32x32x2 MFMA, 32 particles per wave): the state of a tile is
// half as many registers per lane (d=128: 32 instead of 64), so the whole step loop at d=128 fits the 256-VGPR
// budget of 2 waves per SIMD with NO scratch traffic (208 VGPRs, 0 spills).  Measured on MI355X, cfg 2:
// 4 waves/SIMD (128 VGPRs, spills) 10.2 ms, 2 waves/SIMD 7.6 ms, 1 wave/SIMD 9.6 ms.  On gfx950 MFMA and
// VALU issue of the waves of one SIMD do not overlap (tools/ubench/pipe_share.hip), so extra occupancy buys
// nothing once memory latency is covered; instruction count is what matters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "image_format.hpp"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SD_H 64            // hidden channels (models/mlp.py: channels=64)
#define SD_HT 4            // hidden channel tiles (64 / 16)
#ifndef SD_WAVES
#define SD_WAVES 8         // waves per workgroup (2 per SIMD, 256-VGPR budget)
#endif
#define SD_THREADS (SD_WAVES * 64)
#define SD_WAVES_MAX 12    // step-loop instantiations that fit the 168-register budget run 3 waves per SIMD (sim_kernel.hpp sd_waves_of)

// Packed drift-net image (the format: image_format.hpp), one image per layer and the vectors behind them:
//   W_in [4 x NT tiles], W_h1 [4 x 4], W_h2 [4 x 4], W_out [NT x 4]; then b_in, b_h1, b_h2 (64 each), b_out (16*NT); then the
//   power-of-two prescales of the four matrices: scale[4] = 2^e per layer (in, h1, h2, out), then inv[4] = 2^-e.
__host__ __device__ constexpr int sd_off_win(int NT) { return 0; }
__host__ __device__ constexpr int sd_off_wh1(int NT) { return sd_image_floats(SD_HT, NT); }
__host__ __device__ constexpr int sd_off_wh2(int NT) { return sd_off_wh1(NT) + sd_image_floats(SD_HT, SD_HT); }
__host__ __device__ constexpr int sd_off_wout(int NT) { return sd_off_wh2(NT) + sd_image_floats(SD_HT, SD_HT); }
__host__ __device__ constexpr int sd_lds_weight_floats(int NT) { return sd_off_wout(NT) + sd_image_floats(NT, SD_HT); }
__host__ __device__ constexpr int sd_off_bias(int NT) { return sd_lds_weight_floats(NT); }
#define SD_N_SCALES 8
__host__ __device__ constexpr int sd_off_scales(int NT) { return sd_off_bias(NT) + 3 * 64 + 16 * NT; }
__host__ __device__ constexpr int sd_pack_floats(int NT) { return sd_off_scales(NT) + SD_N_SCALES; }
// per-wave LDS copy of one step's reference table [K][2][dpad]; used while K*2*dpad <= SD_REFTAB_FLOATS
#define SD_REFTAB_FLOATS 1024
// workgroup-shared copy of a larger mixture's table (RF_GMM_BIG): `share` chunks of 1 KiB per wave, two buffers
#define SD_SHARE_MAX 4
__host__ __device__ inline int sd_share_buf_floats(int share) { return share * SD_WAVES * 256; }
__host__ __device__ inline int sd_lds_total_bytes(int NT, bool with_ref, int waves = SD_WAVES) {
  return (sd_lds_weight_floats(NT) + (with_ref ? waves * SD_REFTAB_FLOATS : 0)) * 4;
}

// device-side view of a distribution (tables prepared by k_dist_tables)
struct DistDev {
  int kind;
  int k;
  const float* tab;     // GMM/GAUSS_DIAG: [k][2][dpad]  (mean, 1/var); GAUSS_FULL: precision [d,d]
  const float* consts;  // GMM/GAUSS_DIAG: [k][4]
  const float* aux0;    // LOGREG: X; GAUSS_FULL: loc
  const float* aux1;    // LOGREG: y; GAUSS_FULL: L^-1
  float p0, p1, p2, p3;
  float clip;
};

// logistic-regression target, in-kernel form (images built by k_logreg_images; see sim_device.hpp)
struct LogregDev {
  const float* image;       // global copy of the two LDS images: logits image, then grad image
  const float* y_pad;       // [32 * row K-blocks] labels (0 on pad rows)
  float inv_w_scale2, c_mean, inv_c_scale2;   // 1/weight_scale^2, intercept_mean, 1/intercept_scale^2
  float p_lo, p_hi;         // sigmoid range with non-zero gradient (clip threshold and eps clamp)
  int n_rows;               // data rows n (0: no logistic-regression target)
  int in_lds;               // 1: the two images fit behind the drift-net weights in LDS; 0: the kernel reads them through L2
};

// initial particles drawn by the engine (k_sample_x0; sdeng_desc.x_in == NULL): x0 = loc + scale * z, z = Philox stream 1 at step 0
struct X0Dev {
  int kind;            // ISO_GAUSS / GAUSS_DIAG
  const float* loc;    // GAUSS_DIAG [d]
  const float* scale;  // GAUSS_DIAG [d], or nullptr: x0 = loc (Delta)
  float p0, p1;        // ISO_GAUSS: loc, scale
};

struct SimArgs {
  int form;
  unsigned flags;
  int B, d, N;
  long long particle0;
  unsigned seed_lo, seed_hi;
  const float* coef;      // [N][16]
  const float* x_in;
  float* x_out;
  float* rnd_out;
  float* xs_out;
  const float* noise_in;
  const float* wpack;     // packed drift-net image (global copy)
  const float* temb;      // [N][64] time embedding of the drift net, per step
  const float* stheta;    // [N] clipped score_model(t) or nullptr
  int ctrl_kind;
  float clip_model, clip_score, scale_score;
  int ref_k;
  int ref_share;            // RF_GMM_BIG: > 0 = 1 KiB chunks per wave of the workgroup-shared, double-buffered table copy
  int ref_kc;               //   components per staged piece of the table (>= ref_k: the whole table in one piece)
  const float* ref_tab;     // [N][K][2][dpad]
  const float* ref_consts;  // [N][K][2]  (0.5*sum log var, log w)
  const float* ref_mean;      // RF_GMM_FULL: [N][K][dpad] noised means (ref_tab then holds the precision images [N][K][sd_image_floats(NT, NT)])
  const float* ref_same_var;  // [1] 1.0: all components share one variance vector (written by k_ref_tables)
  float ref_c1;             // 0.5*d*log(2*pi)
  DistDev target;         // in-loop target score (ScoreCtrl / LerpCtrl / CMCD)
  DistDev prior;          // LerpCtrl / CMCD prior score
  const float* rnd_init;  // [B] initial log-weight (log p_prior(x0)) or nullptr
  float* trash;           // [SD_THREADS*4] dump slots for masked stores
  float cmcd_g, cmcd_clip;
  int ntiles;             // ceil(B / 16)
  LogregDev lr;           // in-loop logistic-regression score (ScoreCtrl on a LOGREG target, CMCD)
};

// ---- host side: launching one kernel instance -----------------------------------------------------------------------------------
// One persistent workgroup per CU (LDS image + 2 waves/SIMD fill a CU); tiles are dealt to workgroups first, to the waves of a
// workgroup second, so a small batch spreads over the whole chip.
inline int sd_grid(int ntiles) { return ntiles > 256 ? 256 : (ntiles < 1 ? 1 : ntiles); }

// Raise the kernel's dynamic-LDS limit to what this launch asks for, launch, and report the launch error.
template <class... Formals, class... Actuals>
inline int sd_launch_kernel(void (*kernel)(Formals...), int grid, int block, size_t lds_bytes, hipStream_t stream, const Actuals&... args) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes));
  if (e != hipSuccess) return static_cast<int>(e);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_bytes, stream, args...);
  return static_cast<int>(hipGetLastError());
}

// Registry of the step-loop kernel instances (gen/registry.hip, generated by build.py from its INSTANCES list).  A key is the family,
// the feature tiles NT and the family's own template parameters after NT, in order:
//   SIM (REF, SC, FORM, PAR)   CTRL (SC)   SPLIT (REF, FORM, PERT)   EULER (SC)   CMCD (TGT, EUBO, PAR)   VJP (GX)   ADJ (SCORE)   CADJ (TGT)
// A launcher takes the family's argument block (SimArgs, CmcdArgs, VjpArgs, AdjArgs or CmcdAdjArgs) and launches exactly that instance.
enum { SD_FAM_SIM = 0, SD_FAM_CTRL, SD_FAM_SPLIT, SD_FAM_EULER, SD_FAM_CMCD, SD_FAM_VJP, SD_FAM_ADJ, SD_FAM_CADJ };
constexpr uint32_t sd_key(int fam, int nt, int p0 = 0, int p1 = 0, int p2 = 0, int p3 = 0) {  // every field < 16
  return static_cast<uint32_t>(fam) << 24 | static_cast<uint32_t>(nt) << 16 | p0 << 12 | p1 << 8 | p2 << 4 | p3;
}
typedef int (*sd_launcher)(const void* args, hipStream_t stream);
struct SdKernelEntry {
  uint32_t key;
  sd_launcher fn;
};
extern const SdKernelEntry sd_registry[];  // sorted by key
extern const int sd_registry_size;
