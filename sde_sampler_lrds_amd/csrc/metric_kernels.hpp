// Argument blocks, workspace layouts and host drivers of the sample-metric kernels in metric_kernels.hip
// (sdeng_sinkhorn, sdeng_mmd_median of include/sdeng.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/sdeng.h"

#define SD_MET_TILE 64        // a pair tile is 64 x 64 distances, 4 x 4 per thread of a 256-thread block
#define SD_MET_KC 32          // features staged through LDS per step of a tile
#define SD_MET_GROUPS 16      // k_mmd_*: blocks per tile row (each walks every 16th tile column)
#define SD_MET_COL_CHUNKS 64  // k_sk_cols: at most this many row chunks per column (the partials stay linear in m)
#define SD_MET_RADIX_BINS 2048

static inline size_t sd_met_align(size_t bytes) { return (bytes + 255) & ~static_cast<size_t>(255); }

// ---- Sinkhorn ----------------------------------------------------------------------------------------------------------------------
struct SkLayout {  // byte offsets into the workspace
  size_t u, v, loga, logb, du, dv, rowsum, part, part_idx, errs, small_bytes, M, total_bytes;
  int chunks, rows_per_chunk;
};
static inline SkLayout sd_sk_layout(int n, int m) {
  SkLayout L;
  L.chunks = (n + 127) / 128 < SD_MET_COL_CHUNKS ? (n + 127) / 128 : SD_MET_COL_CHUNKS;
  L.rows_per_chunk = (n + L.chunks - 1) / L.chunks;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += sd_met_align(bytes); return at; };
  L.u = take(sizeof(double) * n);
  L.v = take(sizeof(double) * m);
  L.loga = take(sizeof(double) * n);
  L.logb = take(sizeof(double) * m);
  L.du = take(sizeof(double) * n);
  L.dv = take(sizeof(double) * m);
  L.rowsum = take(sizeof(double) * n);
  L.part = take(sizeof(double) * 2 * L.chunks * static_cast<size_t>(m));
  L.part_idx = take(sizeof(int) * L.chunks * static_cast<size_t>(m));
  L.errs = take(sizeof(double) * 4);
  L.small_bytes = o;
  L.M = o;
  L.total_bytes = o + sd_met_align(sizeof(float) * static_cast<size_t>(n) * m);
  return L;
}

struct SkArgs {
  const float *x, *y;       // [n][d], [m][d]
  const float *w_x, *w_y;   // [n], [m] or both NULL (uniform)
  const float* M;           // [n][m] cost matrix, or NULL: every pass recomputes the costs from x and y
  int n, m, d, p;
  double eps, inv_eps;
  double *u, *v, *loga, *logb, *du, *dv, *rowsum, *part, *errs;
  int* part_idx;
  int chunks, rows_per_chunk;
  float *u_out, *v_out;     // [n], [m] or NULL
  int *corr_xy, *corr_yx;   // [n], [m] or NULL
};
// Runs the whole iteration (one 16-byte read-back per iteration for the stop test); fills `res`.  Returns a hipError_t as int.
int sd_run_sinkhorn(SkArgs a, float* M_store, int max_iters, double stop_thresh, sdeng_sinkhorn_result* res, hipStream_t s);

// ---- MMD with the median bandwidth ---------------------------------------------------------------------------------------------------
struct MmdLayout {
  size_t hist, state, part, total_bytes;
  int tiles, groups;
};
static inline MmdLayout sd_mmd_layout(int n) {
  MmdLayout L;
  L.tiles = (2 * n + SD_MET_TILE - 1) / SD_MET_TILE;
  L.groups = L.tiles < SD_MET_GROUPS ? L.tiles : SD_MET_GROUPS;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += sd_met_align(bytes); return at; };
  L.hist = take(sizeof(unsigned long long) * 3 * SD_MET_RADIX_BINS);
  L.state = take(sizeof(unsigned long long) * 4);
  L.part = take(sizeof(double) * 3 * static_cast<size_t>(L.tiles) * L.groups);
  L.total_bytes = o;
  return L;
}
struct MmdArgs {
  const float *X, *Y;  // [n][d] each
  int n, d, tiles, groups;
  unsigned long long* hist;   // [3][SD_MET_RADIX_BINS]
  unsigned long long* state;  // [0] key prefix found so far, [1] rank left inside it
  double* part;               // [tiles * groups][3]: kernel sums over XX (i < j), YY (i < j), XY
  float* out;                 // [2]: mmd, bandwidth_sq
};
int sd_run_mmd_median(MmdArgs a, hipStream_t s);
