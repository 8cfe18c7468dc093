// Sample-quality metrics on point clouds (gfx950): the two quadratic ones of the reference's evaluation layer.
//   k_pair_cost        cost matrix M_ij = (sum_k |x_ik - y_jk|^p)^(1/p), p in {1, 2}              (eval/sinkhorn.py:113-119)
//   k_sk_rows / _cols  one Sinkhorn half-iteration each: online log-sum-exp along a row / a column  (eval/sinkhorn.py:148-160)
//   k_sk_* <FINAL>     transport cost sum_ij P_ij M_ij and the two argmax correspondences           (eval/sinkhorn.py:162-171)
//   k_mmd_hist         radix histograms of the squared distances of the pooled sample (exact median) (additions/mmd.py:41-45)
//   k_mmd_sums         the three Gaussian-kernel sums                                                (additions/mmd.py:47-56)
// Distances are sums over k of differences (x_ik - y_jk) in double, rounded once to fp32: with eps = 1e-3 an absolute error in
// M_ij enters the exponent a thousand times larger, so the |x|^2 + |y|^2 - 2 x.y expansion is not used.  The scaling vectors u, v
// and the log-sum-exp arguments stay in double (their differences are what the exponent sees); exponentials of the online
// log-sum-exp are fp32.  Every reduction has a fixed order and the only atomics are integer counters: reruns are bit-identical.
#include "metric_kernels.hpp"

#include <cmath>

namespace {

constexpr int T = SD_MET_TILE, KC = SD_MET_KC, NTHR = 256;

// rows of one or two row-major arrays seen as one: row r is p0[r] for r < n0, p1[r - n0] otherwise
struct Rows {
  const float *p0, *p1;
  int n0, n;
};
__device__ inline const float* row_ptr(const Rows& R, int r, int d) {
  return r < R.n0 ? R.p0 + static_cast<size_t>(r) * d : R.p1 + static_cast<size_t>(r - R.n0) * d;
}

// acc[a][b] = sum_k |A[i0 + 4 ty + a][k] - B[j0 + tx + 16 b][k]|^P  (tx = tid & 15, ty = tid >> 4), k ascending.
// Rows beyond A.n / B.n read as zero; the caller masks them.
template <int P>
__device__ inline void pair_tile(const Rows& A, int i0, const Rows& B, int j0, int d, float (*sA)[T + 1], float (*sB)[T + 1],
                                 double (&acc)[4][4]) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (int k0 = 0; k0 < d; k0 += KC) {
    __syncthreads();  // the previous chunk has been read
    const int k = tid & (KC - 1), kk = k0 + k;
#pragma unroll
    for (int q = 0; q < T * KC / NTHR; ++q) {
      const int r = (tid / KC) + (NTHR / KC) * q;
      sA[k][r] = (i0 + r < A.n && kk < d) ? row_ptr(A, i0 + r, d)[kk] : 0.0f;
      sB[k][r] = (j0 + r < B.n && kk < d) ? row_ptr(B, j0 + r, d)[kk] : 0.0f;
    }
    __syncthreads();
    const int kn = d - k0 < KC ? d - k0 : KC;
    for (int k2 = 0; k2 < kn; ++k2) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = sA[k2][4 * ty + a];
#pragma unroll
      for (int b = 0; b < 4; ++b) bv[b] = sB[k2][tx + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double df = av[a] - bv[b];
          acc[a][b] += P == 2 ? df * df : fabs(df);
        }
    }
  }
}

__device__ inline float cost_of(double acc, int p) { return p == 2 ? static_cast<float>(sqrt(acc)) : static_cast<float>(acc); }

// ---- Sinkhorn ----------------------------------------------------------------------------------------------------------------------
template <int P>
__global__ void __launch_bounds__(NTHR) k_pair_cost(SkArgs a, float* M) {
  __shared__ float sA[KC][T + 1], sB[KC][T + 1];
  const int i0 = blockIdx.y * T, j0 = blockIdx.x * T, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4];
  pair_tile<P>(Rows{a.x, a.x, a.n, a.n}, i0, Rows{a.y, a.y, a.m, a.m}, j0, a.d, sA, sB, acc);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + 4 * ty + r, j = j0 + tx + 16 * c;
      if (i < a.n && j < a.m) M[static_cast<size_t>(i) * a.m + j] = cost_of(acc[r][c], P);
    }
}

// the cost of one pair: read from the matrix, or recomputed with the arithmetic of pair_tile (same order, same value)
__device__ inline double sk_cost(const SkArgs& a, int i, int j) {
  if (a.M) return a.M[static_cast<size_t>(i) * a.m + j];
  const float *xi = a.x + static_cast<size_t>(i) * a.d, *yj = a.y + static_cast<size_t>(j) * a.d;
  double acc = 0.0;
  for (int k = 0; k < a.d; ++k) {
    const double df = static_cast<double>(xi[k]) - static_cast<double>(yj[k]);
    acc += a.p == 2 ? df * df : fabs(df);
  }
  return cost_of(acc, a.p);
}

__global__ void k_sk_init(SkArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.n) {
    a.loga[i] = log(a.w_x ? static_cast<double>(a.w_x[i]) : 1.0 / a.n);
    a.u[i] = 0.0;
  }
  if (i < a.m) {  // uniform: ones(m) / m, then *= n / m (eval/sinkhorn.py:123-126)
    a.logb[i] = log(a.w_y ? static_cast<double>(a.w_y[i]) : (1.0 / a.m) * (static_cast<double>(a.n) / a.m));
    a.v[i] = a.eps * a.logb[i];
  }
}

// online log-sum-exp state: sum_k exp(t_k) = s * exp(mx)
struct Lse {
  double mx, s;
};
__device__ inline void lse_push(Lse& l, double t) {
  if (!(t > -INFINITY)) return;  // a zero weight: contributes nothing
  const float e = expf(-static_cast<float>(fabs(t - l.mx)));  // mx = -inf at the start: e = 0
  if (t > l.mx) {
    l.s = l.s * e + 1.0;
    l.mx = t;
  } else {
    l.s += e;
  }
}
__device__ inline Lse lse_merge(const Lse& p, const Lse& q) {
  if (!(q.mx > -INFINITY)) return p;
  if (!(p.mx > -INFINITY)) return q;
  const double mx = fmax(p.mx, q.mx);
  return Lse{mx, p.s * exp(p.mx - mx) + q.s * exp(q.mx - mx)};
}
// argmax state, first index on ties
struct Best {
  double t;
  int idx;
};
__device__ inline Best best_merge(const Best& p, const Best& q) { return (q.t > p.t || (q.t == p.t && q.idx < p.idx)) ? q : p; }

// One block per row i.  FINAL = 0: u_i = eps (log a_i - LSE_j((v_j - M_ij) / eps)), du_i = |change|.
// FINAL = 1: rowsum_i = sum_j P_ij M_ij and corr_xy[i] = argmax_j P_ij with P_ij = exp((u_i + v_j - M_ij) / eps).
template <int FINAL>
__global__ void __launch_bounds__(NTHR) k_sk_rows(SkArgs a) {
  __shared__ double r0[NTHR], r1[NTHR];
  __shared__ int ri[NTHR];
  const int i = blockIdx.x, tid = threadIdx.x;
  if (!FINAL) {
    Lse l{-INFINITY, 0.0};
    for (int j = tid; j < a.m; j += NTHR) lse_push(l, (a.v[j] - sk_cost(a, i, j)) * a.inv_eps);
    r0[tid] = l.mx;
    r1[tid] = l.s;
    __syncthreads();
    for (int s = NTHR / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const Lse q = lse_merge(Lse{r0[tid], r1[tid]}, Lse{r0[tid + s], r1[tid + s]});
        r0[tid] = q.mx;
        r1[tid] = q.s;
      }
      __syncthreads();
    }
    if (tid == 0) {
      const double un = a.eps * (a.loga[i] - (r0[0] + log(r1[0])));
      a.du[i] = fabs(un - a.u[i]);
      a.u[i] = un;
    }
  } else {
    const double ui = a.u[i];
    double sum = 0.0;
    Best b{-INFINITY, 0x7fffffff};
    for (int j = tid; j < a.m; j += NTHR) {
      const double c = sk_cost(a, i, j), t = (ui + a.v[j] - c) * a.inv_eps;
      sum += exp(t) * c;
      if (t > b.t) b = Best{t, j};
    }
    r0[tid] = sum;
    r1[tid] = b.t;
    ri[tid] = b.idx;
    __syncthreads();
    for (int s = NTHR / 2; s > 0; s >>= 1) {
      if (tid < s) {
        r0[tid] += r0[tid + s];
        const Best q = best_merge(Best{r1[tid], ri[tid]}, Best{r1[tid + s], ri[tid + s]});
        r1[tid] = q.t;
        ri[tid] = q.idx;
      }
      __syncthreads();
    }
    if (tid == 0) {
      a.rowsum[i] = r0[0];
      if (a.corr_xy) a.corr_xy[i] = ri[0] < a.m ? ri[0] : 0;
    }
  }
}

// Column direction, stage 1: thread = column j, block row = chunk c of rows; a wave reads 256 contiguous bytes of each row.
// FINAL = 0: partial log-sum-exp over the chunk's rows of (u_i - M_ij) / eps.  FINAL = 1: partial argmax_i P_ij.
template <int FINAL>
__global__ void __launch_bounds__(NTHR) k_sk_cols(SkArgs a) {
  const int j = blockIdx.x * NTHR + threadIdx.x, c = blockIdx.y;
  if (j >= a.m) return;
  const int i0 = c * a.rows_per_chunk, i1 = min(a.n, i0 + a.rows_per_chunk);
  const size_t at = static_cast<size_t>(c) * a.m + j;
  if (!FINAL) {
    Lse l{-INFINITY, 0.0};
#pragma unroll 4
    for (int i = i0; i < i1; ++i) lse_push(l, (a.u[i] - sk_cost(a, i, j)) * a.inv_eps);
    a.part[2 * at] = l.mx;
    a.part[2 * at + 1] = l.s;
  } else {
    const double vj = a.v[j];
    Best b{-INFINITY, 0x7fffffff};
    for (int i = i0; i < i1; ++i) {
      const double t = (a.u[i] + vj - sk_cost(a, i, j)) * a.inv_eps;
      if (t > b.t) b = Best{t, i};
    }
    a.part[2 * at] = b.t;
    a.part_idx[at] = b.idx;
  }
}
// stage 2: the chunks of a column in ascending order.  v_j = eps (log b_j - LSE_i((u_i - M_ij) / eps)) with the new u.
template <int FINAL>
__global__ void __launch_bounds__(NTHR) k_sk_cols_finish(SkArgs a) {
  const int j = blockIdx.x * NTHR + threadIdx.x;
  if (j >= a.m) return;
  if (!FINAL) {
    Lse l{-INFINITY, 0.0};
    for (int c = 0; c < a.chunks; ++c) {
      const size_t at = static_cast<size_t>(c) * a.m + j;
      l = lse_merge(l, Lse{a.part[2 * at], a.part[2 * at + 1]});
    }
    const double vn = a.eps * (a.logb[j] - (l.mx + log(l.s)));
    a.dv[j] = fabs(vn - a.v[j]);
    a.v[j] = vn;
  } else if (a.corr_yx) {
    Best b{-INFINITY, 0x7fffffff};
    for (int c = 0; c < a.chunks; ++c) {
      const size_t at = static_cast<size_t>(c) * a.m + j;
      b = best_merge(b, Best{a.part[2 * at], a.part_idx[at]});
    }
    a.corr_yx[j] = b.idx < a.n ? b.idx : 0;
  }
}

// errs[0] = max_i du_i, errs[1] = max_j dv_j (one block; a NaN change propagates so that the host sees it)
__global__ void __launch_bounds__(NTHR) k_sk_errs(SkArgs a) {
  __shared__ double r0[NTHR], r1[NTHR];
  const int tid = threadIdx.x;
  double eu = 0.0, ev = 0.0;
  for (int i = tid; i < a.n; i += NTHR) eu = (a.du[i] > eu || a.du[i] != a.du[i]) ? a.du[i] : eu;
  for (int j = tid; j < a.m; j += NTHR) ev = (a.dv[j] > ev || a.dv[j] != a.dv[j]) ? a.dv[j] : ev;
  r0[tid] = eu;
  r1[tid] = ev;
  __syncthreads();
  for (int s = NTHR / 2; s > 0; s >>= 1) {
    if (tid < s) {
      r0[tid] = (r0[tid + s] > r0[tid] || r0[tid + s] != r0[tid + s]) ? r0[tid + s] : r0[tid];
      r1[tid] = (r1[tid + s] > r1[tid] || r1[tid + s] != r1[tid + s]) ? r1[tid + s] : r1[tid];
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.errs[0] = r0[0];
    a.errs[1] = r1[0];
  }
}

// errs[2] = sum_i rowsum_i (thread t adds rows t, t + 256, ... in order, then a fixed tree); u, v leave as fp32
__global__ void __launch_bounds__(NTHR) k_sk_distance(SkArgs a) {
  __shared__ double r0[NTHR];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < a.n; i += NTHR) s += a.rowsum[i];
  r0[tid] = s;
  __syncthreads();
  for (int st = NTHR / 2; st > 0; st >>= 1) {
    if (tid < st) r0[tid] += r0[tid + st];
    __syncthreads();
  }
  if (tid == 0) a.errs[2] = r0[0];
  if (a.u_out)
    for (int i = tid; i < a.n; i += NTHR) a.u_out[i] = static_cast<float>(a.u[i]);
  if (a.v_out)
    for (int j = tid; j < a.m; j += NTHR) a.v_out[j] = static_cast<float>(a.v[j]);
}

// ---- MMD -----------------------------------------------------------------------------------------------------------------------------
// The pooled sample Z = [X; Y] has 2n rows; its pairs i < j are exactly the reference's multiset {XX, i<j} + {YY, i<j} + {XY, all}.
// Block (ti, g) walks the tiles (ti, tj), tj = ti + g, ti + g + groups, ...
__device__ inline unsigned long long mmd_count(int n) { return static_cast<unsigned long long>(n) * (2ull * n - 1ull); }

// PASS 0 / 1 / 2: histogram of key bits [31:21] / [20:10] / [9:0] over the keys whose higher bits equal state[0].
// key = bit pattern of the fp32 squared distance (non-negative floats order like their bit patterns).
template <int PASS>
__global__ void __launch_bounds__(NTHR) k_mmd_hist(MmdArgs a) {
  __shared__ float sA[KC][T + 1], sB[KC][T + 1];
  __shared__ unsigned hist[SD_MET_RADIX_BINS];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, ti = blockIdx.x;
  for (int b = tid; b < SD_MET_RADIX_BINS; b += NTHR) hist[b] = 0u;
  const unsigned prefix = static_cast<unsigned>(a.state[0]);
  const Rows Z{a.X, a.Y, a.n, 2 * a.n};
  double acc[4][4];
  for (int tj = ti + blockIdx.y; tj < a.tiles; tj += a.groups) {
    pair_tile<2>(Z, ti * T, Z, tj * T, a.d, sA, sB, acc);  // (its first barrier orders the zeroing of hist, too)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = ti * T + 4 * ty + r, j = tj * T + tx + 16 * c;
        if (i < j && j < 2 * a.n) {
          const unsigned key = __float_as_uint(static_cast<float>(acc[r][c]));
          if (PASS == 0) atomicAdd(&hist[key >> 21], 1u);
          if (PASS == 1 && (key >> 21) == prefix) atomicAdd(&hist[(key >> 10) & 0x7FFu], 1u);
          if (PASS == 2 && (key >> 10) == prefix) atomicAdd(&hist[key & 0x3FFu], 1u);
        }
      }
  }
  __syncthreads();
  for (int b = tid; b < SD_MET_RADIX_BINS; b += NTHR)
    if (hist[b]) atomicAdd(&a.hist[PASS * SD_MET_RADIX_BINS + b], static_cast<unsigned long long>(hist[b]));
}

// the bin that holds the wanted rank; the lower median is the element of rank (N - 1) / 2 (torch.median)
template <int PASS>
__global__ void k_mmd_select(MmdArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  unsigned long long rank = PASS == 0 ? (mmd_count(a.n) - 1ull) / 2ull : a.state[1];
  const unsigned long long* h = a.hist + PASS * SD_MET_RADIX_BINS;
  int b = 0;
  for (; b < SD_MET_RADIX_BINS - 1; ++b) {
    if (rank < h[b]) break;
    rank -= h[b];
  }
  const unsigned long long prefix = PASS == 0 ? 0ull : a.state[0];
  a.state[0] = PASS == 0 ? b : ((prefix << (PASS == 1 ? 11 : 10)) | static_cast<unsigned long long>(b));
  a.state[1] = rank;
}

__global__ void __launch_bounds__(NTHR) k_mmd_sums(MmdArgs a) {
  __shared__ float sA[KC][T + 1], sB[KC][T + 1];
  __shared__ double red[3][NTHR];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, ti = blockIdx.x;
  const double bw = __uint_as_float(static_cast<unsigned>(a.state[0]));
  const Rows Z{a.X, a.Y, a.n, 2 * a.n};
  double acc[4][4], s[3] = {0.0, 0.0, 0.0};
  for (int tj = ti + blockIdx.y; tj < a.tiles; tj += a.groups) {
    pair_tile<2>(Z, ti * T, Z, tj * T, a.d, sA, sB, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = ti * T + 4 * ty + r, j = tj * T + tx + 16 * c;
        if (i < j && j < 2 * a.n) {
          const double kv = exp(-(acc[r][c] / bw) / 2.0);  // additions/mmd.py:24-27
          s[j < a.n ? 0 : (i >= a.n ? 1 : 2)] += kv;
        }
      }
  }
  for (int q = 0; q < 3; ++q) red[q][tid] = s[q];
  __syncthreads();
  for (int st = NTHR / 2; st > 0; st >>= 1) {
    if (tid < st)
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + st];
    __syncthreads();
  }
  if (tid < 3) a.part[3 * (static_cast<size_t>(ti) * a.groups + blockIdx.y) + tid] = red[tid][0];
}

__global__ void __launch_bounds__(NTHR) k_mmd_final(MmdArgs a) {
  __shared__ double red[3][NTHR];
  const int tid = threadIdx.x, np = a.tiles * a.groups;
  double s[3] = {0.0, 0.0, 0.0};
  for (int b = tid; b < np; b += NTHR)
    for (int q = 0; q < 3; ++q) s[q] += a.part[3 * static_cast<size_t>(b) + q];
  for (int q = 0; q < 3; ++q) red[q][tid] = s[q];
  __syncthreads();
  for (int st = NTHR / 2; st > 0; st >>= 1) {
    if (tid < st)
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + st];
    __syncthreads();
  }
  if (tid == 0) {
    // (K_XX.sum() - n) / (n (n - 1)) + (K_YY.sum() - n) / (n (n - 1)) - 2 K_XY.mean(): the diagonals are the n ones it subtracts
    const double n = a.n, off = n * (n - 1.0);
    const double mmd2 = 2.0 * red[0][0] / off + 2.0 * red[1][0] / off - 2.0 * red[2][0] / (n * n);
    a.out[0] = static_cast<float>(sqrt(fmax(1e-20, mmd2)));
    a.out[1] = __uint_as_float(static_cast<unsigned>(a.state[0]));
  }
}

}  // namespace

#define SD_RET(expr)                 \
  do {                               \
    const int e_ = (expr);           \
    if (e_ != 0) return e_;          \
  } while (0)
#define SD_LAUNCHED() SD_RET(static_cast<int>(hipGetLastError()))

int sd_run_sinkhorn(SkArgs a, float* M_store, int max_iters, double stop_thresh, sdeng_sinkhorn_result* res, hipStream_t s) {
  const dim3 blk(NTHR);
  const dim3 g_cols((a.m + NTHR - 1) / NTHR, a.chunks), g_fin((a.m + NTHR - 1) / NTHR);
  a.M = nullptr;
  if (M_store) {
    const dim3 g((a.m + T - 1) / T, (a.n + T - 1) / T);
    if (a.p == 2) hipLaunchKernelGGL(k_pair_cost<2>, g, blk, 0, s, a, M_store);
    else hipLaunchKernelGGL(k_pair_cost<1>, g, blk, 0, s, a, M_store);
    SD_LAUNCHED();
    a.M = M_store;
  }
  hipLaunchKernelGGL(k_sk_init, dim3(((a.n > a.m ? a.n : a.m) + NTHR - 1) / NTHR), blk, 0, s, a);
  SD_LAUNCHED();
  double e[3] = {0.0, 0.0, 0.0};
  int it = 0;
  while (it < max_iters) {
    hipLaunchKernelGGL(k_sk_rows<0>, dim3(a.n), blk, 0, s, a);
    hipLaunchKernelGGL(k_sk_cols<0>, g_cols, blk, 0, s, a);
    hipLaunchKernelGGL(k_sk_cols_finish<0>, g_fin, blk, 0, s, a);
    hipLaunchKernelGGL(k_sk_errs, dim3(1), blk, 0, s, a);
    SD_LAUNCHED();
    SD_RET(static_cast<int>(hipMemcpyAsync(e, a.errs, 2 * sizeof(double), hipMemcpyDeviceToHost, s)));  // the stop test: the one read-back
    SD_RET(static_cast<int>(hipStreamSynchronize(s)));
    ++it;
    if (e[0] < stop_thresh && e[1] < stop_thresh) break;
  }
  hipLaunchKernelGGL(k_sk_rows<1>, dim3(a.n), blk, 0, s, a);
  hipLaunchKernelGGL(k_sk_cols<1>, g_cols, blk, 0, s, a);
  hipLaunchKernelGGL(k_sk_cols_finish<1>, g_fin, blk, 0, s, a);
  hipLaunchKernelGGL(k_sk_distance, dim3(1), blk, 0, s, a);
  SD_LAUNCHED();
  SD_RET(static_cast<int>(hipMemcpyAsync(e + 2, a.errs + 2, sizeof(double), hipMemcpyDeviceToHost, s)));
  SD_RET(static_cast<int>(hipStreamSynchronize(s)));
  res->distance = e[2];
  res->max_err_u = e[0];
  res->max_err_v = e[1];
  res->iters = it;
  res->materialised = M_store ? 1 : 0;
  return 0;
}

int sd_run_mmd_median(MmdArgs a, hipStream_t s) {
  const dim3 blk(NTHR), g(a.tiles, a.groups);
  SD_RET(static_cast<int>(hipMemsetAsync(a.hist, 0, sizeof(unsigned long long) * (3 * SD_MET_RADIX_BINS), s)));
  SD_RET(static_cast<int>(hipMemsetAsync(a.state, 0, sizeof(unsigned long long) * 4, s)));
  hipLaunchKernelGGL(k_mmd_hist<0>, g, blk, 0, s, a);
  hipLaunchKernelGGL(k_mmd_select<0>, dim3(1), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_mmd_hist<1>, g, blk, 0, s, a);
  hipLaunchKernelGGL(k_mmd_select<1>, dim3(1), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_mmd_hist<2>, g, blk, 0, s, a);
  hipLaunchKernelGGL(k_mmd_select<2>, dim3(1), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_mmd_sums, g, blk, 0, s, a);
  hipLaunchKernelGGL(k_mmd_final, dim3(1), blk, 0, s, a);
  SD_LAUNCHED();
  return 0;
}
