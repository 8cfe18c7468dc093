// extern "C" entry points of libsdeng.so (see include/sdeng.h).  An entry point that runs a step-loop kernel works in three phases:
//   1. validate the descriptor (plan_* / check_*: pure host code),
//   2. select the kernel instance: every template parameter, looked up in the generated registry (gen/registry.hip),
//   3. check the workspace, run the preparation kernels, launch.
// No HIP call is made for a descriptor that is rejected.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>

#include "../../include/sdeng.h"
#include "prep_kernels.hpp"
#include "sim_kernel.hpp"
#include "cmcd_kernel.hpp"
#include "grad_kernel.hpp"
#include "cmcd_adjoint_kernel.hpp"
#include "metric_kernels.hpp"
#include "tilted_kernel.hpp"
#include "tilted_rds.hpp"

// ---- error string ------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
#define SD_HIP(expr)                                                                  \
  do {                                                                                \
    int e_ = (expr);                                                                  \
    if (e_ != 0) return fail(SDENG_E_HIP, "%s failed: %s", #expr, hipGetErrorString(static_cast<hipError_t>(e_))); \
  } while (0)
#define SD_TRY(expr)      \
  do {                    \
    int rc_ = (expr);     \
    if (rc_) return rc_;  \
  } while (0)

extern "C" int sdeng_abi_version(void) { return SDENG_ABI_VERSION; }
extern "C" const char* sdeng_last_error(void) { return g_err; }

// ---- small shared pieces -------------------------------------------------------------------------
static inline size_t align64(size_t n_floats) { return (n_floats + 63) & ~static_cast<size_t>(63); }
static inline int pad16(int d) { return 16 * ((d + 15) / 16); }
static inline float half_d_log_2pi(int d) { return static_cast<float>(0.5 * d * std::log(2.0 * M_PI)); }  // distr/gauss.py:71
struct Seed {
  unsigned lo, hi;
};
static inline Seed split_seed(uint64_t seed) { return {static_cast<unsigned>(seed & 0xFFFFFFFFull), static_cast<unsigned>(seed >> 32)}; }
static int check_abi(const sdeng_desc* d) {
  return d->abi_version == SDENG_ABI_VERSION ? 0 : fail(SDENG_E_INVALID, "ABI version %d, library has %d", d->abi_version, SDENG_ABI_VERSION);
}
static int check_lerp_prior(const sdeng_desc* d) {
  if (d->net.ctrl_kind == SDENG_CTRL_LERP && d->prior.kind != SDENG_DIST_ISO_GAUSS)
    return fail(SDENG_E_UNSUPPORTED, "LerpCtrl needs an IsotropicGauss prior (kind %d given)", d->prior.kind);
  return 0;
}
static int ref_components(const sdeng_desc* d) {  // K of the reference mixture: 0 = no reference
  return d->ref.kind == SDENG_REF_NONE ? 0 : (d->ref.kind == SDENG_REF_GAUSS_DIAG ? 1 : d->ref.k);
}
static bool score_like(int ctrl_kind) {
  return ctrl_kind == SDENG_CTRL_SCORE || ctrl_kind == SDENG_CTRL_LERP || ctrl_kind == SDENG_CTRL_CANCEL_DRIFT;
}
// in-loop target score of a control or a Langevin drift: SC_GMM (mixture, or rings in the d <= 16 kernel), SC_PHI4, SC_LOGREG; -1 = none built
static int in_loop_score(int target_kind) {
  if (target_kind == SDENG_DIST_GMM_DIAG || target_kind == SDENG_DIST_RINGS) return SC_GMM;
  if (target_kind == SDENG_DIST_PHI4) return SC_PHI4;
  if (target_kind == SDENG_DIST_LOGREG) return SC_LOGREG;
  return -1;
}

// ---- kernel selection: the generated registry -------------------------------------------------------
struct KernelKey {
  int fam, nt, p[4];  // family (SD_FAM_*), feature tiles, the family's template parameters after NT (sim_common.hpp)
  sd_launcher fn;
};
static int select_kernel(KernelKey& k, int fam, int nt, int p0 = 0, int p1 = 0, int p2 = 0, int p3 = 0) {
  static const char* const kFamily[] = {"k_simulate", "k_ctrl_forward", "k_simulate_split", "k_euler", "k_simulate_cmcd", "k_ctrl_vjp", "k_kl_adjoint", "k_cmcd_kl_adjoint"};
  k = KernelKey{fam, nt, {p0, p1, p2, p3}, nullptr};
  const uint32_t key = sd_key(fam, nt, p0, p1, p2, p3);
  const SdKernelEntry* end = sd_registry + sd_registry_size;
  const SdKernelEntry* e = std::lower_bound(sd_registry, end, key, [](const SdKernelEntry& x, uint32_t v) { return x.key < v; });
  if (e == end || e->key != key)
    return fail(SDENG_E_UNSUPPORTED, "no kernel instance %s<NT=%d, %d, %d, %d, %d>", kFamily[fam], nt, p0, p1, p2, p3);
  k.fn = e->fn;
  return 0;
}
static int launch_timed(const sdeng_desc* d, const KernelKey& k, const void* args, hipStream_t s) {  // bracketed by the caller's events
  if (d->ev_start) SD_HIP(hipEventRecord(static_cast<hipEvent_t>(d->ev_start), s));
  SD_HIP(k.fn(args, s));
  if (d->ev_stop) SD_HIP(hipEventRecord(static_cast<hipEvent_t>(d->ev_stop), s));
  return 0;
}

// ---- workspace layout ----------------------------------------------------------------------------
// feature tiles of 16: one instantiation per tile count, NT = ceil(d / 16) exactly (d = 100 runs 7 tiles, not 8: no vector or
// matrix work on whole tiles of pad features).  The full-covariance reference kernels stage each precision image in two
// pieces of NT/2 output tiles when NT > 4, so 5 and 7 tiles run on the 6- and 8-tile instantiations.
static int tiles_exact(int d) { return (d + 15) / 16; }
static int tiles_of(const sdeng_desc* d) {
  const int nt = tiles_exact(d->d);
  return (d->ref.kind == SDENG_REF_GMM_FULL && (nt == 5 || nt == 7)) ? nt + 1 : nt;
}

static size_t dist_floats(const sdeng_dist& ds, int dpad) {
  if (ds.kind == SDENG_DIST_GMM_DIAG) return align64(static_cast<size_t>(ds.k) * 2 * dpad) + align64(static_cast<size_t>(ds.k) * 4);
  if (ds.kind == SDENG_DIST_GAUSS_DIAG) return align64(2 * dpad) + align64(4);
  return 0;
}

// SDENG_FLAG_SPLIT_TILES: is the low-latency kernel built for this call?  (The reference kind is checked where it is known.)
static bool split_eligible(const sdeng_desc* d, int DT) {
  return (d->flags & SDENG_FLAG_SPLIT_TILES) && d->B <= 8192 && DT >= 5 && d->net.ctrl_kind == SDENG_CTRL_CLIPPED &&
         (d->form == SDENG_FORM_LIN || d->form == SDENG_FORM_EM) && !d->noise_in &&
         (d->ref.kind == SDENG_REF_NONE || d->ref.kind == SDENG_REF_GAUSS_DIAG || (d->ref.kind == SDENG_REF_GMM_DIAG && d->ref.k <= 4));
}

// floats of LDS per buffer left for a workgroup-shared reference table behind the drift-net weights (160 KiB per workgroup, two buffers)
static int share_room(int DT) { return (160 * 1024 - static_cast<int>(sizeof(float)) * sd_lds_weight_floats(DT)) / 2 / static_cast<int>(sizeof(float)); }
static int mm_piece(int K, int DT) {  // RF_GMM_MM: floats of the larger of the logit / mean images
  const int kt = (K + 15) / 16;
  return std::max(sd_mm_logit_floats(kt, DT), sd_mm_mean_floats(kt, DT));
}
// Diagonal mixture references with 4 < K <= 64 components that share one variance vector run on the matrix pipe (RF_GMM_MM):
// forward forms with a ClippedCtrl.  SDENG_REF_MM=0 keeps the vector path (A/B measurements).
static bool use_mm(const sdeng_desc* d, int DT) {
  static const bool allow = [] { const char* e = getenv("SDENG_REF_MM"); return !(e && e[0] == '0'); }();
  if (!allow || d->ref.kind != SDENG_REF_GMM_DIAG || !d->ref.shared_var) return false;
  const int K = d->ref.k;
  if (K <= 4 && K * 2 * 16 * DT <= SD_REFTAB_FLOATS) return false;  // small mixtures: responsibilities in registers (RF_GMM)
  if (K > 64) return false;
  if (d->net.ctrl_kind != SDENG_CTRL_CLIPPED || (d->form != SDENG_FORM_LIN && d->form != SDENG_FORM_EM)) return false;
  const int piece = mm_piece(K, DT);
  return piece <= share_room(DT) && piece <= sd_share_buf_floats(SD_SHARE_MAX);
}

struct Layout {
  size_t wpack, temb, stheta, ref_tab, ref_mean, ref_consts, target, ref_dist, prior, rnd_init, trash, logz, cmcd, x0, total;
};

static bool make_layout(const sdeng_desc* d, Layout& L) {
  if (!d || d->d < 1 || d->d > 128 || d->N < 0 || d->B < 0) return false;
  const int DT = tiles_of(d), dpad = 16 * DT;
  size_t o = 0;
  L.wpack = o; o += align64(sd_pack_floats(DT));
  L.temb = o; o += align64(static_cast<size_t>(d->N + 1) * SD_H);  // CMCD evaluates the net at N+1 times
  L.stheta = o; o += align64(d->N + 1);
  const int K = ref_components(d);
  if (d->ref.kind == SDENG_REF_GMM_FULL) {  // precision images + noised means
    L.ref_tab = o; o += align64(static_cast<size_t>(d->N) * K * sd_image_floats(DT, DT) + 256);
    L.ref_mean = o; o += align64(static_cast<size_t>(d->N) * K * dpad);
  } else if (use_mm(d, DT)) {  // logit + mean images, centre / 1/var vectors (+ 64 logit constants per step under ref_consts)
    const int kt = (K + 15) / 16;
    L.ref_tab = o; o += align64(static_cast<size_t>(d->N) * (sd_mm_logit_floats(kt, DT) + sd_mm_mean_floats(kt, DT)) + 1024);
    L.ref_mean = o; o += align64(static_cast<size_t>(d->N) * 2 * dpad);
  } else {
    L.ref_tab = o; o += align64(static_cast<size_t>(d->N) * K * 2 * dpad);
    L.ref_mean = o;
  }
  L.ref_consts = o; o += align64(static_cast<size_t>(d->N) * (K * 2 > 64 ? K * 2 : 64) + 1);  // + the shared-variance flag (MM: 64 per step)
  L.target = o; o += dist_floats(d->target, dpad);
  L.ref_dist = o; o += dist_floats(d->ref_dist, dpad);
  L.prior = o; o += dist_floats(d->prior, dpad);
  L.rnd_init = o; o += align64(d->B);
  L.trash = o; o += align64((SD_WAVES_MAX > SD_WAVES ? SD_WAVES_MAX : SD_WAVES) * 64 * 4);
  L.logz = o; o += align64(5 * SD_LOGZ_MAX_BLOCKS);
  L.cmcd = o;
  {  // logistic-regression images (CMCD, or the in-loop score of a Score/LerpCtrl) and the CMCD prior's packed precision
    const bool lr_used = d->target.kind == SDENG_DIST_LOGREG && d->target.k > 0 &&
                         (d->form == SDENG_FORM_CMCD || d->form == SDENG_FORM_CMCD_EUBO || d->net.ctrl_kind != SDENG_CTRL_CLIPPED);
    const int n = lr_used ? d->target.k : 0;
    o += align64(sd_lr_floats(DT, n)) + align64(32 * sd_lr_row_kb(n));
    if (d->form == SDENG_FORM_CMCD || d->form == SDENG_FORM_CMCD_EUBO) o += align64(sd_image_floats(DT, DT)) + align64(16 * DT);
  }
  L.x0 = o;
  if (!d->x_in && !d->x0_out) o += align64(static_cast<size_t>(d->B) * d->d);  // the engine's own x0 draw
  L.total = o;
  return true;
}

// A full-covariance mixture as the target of a score control (SDENG_DIST_GMM_FULL) is evaluated by the machinery of the full-covariance
// REFERENCE: the descriptor is rewritten so that the mixture occupies the (empty) reference slot -- layout, table kernel and the
// RF_GMM_FULL step loop then need no second copy -- and the caller remembers that the slot feeds the control, not the drift.
static bool slot_target(const sdeng_desc* d, sdeng_desc& out) {
  if (!d || d->target.kind != SDENG_DIST_GMM_FULL) return false;
  out = *d;
  out.ref.kind = SDENG_REF_GMM_FULL;
  out.ref.k = d->target.k;
  out.ref.means_init = d->target.loc;
  out.ref.vars_init = d->target.scale;
  out.ref.eigvecs = d->target.aux;
  out.ref.weights = d->target.w;
  out.ref.shared_var = 0;
  memset(&out.target, 0, sizeof(out.target));
  return true;
}
static int check_slot_target(const sdeng_desc* d) {  // d: the caller's descriptor
  if (d->ref.kind != SDENG_REF_NONE)
    return fail(SDENG_E_UNSUPPORTED, "full-covariance mixture target of a score control together with a reference drift (ref.kind %d)", d->ref.kind);
  if (!score_like(d->net.ctrl_kind))
    return fail(SDENG_E_UNSUPPORTED, "SDENG_DIST_GMM_FULL is the target of a Score / Lerp / CancelDrift control only (ctrl_kind %d)", d->net.ctrl_kind);
  if (d->form != SDENG_FORM_LIN && d->form != SDENG_FORM_EM)
    return fail(SDENG_E_UNSUPPORTED, "full-covariance mixture target of a score control: forward forms only (form %d)", d->form);
  if (d->flags & (SDENG_FLAG_TERM_TARGET | SDENG_FLAG_REMOVE_REF))
    return fail(SDENG_E_UNSUPPORTED, "SDENG_DIST_GMM_FULL: no log-density kernel (FLAG_TERM_TARGET) and no RemoveReferenceCtrl");
  if (d->target.k < 1 || !d->target.loc || !d->target.scale || !d->target.aux)
    return fail(SDENG_E_INVALID, "SDENG_DIST_GMM_FULL: null means / eigenvalues / eigenvectors or k < 1");
  return 0;
}

extern "C" size_t sdeng_workspace_bytes(const sdeng_desc* desc) {
  Layout L;
  sdeng_desc ds;
  if (slot_target(desc, ds)) desc = &ds;
  if (!make_layout(desc, L)) return 0;
  return L.total * sizeof(float);
}

// ---- distribution descriptor -> device view (+ table kernels) -------------------------------------
static int check_dist(const sdeng_dist& in, int d) {
  switch (in.kind) {
    case SDENG_DIST_NONE:
    case SDENG_DIST_ISO_GAUSS:
    case SDENG_DIST_PHI4:
      return 0;
    case SDENG_DIST_GMM_DIAG:
    case SDENG_DIST_GAUSS_DIAG: {
      const int K = in.kind == SDENG_DIST_GMM_DIAG ? in.k : 1;
      if (K < 1 || !in.loc || !in.scale || (in.kind == SDENG_DIST_GMM_DIAG && !in.w))
        return fail(SDENG_E_INVALID, "diagonal Gaussian/mixture needs loc, scale%s", in.kind == SDENG_DIST_GMM_DIAG ? ", w and k >= 1" : "");
      return 0;
    }
    case SDENG_DIST_GAUSS_FULL:
      return (in.loc && in.scale && in.w) ? 0 : fail(SDENG_E_INVALID, "GAUSS_FULL needs loc, precision, inverse Cholesky factor");
    case SDENG_DIST_LOGREG:
      return (in.loc && in.scale && in.k >= 1) ? 0 : fail(SDENG_E_INVALID, "LOGREG needs X, y and k >= 1 rows");
    case SDENG_DIST_RINGS:
      if (d != 2) return fail(SDENG_E_INVALID, "RINGS is two-dimensional (d = %d)", d);
      if (!in.loc || !in.w || in.k < 1 || in.k > 8 || !(in.p0 > 0.0f)) return fail(SDENG_E_INVALID, "RINGS needs radii, weights, 1 <= k <= 8, scale > 0");
      return 0;
    case SDENG_DIST_CHECKERBOARD:
      if (d != 2) return fail(SDENG_E_INVALID, "CHECKERBOARD is two-dimensional (d = %d)", d);
      if (!in.loc || !in.scale || !in.w || in.k < 1) return fail(SDENG_E_INVALID, "CHECKERBOARD needs the low / high corner tables, the per-square constants and k >= 1");
      return 0;
    default:
      return fail(SDENG_E_UNSUPPORTED, "unknown distribution kind %d", in.kind);
  }
}
static int build_dist(const sdeng_dist& in, int d, int dpad, float* ws, DistDev& out, hipStream_t s) {
  SD_TRY(check_dist(in, d));
  memset(&out, 0, sizeof(out));
  out.kind = in.kind;
  out.k = in.k;
  out.p0 = in.p0; out.p1 = in.p1; out.p2 = in.p2; out.p3 = in.p3;
  out.clip = in.clip;
  switch (in.kind) {
    case SDENG_DIST_GMM_DIAG:
    case SDENG_DIST_GAUSS_DIAG: {
      DistTabArgs t;
      t.K = in.kind == SDENG_DIST_GMM_DIAG ? in.k : 1; t.d = d; t.dpad = dpad;
      t.loc = in.loc; t.scale = in.scale; t.weights = in.kind == SDENG_DIST_GMM_DIAG ? in.w : nullptr;
      t.tab = ws; t.consts = ws + align64(static_cast<size_t>(t.K) * 2 * dpad);
      SD_HIP(sd_launch_dist_tables(t, s));
      out.k = t.K;
      out.tab = t.tab; out.consts = t.consts;
      out.p0 = half_d_log_2pi(d);
      return 0;
    }
    case SDENG_DIST_GAUSS_FULL: out.aux0 = in.loc; out.tab = in.scale; out.aux1 = in.w; return 0;
    case SDENG_DIST_LOGREG: out.aux0 = in.loc; out.aux1 = in.scale; return 0;
    case SDENG_DIST_RINGS: out.aux0 = in.loc; out.aux1 = in.w; return 0;
    case SDENG_DIST_CHECKERBOARD: out.aux0 = in.loc; out.aux1 = in.scale; out.tab = in.w; return 0;
    default: return 0;
  }
}
static int dist_eval(const DistDev& ds, int B, int d, int dpad, const float* x, float* logp, float* score, hipStream_t s) {
  DistEvalArgs e;
  e.ds = ds; e.B = B; e.d = d; e.dpad = dpad; e.x = x; e.logp_out = logp; e.score_out = score;
  SD_HIP(sd_launch_dist_eval(e, s));
  return 0;
}
// rnd += [log p_ref(x)] - [log pi~(x)]
static int terminal(const sdeng_desc* d, int dpad, const DistDev& ref, const DistDev& target, bool use_ref, bool use_target, const float* x,
                    float* rnd, hipStream_t s) {
  TerminalArgs t;
  t.ref = ref; t.target = target; t.use_ref = use_ref; t.use_target = use_target;
  t.B = d->B; t.d = d->d; t.dpad = dpad; t.x = x; t.rnd = rnd;
  SD_HIP(sd_launch_terminal(t, s));
  return 0;
}

// ---- the drift net --------------------------------------------------------------------------------
static int check_net(const sdeng_net& n) {
  if (!n.w_in || !n.b_in || !n.w_h1 || !n.b_h1 || !n.w_h2 || !n.b_h2 || !n.w_out || !n.b_out)
    return fail(SDENG_E_INVALID, "drift net: null weight pointer");
  const sdeng_time_embed& te = n.t_embed;
  if (!te.coeff || !te.phase || te.n_hidden != 1 || te.dim_out != SD_H || !te.w[0] || !te.b[0] || !te.w_out || !te.b_out)
    return fail(SDENG_E_UNSUPPORTED, "drift net time embedding must be TimeEmbed(num_layers=2, channels=64)");
  if (n.ctrl_kind != SDENG_CTRL_CLIPPED) {
    const sdeng_time_embed& sm = n.score_model;
    if (sm.n_hidden > 0) {
      if (sm.n_hidden > 4 || sm.dim_out != 1 || !sm.coeff || !sm.phase || !sm.w_out || !sm.b_out)
        return fail(SDENG_E_UNSUPPORTED, "score_model must be TimeEmbed(dim_out=1, num_layers<=5)");
      for (int i = 0; i < sm.n_hidden; ++i)
        if (!sm.w[i] || !sm.b[i]) return fail(SDENG_E_INVALID, "score_model: null weight pointer");
    }
  }
  return 0;
}
// one more job of a k_pack_images launch (PackJob, prep_kernels.hpp): the image of src [n_out x n_in] -- or, with `transpose`, of the transpose
// of src [n_in x n_out] -- unscaled and without a bias; the caller names a scale source and a bias where there is one
static PackJob& add_pack_job(PackJobs& p, const float* src, int ld, int n_out, int n_in, bool transpose, int out_tiles, int k_blocks, float* dst) {
  PackJob& j = p.job[p.njobs++];
  j = PackJob{};
  j.src = src; j.ld = ld; j.n_out = n_out; j.n_in = n_in; j.transpose = transpose;
  j.out_tiles = static_cast<int16_t>(out_tiles); j.k_blocks = static_cast<int16_t>(k_blocks); j.dst = dst;
  return j;
}
static void scale_by(PackJob& j, const float* matrix, int n, float* scale_dst = nullptr, int inv_off = 0) {
  j.scale_src = matrix; j.scale_n = n; j.scale_dst = scale_dst; j.inv_off = inv_off;
}
static void with_bias(PackJob& j, const float* bias, float* dst, int padded) {
  j.bias = bias; j.bias_dst = dst; j.bias_pad = static_cast<int16_t>(padded);
}
// the packed image of the net at `out`; with `out_t`, in the same launch the image of the TRANSPOSED net for the backward products
// (grad_kernel.hpp): slot of W_in <- W_out^T, W_1 <- W_2^T, W_2 <- W_1^T, W_out <- W_in^T, each with the scale of its own matrix; no biases
static int pack_net(const sdeng_desc* d, int DT, float* out, float* out_t, hipStream_t s) {
  const sdeng_net& n = d->net;
  const int dim = d->d, KBD = sd_kb(DT), KBH = sd_kb(SD_HT);
  const float* W[4] = {n.w_in, n.w_h1, n.w_h2, n.w_out};
  const float* b[4] = {n.b_in, n.b_h1, n.b_h2, n.b_out};
  const int n_out[4] = {SD_H, SD_H, SD_H, dim}, n_in[4] = {dim, SD_H, SD_H, SD_H};
  const int tiles[4] = {SD_HT, SD_HT, SD_HT, DT}, kbs[4] = {KBD, KBH, KBH, KBH};
  const int off[4] = {sd_off_win(DT), sd_off_wh1(DT), sd_off_wh2(DT), sd_off_wout(DT)};
  PackJobs pk;
  pk.njobs = 0;
  for (int l = 0; l < 4; ++l) {
    PackJob& j = add_pack_job(pk, W[l], n_in[l], n_out[l], n_in[l], false, tiles[l], kbs[l], out + off[l]);
    scale_by(j, W[l], n_out[l] * n_in[l], out + sd_off_scales(DT) + l, 4);
    with_bias(j, b[l], out + sd_off_bias(DT) + 64 * l, 16 * tiles[l]);
  }
  for (int l = 0; out_t && l < 4; ++l) {  // slot l has the shape of layer l and holds the transpose of matrix m = 3 - l, stored [n_in x n_out]
    const int m = 3 - l;
    scale_by(add_pack_job(pk, W[m], n_out[l], n_out[l], n_in[l], true, tiles[l], kbs[l], out_t + off[l]), W[m], n_out[m] * n_in[m]);
  }
  SD_HIP(sd_launch_pack_images(pk, s));
  return 0;
}
// time embedding of the drift net at n_times rows of coef (t_direct: at t_value), and the clipped score_model(t) when the control has one
static int embed_times(const sdeng_desc* d, int n_times, bool t_direct, float t_value, float* temb, float* stheta_ws, const float** stheta,
                       hipStream_t s) {
  TimeEmbedArgs te;
  te.te = d->net.t_embed; te.coef = d->coef; te.col = 0; te.t_direct = t_direct; te.t_value = t_value; te.clip = 0.0f; te.out = temb;
  SD_HIP(sd_launch_time_embed(te, n_times, s));
  *stheta = nullptr;
  if (d->net.ctrl_kind != SDENG_CTRL_CLIPPED && d->net.score_model.n_hidden > 0) {
    te.te = d->net.score_model;
    te.clip = d->net.clip_model;  // reparam.py:102-110 clips the score model with clip_model
    te.out = stheta_ws;
    SD_HIP(sd_launch_time_embed(te, n_times, s));
    *stheta = stheta_ws;
  }
  return 0;
}
// common preparation for simulate / ctrl_forward: packed weights, time embeddings, control constants
static int prepare_net(const sdeng_desc* d, const Layout& L, float* ws, int DT, SimArgs& a, hipStream_t s, int n_times, bool t_direct,
                       float t_value) {
  SD_TRY(pack_net(d, DT, ws + L.wpack, nullptr, s));
  a.wpack = ws + L.wpack;
  if (n_times > 0) SD_TRY(embed_times(d, n_times, t_direct, t_value, ws + L.temb, ws + L.stheta, &a.stheta, s));
  a.temb = ws + L.temb;
  a.ctrl_kind = d->net.ctrl_kind;
  a.clip_model = d->net.clip_model;
  a.clip_score = d->net.clip_score;
  a.scale_score = d->net.scale_score;
  return 0;
}

// ScoreCtrl / LerpCtrl / CancelDriftCtrl: the in-loop score kind of the target (SC_NONE for a ClippedCtrl)
static int score_kind(const sdeng_desc* d, int& sc) {
  sc = SC_NONE;
  if (d->net.ctrl_kind == SDENG_CTRL_CLIPPED) return 0;
  if (!score_like(d->net.ctrl_kind)) return fail(SDENG_E_UNSUPPORTED, "unknown ctrl_kind %d", d->net.ctrl_kind);
  sc = in_loop_score(d->target.kind);
  if (sc < 0) return fail(SDENG_E_UNSUPPORTED, "ScoreCtrl/LerpCtrl: no in-loop score kernel for target kind %d", d->target.kind);
  return check_lerp_prior(d);
}

// logistic-regression target -> the two LDS images + the in-kernel constants (a.lr); *next = the first float after them
static int prepare_logreg(const sdeng_desc* d, const Layout& L, float* ws, int DT, SimArgs& a, hipStream_t s, float** next) {
  const int n = d->target.k;
  float* image = ws + L.cmcd;
  float* y_pad = image + align64(sd_lr_floats(DT, n));
  *next = y_pad + align64(32 * sd_lr_row_kb(n));
  SD_HIP(sd_launch_logreg_images(d->target.loc, d->target.scale, n, d->d - 1, DT, image, y_pad, s));
  a.lr.image = image; a.lr.y_pad = y_pad; a.lr.n_rows = n;
  // sonar (166 x 61) sits in LDS next to the drift net; larger design matrices (credit: 800 rows) are read through L2 instead
  a.lr.in_lds = static_cast<size_t>(cmcd_lds_floats(DT, n)) * sizeof(float) <= 160 * 1024 ? 1 : 0;
  a.lr.inv_w_scale2 = 1.0f / (d->target.p0 * d->target.p0); a.lr.c_mean = d->target.p1; a.lr.inv_c_scale2 = 1.0f / (d->target.p2 * d->target.p2);
  // sigmoid range with a gradient: inside clip(thr, 1 - thr) and inside the eps clamp of probs_to_logits
  const float thr = d->target.p3, eps = 1.1920928955078125e-07f;
  a.lr.p_lo = thr > eps ? thr : eps;
  a.lr.p_hi = (1.0f - thr) < (1.0f - eps) ? (1.0f - thr) : (1.0f - eps);
  return 0;
}

static int check_x0_dist(const sdeng_desc* d) {
  const sdeng_dist& q = d->x0_dist;
  if (d->form == SDENG_FORM_EUBO || d->form == SDENG_FORM_CMCD_EUBO)
    return fail(SDENG_E_INVALID, "the noising loops start from samples of the TARGET: x_in is required");
  if (q.kind == SDENG_DIST_ISO_GAUSS) return 0;
  if (q.kind == SDENG_DIST_GAUSS_DIAG) return q.loc ? 0 : fail(SDENG_E_INVALID, "x0_dist GAUSS_DIAG needs loc (scale may be NULL: x0 = loc)");
  if (q.kind == SDENG_DIST_GAUSS_FULL) return (q.loc && q.aux) ? 0 : fail(SDENG_E_INVALID, "x0_dist GAUSS_FULL needs loc and the Cholesky factor (aux)");
  return fail(SDENG_E_UNSUPPORTED, "x_in == NULL: no sampler for x0_dist kind %d (ISO_GAUSS, GAUSS_DIAG, GAUSS_FULL)", q.kind);
}

// ---- sdeng_simulate: phases 1 and 2 ---------------------------------------------------------------
struct SimPlan {
  const sdeng_desc* d;  // the descriptor the kernels see: the caller's, or its slot-target rewrite (stored in `slot`)
  sdeng_desc slot;
  bool in_slot;
  Layout L;
  int DT, rf, sc;
  KernelKey k;
};

// ControlledLangevinSDELoss.simulate (losses/oc.py:666-755): logistic-regression, mixture, phi^4, rings or checkerboard target, Gaussian prior
static int plan_cmcd(SimPlan& p) {
  const sdeng_desc* d = p.d;
  const bool logreg = d->target.kind == SDENG_DIST_LOGREG;
  const bool toy = d->target.kind == SDENG_DIST_RINGS || d->target.kind == SDENG_DIST_CHECKERBOARD;  // 2-D: check_dist checks d = 2
  if (!logreg && !toy && d->target.kind != SDENG_DIST_GMM_DIAG && d->target.kind != SDENG_DIST_GAUSS_DIAG && d->target.kind != SDENG_DIST_PHI4)
    return fail(SDENG_E_UNSUPPORTED, "CMCD kernel: target must be LOGREG, GMM_DIAG, GAUSS_DIAG, PHI4, RINGS or CHECKERBOARD (kind %d)", d->target.kind);
  if (logreg && p.DT > 4) return fail(SDENG_E_UNSUPPORTED, "CMCD kernel: logistic regression with d <= 64 (got %d)", d->d);
  if (logreg && d->target.k < 1) return fail(SDENG_E_INVALID, "CMCD kernel: logistic regression without data rows");
  if (d->prior.kind != SDENG_DIST_GAUSS_FULL && d->prior.kind != SDENG_DIST_ISO_GAUSS && d->prior.kind != SDENG_DIST_GAUSS_DIAG)
    return fail(SDENG_E_UNSUPPORTED, "CMCD kernel: prior must be GAUSS_FULL, GAUSS_DIAG or ISO_GAUSS (kind %d)", d->prior.kind);
  if (d->net.ctrl_kind != SDENG_CTRL_CLIPPED && d->net.ctrl_kind != SDENG_CTRL_SCORE)
    return fail(SDENG_E_UNSUPPORTED, "CMCD kernel: ClippedCtrl or ScoreCtrl");
  if (!(d->flags & SDENG_FLAG_INIT_LOGP) || !(d->flags & SDENG_FLAG_TERM_TARGET))
    return fail(SDENG_E_UNSUPPORTED, "CMCD kernel implements the eval path (rnd0 = log p_prior, terminal -log pi)");
  SD_TRY(check_net(d->net));
  SD_TRY(check_dist(d->target, d->d));
  SD_TRY(check_dist(d->prior, d->d));
  const bool eubo = d->form == SDENG_FORM_CMCD_EUBO;
  if (eubo && d->target.kind != SDENG_DIST_GMM_DIAG && d->target.kind != SDENG_DIST_GAUSS_DIAG && !toy)
    return fail(SDENG_E_UNSUPPORTED, "CMCD compute_eubo kernels: diagonal Gaussian / mixture, rings or checkerboard targets (kind %d)", d->target.kind);
  // target kind: the toy targets (d = 2, one tile) in both directions; otherwise the noising loop samples mixture / Gaussian targets
  const int tgt = d->target.kind == SDENG_DIST_RINGS ? CT_RINGS : d->target.kind == SDENG_DIST_CHECKERBOARD ? CT_ZERO : eubo ? CT_GMM :
                  d->target.kind == SDENG_DIST_PHI4 ? CT_PHI4 : logreg ? CT_LOGREG : CT_GMM;
  return select_kernel(p.k, SD_FAM_CMCD, p.DT, tgt, eubo, (d->noise_in || d->xs_out) ? 1 : 0);
}

// SDENG_CTRL_NONE: Euler-Maruyama of an SDE without a drift net (euler_kernel.hpp)
static int plan_euler(SimPlan& p) {
  const sdeng_desc* d = p.d;
  if (d->form != SDENG_FORM_EM) return fail(SDENG_E_UNSUPPORTED, "CTRL_NONE (no drift net) runs the Euler-Maruyama form only (form %d given)", d->form);
  if (d->ref.kind != SDENG_REF_NONE) return fail(SDENG_E_UNSUPPORTED, "CTRL_NONE with a reference drift");
  if (d->flags & (SDENG_FLAG_TERM_REF | SDENG_FLAG_TERM_TARGET | SDENG_FLAG_INIT_LOGP))
    return fail(SDENG_E_UNSUPPORTED, "CTRL_NONE carries no log-weight: terminal / initial cost flags are not accepted");
  SD_TRY(check_dist(d->target, d->d));
  const int sc = d->target.kind == SDENG_DIST_NONE ? SC_NONE : in_loop_score(d->target.kind);
  if (sc < 0 || sc == SC_LOGREG) return fail(SDENG_E_UNSUPPORTED, "Langevin drift: no in-loop score kernel for target kind %d", d->target.kind);
  return select_kernel(p.k, SD_FAM_EULER, p.DT, sc);
}

// the drift-net step loop (k_simulate), or its low-latency split-tile twin
static int plan_sim(SimPlan& p) {
  const sdeng_desc* d = p.d;
  const int DT = p.DT;
  SD_TRY(check_net(d->net));
  if (p.in_slot) {
    p.sc = SC_REFSLOT;
    SD_TRY(check_lerp_prior(d));
  } else {
    SD_TRY(score_kind(d, p.sc));
  }
  const int sc = p.sc;
  int& rf = p.rf;
  if (d->ref.kind == SDENG_REF_GAUSS_DIAG || d->ref.kind == SDENG_REF_GMM_DIAG) {
    const int K = ref_components(d);
    rf = d->ref.kind == SDENG_REF_GAUSS_DIAG ? RF_GAUSS : ((K <= 4 && K * 2 * 16 * DT <= SD_REFTAB_FLOATS) ? RF_GMM : RF_GMM_BIG);
    if (K < 1 || !d->ref.means_init || !d->ref.vars_init) return fail(SDENG_E_INVALID, "reference: null means/vars or k < 1");
    if (use_mm(d, DT)) rf = RF_GMM_MM;
  } else if (d->ref.kind == SDENG_REF_GMM_FULL) {
    rf = RF_GMM_FULL;
    if (d->ref.k < 1 || !d->ref.means_init || !d->ref.vars_init || !d->ref.eigvecs)
      return fail(SDENG_E_INVALID, "full-covariance reference: null means / eigenvalues / eigenvectors or k < 1");
  } else if (d->ref.kind != SDENG_REF_NONE) {
    return fail(SDENG_E_UNSUPPORTED, "reference kind %d", d->ref.kind);
  }
  SD_TRY(check_dist(d->target, d->d));
  SD_TRY(check_dist(d->ref_dist, d->d));
  SD_TRY(check_dist(d->prior, d->d));
  const bool eubo = d->form == SDENG_FORM_EUBO, init_logp = d->flags & SDENG_FLAG_INIT_LOGP;
  if (init_logp && !eubo && d->prior.kind == SDENG_DIST_NONE) return fail(SDENG_E_INVALID, "FLAG_INIT_LOGP without a prior");
  if ((d->flags & SDENG_FLAG_TERM_REF) && d->ref_dist.kind == SDENG_DIST_NONE) return fail(SDENG_E_INVALID, "FLAG_TERM_REF without ref_dist");
  if ((d->flags & SDENG_FLAG_TERM_TARGET) && d->target.kind == SDENG_DIST_NONE) return fail(SDENG_E_INVALID, "FLAG_TERM_TARGET without target");
  if ((d->flags & SDENG_FLAG_REMOVE_REF) && (sc == SC_NONE || sc == SC_LOGREG || sc == SC_REFSLOT || rf == RF_NONE || rf == RF_GMM_MM || eubo))
    return fail(SDENG_E_UNSUPPORTED, "FLAG_REMOVE_REF (RemoveReferenceCtrl): forward forms with a Score / Lerp / CancelDrift control on a mixture or "
                                     "phi^4 target and a Gaussian / mixture reference (ctrl_kind %d, ref.kind %d, form %d)",
                d->net.ctrl_kind, d->ref.kind, d->form);
  if (eubo) {
    if (rf == RF_NONE && sc == SC_NONE)
      return fail(SDENG_E_UNSUPPORTED, "compute_eubo kernels: a reference drift, or no reference with a Score/LerpCtrl "
                                       "(ref.kind %d, ctrl_kind %d)", d->ref.kind, d->net.ctrl_kind);
    if (sc == SC_LOGREG) return fail(SDENG_E_UNSUPPORTED, "compute_eubo kernels: no logistic-regression control score");
    if (init_logp && d->prior.kind == SDENG_DIST_NONE) return fail(SDENG_E_INVALID, "FLAG_INIT_LOGP without a prior");
  } else if (sc == SC_LOGREG) {  // ScoreCtrl / LerpCtrl on a logistic-regression target (PIS, DDS, DIS on the Bayesian benchmarks)
    if (rf != RF_NONE) return fail(SDENG_E_UNSUPPORTED, "in-loop logistic-regression score together with a reference drift");
    if (DT > 4) return fail(SDENG_E_UNSUPPORTED, "in-loop logistic-regression score: d <= 64 (got %d)", d->d);
  }
  // defensive: use_mm keeps score controls and the noising form on the vector path, so no such instance is ever asked for
  if (rf == RF_GMM_MM && (sc != SC_NONE || eubo))
    return fail(SDENG_E_UNSUPPORTED, "matrix-pipe mixture reference: forward forms with a ClippedCtrl only");
  const bool pert = d->flags & (SDENG_FLAG_CTRL_NOISE | SDENG_FLAG_CTRL_DROPOUT);  // (forward forms only: plan_simulate checks)
  if (split_eligible(d, DT) && (rf == RF_NONE || rf == RF_GAUSS || rf == RF_GMM)) return select_kernel(p.k, SD_FAM_SPLIT, DT, rf, d->form, pert);
  return select_kernel(p.k, SD_FAM_SIM, DT, rf, sc, d->form, pert ? 2 : (d->noise_in || d->xs_out) ? 1 : 0);
}

static int plan_simulate(const sdeng_desc* d, SimPlan& p) {
  if (!d) return fail(SDENG_E_INVALID, "null descriptor");
  SD_TRY(check_abi(d));
  p.in_slot = d->target.kind == SDENG_DIST_GMM_FULL;
  if (p.in_slot) {
    SD_TRY(check_slot_target(d));
    slot_target(d, p.slot);
    d = &p.slot;
  }
  p.d = d;
  if (!make_layout(d, p.L)) return fail(SDENG_E_INVALID, "bad sizes: B=%d d=%d N=%d (need 1 <= d <= 128)", d->B, d->d, d->N);
  if (d->B == 0) return 0;
  if ((!d->coef && d->N > 0) || !d->x_out || !d->rnd_out) return fail(SDENG_E_INVALID, "null coef/x_out/rnd_out");
  if (!d->x_in) SD_TRY(check_x0_dist(d));
  if (static_cast<long long>(d->B) * d->d >= (1ll << 31)) return fail(SDENG_E_UNSUPPORTED, "B*d >= 2^31");
  if (d->form != SDENG_FORM_LIN && d->form != SDENG_FORM_EM && d->form != SDENG_FORM_CMCD && d->form != SDENG_FORM_EUBO &&
      d->form != SDENG_FORM_CMCD_EUBO)
    return fail(SDENG_E_INVALID, "unknown form %d", d->form);
  if ((d->flags & (SDENG_FLAG_CTRL_NOISE | SDENG_FLAG_CTRL_DROPOUT)) &&
      ((d->form != SDENG_FORM_LIN && d->form != SDENG_FORM_EM) || d->net.ctrl_kind == SDENG_CTRL_NONE))
    return fail(SDENG_E_UNSUPPORTED, "FLAG_CTRL_NOISE / FLAG_CTRL_DROPOUT: forward forms (LIN / EM) with a drift net only (form %d, ctrl_kind %d)",
                d->form, d->net.ctrl_kind);
  p.DT = tiles_of(d);
  p.rf = RF_NONE;
  p.sc = SC_NONE;
  if (d->form == SDENG_FORM_CMCD || d->form == SDENG_FORM_CMCD_EUBO) return plan_cmcd(p);
  if (d->net.ctrl_kind == SDENG_CTRL_NONE) return plan_euler(p);
  return plan_sim(p);
}

// ---- sdeng_simulate: phase 3 --------------------------------------------------------------------------
static int run_cmcd(const SimPlan& p, const sdeng_desc* d, float* ws, SimArgs& a, hipStream_t s) {
  const Layout& L = p.L;
  const int DT = p.DT, dpad = 16 * DT;
  SD_TRY(prepare_net(d, L, ws, DT, a, s, d->N + 1, false, 0.0f));
  DistDev target, prior;
  SD_TRY(build_dist(d->target, d->d, dpad, ws + L.target, target, s));
  SD_TRY(build_dist(d->prior, d->d, dpad, ws + L.prior, prior, s));
  CmcdArgs c;
  memset(&c, 0, sizeof(c));
  float* prec = ws + L.cmcd;
  if (d->target.kind == SDENG_DIST_LOGREG) SD_TRY(prepare_logreg(d, L, ws, DT, a, s, &prec));
  float* locp = prec + align64(sd_image_floats(DT, DT));
  if (d->prior.kind == SDENG_DIST_GAUSS_FULL) {
    PackJobs pk;  // the precision, unscaled, with loc as its padded "bias"
    pk.njobs = 0;
    with_bias(add_pack_job(pk, d->prior.scale, d->d, d->d, d->d, false, DT, sd_kb(DT), prec), d->prior.loc, locp, 16 * DT);
    SD_HIP(sd_launch_pack_images(pk, s));
    c.prec_pack = prec; c.prior_loc = locp;
  } else if (d->prior.kind == SDENG_DIST_ISO_GAUSS) {
    c.iso_loc = d->prior.p0; c.inv_iso_var = 1.0f / d->prior.p3;
  }
  const bool eubo = d->form == SDENG_FORM_CMCD_EUBO;
  if (eubo) {  // rnd0 = -log pi~(x_in)   (losses/oc.py:779)
    SD_HIP(hipMemsetAsync(ws + L.rnd_init, 0, sizeof(float) * d->B, s));
    SD_TRY(terminal(d, dpad, target, target, false, true, d->x_in, ws + L.rnd_init, s));
  } else {     // rnd0 = log p_prior(x0)
    SD_TRY(dist_eval(prior, d->B, d->d, dpad, d->x_in, ws + L.rnd_init, nullptr, s));
  }
  a.rnd_init = ws + L.rnd_init;
  a.cmcd_g = d->cmcd_g; a.cmcd_clip = d->cmcd_clip;
  a.target = target; a.prior = prior;
  c.s = a;
  SD_TRY(launch_timed(d, p.k, &c, s));
  // terminal: -log pi~(x_N)  (:752), or for the noising loop + log p_prior(x_noised)  (:825)
  if (eubo) return terminal(d, dpad, prior, prior, true, false, d->x_out, d->rnd_out, s);
  return terminal(d, dpad, target, target, false, true, d->x_out, d->rnd_out, s);
}

static int run_euler(const SimPlan& p, const sdeng_desc* d, float* ws, SimArgs& a, hipStream_t s) {
  SD_TRY(build_dist(d->target, d->d, 16 * p.DT, ws + p.L.target, a.target, s));
  a.clip_score = d->net.clip_score;
  return launch_timed(d, p.k, &a, s);
}

// reference drift tables of every step, and the reference fields of the step loop's arguments
static int prepare_ref(const SimPlan& p, const sdeng_desc* d, float* ws, SimArgs& a, hipStream_t s) {
  const Layout& L = p.L;
  const int DT = p.DT, dpad = 16 * DT, K = ref_components(d), rf = p.rf;
  if (rf == RF_NONE) return 0;
  a.ref_k = K;
  a.ref_tab = ws + L.ref_tab; a.ref_consts = ws + L.ref_consts;
  a.ref_c1 = half_d_log_2pi(d->d);
  if (rf == RF_GMM_FULL) {
    if (d->N > 0) {
      RefFullArgs r;
      r.K = K; r.d = d->d; r.dpad = dpad; r.NT = DT; r.coef = p.in_slot ? nullptr : d->coef;  // a target does not diffuse
      r.means = d->ref.means_init; r.eigvals = d->ref.vars_init; r.eigvecs = d->ref.eigvecs; r.weights = d->ref.weights;
      r.images = ws + L.ref_tab; r.means_out = ws + L.ref_mean; r.consts = ws + L.ref_consts;
      SD_HIP(sd_launch_ref_full_tables(r, d->N, s));
    }
    a.ref_mean = ws + L.ref_mean;
    a.ref_share = (sd_full_piece_floats(DT) / 256 + SD_WAVES - 1) / SD_WAVES;
    return 0;
  }
  if (rf == RF_GMM_MM) {
    const int kt = (K + 15) / 16;
    if (d->N > 0) {
      RefMMArgs r;
      r.K = K; r.d = d->d; r.dpad = dpad; r.NT = DT; r.kt = kt; r.coef = d->coef;
      r.means = d->ref.means_init; r.vars = d->ref.vars_init; r.weights = d->ref.weights;
      r.images = ws + L.ref_tab; r.centre = ws + L.ref_mean; r.consts = ws + L.ref_consts;
      r.same_var = ws + L.ref_consts + static_cast<size_t>(d->N) * 64;  // the slot behind the per-step constants (make_layout: N * 64 + 1)
      SD_HIP(sd_launch_ref_mm_tables(r, d->N, s));
    }
    a.ref_kc = kt;
    a.ref_mean = ws + L.ref_mean;
    a.ref_share = (mm_piece(K, DT) / 256 + SD_WAVES - 1) / SD_WAVES;
    return 0;
  }
  if (d->N > 0) {
    RefTabArgs r;
    r.K = K; r.d = d->d; r.dpad = dpad; r.coef = d->coef;
    r.means = d->ref.means_init; r.vars = d->ref.vars_init; r.weights = rf != RF_GAUSS ? d->ref.weights : nullptr;
    r.tab = ws + L.ref_tab; r.consts = ws + L.ref_consts;
    r.same_var = ws + L.ref_consts + static_cast<size_t>(d->N) * K * 2;
    r.centred = (rf == RF_GMM && p.k.fam != SD_FAM_SPLIT) ? 1 : 0;  // the split-tile kernel reads the plain (mean, 1/var) table
    SD_HIP(sd_launch_ref_tables(r, d->N, s));
  }
  a.ref_same_var = ws + L.ref_consts + static_cast<size_t>(d->N) * K * 2;
  if (rf == RF_GMM_BIG) {
    // workgroup-shared table copy: two LDS buffers of whole 1 KiB chunks behind the drift-net weights (160 KiB of
    // LDS per workgroup), each holding a piece of kc components -- the whole table when it fits, otherwise the
    // fewest equal pieces that do.  SDENG_REF_SHARE=0 keeps the streamed-from-L2 path (A/B measurements).
    static const bool allow = [] { const char* e = getenv("SDENG_REF_SHARE"); return !(e && e[0] == '0'); }();
    const int cap = std::min(share_room(DT), sd_share_buf_floats(SD_SHARE_MAX)) / 256 * 256;  // floats per buffer
    const int kc_max = cap / (2 * dpad);
    if (allow && kc_max >= 1) {
      const int nch = (K + kc_max - 1) / kc_max;
      const int kc = (K + nch - 1) / nch;
      const int chunks = (kc * 2 * dpad + 255) / 256;
      a.ref_share = (chunks + SD_WAVES - 1) / SD_WAVES;
      a.ref_kc = kc;
    }
  }
  return 0;
}

static int run_sim(const SimPlan& p, const sdeng_desc* d, float* ws, SimArgs& a, hipStream_t s) {
  const Layout& L = p.L;
  const int DT = p.DT, dpad = 16 * DT;
  SD_TRY(prepare_net(d, L, ws, DT, a, s, d->N, false, 0.0f));
  SD_TRY(prepare_ref(p, d, ws, a, s));
  DistDev target, ref_dist, prior;
  SD_TRY(build_dist(d->target, d->d, dpad, ws + L.target, target, s));
  SD_TRY(build_dist(d->ref_dist, d->d, dpad, ws + L.ref_dist, ref_dist, s));
  SD_TRY(build_dist(d->prior, d->d, dpad, ws + L.prior, prior, s));
  a.target = target;
  a.prior = prior;
  const bool eubo = d->form == SDENG_FORM_EUBO;
  const bool tr = d->flags & SDENG_FLAG_TERM_REF, tt = d->flags & SDENG_FLAG_TERM_TARGET;
  // initial cost (EUBO: the prior log-density is added at the END, on the noised samples: losses/oc.py:1032)
  if ((d->flags & SDENG_FLAG_INIT_LOGP) && !eubo) {
    SD_TRY(dist_eval(prior, d->B, d->d, dpad, d->x_in, ws + L.rnd_init, nullptr, s));
    a.rnd_init = ws + L.rnd_init;
  }
  if (eubo && (tr || tt)) {  // cost at the data distribution: rnd0 = [log p_ref(x_in)] - log pi~(x_in)   (losses/oc.py:322, :536, :1003)
    SD_HIP(hipMemsetAsync(ws + L.rnd_init, 0, sizeof(float) * d->B, s));
    SD_TRY(terminal(d, dpad, ref_dist, target, tr, tt, d->x_in, ws + L.rnd_init, s));
    a.rnd_init = ws + L.rnd_init;
  }
  if (p.sc == SC_LOGREG) {  // design matrix in LDS
    float* unused;
    SD_TRY(prepare_logreg(d, L, ws, DT, a, s, &unused));
  }
  SD_TRY(launch_timed(d, p.k, &a, s));
  // terminal cost; the noising loop adds log p_prior(x_noised)
  if (!eubo && (tr || tt)) SD_TRY(terminal(d, dpad, ref_dist, target, tr, tt, d->x_out, d->rnd_out, s));
  if (eubo && (d->flags & SDENG_FLAG_INIT_LOGP)) SD_TRY(terminal(d, dpad, prior, prior, true, false, d->x_out, d->rnd_out, s));
  return 0;
}

extern "C" int sdeng_simulate(const sdeng_desc* desc, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  SimPlan p;
  int rc = plan_simulate(desc, p);
  if (rc || desc->B == 0) return rc;
  const sdeng_desc* d = p.d;
  if (!d->workspace || d->workspace_bytes < p.L.total * sizeof(float))
    return fail(SDENG_E_WORKSPACE, "workspace %zu bytes, need %zu", d->workspace_bytes, p.L.total * sizeof(float));
  float* ws = static_cast<float*>(d->workspace);
  SimArgs a;
  memset(&a, 0, sizeof(a));
  a.form = d->form; a.flags = d->flags;
  a.B = d->B; a.d = d->d; a.N = d->N;
  a.particle0 = d->particle0;
  const Seed seed = split_seed(d->seed);
  a.seed_lo = seed.lo; a.seed_hi = seed.hi;
  a.coef = d->coef; a.x_in = d->x_in; a.x_out = d->x_out; a.rnd_out = d->rnd_out;
  a.xs_out = d->xs_out; a.noise_in = d->noise_in;
  a.trash = ws + p.L.trash;
  a.ntiles = (d->B + 15) / 16;
  // x0 drawn by the engine: k_sample_x0 writes it (workspace, or the caller's x0_out), then everything runs as if the caller had passed
  // it.  A twin of the step-loop kernel that drew x0 in registers was built and dropped: same instruction count, but its loop came out
  // of the register allocator 4 % slower on cfg 2 and 1.3 % on cfg 3 (profiles/r02_x0_draw_ab.log); the sampler kernel costs 0.2 %.
  sdeng_desc dm;
  if (!d->x_in) {
    float* x0 = d->x0_out ? d->x0_out : ws + p.L.x0;
    SD_HIP(sd_launch_sample_x0(d->x0_dist, seed.lo, seed.hi, d->particle0, d->B, d->d, x0, s));
    dm = *d;
    dm.x_in = x0;
    d = &dm;
    a.x_in = x0;
  }
  if (p.k.fam == SD_FAM_CMCD) return run_cmcd(p, d, ws, a, s);
  if (p.k.fam == SD_FAM_EULER) return run_euler(p, d, ws, a, s);
  return run_sim(p, d, ws, a, s);
}

extern "C" int sdeng_sample_x0(const sdeng_dist* dist, uint64_t seed, int64_t particle0, int32_t B, int32_t d, float* out, void* stream) {
  if (!dist || !out || B < 0 || d < 1 || d > 128) return fail(SDENG_E_INVALID, "bad argument");
  if (B == 0) return 0;
  sdeng_desc tmp;
  memset(&tmp, 0, sizeof(tmp));
  tmp.x0_dist = *dist;
  SD_TRY(check_x0_dist(&tmp));
  const Seed sd = split_seed(seed);
  SD_HIP(sd_launch_sample_x0(*dist, sd.lo, sd.hi, particle0, B, d, out, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int sdeng_ctrl_forward(const sdeng_desc* d, float t_net, float score_gain, float lerp_w, const float* x, float* u_out,
                                  void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!d || !x || !u_out) return fail(SDENG_E_INVALID, "null argument");
  Layout L;
  if (!make_layout(d, L)) return fail(SDENG_E_INVALID, "bad sizes");
  const bool ws_ok = d->workspace && d->workspace_bytes >= L.total * sizeof(float);
  if (d->B == 0) return ws_ok ? 0 : fail(SDENG_E_WORKSPACE, "workspace too small");
  const int DT = tiles_of(d), dpad = 16 * DT;
  int sc;
  KernelKey k;
  SD_TRY(check_net(d->net));
  SD_TRY(score_kind(d, sc));
  SD_TRY(check_dist(d->target, d->d));
  SD_TRY(check_dist(d->prior, d->d));
  if (sc == SC_LOGREG) return fail(SDENG_E_UNSUPPORTED, "ctrl_forward: no in-loop logistic-regression score (the step loop's only)");
  SD_TRY(select_kernel(k, SD_FAM_CTRL, DT, sc));
  if (!ws_ok) return fail(SDENG_E_WORKSPACE, "workspace too small");
  float* ws = static_cast<float*>(d->workspace);
  SimArgs a;
  memset(&a, 0, sizeof(a));
  a.B = d->B; a.d = d->d; a.N = 1;
  a.x_in = x; a.x_out = u_out;
  a.trash = ws + L.trash;
  a.ntiles = (d->B + 15) / 16;
  SD_TRY(prepare_net(d, L, ws, DT, a, s, 1, true, t_net));
  SD_TRY(build_dist(d->target, d->d, dpad, ws + L.target, a.target, s));
  SD_TRY(build_dist(d->prior, d->d, dpad, ws + L.prior, a.prior, s));
  // one-row coefficient table for (score_gain, lerp_w), kept in the (unused) log Z slot
  float host_coef[SDENG_NCOEF] = {0};
  host_coef[0] = t_net; host_coef[7] = score_gain; host_coef[8] = lerp_w;
  float* dev_coef = ws + L.logz;
  SD_HIP(hipMemcpyAsync(dev_coef, host_coef, sizeof(host_coef), hipMemcpyHostToDevice, s));
  a.coef = dev_coef;
  SD_HIP(k.fn(&a, s));
  return 0;
}

// ---- fused forward + backward of the drift net over N * B rows (training direction) ---------------------------------------------
struct VjpLayout {
  size_t wt, temb, trash, total;  // (the forward image at 0)
};
static VjpLayout vjp_layout(int DT, int n_times) {
  VjpLayout v;
  size_t o = align64(sd_pack_floats(DT));
  v.wt = o; o += align64(sd_lds_weight_floats(DT));
  v.temb = o; o += align64(static_cast<size_t>(n_times) * SD_H);
  v.trash = o; o += align64(SD_WAVES_MAX * 64 * 4);
  v.total = o;
  return v;
}
extern "C" size_t sdeng_ctrl_vjp_workspace_bytes(int32_t d, int32_t n_times) {
  if (d < 1 || d > 128 || n_times < 1) return 0;
  return vjp_layout(tiles_exact(d), n_times).total * sizeof(float);
}
// The part the three training entry points share, after their own validation and kernel selection: the workspace check (no HIP call
// before it), both weight images at the front of the workspace (`pack` = 0: the caller's are still there), the time embeddings of
// n_times rows of coef -- and the clipped score model's at `stheta_off` when the control has one --, and the VjpArgs of rows_per_time
// rows per time with the seven per-row outputs.  V is the head of the caller's own layout of `total` floats: nothing moves.
struct VjpOut { float *a0, *a1, *a2, *d0, *d1, *d2, *dout; };
static int prepare_vjp(const sdeng_desc* d, int DT, const VjpLayout& V, size_t total, bool pack, int n_times, int rows_per_time, const float* x,
                       const VjpOut& o, size_t stheta_off, const float** stheta, VjpArgs& v, hipStream_t s) {
  const size_t need = total * sizeof(float);
  if (!d->workspace || d->workspace_bytes < need) return fail(SDENG_E_WORKSPACE, "workspace %zu bytes, need %zu", d->workspace_bytes, need);
  float* ws = static_cast<float*>(d->workspace);
  if (pack) SD_TRY(pack_net(d, DT, ws, ws + V.wt, s));
  SD_TRY(embed_times(d, n_times, false, 0.0f, ws + V.temb, ws + stheta_off, stheta, s));
  v.M = n_times * rows_per_time; v.B = rows_per_time; v.d = d->d; v.N = n_times;
  v.x = x; v.wpack = ws; v.wpack_t = ws + V.wt; v.temb = ws + V.temb;
  v.clip_model = d->net.clip_model;
  v.a0 = o.a0; v.a1 = o.a1; v.a2 = o.a2; v.d0 = o.d0; v.d1 = o.d1; v.d2 = o.d2; v.dout = o.dout;
  v.trash = ws + V.trash;
  return 0;
}
extern "C" int sdeng_ctrl_vjp(const sdeng_desc* d, int32_t n_times, int32_t rows_per_time, const float* x, const float* cot, float* a0,
                              float* a1, float* a2, float* d0, float* d1, float* d2, float* dout, float* gx, float* u_out, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!d || !x) return fail(SDENG_E_INVALID, "null argument");
  if (cot && (!a0 || !a1 || !a2 || !d0 || !d1 || !d2 || !dout)) return fail(SDENG_E_INVALID, "backward pass: every per-row output is required");
  if (!cot && !u_out) return fail(SDENG_E_INVALID, "nothing to compute: no cotangent and no u_out");
  SD_TRY(check_abi(d));
  if (d->d < 1 || d->d > 128 || n_times < 1 || rows_per_time < 1 || !d->coef) return fail(SDENG_E_INVALID, "bad sizes (1 <= d <= 128, n_times, rows_per_time >= 1) or null coef");
  if (d->net.ctrl_kind != SDENG_CTRL_CLIPPED) return fail(SDENG_E_UNSUPPORTED, "ctrl_vjp: ClippedCtrl around the FourierMLP (ctrl_kind %d given)", d->net.ctrl_kind);
  const long long M = static_cast<long long>(n_times) * rows_per_time;
  if (M * d->d >= (1ll << 31)) return fail(SDENG_E_UNSUPPORTED, "rows * d >= 2^31");
  SD_TRY(check_net(d->net));
  const int DT = tiles_exact(d->d);
  KernelKey k;
  SD_TRY(select_kernel(k, SD_FAM_VJP, DT, gx ? 1 : 0));
  const VjpLayout V = vjp_layout(DT, n_times);
  VjpArgs a;
  memset(&a, 0, sizeof(a));
  const float* no_stheta;  // (ClippedCtrl: no score model)
  // (a caller stepping through the times one by one packs once: the images stay valid in the workspace)
  SD_TRY(prepare_vjp(d, DT, V, V.total, !(d->flags & SDENG_FLAG_REUSE_PACK), n_times, rows_per_time, x, {a0, a1, a2, d0, d1, d2, dout}, 0, &no_stheta, a, s));
  a.cot = cot; a.gx = gx; a.u_out = u_out;
  a.ntiles = static_cast<int>((M + 15) / 16);
  SD_HIP(k.fn(&a, s));
  return 0;
}

// ---- KL training: the adjoint of the step loop (grad_kernel.hpp k_kl_adjoint) ------------------------------------------------------
struct AdjLayout {
  VjpLayout v;
  size_t tab, consts, stheta, target, total;
};
static AdjLayout adjoint_layout(const sdeng_desc* d, int DT) {
  AdjLayout A;
  A.v = vjp_layout(DT, d->N);
  size_t o = A.v.total;
  const int K = ref_components(d);
  A.tab = o; o += align64(static_cast<size_t>(d->N) * K * 2 * 16 * DT);
  A.consts = o; o += align64(static_cast<size_t>(d->N) * K * 2 + 1);
  A.stheta = o; o += align64(static_cast<size_t>(d->N));
  A.target = o; o += dist_floats(d->target, 16 * DT);
  A.total = o;
  return A;
}
static int check_adjoint(const sdeng_desc* d, bool ext_score) {
  if (!d) return fail(SDENG_E_INVALID, "null descriptor");
  SD_TRY(check_abi(d));
  if (d->d < 1 || d->d > 128 || d->N < 1 || d->B < 1 || !d->coef) return fail(SDENG_E_INVALID, "bad sizes (1 <= d <= 128, N, B >= 1) or null coef");
  if (d->form != SDENG_FORM_LIN && d->form != SDENG_FORM_EM) return fail(SDENG_E_UNSUPPORTED, "kl_adjoint: forward forms LIN / EM (form %d)", d->form);
  if (d->net.ctrl_kind != SDENG_CTRL_CLIPPED &&
      !(score_like(d->net.ctrl_kind) && (ext_score || d->target.kind == SDENG_DIST_GMM_DIAG || d->target.kind == SDENG_DIST_PHI4)))
    return fail(SDENG_E_UNSUPPORTED, "kl_adjoint: ClippedCtrl, or Score / Lerp / CancelDrift control on a diagonal mixture / phi^4 target (ctrl_kind %d, "
                                     "target kind %d)", d->net.ctrl_kind, d->target.kind);
  SD_TRY(check_lerp_prior(d));
  if (d->target.kind == SDENG_DIST_CHECKERBOARD || d->prior.kind == SDENG_DIST_CHECKERBOARD)
    return fail(SDENG_E_UNSUPPORTED, "kl_adjoint: no adjoint for a checkerboard target (KL training takes the per-step path)");
  if (d->ref.kind != SDENG_REF_NONE && d->ref.kind != SDENG_REF_GAUSS_DIAG && d->ref.kind != SDENG_REF_GMM_DIAG)
    return fail(SDENG_E_UNSUPPORTED, "kl_adjoint: no reference, or a diagonal Gaussian / mixture reference (ref.kind %d)", d->ref.kind);
  if (d->ref.kind != SDENG_REF_NONE && ((d->ref.kind == SDENG_REF_GMM_DIAG && d->ref.k < 1) || !d->ref.means_init || !d->ref.vars_init))
    return fail(SDENG_E_INVALID, "reference: null means/vars or k < 1");
  if (static_cast<long long>(d->N) * d->B * d->d >= (1ll << 31)) return fail(SDENG_E_UNSUPPORTED, "N * B * d >= 2^31");
  return check_net(d->net);
}
extern "C" size_t sdeng_kl_adjoint_workspace_bytes(const sdeng_desc* d) {
  if (!d || d->d < 1 || d->d > 128 || d->N < 1) return 0;
  return adjoint_layout(d, tiles_exact(d->d)).total * sizeof(float);
}
extern "C" int sdeng_kl_adjoint(const sdeng_desc* d, const sdeng_adjoint* adj, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  SD_TRY(check_adjoint(d, adj && adj->score));
  if (!adj || !adj->xs || !adj->w || !adj->lam_in || !adj->a0 || !adj->a1 || !adj->a2 || !adj->d0 || !adj->d1 || !adj->d2 || !adj->dout)
    return fail(SDENG_E_INVALID, "kl_adjoint: null states / weights / lambda_N / per-row outputs");
  const bool ito = d->flags & SDENG_FLAG_ITO;
  if (ito && !adj->noise) return fail(SDENG_E_INVALID, "kl_adjoint: FLAG_ITO needs the normals of the trajectory");
  const bool score = d->net.ctrl_kind != SDENG_CTRL_CLIPPED;
  if (score && !adj->dst) return fail(SDENG_E_INVALID, "kl_adjoint: a score control needs the dst output");
  if (score && !adj->score) SD_TRY(check_dist(d->target, d->d));
  const int has_score = !score ? ADJ_NONE : adj->score ? ADJ_EXT : (d->target.kind == SDENG_DIST_PHI4 ? ADJ_PHI4 : ADJ_GMM);
  const int DT = tiles_exact(d->d), dpad = 16 * DT;
  KernelKey k;
  SD_TRY(select_kernel(k, SD_FAM_ADJ, DT, has_score));
  const AdjLayout A = adjoint_layout(d, DT);
  AdjArgs a;
  memset(&a, 0, sizeof(a));
  SD_TRY(prepare_vjp(d, DT, A.v, A.total, true, d->N, d->B, adj->xs, {adj->a0, adj->a1, adj->a2, adj->d0, adj->d1, adj->d2, adj->dout}, A.stheta, &a.stheta,
                     a.v, s));
  float* ws = static_cast<float*>(d->workspace);
  if (d->ref.kind != SDENG_REF_NONE) {  // the noised reference of every step: (mean, 1/var) tables + logit constants, as the step loop reads them
    const int K = ref_components(d);
    RefTabArgs r;
    r.K = K; r.d = d->d; r.dpad = dpad; r.coef = d->coef;
    r.means = d->ref.means_init; r.vars = d->ref.vars_init; r.weights = d->ref.kind == SDENG_REF_GMM_DIAG ? d->ref.weights : nullptr;
    r.tab = ws + A.tab; r.consts = ws + A.consts;
    r.same_var = ws + A.consts + static_cast<size_t>(d->N) * K * 2;
    r.centred = 0;
    SD_HIP(sd_launch_ref_tables(r, d->N, s));
    a.ref_tab = ws + A.tab; a.ref_consts = ws + A.consts; a.ref_k = K;
    a.ref_c1 = half_d_log_2pi(d->d);
  }
  a.has_score = has_score;
  if (score) {
    a.score_ext = adj->score;
    if (!adj->score) SD_TRY(build_dist(d->target, d->d, dpad, ws + A.target, a.target, s));
    a.scale_score = d->net.scale_score; a.clip_score = d->net.clip_score;
    a.ctrl_kind = d->net.ctrl_kind;
    a.prior_loc = d->prior.p0; a.prior_scale = d->net.ctrl_kind == SDENG_CTRL_LERP ? d->prior.p1 : 1.0f;
    a.score_detached = adj->detach_score ? 1 : 0;
    a.dst = adj->dst;
  }
  a.coef = d->coef; a.noise = ito ? adj->noise : nullptr; a.w = adj->w; a.lam_in = adj->lam_in; a.lam_out = adj->lam_out;
  a.lin = d->form == SDENG_FORM_LIN ? 1 : 0;
  a.ntiles_b = (d->B + 15) / 16;
  SD_HIP(k.fn(&a, s));
  return 0;
}

// ---- KL training of CMCD: the adjoint over the N + 1 evaluation points (cmcd_adjoint_kernel.hpp k_cmcd_kl_adjoint) -------------------
struct CmcdAdjLayout {
  VjpLayout v;
  size_t stheta, target, prior, total;
};
static CmcdAdjLayout cmcd_adjoint_layout(const sdeng_desc* d, int DT) {
  CmcdAdjLayout A;
  A.v = vjp_layout(DT, d->N + 1);
  size_t o = A.v.total;
  A.stheta = o; o += align64(static_cast<size_t>(d->N) + 1);
  A.target = o; o += dist_floats(d->target, 16 * DT);
  A.prior = o; o += dist_floats(d->prior, 16 * DT);
  A.total = o;
  return A;
}
static int check_cmcd_adjoint(const sdeng_desc* d, bool ext_score) {
  if (!d) return fail(SDENG_E_INVALID, "null descriptor");
  SD_TRY(check_abi(d));
  if (d->d > 128) return fail(SDENG_E_UNSUPPORTED, "cmcd_kl_adjoint: d <= 128 (got %d)", d->d);
  if (d->d < 1 || d->N < 1 || d->B < 1 || !d->coef) return fail(SDENG_E_INVALID, "bad sizes (1 <= d, N, B >= 1) or null coef");
  if (d->net.ctrl_kind != SDENG_CTRL_CLIPPED && d->net.ctrl_kind != SDENG_CTRL_SCORE)
    return fail(SDENG_E_UNSUPPORTED, "cmcd_kl_adjoint: ClippedCtrl or ScoreCtrl (ctrl_kind %d)", d->net.ctrl_kind);
  if (d->prior.kind == SDENG_DIST_GAUSS_FULL)
    return fail(SDENG_E_UNSUPPORTED, "cmcd_kl_adjoint: no adjoint for a full-covariance prior (KL training takes the per-step path)");
  if (d->prior.kind != SDENG_DIST_ISO_GAUSS && d->prior.kind != SDENG_DIST_GAUSS_DIAG)
    return fail(SDENG_E_UNSUPPORTED, "cmcd_kl_adjoint: prior must be ISO_GAUSS or GAUSS_DIAG (kind %d)", d->prior.kind);
  switch (d->target.kind) {
    case SDENG_DIST_GAUSS_FULL:
    case SDENG_DIST_GMM_FULL:
      return fail(SDENG_E_UNSUPPORTED, "cmcd_kl_adjoint: no adjoint for a full-covariance target (kind %d)", d->target.kind);
    case SDENG_DIST_RINGS:
      return fail(SDENG_E_UNSUPPORTED, "cmcd_kl_adjoint: no adjoint for a rings target (KL training takes the per-step path)");
    case SDENG_DIST_CHECKERBOARD:
      return fail(SDENG_E_UNSUPPORTED, "cmcd_kl_adjoint: no adjoint for a checkerboard target (KL training takes the per-step path)");
    case SDENG_DIST_LOGREG:
      if (!ext_score) return fail(SDENG_E_INVALID, "cmcd_kl_adjoint: a logistic-regression target needs the score of every row (adj->score)");
      if (d->d > 64) return fail(SDENG_E_UNSUPPORTED, "cmcd_kl_adjoint: logistic regression with d <= 64 (got %d), as its step loop", d->d);
      break;
    case SDENG_DIST_GMM_DIAG:
    case SDENG_DIST_GAUSS_DIAG:
    case SDENG_DIST_PHI4:
      if (ext_score) return fail(SDENG_E_INVALID, "cmcd_kl_adjoint: adj->score is for targets with a graph-less score (LOGREG); kind %d has a closed form", d->target.kind);
      break;
    default:
      return fail(SDENG_E_UNSUPPORTED, "cmcd_kl_adjoint: target must be GMM_DIAG, GAUSS_DIAG, PHI4 or LOGREG (kind %d)", d->target.kind);
  }
  if ((static_cast<long long>(d->N) + 1) * d->B * d->d >= (1ll << 31)) return fail(SDENG_E_UNSUPPORTED, "(N + 1) * B * d >= 2^31");
  SD_TRY(check_net(d->net));
  SD_TRY(check_dist(d->prior, d->d));
  return ext_score ? 0 : check_dist(d->target, d->d);
}
extern "C" size_t sdeng_cmcd_kl_adjoint_workspace_bytes(const sdeng_desc* d) {
  if (!d || d->d < 1 || d->d > 128 || d->N < 1) return 0;
  return cmcd_adjoint_layout(d, tiles_exact(d->d)).total * sizeof(float);
}
extern "C" int sdeng_cmcd_kl_adjoint(const sdeng_desc* d, const sdeng_cmcd_adjoint* adj, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  SD_TRY(check_cmcd_adjoint(d, adj && adj->score));
  if (!adj || !adj->xs || !adj->cbar || !adj->w || !adj->lam_in || !adj->a0 || !adj->a1 || !adj->a2 || !adj->d0 || !adj->d1 || !adj->d2 || !adj->dout)
    return fail(SDENG_E_INVALID, "cmcd_kl_adjoint: null states / costs / weights / lam_in / per-row outputs");
  const bool score = d->net.ctrl_kind == SDENG_CTRL_SCORE;
  if (score && !adj->dst) return fail(SDENG_E_INVALID, "cmcd_kl_adjoint: a ScoreCtrl needs the dst output");
  const int tgt = adj->score ? CADJ_EXT : (d->target.kind == SDENG_DIST_PHI4 ? CADJ_PHI4 : CADJ_GMM);
  const int DT = tiles_exact(d->d), dpad = 16 * DT;
  KernelKey k;
  SD_TRY(select_kernel(k, SD_FAM_CADJ, DT, tgt));
  const CmcdAdjLayout A = cmcd_adjoint_layout(d, DT);
  CmcdAdjArgs a;
  memset(&a, 0, sizeof(a));
  SD_TRY(prepare_vjp(d, DT, A.v, A.total, true, d->N + 1, d->B, adj->xs, {adj->a0, adj->a1, adj->a2, adj->d0, adj->d1, adj->d2, adj->dout}, A.stheta,
                     &a.stheta, a.v, s));
  float* ws = static_cast<float*>(d->workspace);
  if (tgt != CADJ_EXT) SD_TRY(build_dist(d->target, d->d, dpad, ws + A.target, a.target, s));
  if (d->prior.kind == SDENG_DIST_GAUSS_DIAG) {
    DistDev prior;
    SD_TRY(build_dist(d->prior, d->d, dpad, ws + A.prior, prior, s));
    a.prior_tab = prior.tab;
  } else {
    a.iso_loc = d->prior.p0; a.inv_iso_var = 1.0f / d->prior.p3;  // (as the step loop, run_cmcd)
  }
  a.g = d->cmcd_g; a.clip = d->cmcd_clip;
  a.has_score = score ? 1 : 0;
  if (score) {
    a.scale_score = d->net.scale_score; a.clip_score = d->net.clip_score;
    a.score_detached = adj->detach_score ? 1 : 0;
    a.dst = adj->dst;
  }
  a.score_ext = adj->score;
  a.coef = d->coef; a.cbar = adj->cbar; a.w = adj->w; a.lam_in = adj->lam_in; a.lam_out = adj->lam_out;
  a.steps = d->N;
  a.ntiles_b = (d->B + 15) / 16;
  SD_HIP(k.fn(&a, s));
  return 0;
}

extern "C" int sdeng_dist_eval(const sdeng_dist* dist, int32_t B, int32_t d, const float* x, float* logp_out, float* score_out,
                               void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!dist || !x || d < 1 || B < 0) return fail(SDENG_E_INVALID, "bad argument");
  if (d > 255) return fail(SDENG_E_UNSUPPORTED, "dist_eval: d <= 255 (rows are staged through LDS), got %d", d);
  if (B == 0) return 0;
  const int dpad = pad16(d);
  const size_t need = dist_floats(*dist, dpad) * sizeof(float);
  if (need > 0 && (!workspace || workspace_bytes < need)) return fail(SDENG_E_WORKSPACE, "workspace %zu bytes, need %zu", workspace_bytes, need);
  DistDev dd;
  SD_TRY(build_dist(*dist, d, dpad, static_cast<float*>(workspace), dd, s));
  return dist_eval(dd, B, d, dpad, x, logp_out, score_out, s);
}

// ---- local moves in one launch: Langevin moves of the annealed samplers and random-walk Metropolis moves of the
// learned-reference data set (experiments/benchmark_utils.py:281-290).  One host path; RWMH has no prior, gradient, weights or ULA flag.
static size_t moves_workspace_bytes(const sdeng_dist* prior, const sdeng_dist* target, int32_t d) {
  if (!target || d < 1) return 0;
  const int dpad = pad16(d);
  return (dist_floats(*target, dpad) + (prior ? dist_floats(*prior, dpad) : 0) + 64) * sizeof(float);
}
static int run_moves(int move, const char* who, const sdeng_dist* prior, const sdeng_dist* target, int32_t B, int32_t d, int32_t n_moves,
                     int32_t keep_from, int32_t unadjusted, float target_acceptance, const float* t, float* x, float* lp, float* grad,
                     float* step, const float* z, const float* u, uint64_t seed, int64_t chain0, float* samples, float* acc_sum,
                     float* acc_last, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool langevin = move == SD_MOVE_LANGEVIN;
  if (!target || !x || !lp || (langevin && !grad) || !step || B < 0 || d < 1 || n_moves < 0 || keep_from < 0 || keep_from > n_moves)
    return fail(SDENG_E_INVALID, "%s: bad argument", who);
  if (target->kind == SDENG_DIST_NONE) return fail(SDENG_E_INVALID, "%s: no target distribution", who);
  if (d > 255) return fail(SDENG_E_UNSUPPORTED, "%s: d <= 255 (chain rows live in LDS), got %d", who, d);
  if ((z == nullptr) != (u == nullptr) && !unadjusted)  // (unadjusted moves read no uniforms)
    return fail(SDENG_E_INVALID, "%s: inject both the normals and the uniforms, or neither (unadjusted moves: the normals alone)", who);
  if (langevin && (target->kind == SDENG_DIST_CHECKERBOARD || (prior && prior->kind == SDENG_DIST_CHECKERBOARD)))
    return fail(SDENG_E_UNSUPPORTED, "%s: no moves on a checkerboard (its log-density is -inf on a set of positive mass)", who);
  const bool has_prior = prior && prior->kind != SDENG_DIST_NONE;
  SD_TRY(check_dist(*target, d));
  if (has_prior) SD_TRY(check_dist(*prior, d));
  if (B == 0 || n_moves == 0) return 0;
  const int dpad = pad16(d);
  const size_t need = moves_workspace_bytes(prior, target, d);
  if (!workspace || workspace_bytes < need) return fail(SDENG_E_WORKSPACE, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, need);
  float* ws = static_cast<float*>(workspace);
  MovesArgs a;
  memset(&a, 0, sizeof(a));
  SD_TRY(build_dist(*target, d, dpad, ws, a.target.ds, s));
  a.target.d = d; a.target.dpad = dpad; a.target.B = B;
  a.prior.ds.kind = SDENG_DIST_NONE;
  if (has_prior) SD_TRY(build_dist(*prior, d, dpad, ws + dist_floats(*target, dpad), a.prior.ds, s));
  a.prior.d = d; a.prior.dpad = dpad; a.prior.B = B;
  a.B = B; a.d = d; a.K = n_moves; a.keep_from = keep_from; a.ula = unadjusted ? 1 : 0; a.target_acc = target_acceptance;
  a.t = t; a.x = x; a.lp = lp; a.grad = grad; a.step = step; a.z = z; a.u = u;
  const Seed sd = split_seed(seed);
  a.seed_lo = sd.lo; a.seed_hi = sd.hi; a.chain0 = chain0;
  a.samples = samples; a.acc_sum = acc_sum; a.acc_last = acc_last;
  SD_HIP(sd_launch_moves(a, move, s));
  return 0;
}

extern "C" size_t sdeng_langevin_moves_workspace_bytes(const sdeng_dist* prior, const sdeng_dist* target, int32_t d) {
  return moves_workspace_bytes(prior, target, d);
}
extern "C" int sdeng_langevin_moves(const sdeng_dist* prior, const sdeng_dist* target, int32_t B, int32_t d, int32_t n_moves, int32_t keep_from,
                                    int32_t unadjusted, float target_acceptance, const float* t, float* x, float* lp, float* grad, float* step,
                                    const float* z, const float* u, uint64_t seed, int64_t chain0, float* samples, float* acc_sum,
                                    float* acc_last, void* workspace, size_t workspace_bytes, void* stream) {
  return run_moves(SD_MOVE_LANGEVIN, "langevin_moves", prior, target, B, d, n_moves, keep_from, unadjusted, target_acceptance, t, x, lp, grad, step,
                   z, u, seed, chain0, samples, acc_sum, acc_last, workspace, workspace_bytes, stream);
}
extern "C" size_t sdeng_rwmh_moves_workspace_bytes(const sdeng_dist* target, int32_t d) { return moves_workspace_bytes(nullptr, target, d); }
extern "C" int sdeng_rwmh_moves(const sdeng_dist* target, int32_t B, int32_t d, int32_t n_moves, int32_t keep_from, float target_acceptance,
                                float* x, float* lp, float* step, const float* z, const float* u, uint64_t seed, int64_t chain0,
                                float* samples, float* acc_sum, float* acc_last, void* workspace, size_t workspace_bytes, void* stream) {
  return run_moves(SD_MOVE_RWMH, "rwmh_moves", nullptr, target, B, d, n_moves, keep_from, 0, target_acceptance, nullptr, x, lp, nullptr, step, z, u,
                   seed, chain0, samples, acc_sum, acc_last, workspace, workspace_bytes, stream);
}

extern "C" size_t sdeng_dist_workspace_bytes(const sdeng_dist* dist, int32_t d) {
  if (!dist || d < 1) return 0;
  return dist_floats(*dist, pad16(d)) * sizeof(float);
}

extern "C" size_t sdeng_logz_workspace_bytes(void) { return 5 * SD_LOGZ_MAX_BLOCKS * sizeof(float); }

extern "C" int sdeng_logz(const float* rnd, int64_t B, float* stats, float* weights_out, void* workspace, size_t workspace_bytes,
                          void* stream) {
  if (!rnd || !stats || B < 1) return fail(SDENG_E_INVALID, "bad argument");
  if (!workspace || workspace_bytes < sdeng_logz_workspace_bytes()) return fail(SDENG_E_WORKSPACE, "logz workspace too small");
  SD_HIP(sd_launch_logz(rnd, B, stats, weights_out, static_cast<float*>(workspace), static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int sdeng_philox_normal(uint64_t seed, int32_t step, int64_t particle0, int32_t B, int32_t d, uint32_t stream_id, float* out,
                                   void* stream) {
  return sdeng_philox_normal_steps(seed, step, 1, particle0, B, d, stream_id, out, stream);
}
extern "C" int sdeng_philox_normal_steps(uint64_t seed, int32_t step0, int32_t n_steps, int64_t particle0, int32_t B, int32_t d,
                                         uint32_t stream_id, float* out, void* stream) {
  if (!out || B < 0 || d < 1 || n_steps < 0) return fail(SDENG_E_INVALID, "bad argument");
  if (B == 0 || n_steps == 0) return 0;
  const Seed sd = split_seed(seed);
  SD_HIP(sd_launch_philox(sd.lo, sd.hi, step0, n_steps, particle0, B, d, stream_id, out, static_cast<hipStream_t>(stream)));
  return 0;
}

// ---- sample-quality metrics (eval/sinkhorn.py, additions/mmd.py) ---------------------------------------------------------------------
static bool sk_fits(int32_t n, int32_t m) { return sizeof(float) * static_cast<size_t>(n) * m <= SDENG_SINKHORN_MATRIX_MAX_BYTES; }
extern "C" size_t sdeng_sinkhorn_workspace_bytes(int32_t n, int32_t m, int32_t d, int32_t materialise) {
  if (n < 1 || m < 1 || d < 1) return 0;
  const SkLayout L = sd_sk_layout(n, m);
  return materialise && sk_fits(n, m) ? L.total_bytes : L.small_bytes;
}
extern "C" int sdeng_sinkhorn(const float* x, const float* y, int32_t n, int32_t m, int32_t d, int32_t p, double eps, int32_t max_iters,
                              double stop_thresh, const float* w_x, const float* w_y, float* u_out, float* v_out, int32_t* corr_x_to_y,
                              int32_t* corr_y_to_x, sdeng_sinkhorn_result* result, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !y || !result || n < 1 || m < 1 || d < 1 || max_iters < 1 || !(eps > 0.0)) return fail(SDENG_E_INVALID, "sinkhorn: bad argument");
  if ((w_x == nullptr) != (w_y == nullptr)) return fail(SDENG_E_INVALID, "sinkhorn: give both weight vectors, or neither");
  if (p != 1 && p != 2) return fail(SDENG_E_UNSUPPORTED, "sinkhorn: p in {1, 2}, got %d", p);
  const SkLayout L = sd_sk_layout(n, m);
  if (!workspace || workspace_bytes < L.small_bytes) return fail(SDENG_E_WORKSPACE, "workspace %zu bytes, need %zu", workspace_bytes, L.small_bytes);
  char* ws = static_cast<char*>(workspace);
  SkArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.w_x = w_x; a.w_y = w_y; a.n = n; a.m = m; a.d = d; a.p = p; a.eps = eps; a.inv_eps = 1.0 / eps;
  a.u = reinterpret_cast<double*>(ws + L.u); a.v = reinterpret_cast<double*>(ws + L.v);
  a.loga = reinterpret_cast<double*>(ws + L.loga); a.logb = reinterpret_cast<double*>(ws + L.logb);
  a.du = reinterpret_cast<double*>(ws + L.du); a.dv = reinterpret_cast<double*>(ws + L.dv);
  a.rowsum = reinterpret_cast<double*>(ws + L.rowsum); a.part = reinterpret_cast<double*>(ws + L.part);
  a.part_idx = reinterpret_cast<int*>(ws + L.part_idx); a.errs = reinterpret_cast<double*>(ws + L.errs);
  a.chunks = L.chunks; a.rows_per_chunk = L.rows_per_chunk;
  a.u_out = u_out; a.v_out = v_out; a.corr_xy = corr_x_to_y; a.corr_yx = corr_y_to_x;
  float* M = sk_fits(n, m) && workspace_bytes >= L.total_bytes ? reinterpret_cast<float*>(ws + L.M) : nullptr;
  SD_HIP(sd_run_sinkhorn(a, M, max_iters, stop_thresh, result, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" size_t sdeng_mmd_median_workspace_bytes(int32_t n, int32_t d) {
  if (n < 2 || d < 1) return 0;
  return sd_mmd_layout(n).total_bytes;
}
extern "C" int sdeng_mmd_median(const float* X, const float* Y, int32_t n, int32_t m, int32_t d, float* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!X || !Y || !out || d < 1) return fail(SDENG_E_INVALID, "mmd_median: bad argument");
  if (n != m || n < 2) return fail(SDENG_E_INVALID, "mmd_median: n == m >= 2 (additions/mmd.py:33-36), got %d and %d", n, m);
  if (n > (1 << 29)) return fail(SDENG_E_UNSUPPORTED, "mmd_median: n <= 2^29");
  const MmdLayout L = sd_mmd_layout(n);
  if (!workspace || workspace_bytes < L.total_bytes) return fail(SDENG_E_WORKSPACE, "workspace %zu bytes, need %zu", workspace_bytes, L.total_bytes);
  char* ws = static_cast<char*>(workspace);
  MmdArgs a;
  a.X = X; a.Y = Y; a.n = n; a.d = d; a.tiles = L.tiles; a.groups = L.groups;
  a.hist = reinterpret_cast<unsigned long long*>(ws + L.hist); a.state = reinterpret_cast<unsigned long long*>(ws + L.state);
  a.part = reinterpret_cast<double*>(ws + L.part); a.out = out;
  SD_HIP(sd_run_mmd_median(a, static_cast<hipStream_t>(stream)));
  return 0;
}

// ---- energy-based (tilted-potential) references: tilted_kernel.hpp ---------------------------------------------------------------
struct TiltedLayout {
  size_t pack, consts, trash, hbuf, total;  // floats
  int ntiles, waves, grid, nimg;
};
static TiltedLayout tilted_layout(const sdeng_tilted* t, bool train = false) {
  TiltedLayout L;
  L.ntiles = (t->M + 15) / 16;
  L.waves = sd_tilted_waves(L.ntiles);
  L.grid = sd_tilted_grid(L.ntiles, L.waves);
  L.nimg = TL_EIG + (t->full_cov ? 2 * t->k : 0);
  size_t o = 0;
  L.pack = o; o += static_cast<size_t>(L.nimg) * TL_SLOT;
  L.consts = o; o += align64(TL_C_TOTAL);
  L.trash = o; o += align64(512 * 4);
  L.hbuf = o; o += (t->grad || train) ? static_cast<size_t>(L.grid) * L.waves * TL_HBUF_FLOATS : 0;
  L.total = o;
  return L;
}
// `who`: the entry point, for the messages; `train`: sdeng_tilted_vjp, where log_prob and grad may both be absent; `moves`:
// sdeng_tilted_moves, which ignores x, log_prob and grad (the chain state is in its own argument block); `sim`: sdeng_tilted_simulate,
// which ignores those three and rows_per_time (M particles walk n_times steps)
static int check_tilted(const sdeng_tilted* t, const char* who = "tilted_eval", bool train = false, bool moves = false, bool sim = false) {
  if (!t) return fail(SDENG_E_INVALID, "%s: null descriptor", who);
  if (t->abi_version != SDENG_ABI_VERSION) return fail(SDENG_E_INVALID, "ABI version %d, library has %d", t->abi_version, SDENG_ABI_VERSION);
  if (t->d < 1 || t->d > 128) return fail(SDENG_E_INVALID, "%s: d = %d outside [1, 128]", who, t->d);
  if (t->k < 1 || t->k > TL_KMAX) return fail(SDENG_E_INVALID, "%s: k = %d components outside [1, %d]", who, t->k, TL_KMAX);
  if (sim && (t->M < 1 || t->n_times < 1)) return fail(SDENG_E_INVALID, "%s: M = %d particles, n_times = %d steps", who, t->M, t->n_times);
  if (!sim && (t->M < 1 || t->n_times < 1 || t->rows_per_time < 1 || static_cast<long long>(t->n_times) * t->rows_per_time != t->M))
    return fail(SDENG_E_INVALID, "%s: M = %d rows is not n_times * rows_per_time = %d * %d", who, t->M, t->n_times, t->rows_per_time);
  if (static_cast<long long>(t->M) * t->d >= (1ll << 31)) return fail(SDENG_E_UNSUPPORTED, "%s: rows * d >= 2^31", who);
  if (t->num_layers != 6 || t->channels != TL_H)
    return fail(SDENG_E_UNSUPPORTED, "%s: the kernel is built for FourierMLP(num_layers=6, channels=128), got num_layers=%d channels=%d", who,
                t->num_layers, t->channels);
  if (t->tilt_type != SDENG_TILT_DOT) return fail(SDENG_E_UNSUPPORTED, "%s: tilt_type 'dot' only (type %d given)", who, t->tilt_type);
  if (t->use_scaling_factor) return fail(SDENG_E_UNSUPPORTED, "%s: use_scaling_factor (the DRL scaling argument) is not supported", who);
  const void* need[] = {moves ? t->tinfo : t->x, t->tinfo, t->w_in, t->b_in, t->w_out, t->b_out, t->te_coeff, t->te_phase, t->te_w1, t->te_b1, t->te_w2, t->te_b2,
                        t->mean_gauss, t->var_gauss, t->weights, t->means, t->vars, t->w_h[0], t->w_h[1], t->w_h[2], t->w_h[3],
                        t->b_h[0], t->b_h[1], t->b_h[2], t->b_h[3]};
  for (const void* p : need)
    if (!p) return fail(SDENG_E_INVALID, "%s: null pointer in the descriptor", who);
  if (t->full_cov && !t->eigvecs) return fail(SDENG_E_INVALID, "%s: full_cov without eigvecs", who);
  if (!train && !moves && !t->log_prob && !t->grad) return fail(SDENG_E_INVALID, "%s: nothing to compute (log_prob and grad are both NULL)", who);
  return 0;
}
extern "C" size_t sdeng_tilted_eval_workspace_bytes(const sdeng_tilted* t) {
  if (check_tilted(t)) return 0;
  return tilted_layout(t).total * sizeof(float);
}
// the packed images and constants of the net and the prior, at the head of the workspace of every tilted entry point
static int pack_tilted(const sdeng_tilted* t, const TiltedLayout& L, float* ws, hipStream_t s) {
  const int d = t->d, H = TL_H;
  float* consts = ws + L.consts;
  static_assert(TL_NIMG <= SD_PACK_MAX_JOBS, "one job per image slot");
  PackJobs p;
  p.njobs = 0;
  // one matrix (or a column range of it) -> slot `slot`, its scale at TL_C_SCALE / TL_C_INV + slot, its scaled bias at `bias_off`
  auto job = [&](int slot, const float* W, int n_out, int n_in, int ld, int col0, int transpose, int scale_n, const float* bias, int bias_off) {
    PackJob& j = add_pack_job(p, W, ld, n_out, n_in, transpose, (n_out + 15) / 16, (n_in + 31) / 32, ws + L.pack + static_cast<size_t>(slot) * TL_SLOT);
    j.col0 = col0;
    scale_by(j, W, scale_n, consts + TL_C_SCALE + slot, TL_C_INV - TL_C_SCALE);
    if (bias) with_bias(j, bias, consts + bias_off, 128);
  };
  job(TL_TE1S, t->te_w1, H, H, 2 * H, 0, 0, 2 * H * H, t->te_b1, TL_C_BTE1);  // the sine and cosine halves share the matrix's scale
  job(TL_TE1C, t->te_w1, H, H, 2 * H, H, 0, 2 * H * H, nullptr, 0);
  job(TL_TE2, t->te_w2, H, H, H, 0, 0, H * H, t->te_b2, TL_C_BTE2);
  job(TL_WIN, t->w_in, H, d, d, 0, 0, H * d, t->b_in, TL_C_BIN);
  for (int l = 0; l < 4; ++l) job(TL_WH + l, t->w_h[l], H, H, H, 0, 0, H * H, t->b_h[l], TL_C_BH + 128 * l);
  job(TL_WOUT, t->w_out, d, H, H, 0, 0, d * H, t->b_out, TL_C_BOUT);
  job(TL_WOUT_T, t->w_out, H, d, H, 0, 1, d * H, nullptr, 0);  // W_out^T: [128 x d]
  for (int l = 0; l < 4; ++l) job(TL_WH_T + l, t->w_h[l], H, H, H, 0, 1, H * H, nullptr, 0);
  job(TL_WIN_T, t->w_in, d, H, d, 0, 1, H * d, nullptr, 0);    // W_in^T: [d x 128]
  if (t->full_cov)
    for (int k = 0; k < t->k; ++k) {
      const float* P = t->eigvecs + static_cast<size_t>(k) * d * d;
      job(TL_EIG + 2 * k, P, d, d, d, 0, 1, d * d, nullptr, 0);      // y = P^T z
      job(TL_EIG + 2 * k + 1, P, d, d, d, 0, 0, d * d, nullptr, 0);  // P q
    }
  SD_HIP(sd_launch_pack_images(p, s));
  TiltedConstArgs c;
  c.consts = consts; c.coeff = t->te_coeff; c.phase = t->te_phase; c.mean_gauss = t->mean_gauss; c.var_gauss = t->var_gauss;
  c.weights = t->weights; c.means = t->means; c.vars = t->vars; c.d = d; c.K = t->k;
  SD_HIP(sd_launch_tilted_consts(c, s));
  return 0;
}
// the shapes, the times and the workspace's pieces: what every tilted kernel takes; the rows to evaluate and the outputs are the caller's
static TiltedArgs tilted_args(const sdeng_tilted* t, const TiltedLayout& L, float* ws) {
  TiltedArgs a;
  memset(&a, 0, sizeof(a));
  a.M = t->M; a.B = t->rows_per_time; a.d = t->d; a.N = t->n_times; a.K = t->k; a.full = t->full_cov ? 1 : 0;
  a.use_st = t->use_s_t_scaling ? 1 : 0; a.ntiles = L.ntiles;
  a.tinfo = t->tinfo; a.pack = ws + L.pack; a.consts = ws + L.consts; a.hbuf = ws + L.hbuf; a.trash = ws + L.trash;
  return a;
}
// the pack (unless reused) and the one launch of either entry point; `rows`: the training instantiation
static int run_tilted(const sdeng_tilted* t, const TiltedRows* rows, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const TiltedLayout L = tilted_layout(t, rows != nullptr);
  const size_t need = L.total * sizeof(float);
  if (!t->workspace || t->workspace_bytes < need) return fail(SDENG_E_WORKSPACE, "workspace %zu bytes, need %zu", t->workspace_bytes, need);
  float* ws = static_cast<float*>(t->workspace);
  const int d = t->d;
  if (!(t->flags & SDENG_FLAG_REUSE_PACK)) SD_TRY(pack_tilted(t, L, ws, s));
  TiltedArgs a = tilted_args(t, L, ws);
  a.x = t->x; a.log_prob = t->log_prob; a.grad = t->grad;
  if (!t->grad && !rows) a.hbuf = nullptr;  // no backward pass: no pre-activations kept
  if (rows) SD_HIP(sd_launch_tilted_train(a, *rows, tiles_exact(d), L.grid, L.waves, s));
  else SD_HIP(sd_launch_tilted(a, tiles_exact(d), L.grid, L.waves, s));
  return 0;
}
extern "C" int sdeng_tilted_eval(const sdeng_tilted* t, void* stream) {
  SD_TRY(check_tilted(t));
  return run_tilted(t, nullptr, stream);
}
static int check_tilted_rows(const sdeng_tilted_rows* r) {
  if (!r) return fail(SDENG_E_INVALID, "tilted_vjp: null rows");
  for (int l = 0; l < 5; ++l) {
    if (!r->a[l]) return fail(SDENG_E_INVALID, "tilted_vjp: rows->a[%d] is NULL", l);
    if (!r->d[l]) return fail(SDENG_E_INVALID, "tilted_vjp: rows->d[%d] is NULL", l);
  }
  if (!r->xs) return fail(SDENG_E_INVALID, "tilted_vjp: rows->xs is NULL");
  if (!r->dv) return fail(SDENG_E_INVALID, "tilted_vjp: rows->dv is NULL");
  return 0;
}
extern "C" size_t sdeng_tilted_vjp_workspace_bytes(const sdeng_tilted* t) {
  if (check_tilted(t, "tilted_vjp", true)) return 0;
  return tilted_layout(t, true).total * sizeof(float);
}
extern "C" int sdeng_tilted_vjp(const sdeng_tilted* t, const sdeng_tilted_rows* r, void* stream) {
  SD_TRY(check_tilted(t, "tilted_vjp", true));
  SD_TRY(check_tilted_rows(r));
  TiltedRows rows;
  for (int l = 0; l < 5; ++l) { rows.a[l] = r->a[l]; rows.d[l] = r->d[l]; }
  rows.xs = r->xs; rows.dv = r->dv;
  return run_tilted(t, &rows, stream);
}

// ---- Langevin moves over an energy-based reference: tilted_moves_inst.hip ------------------------------------------------------------
// workspace: the layout of an evaluation with grad (so the packed images are where sdeng_tilted_eval keeps them), the per-wave slots one
// layer longer (the time embedding's accumulator), then the proposal and proposal-gradient rows
struct TiltedMovesLayout {
  TiltedLayout L;
  size_t prop, gprop, total;  // floats
};
static TiltedMovesLayout tilted_moves_layout(const sdeng_tilted* t) {
  TiltedMovesLayout ml;
  ml.L = tilted_layout(t, true);
  size_t o = ml.L.hbuf + static_cast<size_t>(ml.L.grid) * ml.L.waves * TLM_HBUF_FLOATS;
  const size_t rows = align64(static_cast<size_t>(t->M) * t->d);
  ml.prop = o; o += rows;
  ml.gprop = o; o += rows;
  ml.total = o;
  return ml;
}
static int check_tilted_moves(const sdeng_tilted* t, const sdeng_tilted_moves_state* mv) {
  const char* who = "tilted_moves";
  SD_TRY(check_tilted(t, who, false, true));
  if (!mv) return fail(SDENG_E_INVALID, "%s: null move state", who);
  if (!mv->x || !mv->lp || !mv->grad || !mv->step) return fail(SDENG_E_INVALID, "%s: x, lp, grad and step are all required", who);
  if (mv->n_moves < 0) return fail(SDENG_E_INVALID, "%s: n_moves = %d < 0", who, mv->n_moves);
  if (mv->keep_from < 0 || mv->keep_from > mv->n_moves)
    return fail(SDENG_E_INVALID, "%s: keep_from = %d outside [0, n_moves = %d]", who, mv->keep_from, mv->n_moves);
  if ((mv->z == nullptr) != (mv->u == nullptr) && !mv->unadjusted)  // (unadjusted moves read no uniforms)
    return fail(SDENG_E_INVALID, "%s: inject both the normals and the uniforms, or neither (unadjusted moves: the normals alone)", who);
  return 0;
}
extern "C" size_t sdeng_tilted_moves_workspace_bytes(const sdeng_tilted* t) {
  if (check_tilted(t, "tilted_moves", false, true)) return 0;
  return tilted_moves_layout(t).total * sizeof(float);
}
extern "C" int sdeng_tilted_moves(const sdeng_tilted* t, const sdeng_tilted_moves_state* mv, void* stream) {
  SD_TRY(check_tilted_moves(t, mv));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const TiltedMovesLayout ml = tilted_moves_layout(t);
  const TiltedLayout& L = ml.L;
  const size_t need = ml.total * sizeof(float);
  if (!t->workspace || t->workspace_bytes < need)
    return fail(SDENG_E_WORKSPACE, "tilted_moves: workspace %zu bytes, need %zu", t->workspace_bytes, need);
  if (mv->n_moves == 0) return 0;
  float* ws = static_cast<float*>(t->workspace);
  if (!(t->flags & SDENG_FLAG_REUSE_PACK)) SD_TRY(pack_tilted(t, L, ws, s));
  const TiltedArgs a = tilted_args(t, L, ws);  // x, log_prob and grad stay null: the chain state is in m
  TiltedMovesArgs m;
  memset(&m, 0, sizeof(m));
  m.x = mv->x; m.grad = mv->grad; m.lp = mv->lp; m.step = mv->step; m.prop = ws + ml.prop; m.gprop = ws + ml.gprop;
  m.z = mv->z; m.u = mv->unadjusted ? nullptr : mv->u; m.samples = mv->samples; m.acc_sum = mv->acc_sum; m.acc_last = mv->acc_last;
  m.K = mv->n_moves; m.keep_from = mv->keep_from; m.ula = mv->unadjusted ? 1 : 0; m.target_acc = mv->target_acceptance;
  const Seed sd = split_seed(mv->seed);
  m.seed_lo = sd.lo; m.seed_hi = sd.hi; m.chain0 = mv->chain0;
  SD_HIP(sd_launch_tilted_moves(a, m, tiles_exact(t->d), L.grid, L.waves, s));
  return 0;
}

// ---- the RDS step loop over an energy-based reference: tilted_rds_inst.hip -------------------------------------------------------------
// workspace: the layout of an evaluation with grad (so the packed images are where sdeng_tilted_eval keeps them), then the packed drift net,
// its time embeddings, the EBM's time embeddings, the score rows and the two ping-pong state rows
struct TiltedRdsLayout {
  TiltedLayout L;
  size_t wpack, temb, te_tab, score, ping, total;  // floats
};
static TiltedRdsLayout tilted_rds_layout(const sdeng_tilted* t, const sdeng_tilted_rds* r) {
  TiltedRdsLayout rl;
  rl.L = tilted_layout(t, true);
  size_t o = rl.L.total;
  const size_t rows = align64(static_cast<size_t>(t->M) * t->d);
  rl.wpack = o; o += align64(sd_pack_floats(tiles_exact(t->d)));
  rl.temb = o; o += align64(static_cast<size_t>(r->N) * SD_H);
  rl.te_tab = o; o += align64(static_cast<size_t>(r->N) * TL_H);
  rl.score = o; o += rows;
  rl.ping = o; o += 2 * rows;
  rl.total = o;
  return rl;
}
static int check_tilted_rds(const sdeng_tilted* t, const sdeng_tilted_rds* r) {
  const char* who = "tilted_simulate";
  SD_TRY(check_tilted(t, who, false, true, true));
  if (!r) return fail(SDENG_E_INVALID, "%s: null run", who);
  if (!r->coef || !r->x_in || !r->x_out || !r->rnd_out) return fail(SDENG_E_INVALID, "%s: coef, x_in, x_out and rnd_out are all required", who);
  if (r->N < 1 || r->N != t->n_times) return fail(SDENG_E_INVALID, "%s: N = %d steps (>= 1, and the n_times = %d of the reference's time table)", who, r->N, t->n_times);
  if (r->net.ctrl_kind != SDENG_CTRL_CLIPPED)
    return fail(SDENG_E_UNSUPPORTED, "%s: ClippedCtrl around the FourierMLP only (ctrl_kind %d given): a Score / Lerp / CancelDrift control has no "
                "kernel over an energy-based reference", who, r->net.ctrl_kind);
  if (r->form != SDENG_FORM_LIN && r->form != SDENG_FORM_EM)
    return fail(SDENG_E_UNSUPPORTED, "%s: SDENG_FORM_LIN and SDENG_FORM_EM only (form %d given; no EUBO or CMCD loop over an energy-based reference)", who, r->form);
  if (r->flags & ~SDENG_FLAG_ITO)
    return fail(SDENG_E_UNSUPPORTED, "%s: flags 0x%x: SDENG_FLAG_ITO only (REMOVE_REF, CTRL_NOISE, CTRL_DROPOUT and SPLIT_TILES have no kernel over an "
                "energy-based reference; initial and terminal costs are the caller's)", who, r->flags);
  SD_TRY(check_net(r->net));
  return 0;
}
extern "C" size_t sdeng_tilted_simulate_workspace_bytes(const sdeng_tilted* t, const sdeng_tilted_rds* r) {
  if (check_tilted_rds(t, r)) return 0;
  return tilted_rds_layout(t, r).total * sizeof(float);
}
extern "C" int sdeng_tilted_simulate(const sdeng_tilted* t, const sdeng_tilted_rds* r, void* stream) {
  SD_TRY(check_tilted_rds(t, r));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const TiltedRdsLayout rl = tilted_rds_layout(t, r);
  const TiltedLayout& L = rl.L;
  const size_t need = rl.total * sizeof(float);
  if (!t->workspace || t->workspace_bytes < need)
    return fail(SDENG_E_WORKSPACE, "tilted_simulate: workspace %zu bytes, need %zu", t->workspace_bytes, need);
  float* ws = static_cast<float*>(t->workspace);
  if (!(t->flags & SDENG_FLAG_REUSE_PACK)) SD_TRY(pack_tilted(t, L, ws, s));
  TiltedArgs a = tilted_args(t, L, ws);  // x, log_prob and grad stay null: the state is in m
  a.B = t->M;  // every row of a step shares the step's time
  sdeng_desc nd;  // what the drift net's packer and its time embedding read of a descriptor
  memset(&nd, 0, sizeof(nd));
  nd.d = t->d; nd.N = r->N; nd.coef = r->coef; nd.net = r->net;
  const int DT = tiles_exact(t->d);
  SD_TRY(pack_net(&nd, DT, ws + rl.wpack, nullptr, s));
  const float* no_stheta;  // (ClippedCtrl: no score model)
  SD_TRY(embed_times(&nd, r->N, false, 0.0f, ws + rl.temb, nullptr, &no_stheta, s));
  SD_HIP(sd_launch_tilted_rds_times(a, ws + rl.te_tab, s));
  TiltedRdsArgs m;
  memset(&m, 0, sizeof(m));
  m.form = r->form; m.flags = r->flags; m.N = r->N; m.coef = r->coef;
  m.wpack = ws + rl.wpack; m.temb = ws + rl.temb; m.te_tab = ws + rl.te_tab; m.clip_model = r->net.clip_model;
  const Seed sd = split_seed(r->seed);
  m.seed_lo = sd.lo; m.seed_hi = sd.hi; m.particle0 = r->particle0;
  m.x_in = r->x_in; m.noise_in = r->noise_in; m.x_out = r->x_out; m.rnd_out = r->rnd_out; m.xs_out = r->xs_out; m.ref_out = r->ref_out;
  m.ping = ws + rl.ping; m.score = ws + rl.score;
  SD_HIP(sd_launch_tilted_rds(a, m, DT, L.grid, L.waves, s));
  return 0;
}
