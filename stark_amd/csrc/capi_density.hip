// C ABI of libstark_hip.so: the chain plan, the lp / grad parity hooks, the host-only launch-info
// calls, the analytic Hessian, the pointwise log-predictive sweep, the PSIS-LOO sweep, the per-draw log
// density, the weighted bootstrap sweep, the Laplace proposal and the posterior predictive replicate sweep.
#include "capi_internal.h"
#include "boot_math.h"
#include "yrep_math.h"

// The chain counts that are ONE sweep launch in the two single-launch parity hooks (stk_log_density_grad's
// own batching and stk_log_density_grad_shards): their acceptance set stays as it was before the
// sampler batched chains -- 16 only where k_sweep16 itself runs (d <= 128).
static bool hook_single_launch(int C, int d) { return stk_sweep_supported(C, d) && (C != 16 || d <= 128); }

// The chain batches of a regression shard's C chains: greedy, largest first, over the single-launch
// sizes {64, 16, 8, 4, 2, 1} a sweep covers at d (stk_sweep_supported, sweep.hip, says whether 16
// is a batch size at d; stk_sweep_plan then picks each batch's kernel).  A pure function of
// (C, d) -- never of n, the shard count or the device -- so every rank derives the same plan.
// No padding, no idle chains.
std::vector<int> chain_batches(int C, int d) {
  std::vector<int> b;
  for (const int sz : {64, 16, 8, 4, 2, 1}) {
    if (!stk_sweep_supported(sz, d)) continue;
    for (; C >= sz; C -= sz) b.push_back(sz);
  }
  if (C != 0) b.clear();   // no sweep covers d
  return b;
}

// A sparse shard's: the sizes k_sweep_sp covers at d (sweep_sparse.hip: 16 up to d = 512, no 64-chain pass).
std::vector<int> chain_batches_sparse(int C, int d) {
  std::vector<int> b;
  for (const int sz : {16, 8, 4, 2, 1}) {
    if (!stk_sweep_sparse_supported(sz, d)) continue;
    for (; C >= sz; C -= sz) b.push_back(sz);
  }
  if (C != 0) b.clear();
  return b;
}
// A categorical shard's: C / 16 launches of 16 chains and one of the C mod 16 left over (k_sweep_cat takes any count up
// to 16: the unused columns carry zero coefficients).  A pure function of (C, K, d); empty outside the envelope.
std::vector<int> chain_batches_cat(int C, int ncat, int d) {
  std::vector<int> b;
  if (C < 1 || !stk_sweep_cat_supported(ncat - 1, d)) return b;
  for (; C >= CAT_MAX_CHAINS; C -= CAT_MAX_CHAINS) b.push_back(CAT_MAX_CHAINS);
  if (C > 0) b.push_back(C);
  return b;
}
std::vector<int> model_chain_batches(const stk_model* m, int C) {
  if (m->family == STK_CATEGORICAL) return chain_batches_cat(C, m->ncat, m->d);
  return m->sparse ? chain_batches_sparse(C, m->d) : chain_batches(C, m->d);
}
int model_sweep_pw(const stk_model* m) {
  return m->family == STK_CATEGORICAL ? stk_sweep_cat_pw(m->ncat, m->d) : sweep_pw(m->family, m->d);
}

// Refuses, before anything is launched, a shard that no sweep covers at its n, d and batch size.
int chain_plan(const stk_model* m, const std::vector<int>& sizes, int first, int count, ChainPlan* cp) {
  *cp = ChainPlan();
  RC(model_ready(m));   // every density, transition and sampler entry point of a regression plans its sweeps here
  for (const int sz : sizes) {
    ChainBatch b;
    b.c0 = cp->Ct;
    b.part_off = cp->partial_bytes / sizeof(double);
    for (int sh = first; sh < first + count;) {
      SweepGroup gr{sh, 1, m->family == STK_CATEGORICAL ? stk_sweep_plan_cat(m->sh[sh].n, m->d, sz, m->ncat)
                           : m->sparse                   ? stk_sweep_plan_sparse(m->sh[sh].n, m->d, sz)
                                                         : stk_sweep_plan(m->sh[sh].n, m->d, sz, 0)};
      ARG_CHECK(gr.launch.kind != SWEEP_NONE,
                "shard %d: no sweep covers n = %lld rows of d = %d covariates at C = %d chains (a chunk of the shard "
                "must fit a buffer descriptor: split the shard)", sh, (long long)m->sh[sh].n, m->d, sz);
      while (sh + gr.nsh < first + count && m->sh[sh + gr.nsh].n == m->sh[sh].n) ++gr.nsh;
      b.Gs = std::max(b.Gs, gr.launch.G);
      if (gr.launch.ws_bytes > cp->ws_at.ws_bytes) cp->ws_at = gr.launch;
      b.groups.push_back(gr);
      sh += gr.nsh;
    }
    cp->partial_bytes += sizeof(double) * (size_t)m->nshards * b.Gs * sz * model_sweep_pw(m);
    cp->Ct += sz;
    cp->batches.push_back(std::move(b));
  }
  cp->ws_bytes = cp->ws_at.ws_bytes * m->nshards;
  return STK_OK;
}
// Every batch's sweep over every shard group; then (plan_reduces) every batch's reduction.  `run`
// holds the run's buffers; a batch's partial-sum region, stride and first chain are filled in here.
static SweepCall batch_call(const stk_model* m, const ChainPlan& cp, const ChainBatch& b, SweepCall c) {
  c.nb = m->nb_dev.as<NbShardDev>();   // NULL but for the negative binomial and the gamma family, whose reduces read it
  c.sp = m->sp_dev.as<SpShardDev>();   // NULL but for a sparse model
  c.partial += b.part_off;
  c.Gs = b.Gs;
  c.Ct = cp.Ct;
  c.c0 = b.c0;
  return c;
}
hipError_t plan_sweeps(const stk_model* m, const ChainPlan& cp, const SweepCall& run, hipStream_t st) {
  for (const auto& b : cp.batches) {
    const SweepCall c = batch_call(m, cp, b, run);
    for (const auto& gr : b.groups)
      if (const hipError_t e = gr.launch.kind == SWEEP_CAT      ? stk_launch_sweep_cat(gr.launch, gr.shard0, gr.nsh, c, st)
                               : gr.launch.kind == SWEEP_SPARSE ? stk_launch_sweep_sparse(m->family, gr.launch, gr.shard0, gr.nsh, c, st)
                                                                : stk_launch_sweep(m->family, gr.launch, gr.shard0, gr.nsh, c, st))
        return e;
  }
  return hipSuccess;
}
hipError_t plan_reduces(const stk_model* m, const ChainPlan& cp, const SweepCall& run, double* lp, double* g,
                        hipStream_t st) {
  for (const auto& b : cp.batches) {
    const SweepCall c = batch_call(m, cp, b, run);
    for (const auto& gr : b.groups)
      if (const hipError_t e = gr.launch.kind == SWEEP_CAT ? stk_launch_sweep_reduce_cat(gr.launch, gr.shard0, gr.nsh, c, lp, g, st)
                                                           : stk_launch_sweep_reduce(m->family, gr.launch, gr.shard0, gr.nsh, c, lp, g, st))
        return e;
  }
  return hipSuccess;
}

// The body of the regression parity hooks.  np points of D doubles at q go to rows [row0, row0 +
// nrows) of the [nshards * plan.Ct][Dp] point buffer (the last point repeated to fill), the plan's
// sweeps and reductions run, and lp / grad of the first np rows come back.  The caller synchronises.
static int hook_eval(stk_model* m, const ChainPlan& plan, size_t row0, size_t nrows, const double* q, size_t np,
                     double* lp, double* grad) {
  stk_ctx* ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const int D = m->Dmax, Dp = (m->Dmax + 7) / 8 * 8;   // one d for every shard of a regression model
  const size_t rows = (size_t)m->nshards * plan.Ct, pitch = sizeof(double) * Dp, width = sizeof(double) * D;
  SweepWs ws{};
  if (plan.ws_bytes) {
    RC(ctx->scratch[SCR_HOOK_WS].ensure(plan.ws_bytes));
    ws = stk_sweep_ws(ctx->scratch[SCR_HOOK_WS].p, plan.ws_at, m->nshards);
  }
  RC(ctx->scratch[SCR_HOOK_Q].ensure(rows * pitch));
  RC(ctx->scratch[SCR_HOOK_LP].ensure(sizeof(double) * rows));
  RC(ctx->scratch[SCR_HOOK_GRAD].ensure(rows * pitch));
  RC(ctx->scratch[SCR_HOOK_PARTIAL].ensure(plan.partial_bytes));
  double* qb = ctx->scratch[SCR_HOOK_Q].as<double>();
  double* lpb = ctx->scratch[SCR_HOOK_LP].as<double>();
  double* gb = ctx->scratch[SCR_HOOK_GRAD].as<double>();
  STK_HIP_CHECK(hipMemcpy2DAsync(qb + row0 * Dp, pitch, q, width, width, np, hipMemcpyDefault, st));
  for (size_t r = np; r < nrows; ++r)
    STK_HIP_CHECK(hipMemcpyAsync(qb + (row0 + r) * Dp, q + (np - 1) * D, width, hipMemcpyDefault, st));
  const SweepCall run{m->sh_dev.as<ShardDev>(), qb, ctx->scratch[SCR_HOOK_PARTIAL].as<double>(), nullptr, 0, nullptr,
                      plan.ws_bytes ? &ws : nullptr, Dp, 0, 0, 0};
  STK_HIP_CHECK(plan_sweeps(m, plan, run, st));
  STK_HIP_CHECK(plan_reduces(m, plan, run, lpb, gb, st));
  STK_HIP_CHECK(hipMemcpyAsync(lp, lpb + row0, sizeof(double) * np, hipMemcpyDefault, st));
  if (grad) STK_HIP_CHECK(hipMemcpy2DAsync(grad, width, gb + row0 * Dp, pitch, width, np, hipMemcpyDefault, st));
  return STK_OK;
}
// Every shard at sum(sizes) points each, in those chain batches.
static int hook_every_shard(stk_model* m, const std::vector<int>& sizes, const double* q, double* lp, double* grad) {
  STK_HIP_CHECK(hipSetDevice(m->ctx->device));
  ChainPlan plan;
  RC(chain_plan(m, sizes, 0, m->nshards, &plan));
  const size_t rows = (size_t)m->nshards * plan.Ct;
  RC(hook_eval(m, plan, 0, rows, q, rows, lp, grad));
  STK_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  return STK_OK;
}

// The sweeps over a draw image.  S draws q [S][D] are staged behind their image, with room for `extra`
// doubles after them, and the image is built (one preparation launch, the log-predictive sweep's).
struct DrawImage { double *img, *q; };
static int stage_draws(stk_model* m, const double* q, int S, size_t extra, DrawImage* out) {
  stk_ctx* ctx = m->ctx;
  const size_t qn = (size_t)S * m->Dmax, img_bytes = stk_predictive_image_bytes(m->d, S);
  RC(ctx->scratch[SCR_DRAW_IMG].ensure(img_bytes + sizeof(double) * (qn + extra)));
  out->img = ctx->scratch[SCR_DRAW_IMG].as<double>();
  out->q = out->img + img_bytes / sizeof(double);
  STK_HIP_CHECK(hipMemcpyAsync(out->q, q, sizeof(double) * qn, hipMemcpyDefault, ctx->stream));
  STK_HIP_CHECK(stk_launch_predictive_prep(m->family, m->d, m->Dmax, S, out->q, out->img, ctx->stream));
  return STK_OK;
}

// The rows-and-totals contract of stk_log_predictive and stk_loo: the same S draws against one shard or
// (shard == -1) every shard, one preparation launch, one sweep launch and one reduce launch for all of
// them.  Per-row output goes straight to `rows` when that is memory of the context's device, else
// through a staging buffer.
typedef hipError_t (*RowsLaunch)(int family, const ShardDev* shards, int shard0, int nsh, int d, int Gs, int S,
                                 const double* img, double* partial, double* rows, const int64_t* rowoff, double* totals,
                                 hipStream_t st);
static int rows_and_totals(stk_model* m, int shard, const double* q, int S, double* rows, double* totals, RowsLaunch launch,
                           int (*chunks)(int64_t n)) {
  stk_ctx* ctx = m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const ShardRange r = shard_range(m, shard, chunks);
  const int shard0 = r.shard0, nsh = r.nsh, Gs = r.Gs;
  std::vector<int64_t> off(nsh);
  int64_t nrows = 0;
  for (int s = 0; s < nsh; ++s) {
    off[s] = nrows;
    nrows += m->sh[shard0 + s].n;
  }
  RC(ctx->scratch[SCR_DRAW_PARTIAL].ensure(sizeof(double) * 8 * ((size_t)nsh * Gs + nsh) + sizeof(int64_t) * nsh));
  double* partial = ctx->scratch[SCR_DRAW_PARTIAL].as<double>();
  double* tb = partial + (size_t)nsh * Gs * 8;
  int64_t* offb = reinterpret_cast<int64_t*>(tb + (size_t)nsh * 8);
  const bool staged = rows && !is_device_ptr(rows, ctx->device);
  if (staged) RC(ctx->scratch[SCR_DRAW_ROWS].ensure(sizeof(double) * 4 * (size_t)nrows));
  double* rb = staged ? ctx->scratch[SCR_DRAW_ROWS].as<double>() : rows;
  DrawImage di;                              // every buffer is there before anything is queued
  RC(stage_draws(m, q, S, 0, &di));
  STK_HIP_CHECK(hipMemcpyAsync(offb, off.data(), sizeof(int64_t) * nsh, hipMemcpyHostToDevice, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));   // off is a local
  STK_HIP_CHECK(launch(m->family, m->sh_dev.as<ShardDev>(), shard0, nsh, m->d, Gs, S, di.img, partial, rb, offb, tb, st));
  if (totals) STK_HIP_CHECK(hipMemcpyAsync(totals, tb, sizeof(double) * 8 * nsh, hipMemcpyDefault, st));
  if (staged) STK_HIP_CHECK(hipMemcpyAsync(rows, rb, sizeof(double) * 4 * (size_t)nrows, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  return STK_OK;
}

extern "C" {

// ---------------------------------------------------------------- lp / grad (parity hook)
int stk_log_density_grad(stk_model* m, int shard, const double* q, int32_t C, double* lp, double* grad) {
  ARG_CHECK(m && q && lp && C > 0 && shard >= 0 && shard < m->nshards, "stk_log_density_grad: bad arguments");
  stk_ctx* ctx = m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  const ShardDev& s = m->sh[shard];
  const int D = s.D;
  hipStream_t st = ctx->stream;
  if (m->family != STK_SCHOOLS) {
    // the chain batch the sampler's sweep uses: 64 (two-pass fp64 MFMA GEMMs) from 64 points,
    // 16 (fp64 MFMA) from 16 when d <= 128, else 4 / 2 / 1; this shard alone, the last point
    // repeated to fill the last batch (the kernel reads rows shard * Cb + c of the point buffer)
    // (a sparse shard: 16 where the sparse sweep covers it at d, no 64)
    // (a categorical shard: one launch of up to 16 points, whatever their count)
    const int Cb = m->family == STK_CATEGORICAL ? std::min<int>(C, CAT_MAX_CHAINS)
                   : m->sparse ? (C <= 1 ? 1 : C <= 2 ? 2 : (C < 16 || !stk_sweep_sparse_supported(16, s.d)) ? 4 : 16)
                               : C <= 1 ? 1 : (C <= 2 ? 2 : (C >= 64 ? 64 : (C < 16 || !hook_single_launch(16, s.d) ? 4 : 16)));
    ChainPlan plan;
    RC(chain_plan(m, {Cb}, shard, 1, &plan));
    for (int c0 = 0; c0 < C; c0 += Cb)
      RC(hook_eval(m, plan, (size_t)shard * Cb, Cb, q + (size_t)c0 * D, std::min(Cb, C - c0), lp + c0,
                   grad ? grad + (size_t)c0 * D : nullptr));
    STK_HIP_CHECK(hipStreamSynchronize(st));
    return STK_OK;
  }
  // 8 schools: the hooks' point, lp and grad buffers, one launch
  const int Dp = (m->Dmax + 7) / 8 * 8;
  RC(ctx->scratch[SCR_HOOK_Q].ensure(sizeof(double) * (size_t)C * Dp));
  RC(ctx->scratch[SCR_HOOK_LP].ensure(sizeof(double) * (size_t)C));
  RC(ctx->scratch[SCR_HOOK_GRAD].ensure(sizeof(double) * (size_t)C * Dp));
  double* qb = ctx->scratch[SCR_HOOK_Q].as<double>();
  double* lpb = ctx->scratch[SCR_HOOK_LP].as<double>();
  double* gb = ctx->scratch[SCR_HOOK_GRAD].as<double>();
  STK_HIP_CHECK(hipMemcpy2DAsync(qb, sizeof(double) * Dp, q, sizeof(double) * D, sizeof(double) * D, C, hipMemcpyDefault, st));
  STK_HIP_CHECK(stk_launch_schools_lpgrad(m->sh_dev.as<ShardDev>(), shard, stk_nch_for(m->Dmax), qb, C, Dp, lpb, gb, st));
  STK_HIP_CHECK(hipMemcpyAsync(lp, lpb, sizeof(double) * C, hipMemcpyDefault, st));
  if (grad)
    STK_HIP_CHECK(hipMemcpy2DAsync(grad, sizeof(double) * D, gb, sizeof(double) * Dp, sizeof(double) * D, C, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  return STK_OK;
}

// Every shard at C points each through the sampler's grouped launches (chain_plan with the one
// batch C): the parity hook for multi-shard grids, shard0 > 0 and a partial-sum stride Gs above a
// group's own G.
int stk_log_density_grad_shards(stk_model* m, const double* q, int32_t C, double* lp, double* grad) {
  ARG_CHECK(m && q && lp && C > 0, "stk_log_density_grad_shards: bad arguments");
  ARG_CHECK(is_density_family(m->family), "stk_log_density_grad_shards: regression families only");
  if (m->family == STK_CATEGORICAL)
    ARG_CHECK(C <= CAT_MAX_CHAINS, "points per shard must be one launch of a categorical model here: 1 .. 16, not %d", C);
  else if (m->sparse)
    ARG_CHECK(stk_sweep_sparse_supported(C, m->d), "points per shard must be a single batch size of a sparse model here: 1, 2, 4, 8 or 16 (d <= 512)");
  else
    ARG_CHECK(hook_single_launch(C, m->d), "points per shard must be a single batch size here: 1, 2, 4, 8, 16 (d <= 128) or 64");
  return hook_every_shard(m, {C}, q, lp, grad);
}

// The same at ANY C >= 1 points per shard: the chain batches and grouped launches of a sampling
// run at chains = C.
int stk_log_density_grad_chains(stk_model* m, const double* q, int32_t C, double* lp, double* grad) {
  ARG_CHECK(m && q && lp && C > 0, "stk_log_density_grad_chains: bad arguments");
  ARG_CHECK(is_density_family(m->family), "stk_log_density_grad_chains: regression families only");
  RC(model_ready(m));
  ARG_CHECK(!model_chain_batches(m, C).empty(), "no sweep covers %d covariates (1..1024)", m->d);
  return hook_every_shard(m, model_chain_batches(m, C), q, lp, grad);
}

// The chain batches a regression shard's C chains run as at d covariates (host only: no device).
int stk_chain_batches(int32_t C, int32_t d, int32_t* sizes, int32_t cap) {
  ARG_CHECK(C >= 1 && d >= 1 && cap >= 0 && (sizes || cap == 0), "stk_chain_batches: need C >= 1, d >= 1, cap >= 0");
  const std::vector<int> b = chain_batches(C, d);
  ARG_CHECK(!b.empty(), "no sweep covers %d covariates (1..1024)", d);
  for (size_t i = 0; i < b.size() && (int32_t)i < cap; ++i) sizes[i] = b[i];
  return (int)b.size();
}

// A categorical shard's at K = ncat classes (host only: no device).
int stk_chain_batches_categorical(int32_t C, int32_t d, int32_t ncat, int32_t* sizes, int32_t cap) {
  ARG_CHECK(C >= 1 && d >= 1 && ncat >= 2 && cap >= 0 && (sizes || cap == 0),
            "stk_chain_batches_categorical: need C >= 1, d >= 1, ncat >= 2, cap >= 0");
  const std::vector<int> b = chain_batches_cat(C, ncat, d);
  ARG_CHECK(!b.empty(), "the categorical sweep does not cover K = %d classes at d = %d covariates: it needs K - 1 <= 16 and "
                        "(K - 1) ceil(d / 16) <= 16", ncat, d);
  for (size_t i = 0; i < b.size() && (int32_t)i < cap; ++i) sizes[i] = b[i];
  return (int)b.size();
}

int stk_categorical_supported(int32_t ncat, int32_t d) {
  return ncat >= 2 && d >= 1 && stk_sweep_cat_supported(ncat - 1, d) && (ncat - 1) * (d + 1) <= 1024 ? 1 : 0;
}

// A sparse shard's (host only: no device).
int stk_chain_batches_sparse(int32_t C, int32_t d, int32_t* sizes, int32_t cap) {
  ARG_CHECK(C >= 1 && d >= 1 && cap >= 0 && (sizes || cap == 0), "stk_chain_batches_sparse: need C >= 1, d >= 1, cap >= 0");
  const std::vector<int> b = chain_batches_sparse(C, d);
  ARG_CHECK(!b.empty(), "no sparse sweep covers %d covariates (1..1024)", d);
  for (size_t i = 0; i < b.size() && (int32_t)i < cap; ++i) sizes[i] = b[i];
  return (int)b.size();
}

// The sparse sweep one batch of C chains runs over a shard of n_rows x d whose longest row has K entries (host only).
int stk_sweep_launch_info_sparse(int64_t n_rows, int32_t d, int32_t K, int32_t C, int64_t out[8]) {
  ARG_CHECK(n_rows >= 1 && d >= 1 && out, "stk_sweep_launch_info_sparse: need n_rows >= 1, d >= 1 and out");
  ARG_CHECK(K >= 0 && K <= d, "stk_sweep_launch_info_sparse: K = %d; a row of d = %d covariates has 0 .. d entries", K, d);
  ARG_CHECK(stk_sweep_sparse_supported(C, d), "%d chains are not one batch of a sparse shard at %d covariates (stk_chain_batches_sparse)", C, d);
  const SweepLaunch p = stk_sweep_plan_sparse(n_rows, d, C);
  const int64_t v[8] = {p.kind, p.T, p.ld, p.G, (int64_t)p.lds, p.waves, (int64_t)p.T * K * 12 <= p.ld ? 1 : 0, 12 * (int64_t)K * n_rows};
  memcpy(out, v, sizeof(v));
  return STK_OK;
}

// The sweep one batch of C chains runs over a shard of n_rows x d (host only: no device).
// out: kind, T, the LD handed to the kernel, G, LDS bytes, 64-chain workspace bytes per shard.
int stk_sweep_launch_info(int64_t n_rows, int32_t d, int32_t C, int64_t out[6]) {
  ARG_CHECK(n_rows >= 1 && d >= 1 && out, "stk_sweep_launch_info: need n_rows >= 1, d >= 1 and out");
  ARG_CHECK(stk_sweep_supported(C, d), "%d chains are not one batch at %d covariates (stk_chain_batches)", C, d);
  const SweepLaunch p = stk_sweep_plan(n_rows, d, C, 0);
  ARG_CHECK(p.kind != SWEEP_NONE, "no sweep covers n = %lld rows of d = %d covariates at C = %d chains",
            (long long)n_rows, d, C);
  const int64_t v[6] = {p.kind, p.T, stk_sweep_args_ld(p), p.G, (int64_t)p.lds, (int64_t)p.ws_bytes};
  memcpy(out, v, sizeof(v));
  return STK_OK;
}

// ---------------------------------------------------------------- analytic Hessian (hessian.hip)
// The Hessian sweep's launch shape over a shard of n_rows x d (host only: no device).
// out: rows per tile, chunks per shard, waves per block, LDS bytes, chunk-partial workspace bytes per shard.
int stk_hessian_launch_info(int64_t n_rows, int32_t d, int64_t out[5]) {
  ARG_CHECK(n_rows >= 1 && d >= 1 && out, "stk_hessian_launch_info: need n_rows >= 1, d >= 1 and out");
  ARG_CHECK(stk_hessian_supported(d), "the Hessian sweep covers 1 <= d <= 128 covariates, not d = %d", d);
  const int64_t v[5] = {stk_hessian_rows_per_tile(), stk_hessian_chunks(n_rows), stk_hessian_waves(),
                        (int64_t)stk_hessian_lds_bytes(d), (int64_t)stk_hessian_ws_bytes(n_rows, d)};
  memcpy(out, v, sizeof(v));
  return STK_OK;
}

// One point per shard.  lp / grad come from stk_log_density_grad itself (one C = 1 sweep per shard), so
// they are its bits; the Hessians of all the call's shards are one sweep launch and one reduce launch.
int stk_log_density_hessian(stk_model* m, int shard, const double* q, double* lp, double* grad, double* hess) {
  ARG_CHECK(m && q && hess && shard >= -1 && shard < m->nshards, "stk_log_density_hessian: bad arguments");
  REFUSE_SPARSE(m, "stk_log_density_hessian");
  ARG_CHECK(is_regression(m->family), "stk_log_density_hessian: no Hessian sweep for the %s family (regressions only)",
            family_name(m->family));
  ARG_CHECK(stk_hessian_supported(m->d), "stk_log_density_hessian: the Hessian sweep covers 1 <= d <= 128 covariates, not d = %d",
            m->d);
  stk_ctx* ctx = m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int D = m->Dmax;
  const ShardRange r = shard_range(m, shard, stk_hessian_chunks);
  if (lp || grad) {
    for (int s = 0; s < r.nsh; ++s) {
      double lp1 = 0.0;   // stk_log_density_grad needs a place for lp
      RC(stk_log_density_grad(m, r.shard0 + s, q + (size_t)s * D, 1, lp ? lp + s : &lp1,
                              grad ? grad + (size_t)s * D : nullptr));
    }
  }
  size_t ws = 0;
  for (int s = r.shard0; s < r.shard0 + r.nsh; ++s) ws = std::max(ws, stk_hessian_ws_bytes(m->sh[s].n, m->d));
  const size_t qn = (size_t)r.nsh * D, hn = qn * D;
  RC(ctx->scratch[SCR_HESS_WS].ensure(ws * r.nsh));
  RC(ctx->scratch[SCR_HESS_QH].ensure(sizeof(double) * (qn + hn)));
  double* qb = ctx->scratch[SCR_HESS_QH].as<double>();
  double* hb = qb + qn;
  STK_HIP_CHECK(hipMemcpyAsync(qb, q, sizeof(double) * qn, hipMemcpyDefault, st));
  STK_HIP_CHECK(stk_launch_hessian(m->family, m->sh_dev.as<ShardDev>(), r.shard0, r.nsh, m->d, D, r.Gs, qb,
                                   ctx->scratch[SCR_HESS_WS].as<double>(), hb, st));
  STK_HIP_CHECK(hipMemcpyAsync(hess, hb, sizeof(double) * hn, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  return STK_OK;
}

// ---------------------------------------------------------------- pointwise log-predictive sweep (predictive.hip)
// The sweep's launch shape over a shard of n_rows x d against S draws (host only: no device).
// out: rows per tile, chunks per shard, waves per block, LDS bytes, draw-image bytes, chunk-partial
// workspace bytes per shard.
int stk_predictive_launch_info(int64_t n_rows, int32_t d, int32_t S, int64_t out[6]) {
  ARG_CHECK(n_rows >= 1 && d >= 1 && out, "stk_predictive_launch_info: need n_rows >= 1, d >= 1 and out");
  ARG_CHECK(stk_predictive_supported(d), "the log-predictive sweep covers 1 <= d <= 128 covariates, not d = %d", d);
  ARG_CHECK(S >= 1, "the log-predictive sweep needs S >= 1 draws, not S = %d", S);
  const int64_t v[6] = {stk_predictive_rows_per_tile(), stk_predictive_chunks(n_rows), stk_predictive_waves(),
                        (int64_t)stk_predictive_lds_bytes(d), (int64_t)stk_predictive_image_bytes(d, S),
                        (int64_t)stk_predictive_ws_bytes(n_rows)};
  memcpy(out, v, sizeof(v));
  return STK_OK;
}

int stk_log_predictive(stk_model* m, int shard, const double* q, int32_t S, double* rows, double* totals) {
  ARG_CHECK(m && shard >= -1 && shard < m->nshards, "stk_log_predictive: bad model or shard");
  REFUSE_SPARSE(m, "stk_log_predictive");
  ARG_CHECK(is_regression(m->family), "stk_log_predictive: no log-predictive sweep for the %s family (regressions only)",
            family_name(m->family));
  ARG_CHECK(stk_predictive_supported(m->d),
            "stk_log_predictive: the log-predictive sweep covers 1 <= d <= 128 covariates, not d = %d (%s family)", m->d,
            family_name(m->family));
  ARG_CHECK(S >= 1, "stk_log_predictive: S = %d draws; the %s family at d = %d needs S >= 1", S, family_name(m->family), m->d);
  ARG_CHECK(q, "stk_log_predictive: q is NULL (%s family, d = %d)", family_name(m->family), m->d);
  ARG_CHECK(rows || totals, "stk_log_predictive: rows and totals are both NULL (%s family, d = %d)", family_name(m->family),
            m->d);
  return rows_and_totals(m, shard, q, S, rows, totals, stk_launch_predictive, stk_predictive_chunks);
}

// ---------------------------------------------------------------- PSIS-LOO sweep (loo.hip)
// The sweep's launch shape over a shard of n_rows x d against S draws (host only: no device).
// out: rows per tile, chunks per shard, waves per block, LDS bytes, draw-image bytes, chunk-partial
// workspace bytes per shard.
int stk_loo_launch_info(int64_t n_rows, int32_t d, int32_t S, int64_t out[6]) {
  ARG_CHECK(n_rows >= 1 && d >= 1 && out, "stk_loo_launch_info: need n_rows >= 1, d >= 1 and out");
  ARG_CHECK(stk_loo_supported(d), "the PSIS-LOO sweep covers 1 <= d <= 128 covariates, not d = %d", d);
  ARG_CHECK(S >= 1, "the PSIS-LOO sweep needs S >= 1 draws, not S = %d", S);
  ARG_CHECK(S <= stk_loo_max_draws(), "the PSIS-LOO sweep keeps a row tile's draws in LDS: at most %d, not S = %d",
            stk_loo_max_draws(), S);
  const int64_t v[6] = {stk_loo_rows_per_tile(), stk_loo_chunks(n_rows), stk_loo_waves(S), (int64_t)stk_loo_lds_bytes(d, S),
                        (int64_t)stk_predictive_image_bytes(d, S), (int64_t)stk_loo_ws_bytes(n_rows)};
  memcpy(out, v, sizeof(v));
  return STK_OK;
}

int stk_loo(stk_model* m, int shard, const double* q, int32_t S, double* rows, double* totals) {
  ARG_CHECK(m && shard >= -1 && shard < m->nshards, "stk_loo: bad model or shard");
  REFUSE_SPARSE(m, "stk_loo");
  ARG_CHECK(is_regression(m->family), "stk_loo: no PSIS-LOO sweep for the %s family (regressions only)", family_name(m->family));
  ARG_CHECK(stk_loo_supported(m->d), "stk_loo: the PSIS-LOO sweep covers 1 <= d <= 128 covariates, not d = %d (%s family)",
            m->d, family_name(m->family));
  ARG_CHECK(S >= 1, "stk_loo: S = %d draws; the %s family at d = %d needs S >= 1", S, family_name(m->family), m->d);
  ARG_CHECK(S <= stk_loo_max_draws(),
            "stk_loo: S = %d draws; a row tile's draws are kept in LDS, at most %d (%s family, d = %d): pass a subset",
            S, stk_loo_max_draws(), family_name(m->family), m->d);
  ARG_CHECK(q, "stk_loo: q is NULL (%s family, d = %d)", family_name(m->family), m->d);
  ARG_CHECK(rows || totals, "stk_loo: rows and totals are both NULL (%s family, d = %d)", family_name(m->family), m->d);
  return rows_and_totals(m, shard, q, S, rows, totals, stk_launch_loo, stk_loo_chunks);
}

// ---------------------------------------------------------------- per-draw log-density sweep (logdens.hip)
// The sweep's launch shape over a shard of n_rows x d against S draws (host only: no device).
// out: rows per tile, chunks per shard, waves per block, LDS bytes, draw-image bytes, chunk-partial
// workspace bytes per shard.  Only the last two depend on S.
int stk_logdens_launch_info(int64_t n_rows, int32_t d, int32_t S, int64_t out[6]) {
  ARG_CHECK(n_rows >= 1 && d >= 1 && out, "stk_logdens_launch_info: need n_rows >= 1, d >= 1 and out");
  ARG_CHECK(stk_logdens_supported(d), "the per-draw log-density sweep covers 1 <= d <= 128 covariates, not d = %d", d);
  ARG_CHECK(S >= 1, "the per-draw log-density sweep needs S >= 1 draws, not S = %d", S);
  const int64_t v[6] = {stk_logdens_rows_per_tile(), stk_logdens_chunks(n_rows), stk_logdens_waves(),
                        (int64_t)stk_logdens_lds_bytes(d), (int64_t)stk_predictive_image_bytes(d, S),
                        (int64_t)stk_logdens_ws_bytes(n_rows, S)};
  memcpy(out, v, sizeof(v));
  return STK_OK;
}

// The same S draws against one shard or (shard == -1) every shard: one preparation launch (the
// log-predictive sweep's draw image), one sweep launch and one reduce launch for all of them.
int stk_log_density_draws(stk_model* m, int shard, const double* q, int32_t S, double* lp) {
  ARG_CHECK(m && shard >= -1 && shard < m->nshards, "stk_log_density_draws: bad model or shard");
  REFUSE_SPARSE(m, "stk_log_density_draws");
  ARG_CHECK(is_regression(m->family), "stk_log_density_draws: no per-draw log-density sweep for the %s family (regressions only)",
            family_name(m->family));
  ARG_CHECK(stk_logdens_supported(m->d),
            "stk_log_density_draws: the per-draw log-density sweep covers 1 <= d <= 128 covariates, not d = %d (%s family)",
            m->d, family_name(m->family));
  ARG_CHECK(S >= 1, "stk_log_density_draws: S = %d draws; the %s family at d = %d needs S >= 1", S, family_name(m->family),
            m->d);
  ARG_CHECK(q && lp, "stk_log_density_draws: q or lp is NULL (%s family, d = %d)", family_name(m->family), m->d);
  stk_ctx* ctx = m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int D = m->Dmax;
  const ShardRange r = shard_range(m, shard, stk_logdens_chunks);
  const size_t Sp = (size_t)16 * stk_predictive_tiles(S), lpn = (size_t)r.nsh * S;
  RC(ctx->scratch[SCR_DRAW_PARTIAL].ensure(sizeof(double) * (size_t)r.nsh * r.Gs * Sp));
  DrawImage di;
  RC(stage_draws(m, q, S, lpn, &di));
  double* lpb = di.q + (size_t)S * D;
  STK_HIP_CHECK(stk_launch_logdens(m->family, m->sh_dev.as<ShardDev>(), r.shard0, r.nsh, m->d, D, r.Gs, S, di.img, di.q,
                                   ctx->scratch[SCR_DRAW_PARTIAL].as<double>(), lpb, st));
  STK_HIP_CHECK(hipMemcpyAsync(lp, lpb, sizeof(double) * lpn, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  return STK_OK;
}

// ---------------------------------------------------------------- weighted bootstrap sweep (boot.hip)
// The sweep's launch shape over a shard of n_rows x d (host only: no device).
// out: rows per sub-tile, chunks per shard, waves per block, LDS bytes, chunk-partial workspace bytes per shard
// and tile of 16 replicates.
int stk_boot_launch_info(int64_t n_rows, int32_t d, int64_t out[5]) {
  ARG_CHECK(n_rows >= 1 && d >= 1 && out, "stk_boot_launch_info: need n_rows >= 1, d >= 1 and out");
  ARG_CHECK(stk_boot_supported(d), "the bootstrap sweep covers 1 <= d <= 128 covariates, not d = %d", d);
  const int64_t v[5] = {stk_boot_rows_per_tile(), stk_boot_chunks(n_rows), stk_boot_waves(), (int64_t)stk_boot_lds_bytes(d),
                        (int64_t)stk_boot_ws_bytes(n_rows, d)};
  memcpy(out, v, sizeof(v));
  return STK_OK;
}

int stk_boot_poisson_thresholds(uint32_t out[13]) {
  ARG_CHECK(out, "stk_boot_poisson_thresholds: out is NULL");
  boot_poisson_thresholds(out);
  return STK_OK;
}

// The twin of the kernel's weights: boot_math.h's boot_weight, row by row (host only: no device, no context).
int stk_boot_weights_host(uint64_t seed, uint32_t stream, int64_t row0, int64_t nrows, int32_t rep0, int32_t R, int32_t kind,
                          double* out) {
  ARG_CHECK(out, "stk_boot_weights_host: out is NULL");
  ARG_CHECK(kind == BOOT_POISSON || kind == BOOT_EXPONENTIAL,
            "stk_boot_weights_host: kind = %d; the weights are 0 (poisson) or 1 (exponential)", kind);
  ARG_CHECK(row0 >= 0 && nrows >= 0, "stk_boot_weights_host: row0 = %lld, nrows = %lld; need both >= 0", (long long)row0,
            (long long)nrows);
  ARG_CHECK(R >= 1, "stk_boot_weights_host: R = %d replicates; need R >= 1", R);
  ARG_CHECK(rep0 >= 0 && (int64_t)rep0 + R <= BOOT_MAX_REPS,
            "stk_boot_weights_host: replicates rep0 = %d .. rep0 + R = %d; a replicate index is below %d", rep0, rep0 + R,
            BOOT_MAX_REPS);
  ARG_CHECK(stream < BOOT_MAX_STREAM, "stk_boot_weights_host: stream = %u; a stream is below 2^20 = %u", stream, BOOT_MAX_STREAM);
  for (int64_t r = 0; r < nrows; ++r)
    for (int32_t b = 0; b < R; ++b) out[r * R + b] = boot_weight(seed, stream, row0 + r, (uint32_t)(rep0 + b), kind);
  return STK_OK;
}

// R replicates against one shard or (shard == -1) every shard at the same points: per tile of 16 replicates
// one sweep launch and one reduce launch for all of them.  The points are staged as [tiles * 16][Dp] with the
// last one repeated to fill the last tile; only the live columns are reduced.
int stk_log_density_grad_boot(stk_model* m, int shard, const double* q, int32_t R, int32_t rep0, uint64_t seed,
                              const int32_t* streams, int32_t kind, double* lp, double* grad, double* wsum) {
  ARG_CHECK(m && shard >= -1 && shard < m->nshards, "stk_log_density_grad_boot: bad model or shard");
  REFUSE_SPARSE(m, "stk_log_density_grad_boot");
  ARG_CHECK(is_regression(m->family), "stk_log_density_grad_boot: no bootstrap sweep for the %s family (regressions only)",
            family_name(m->family));
  ARG_CHECK(stk_boot_supported(m->d),
            "stk_log_density_grad_boot: the bootstrap sweep covers 1 <= d <= 128 covariates, not d = %d (%s family)", m->d,
            family_name(m->family));
  ARG_CHECK(kind == BOOT_POISSON || kind == BOOT_EXPONENTIAL,
            "stk_log_density_grad_boot: kind = %d; the weights are 0 (poisson) or 1 (exponential)", kind);
  ARG_CHECK(R >= 1, "stk_log_density_grad_boot: R = %d replicates; need R >= 1", R);
  ARG_CHECK(rep0 >= 0 && rep0 % 16 == 0, "stk_log_density_grad_boot: rep0 = %d; the first replicate is a multiple of 16", rep0);
  ARG_CHECK((int64_t)rep0 + R <= BOOT_MAX_REPS,
            "stk_log_density_grad_boot: rep0 + R = %lld; a replicate index is below %d", (long long)rep0 + R, BOOT_MAX_REPS);
  ARG_CHECK(q && lp, "stk_log_density_grad_boot: q or lp is NULL (%s family, d = %d)", family_name(m->family), m->d);
  const ShardRange r = shard_range(m, shard, stk_boot_chunks);
  std::vector<int32_t> sv(r.nsh);
  for (int s = 0; s < r.nsh; ++s) {
    sv[s] = streams ? streams[s] : r.shard0 + s;
    ARG_CHECK(sv[s] >= 0 && (uint32_t)sv[s] < BOOT_MAX_STREAM,
              "stk_log_density_grad_boot: stream = %d of shard %d; a stream is in 0 .. 2^20 - 1", sv[s], r.shard0 + s);
    const int64_t n = m->sh[r.shard0 + s].n;
    ARG_CHECK(stk_boot_chunk_rows(n) * m->d * 8 < (int64_t)1 << 31,
              "stk_log_density_grad_boot: shard %d: a chunk of n = %lld rows of d = %d covariates must fit a buffer "
              "descriptor: split the shard", r.shard0 + s, (long long)n, m->d);
  }
  stk_ctx* ctx = m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int D = m->Dmax, Dp = (D + 7) / 8 * 8, d = m->d;
  const int ntile = (R + 15) / 16;
  const size_t qn = (size_t)ntile * 16 * Dp, lpn = (size_t)r.nsh * R, gn = lpn * D;
  const size_t sbytes = (sizeof(int32_t) * r.nsh + 7) / 8 * 8;
  RC(ctx->scratch[SCR_BOOT_IO].ensure(sizeof(double) * (qn + 2 * lpn + gn) + sbytes));
  RC(ctx->scratch[SCR_BOOT_PARTIAL].ensure(sizeof(double) * (size_t)r.nsh * r.Gs * 16 * (d + 3)));
  double* qb = ctx->scratch[SCR_BOOT_IO].as<double>();
  double* lpb = qb + qn;
  double* wsb = lpb + lpn;
  double* gb = wsb + lpn;
  int32_t* sb = reinterpret_cast<int32_t*>(gb + gn);
  const size_t pitch = sizeof(double) * Dp, width = sizeof(double) * D;
  STK_HIP_CHECK(hipMemcpy2DAsync(qb, pitch, q, width, width, R, hipMemcpyDefault, st));
  for (int c = R; c < ntile * 16; ++c)
    STK_HIP_CHECK(hipMemcpyAsync(qb + (size_t)c * Dp, q + (size_t)(R - 1) * D, width, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipMemcpyAsync(sb, sv.data(), sizeof(int32_t) * r.nsh, hipMemcpyHostToDevice, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));   // sv is a local
  for (int t = 0; t < ntile; ++t)
    STK_HIP_CHECK(stk_launch_boot(m->family, m->sh_dev.as<ShardDev>(), r.shard0, r.nsh, d, r.Gs, Dp, qb + (size_t)t * 16 * Dp,
                                  ctx->scratch[SCR_BOOT_PARTIAL].as<double>(), sb, seed, rep0 + 16 * t, kind, R, 16 * t,
                                  std::min(16, R - 16 * t), lpb, gb, wsb, st));
  STK_HIP_CHECK(hipMemcpyAsync(lp, lpb, sizeof(double) * lpn, hipMemcpyDefault, st));
  if (grad) STK_HIP_CHECK(hipMemcpyAsync(grad, gb, sizeof(double) * gn, hipMemcpyDefault, st));
  if (wsum) STK_HIP_CHECK(hipMemcpyAsync(wsum, wsb, sizeof(double) * lpn, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  return STK_OK;
}

// ---------------------------------------------------------------- Laplace proposal (logdens.hip)
int stk_laplace_draws(stk_ctx* ctx, const double* mode, const double* factor, int32_t D, int32_t S, uint64_t seed,
                      uint32_t stream, double* q_out, double* log_q_out) {
  ARG_CHECK(ctx && mode && factor && q_out && log_q_out, "stk_laplace_draws: a NULL argument");
  ARG_CHECK(D >= 1 && D <= stk_laplace_max_dim(), "stk_laplace_draws: D = %d parameters; the generator covers 1 <= D <= %d", D,
            stk_laplace_max_dim());
  ARG_CHECK(S >= 1, "stk_laplace_draws: S = %d draws; need S >= 1", S);
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nD = (size_t)D, qn = (size_t)S * D;
  RC(ctx->scratch[SCR_LAPLACE].ensure(sizeof(double) * (nD + nD * nD + qn + (size_t)S)));
  double* mb = ctx->scratch[SCR_LAPLACE].as<double>();
  double* fb = mb + nD;
  double* qb = fb + nD * nD;
  double* lb = qb + qn;
  STK_HIP_CHECK(hipMemcpyAsync(mb, mode, sizeof(double) * nD, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipMemcpyAsync(fb, factor, sizeof(double) * nD * nD, hipMemcpyDefault, st));
  STK_HIP_CHECK(stk_launch_laplace_draws(mb, fb, D, S, seed, stream, qb, lb, st));
  STK_HIP_CHECK(hipMemcpyAsync(q_out, qb, sizeof(double) * qn, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipMemcpyAsync(log_q_out, lb, sizeof(double) * (size_t)S, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  return STK_OK;
}

// ---------------------------------------------------------------- posterior predictive replicates (ppc.hip)
// The sweep's launch shape over a shard of n_rows x d against S draws (host only: no device).
// out: rows per tile, chunks per shard, waves per block, LDS bytes, draw-image bytes, chunk-partial
// workspace bytes per shard.  Only the last two depend on S.
int stk_ppc_launch_info(int64_t n_rows, int32_t d, int32_t S, int64_t out[6]) {
  ARG_CHECK(n_rows >= 1 && d >= 1 && out, "stk_ppc_launch_info: need n_rows >= 1, d >= 1 and out");
  ARG_CHECK(stk_ppc_supported(d), "the posterior predictive sweep covers 1 <= d <= 128 covariates, not d = %d", d);
  ARG_CHECK(S >= 1, "the posterior predictive sweep needs S >= 1 draws, not S = %d", S);
  const int64_t v[6] = {stk_ppc_rows_per_tile(), stk_ppc_chunks(n_rows), stk_ppc_waves(), (int64_t)stk_ppc_lds_bytes(d),
                        (int64_t)stk_predictive_image_bytes(d, S), (int64_t)stk_ppc_ws_bytes(n_rows, S)};
  memcpy(out, v, sizeof(v));
  return STK_OK;
}

// The twin of the kernel's replicates: yrep_math.h's yrep_element, element by element, on the caller's eta
// (host only: no device, no context).  The exp table is the kernel's, 2^(j/1024).
int stk_yrep_host(int32_t family, uint64_t seed, uint32_t stream, int64_t row0, int64_t nrows, int32_t draw0, int32_t S,
                  const double* eta, const double* u, double* out, double* margin) {
  ARG_CHECK(is_regression(family), "stk_yrep_host: no replicates for the %s family (regressions only)", family_name(family));
  ARG_CHECK(eta && out, "stk_yrep_host: eta or out is NULL");
  ARG_CHECK(family != STK_LINREG || u, "stk_yrep_host: the linear family needs u = log sigma of every draw");
  ARG_CHECK(row0 >= 0 && nrows >= 0 && row0 + nrows <= (int64_t)1 << 40,
            "stk_yrep_host: rows row0 = %lld .. row0 + nrows = %lld; a row index is in 0 .. 2^40 - 1", (long long)row0,
            (long long)(row0 + nrows));
  ARG_CHECK(S >= 1, "stk_yrep_host: S = %d draws; need S >= 1", S);
  ARG_CHECK(draw0 >= 0 && (int64_t)draw0 + S <= YREP_MAX_DRAWS,
            "stk_yrep_host: draws draw0 = %d .. draw0 + S = %lld; a draw index is below 2^24", draw0, (long long)draw0 + S);
  ARG_CHECK(stream < YREP_MAX_STREAM, "stk_yrep_host: stream = %u; a stream is below 2^20 = %u", stream, YREP_MAX_STREAM);
  static const std::vector<double> tab = [] {
    std::vector<double> t(1024);
    for (int i = 0; i < 1024; ++i) t[i] = exp2((double)i / 1024.0);
    return t;
  }();
  for (int64_t r = 0; r < nrows; ++r)
    for (int32_t c = 0; c < S; ++c) {
      const size_t k = (size_t)r * S + c;
      double mg = HUGE_VAL;
      out[k] = yrep_element(family, seed, stream, row0 + r, (uint32_t)(draw0 + c), eta[k], u ? u[c] : 0.0, tab.data(),
                            margin ? &mg : nullptr);
      if (margin) margin[k] = mg;
    }
  return STK_OK;
}

// The same S draws against one shard or (shard == -1) every shard: one preparation launch (the log-predictive
// sweep's draw image), one sweep launch, one launch over y and one reduce launch for all of them.  rows and yrep
// are written in place when they are memory of the context's device, else through a staging buffer.
int stk_posterior_predict(stk_model* m, int shard, const double* q, int32_t S, int32_t draw0, uint64_t seed,
                          const int32_t* streams, double* stats, double* obs, double* rows, double* yrep) {
  ARG_CHECK(m && shard >= -1 && shard < m->nshards, "stk_posterior_predict: bad model or shard");
  REFUSE_SPARSE(m, "stk_posterior_predict");
  ARG_CHECK(is_regression(m->family), "stk_posterior_predict: no posterior predictive sweep for the %s family (regressions only)",
            family_name(m->family));
  ARG_CHECK(stk_ppc_supported(m->d),
            "stk_posterior_predict: the posterior predictive sweep covers 1 <= d <= 128 covariates, not d = %d (%s family)",
            m->d, family_name(m->family));
  ARG_CHECK(S >= 1, "stk_posterior_predict: S = %d draws; the %s family at d = %d needs S >= 1", S, family_name(m->family),
            m->d);
  ARG_CHECK(draw0 >= 0 && (int64_t)draw0 + S <= YREP_MAX_DRAWS,
            "stk_posterior_predict: draws draw0 = %d .. draw0 + S = %lld; a draw index is in 0 .. 2^24 - 1", draw0,
            (long long)draw0 + S);
  ARG_CHECK(q, "stk_posterior_predict: q is NULL (%s family, d = %d)", family_name(m->family), m->d);
  ARG_CHECK(stats, "stk_posterior_predict: stats is NULL (%s family, d = %d)", family_name(m->family), m->d);
  const ShardRange r = shard_range(m, shard, stk_ppc_chunks);
  const int nsh = r.nsh;
  std::vector<int32_t> sv(nsh);
  std::vector<int64_t> off(nsh);
  int64_t nrows = 0;
  for (int s = 0; s < nsh; ++s) {
    sv[s] = streams ? streams[s] : r.shard0 + s;
    ARG_CHECK(sv[s] >= 0 && (uint32_t)sv[s] < YREP_MAX_STREAM,
              "stk_posterior_predict: stream = %d of shard %d; a stream is in 0 .. 2^20 - 1", sv[s], r.shard0 + s);
    off[s] = nrows;
    nrows += m->sh[r.shard0 + s].n;
  }
  stk_ctx* ctx = m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t Sp = (size_t)128 * stk_predictive_tiles(S) + 8;       // doubles per chunk (stk_ppc_ws_bytes)
  const size_t wn = (size_t)nsh * r.Gs * Sp, sn = (size_t)nsh * S * 8, on = (size_t)nsh * 8;
  RC(ctx->scratch[SCR_DRAW_PARTIAL].ensure(sizeof(double) * (wn + sn + on) + sizeof(int64_t) * nsh + sizeof(int32_t) * nsh));
  double* partial = ctx->scratch[SCR_DRAW_PARTIAL].as<double>();
  double* sb = partial + wn;
  double* ob = sb + sn;
  int64_t* offb = reinterpret_cast<int64_t*>(ob + on);
  int32_t* strb = reinterpret_cast<int32_t*>(offb + nsh);
  const size_t rn = (size_t)nrows * 4, yn = (size_t)nrows * S;
  const bool rows_staged = rows && !is_device_ptr(rows, ctx->device), yrep_staged = yrep && !is_device_ptr(yrep, ctx->device);
  if (rows_staged || yrep_staged)
    RC(ctx->scratch[SCR_DRAW_ROWS].ensure(sizeof(double) * ((rows_staged ? rn : 0) + (yrep_staged ? yn : 0))));
  double* rb = rows_staged ? ctx->scratch[SCR_DRAW_ROWS].as<double>() : rows;
  double* yb = yrep_staged ? ctx->scratch[SCR_DRAW_ROWS].as<double>() + (rows_staged ? rn : 0) : yrep;
  DrawImage di;                              // every buffer is there before anything is queued
  RC(stage_draws(m, q, S, 0, &di));
  STK_HIP_CHECK(hipMemcpyAsync(offb, off.data(), sizeof(int64_t) * nsh, hipMemcpyHostToDevice, st));
  STK_HIP_CHECK(hipMemcpyAsync(strb, sv.data(), sizeof(int32_t) * nsh, hipMemcpyHostToDevice, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));   // off and sv are locals
  STK_HIP_CHECK(stk_launch_ppc(m->family, m->sh_dev.as<ShardDev>(), r.shard0, nsh, m->d, r.Gs, S, draw0, seed, strb, di.img,
                               partial, sb, ob, rb, yb, offb, st));
  STK_HIP_CHECK(hipMemcpyAsync(stats, sb, sizeof(double) * sn, hipMemcpyDefault, st));
  if (obs) STK_HIP_CHECK(hipMemcpyAsync(obs, ob, sizeof(double) * on, hipMemcpyDefault, st));
  if (rows_staged) STK_HIP_CHECK(hipMemcpyAsync(rows, rb, sizeof(double) * rn, hipMemcpyDefault, st));
  if (yrep_staged) STK_HIP_CHECK(hipMemcpyAsync(yrep, yb, sizeof(double) * yn, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  return STK_OK;
}

}  // extern "C"
