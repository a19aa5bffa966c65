// C ABI of libstark_hip.so: the sampler -- create, run, info, draws, adaptation.
#include "capi_internal.h"

// ---------------------------------------------------------------- the sampler's device buffers
template <class T>
static SamplerBuf buf_of(T*& field, size_t count, bool saved = true) { return {&field, sizeof(T) * count, saved}; }

// The checkpoint segments first, in the blob's order (state_blob.h: version 2).
std::vector<SamplerBuf> sampler_buffers(stk_sampler* s) {
  NutsArgs& A = s->A;
  const size_t n = (size_t)A.nchains, Dp = (size_t)A.Dp, md = (size_t)A.max_depth;
  const size_t nsh = (size_t)s->m->nshards, S = (size_t)A.S_total;
  std::vector<SamplerBuf> b = {
      buf_of(A.vec, n * V_COUNT * Dp),
      buf_of(A.stk, n * md * SV_COUNT * Dp),
      buf_of(A.sc, n * S_COUNT),
      buf_of(A.stks, n * md * SS_COUNT),
      buf_of(A.iv, n * I_COUNT),
      buf_of(A.cnt, n * C_COUNT),
      buf_of(A.qeval, n * Dp),
      // g_in and lp_in are one block, [nchains][Dp] then [nchains]: the unit of the full-data
      // all-reduce, and in a checkpoint [grad | lp] at the pending requests
      buf_of(A.g_in, n * Dp + n),
      buf_of(A.draws, nsh * A.Pmax * S),
      buf_of(A.stats, nsh * S * N_STATS),
      buf_of(A.udraws, n * (size_t)A.ud_iters * Dp),
      buf_of(A.req_step, nsh)};
  if (A.metric == 1)   // dense_e: the chains' matrices (M^-1, its factor, the window's M2)
    for (double** mat : {&A.d_minv, &A.d_chol, &A.d_m2}) b.push_back(buf_of(*mat, n * Dp * Dp));
  if (s->cfg.shard_ids) b.push_back(buf_of(A.shard_ids, nsh, false));   // the caller's, uploaded once
  return b;
}

static int sbuf(stk_sampler* s, size_t bytes, void** p) {
  s->bufs.emplace_back();
  RC(s->bufs.back().ensure(bytes));
  *p = s->bufs.back().p;
  return STK_OK;
}

// ---------------------------------------------------------------- creation
// dense_e: the caller's D x D initial inverse metric, checked and factored once on the host.
// minv / chol come back [Dp][Dp] with zero padding (chol lower, M^-1 = L L^T).
static int dense_metric_host(const double* src, int D, int Dp, std::vector<double>* minv, std::vector<double>* chol) {
  std::vector<double> a((size_t)D * D);
  if (hipMemcpy(a.data(), src, sizeof(double) * a.size(), hipMemcpyDefault) != hipSuccess) {
    stk_set_error("inv_metric_dense: cannot read %d x %d doubles", D, D);
    return STK_E_ARG;
  }
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      const double x = a[(size_t)i * D + j], y = a[(size_t)j * D + i];
      ARG_CHECK(std::isfinite(x), "inv_metric_dense[%d][%d] is not finite", i, j);
      ARG_CHECK(std::fabs(x - y) <= 1e-12 * std::max(std::fabs(x), std::fabs(y)),
                "inv_metric_dense is not symmetric: [%d][%d] = %.17g, [%d][%d] = %.17g", i, j, x, j, i, y);
    }
  minv->assign((size_t)Dp * Dp, 0.0);
  chol->assign((size_t)Dp * Dp, 0.0);
  for (int i = 0; i < D; ++i)
    for (int j = 0; j <= i; ++j) {   // the lower triangle, mirrored: symmetric to the bit
      (*minv)[(size_t)i * Dp + j] = (*minv)[(size_t)j * Dp + i] = a[(size_t)i * D + j];
      (*chol)[(size_t)i * Dp + j] = a[(size_t)i * D + j];
    }
  double* L = chol->data();
  for (int k = 0; k < D; ++k) {
    const double piv = L[(size_t)k * Dp + k];
    ARG_CHECK(piv > 0.0, "inv_metric_dense is not positive definite (pivot %d = %g)", k, piv);
    const double d = std::sqrt(piv);
    L[(size_t)k * Dp + k] = d;
    for (int i = k + 1; i < D; ++i) L[(size_t)i * Dp + k] /= d;
    for (int i = k + 1; i < D; ++i) {
      const double ci = L[(size_t)i * Dp + k];
      for (int j = k + 1; j <= i; ++j) L[(size_t)i * Dp + j] -= ci * L[(size_t)j * Dp + k];
    }
  }
  return STK_OK;
}

// Step 1: the config alone, against the model's family and dimension.  No device.
static int check_config(const stk_model* m, const stk_config* cfg, int nch) {
  ARG_CHECK(cfg->num_warmup >= 0 && cfg->num_samples > 0 && cfg->chains > 0, "need num_warmup>=0, num_samples>0, chains>0");
  ARG_CHECK(cfg->max_depth >= 1 && cfg->max_depth <= 30, "max_depth must be in [1, 30]");
  ARG_CHECK(cfg->adapt_delta > 0 && cfg->adapt_delta < 1, "adapt_delta must be in (0, 1)");
  ARG_CHECK(cfg->stepsize > 0, "stepsize must be positive");
  ARG_CHECK(cfg->stepsize_jitter >= 0 && cfg->stepsize_jitter <= 1, "stepsize_jitter must be in [0, 1]");
  ARG_CHECK(cfg->nuts_criterion == 0 || cfg->nuts_criterion == 1, "nuts_criterion must be 0 (Stan 2.19) or 1 (Stan >= 2.23)");
  ARG_CHECK(cfg->chains_per_wave >= 0 && cfg->chains_per_wave <= 4 && cfg->chains_per_wave != 3,
            "chains_per_wave must be 0, 1, 2 or 4");
  ARG_CHECK(cfg->metric >= 0 && cfg->metric <= 2, "metric must be 0 (diag_e), 1 (dense_e) or 2 (unit_e)");
  ARG_CHECK(cfg->metric != 1 || m->family != STK_SCHOOLS,
            "metric dense_e is for the regression families (linear, logistic, poisson, neg_binomial, student_t, gamma, categorical): the fused 8-schools kernel "
            "has no dense form; use diag_e or unit_e");
  ARG_CHECK(nch > 0, "dimension %d too large (max 1024)", m->Dmax);
  if (m->family == STK_SCHOOLS) {
    ARG_CHECK(nch <= 2, "8-schools supports J <= 126");
    // the fused kernel keeps a chain's vectors and its max_depth-deep tree stack in LDS
    NutsArgs G{};
    G.Dp = (m->Dmax + 7) / 8 * 8;
    G.max_depth = cfg->max_depth;
    G.uturn_ext = cfg->nuts_criterion;
    G.cpw_cap = cfg->chains_per_wave;
    const size_t lds = stk_fused_lds_bytes(G, nch);
    ARG_CHECK(lds <= BIG_LDS_BYTES,
              "8-schools with J = %d at max_depth %d (nuts_criterion %d) needs %zu bytes of LDS per workgroup, the limit is %zu: "
              "lower max_depth",
              m->Dmax - 2, cfg->max_depth, cfg->nuts_criterion, lds, BIG_LDS_BYTES);
  } else {
    RC(model_ready(m));
    ARG_CHECK(!model_chain_batches(m, cfg->chains).empty(), "no sweep covers %d covariates (1..1024)", m->d);
  }
  return STK_OK;
}

// Step 2: every NutsArgs field but the buffer pointers.
static void fill_args(const stk_model* m, const stk_config* cfg, NutsArgs* args) {
  NutsArgs& A = *args;
  A.nchains = m->nshards * cfg->chains;
  A.C = cfg->chains;
  A.Dp = (m->Dmax + 7) / 8 * 8;
  // The NUTS kernels read the family only for the draw layout (schools; or the last unconstrained
  // coordinate written as its exp): the negative binomial's phi = e^v sits where the linear sigma does, and
  // student_t's sigma = e^s is the linear sigma; so does the gamma family's shape = e^u.
  // categorical writes q as it is, lp__ last: the logistic layout at D = (K - 1)(d + 1).
  A.family = (m->family == STK_NEGBIN || m->family == STK_STUDENT || m->family == STK_GAMMA) ? STK_LINREG
             : m->family == STK_CATEGORICAL                                                  ? STK_LOGREG
                                                                                             : m->family;
  A.max_depth = cfg->max_depth;
  A.num_warmup = cfg->num_warmup;
  A.num_samples = cfg->num_samples;
  A.total_iters = cfg->num_warmup + cfg->num_samples;
  A.adapt = cfg->adapt_engaged && cfg->num_warmup > 0;
  A.skip_ss = cfg->skip_init_stepsize;
  A.iter_offset = cfg->iter_offset;
  unsigned nw = (unsigned)cfg->num_warmup, ib = (unsigned)cfg->adapt_init_buffer, tb = (unsigned)cfg->adapt_term_buffer,
           bw = (unsigned)cfg->adapt_window;
  A.var_on = A.adapt && nw >= 20 && cfg->metric != 2;   // unit_e: the step size alone adapts
  A.metric = cfg->metric;
  if (A.var_on && ib + bw + tb > nw) {   // windowed_adaptation::set_window_params, 15%/75%/10%
    ib = (unsigned)(0.15 * nw);
    tb = (unsigned)(0.1 * nw);
    bw = nw - (ib + tb);
  }
  A.init_buffer = ib;
  A.term_buffer = tb;
  A.base_window = bw;
  A.delta = cfg->adapt_delta;
  A.gamma = cfg->adapt_gamma;
  A.kappa = cfg->adapt_kappa;
  A.t0 = cfg->adapt_t0;
  A.seed = cfg->seed;
  A.jitter = cfg->stepsize_jitter;
  A.uturn_ext = cfg->nuts_criterion;
  A.cpw_cap = cfg->chains_per_wave;
  A.S_total = cfg->chains * cfg->num_samples;
  A.Pmax = m->Pmax;
  A.shards = m->sh_dev.as<ShardDev>();
  A.ud_first = cfg->save_warmup ? 0 : cfg->num_warmup;
  A.ud_iters = A.total_iters - A.ud_first;
}

// Step 3: the caller's init, shard_ids and metric on the device.  The init kernels' inputs come back.
struct InitInputs { double *init = nullptr, *inv_metric = nullptr, *minv = nullptr, *chol = nullptr; };
static int upload_inputs(stk_sampler* s, const std::vector<double>& minv_host, const std::vector<double>& chol_host,
                         InitInputs* in) {
  const stk_model* m = s->m;
  const stk_config* cfg = &s->cfg;
  const NutsArgs& A = s->A;
  const size_t Dp = A.Dp;
  void* p;
  if (!minv_host.empty()) {
    const size_t mb = sizeof(double) * Dp * Dp;
    RC(sbuf(s, 2 * mb, &p));
    in->minv = (double*)p;
    in->chol = in->minv + Dp * Dp;
    if (hipMemcpy(in->minv, minv_host.data(), mb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(in->chol, chol_host.data(), mb, hipMemcpyHostToDevice) != hipSuccess)
      return STK_E_HIP;
  }
  if (cfg->init) {
    // init is nshards * chains * D with per-shard D; k_nuts_init reads init[gid * Dp + e], one
    // stride for every chain (a stride of the chain's own D lets a short shard's chains land on
    // the elements of a longer shard before it)
    std::vector<double> packed((size_t)A.nchains * Dp, 0.0);
    size_t off = 0;
    for (int sh = 0; sh < m->nshards; ++sh) {
      const int D = m->sh[sh].D;
      for (int c = 0; c < cfg->chains; ++c, off += D)
        if (hipMemcpy(&packed[(size_t)(sh * cfg->chains + c) * Dp], cfg->init + off, sizeof(double) * D, hipMemcpyDefault) !=
            hipSuccess)
          return STK_E_ARG;
    }
    RC(sbuf(s, sizeof(double) * packed.size(), &p));
    in->init = (double*)p;
    if (hipMemcpy(in->init, packed.data(), sizeof(double) * packed.size(), hipMemcpyHostToDevice) != hipSuccess)
      return STK_E_HIP;
  }
  if (cfg->shard_ids) {
    std::vector<int32_t> ids(m->nshards);
    ARG_CHECK(hipMemcpy(ids.data(), cfg->shard_ids, sizeof(int32_t) * ids.size(), hipMemcpyDefault) == hipSuccess &&
                  *std::min_element(ids.begin(), ids.end()) >= 0,
              "shard_ids: unreadable or negative");
    if (hipMemcpy(const_cast<int*>(A.shard_ids), ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice) != hipSuccess)
      return STK_E_HIP;
  }
  if (cfg->inv_metric && cfg->metric == 0) {
    RC(sbuf(s, sizeof(double) * m->Dmax, &p));
    in->inv_metric = (double*)p;
    if (hipMemcpy(in->inv_metric, cfg->inv_metric, sizeof(double) * m->Dmax, hipMemcpyDefault) != hipSuccess) return STK_E_HIP;
  }
  return STK_OK;
}

// Everything of a new sampler that can fail: on an error the caller destroys it.
static int sampler_init(stk_sampler* s, ChainPlan* plan, const std::vector<double>& minv_host,
                        const std::vector<double>& chol_host) {
  stk_model* m = s->m;
  hipStream_t st = m->ctx->stream;
  NutsArgs& A = s->A;
  // Every checkpoint segment starts zeroed, so a saved state is a function of the run and never of
  // what the allocator handed out.  Two of them need it to run: draws, and the tree stack (the
  // fused kernel's zero-padding form relies on +0 in every padding slot).
  for (const SamplerBuf& b : sampler_buffers(s)) {
    void* p;
    RC(sbuf(s, b.bytes, &p));
    b.set(p);
    if (b.saved) STK_HIP_CHECK(hipMemsetAsync(p, 0, b.bytes, st));
  }
  A.lp_in = A.g_in + (size_t)A.nchains * A.Dp;
  InitInputs in;
  RC(upload_inputs(s, minv_host, chol_host, &in));
  if (m->family != STK_SCHOOLS) {
    RC(s->partial.ensure(plan->partial_bytes));
    if (plan->ws_bytes) {
      RC(s->ws.ensure(plan->ws_bytes));
      s->sws = stk_sweep_ws(s->ws.p, plan->ws_at, m->nshards);
    }
    s->plan = std::move(*plan);
    RC(s->ran.ensure(sizeof(int) * 64));
  }
  hipError_t e = stk_launch_nuts_init(A, in.init, in.inv_metric, s->cfg.stepsize, s->cfg.init_radius, st);
  if (e == hipSuccess && A.metric == 1) e = stk_launch_dense_init(A, in.minv, in.chol, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    stk_set_error("sampler init: %s", hipGetErrorString(e));
    return STK_E_HIP;
  }
  s->iv_host.resize((size_t)A.nchains * I_COUNT);
  s->cnt_host.resize((size_t)A.nchains * C_COUNT);
  return STK_OK;
}

// ---------------------------------------------------------------- running
// Read chain modes/iterations; returns true when no chain has work below pause_at.
static int poll(stk_sampler* s, int pause_at, bool* idle) {
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipMemcpyAsync(s->iv_host.data(), s->A.iv, sizeof(int) * s->iv_host.size(), hipMemcpyDeviceToHost,
                               ctx->stream));
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  bool any = false;
  for (int c = 0; c < s->A.nchains; ++c) {
    const int mode = s->iv_host[(size_t)c * I_COUNT + I_MODE];
    const int it = s->iv_host[(size_t)c * I_COUNT + I_ITER];
    if (mode == M_INIT || mode == M_PROBE || mode == M_TRAJ) any = true;
    if (mode == M_PAUSED && it < pause_at) any = true;
  }
  *idle = !any;
  return STK_OK;
}

static int run_split_batch(stk_sampler* s, int nsteps, int pause_at) {
  stk_model* m = s->m;
  stk_ctx* ctx = m->ctx;
  hipStream_t st = ctx->stream;
  NutsArgs& A = s->A;
  const int every = ctx->profiling;            // events around the sweeps of every n-th step
  const bool prof = every > 0;
  if (prof) {
    while ((int)s->ev.size() < 2 * nsteps) {
      hipEvent_t e;
      STK_HIP_CHECK(hipEventCreate(&e));
      s->ev.push_back(e);
    }
    STK_HIP_CHECK(hipMemsetAsync(s->ran.p, 0, sizeof(int) * 64, st));
  }
  const int step0 = s->step;
  for (int k = 0; k < nsteps; ++k) {
    const int step_id = s->step;
    const bool pk = prof && step_id % every == 0;
    if (pk) STK_HIP_CHECK(hipEventRecord(s->ev[2 * k], st));
    // one event pair spans the sweeps of all the step's batches
    const SweepCall run{A.shards, A.qeval, s->partial.as<double>(), A.req_step, step_id, prof ? s->ran.as<int>() : nullptr,
                        s->sws.qT ? &s->sws : nullptr, A.Dp, 0, 0, 0};
    STK_HIP_CHECK(plan_sweeps(m, s->plan, run, st));
    if (pk) STK_HIP_CHECK(hipEventRecord(s->ev[2 * k + 1], st));
    STK_HIP_CHECK(plan_reduces(m, s->plan, run, A.lp_in, A.g_in, st));
    if (s->ar_fn) {
      const int r = s->ar_fn(s->ar_user, A.g_in, (int64_t)A.nchains * (A.Dp + 1), (void*)st);
      if (r != 0) {
        stk_set_error("full-data all-reduce callback failed (%d) at step %d", r, step_id);
        return STK_E_STATE;
      }
    }
    if (A.metric == 1) STK_HIP_CHECK(stk_launch_nuts_step_dense(A, s->nch, step_id, pause_at, st));
    else STK_HIP_CHECK(stk_launch_nuts_step(A, s->nch, step_id, pause_at, st));
    s->step++;
    s->steps++;
  }
  if (prof) {
    int ran[64];
    STK_HIP_CHECK(hipMemcpyAsync(ran, s->ran.p, sizeof(int) * 64, hipMemcpyDeviceToHost, st));
    STK_HIP_CHECK(hipStreamSynchronize(st));
    for (int k = 0; k < nsteps; ++k) {
      if ((step0 + k) % every != 0 || !ran[(step0 + k) & 63]) continue;
      float ms = 0.f;
      STK_HIP_CHECK(hipEventElapsedTime(&ms, s->ev[2 * k], s->ev[2 * k + 1]));
      s->sweep_ms += ms;
      s->sweeps += 1;
      s->shard_sweeps += ran[(step0 + k) & 63];
    }
  }
  return STK_OK;
}

extern "C" {

int stk_sampler_destroy(stk_sampler* s) {
  if (!s) return STK_OK;
  stk_model* m = s->m;
  hipSetDevice(m->ctx->device);
  hipStreamSynchronize(m->ctx->stream);
  for (auto& b : s->bufs) b.release();
  for (DevBuf* b : {&s->partial, &s->ran, &s->ws}) b->release();
  for (auto e : s->ev) hipEventDestroy(e);
  delete s;
  model_release(m);
  return STK_OK;
}

int stk_sampler_create(stk_model* m, const stk_config* cfg, stk_sampler** out) {
  ARG_CHECK(m && cfg && out, "stk_sampler_create: bad arguments");
  const int nch = stk_nch_for(m->Dmax);
  RC(check_config(m, cfg, nch));
  STK_HIP_CHECK(hipSetDevice(m->ctx->device));
  std::vector<double> minv_host, chol_host;
  if (cfg->metric == 1 && cfg->inv_metric_dense)
    RC(dense_metric_host(cfg->inv_metric_dense, m->Dmax, (m->Dmax + 7) / 8 * 8, &minv_host, &chol_host));
  ChainPlan plan;   // regressions: the chain batches, each with its sweeps grouped by consecutive shards of equal n
  if (m->family != STK_SCHOOLS) RC(chain_plan(m, model_chain_batches(m, cfg->chains), 0, m->nshards, &plan));
  stk_sampler* s = new stk_sampler();
  s->m = m;
  m->refs++;
  s->cfg = *cfg;
  s->nch = nch;
  fill_args(m, cfg, &s->A);
  const int rc = sampler_init(s, &plan, minv_host, chol_host);
  if (rc != STK_OK) {
    stk_sampler_destroy(s);
    return rc;
  }
  *out = s;
  return STK_OK;
}

int stk_sampler_run(stk_sampler* s, int32_t target_iter, int64_t max_steps) {
  ARG_CHECK(s, "stk_sampler_run: NULL sampler");
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  const int pause_at = std::min(target_iter, s->A.total_iters);
  int64_t done_steps = 0;
  int batch = 4;
  for (;;) {
    bool idle = false;
    RC(poll(s, pause_at, &idle));
    if (idle) break;
    if (max_steps > 0 && done_steps >= max_steps) break;
    if (s->m->family == STK_SCHOOLS) {
      const int ms = 4096;
      STK_HIP_CHECK(stk_launch_nuts_fused(s->A, s->nch, pause_at, ms, ctx->stream));
      done_steps += ms;
      s->steps += 1;
    } else {
      int nb = batch;
      if (max_steps > 0) nb = (int)std::min<int64_t>(nb, max_steps - done_steps);
      RC(run_split_batch(s, nb, pause_at));
      done_steps += nb;
      batch = std::min(batch * 2, 64);
    }
  }
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return STK_OK;
}

int stk_sampler_grad_block(stk_sampler* s, int64_t* count) {
  ARG_CHECK(s && count, "stk_sampler_grad_block: bad arguments");
  *count = (int64_t)s->A.nchains * (s->A.Dp + 1);
  return STK_OK;
}

int stk_sampler_set_allreduce(stk_sampler* s, stk_allreduce_fn fn, void* user, double* dev_block) {
  ARG_CHECK(s, "stk_sampler_set_allreduce: NULL sampler");
  REFUSE_SPARSE(s->m, "stk_sampler_set_allreduce (full-data mode)");
  ARG_CHECK(s->m->family == STK_LOGREG,
            "full-data mode is logistic-only (a purely additive log density: flat priors, no Jacobian term), not for "
            "the %s family (%d)", family_name(s->m->family), s->m->family);
  ARG_CHECK(s->step == 0, "stk_sampler_set_allreduce: call before the first stk_sampler_run");
  for (const auto& sd : s->m->sh)
    ARG_CHECK(sd.pa == 0.0 && sd.pb == 0.0, "full-data mode: flat priors only (a prior would be summed once per rank)");
  const size_t n = (size_t)s->A.nchains * (s->A.Dp + 1);
  if (dev_block) {
    STK_HIP_CHECK(hipSetDevice(s->m->ctx->device));
    STK_HIP_CHECK(hipMemsetAsync(dev_block, 0, sizeof(double) * n, s->m->ctx->stream));
    s->A.g_in = dev_block;
    s->A.lp_in = dev_block + (size_t)s->A.nchains * s->A.Dp;
  }
  s->ar_fn = fn;
  s->ar_user = user;
  return STK_OK;
}

int stk_sampler_info(stk_sampler* s, stk_run_info* info) {
  ARG_CHECK(s && info, "stk_sampler_info: bad arguments");
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  STK_HIP_CHECK(hipMemcpyAsync(s->cnt_host.data(), s->A.cnt, sizeof(unsigned long long) * s->cnt_host.size(),
                               hipMemcpyDeviceToHost, ctx->stream));
  STK_HIP_CHECK(hipMemcpyAsync(s->iv_host.data(), s->A.iv, sizeof(int) * s->iv_host.size(), hipMemcpyDeviceToHost,
                               ctx->stream));
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  memset(info, 0, sizeof(*info));
  info->min_iter = 1 << 30;
  for (int c = 0; c < s->A.nchains; ++c) {
    info->grad_evals += (int64_t)s->cnt_host[(size_t)c * C_COUNT + C_GRAD];
    info->leapfrogs += (int64_t)s->cnt_host[(size_t)c * C_COUNT + C_LEAP];
    info->divergent += (int32_t)s->cnt_host[(size_t)c * C_COUNT + C_DIV];
    const int mode = s->iv_host[(size_t)c * I_COUNT + I_MODE];
    info->min_iter = std::min(info->min_iter, s->iv_host[(size_t)c * I_COUNT + I_ITER]);
    if (mode == M_DONE) info->done++;
    if (mode == M_ERROR) info->errors++;
  }
  info->steps = s->steps;
  info->sweeps = s->sweeps;
  info->shard_sweeps = s->shard_sweeps;
  info->sweep_ms = s->sweep_ms;
  return STK_OK;
}

int stk_sampler_draws(stk_sampler* s, int shard, double* out, double* stats) {
  ARG_CHECK(s && shard >= 0 && shard < s->m->nshards, "stk_sampler_draws: bad shard");
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  const size_t S = (size_t)s->A.S_total;
  const int P = s->m->sh[shard].P;
  if (out)
    STK_HIP_CHECK(hipMemcpyAsync(out, s->A.draws + (size_t)shard * s->A.Pmax * S, sizeof(double) * P * S,
                                 hipMemcpyDefault, ctx->stream));
  if (stats)
    STK_HIP_CHECK(hipMemcpyAsync(stats, s->A.stats + (size_t)shard * S * N_STATS, sizeof(double) * S * N_STATS,
                                 hipMemcpyDefault, ctx->stream));
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return STK_OK;
}

int stk_sampler_draws_unconstrained(stk_sampler* s, int shard, double* out) {
  ARG_CHECK(s && out && shard >= 0 && shard < s->m->nshards, "bad arguments");
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  const int D = s->m->sh[shard].D;
  const size_t rows = (size_t)s->A.C * s->A.ud_iters;
  const double* src = s->A.udraws + (size_t)shard * rows * s->A.Dp;
  STK_HIP_CHECK(hipMemcpy2DAsync(out, sizeof(double) * D, src, sizeof(double) * s->A.Dp, sizeof(double) * D, rows,
                                 hipMemcpyDefault, ctx->stream));
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return STK_OK;
}

// Every chain's step size, one double each.
static int copy_stepsizes(stk_sampler* s, double* stepsize) {
  STK_HIP_CHECK(hipMemcpy2DAsync(stepsize, sizeof(double), s->A.sc + S_NOMEPS, sizeof(double) * S_COUNT, sizeof(double),
                                 s->A.nchains, hipMemcpyDefault, s->m->ctx->stream));
  return STK_OK;
}

int stk_sampler_adaptation(stk_sampler* s, double* stepsize, double* inv_metric) {
  ARG_CHECK(s, "NULL sampler");
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  if (stepsize) RC(copy_stepsizes(s, stepsize));
  if (inv_metric) {
    for (int c = 0; c < s->A.nchains; ++c) {
      const int D = s->m->sh[c / s->A.C].D;
      STK_HIP_CHECK(hipMemcpyAsync(inv_metric + (size_t)c * s->m->Dmax,
                                   s->A.vec + ((size_t)c * V_COUNT + V_IM) * s->A.Dp, sizeof(double) * D,
                                   hipMemcpyDefault, ctx->stream));
    }
  }
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return STK_OK;
}

// Every chain's D x D block of a [nchains][Dp][Dp] dense_e matrix buffer, packed.
static int copy_dense(stk_sampler* s, const double* src, double* out) {
  const size_t D = (size_t)s->m->Dmax, Dp = (size_t)s->A.Dp;
  for (int c = 0; c < s->A.nchains; ++c)
    STK_HIP_CHECK(hipMemcpy2DAsync(out + (size_t)c * D * D, sizeof(double) * D, src + (size_t)c * Dp * Dp,
                                   sizeof(double) * Dp, sizeof(double) * D, D, hipMemcpyDefault, s->m->ctx->stream));
  return STK_OK;
}

int stk_sampler_adaptation_dense(stk_sampler* s, double* stepsize, double* inv_metric) {
  ARG_CHECK(s, "NULL sampler");
  ARG_CHECK(s->A.metric == 1, "stk_sampler_adaptation_dense: the sampler's metric is not dense_e");
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  if (stepsize) RC(copy_stepsizes(s, stepsize));
  if (inv_metric) RC(copy_dense(s, s->A.d_minv, inv_metric));
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return STK_OK;
}

int stk_sampler_metric_factor_dense(stk_sampler* s, double* chol) {
  ARG_CHECK(s && chol, "stk_sampler_metric_factor_dense: bad arguments");
  ARG_CHECK(s->A.metric == 1, "stk_sampler_metric_factor_dense: the sampler's metric is not dense_e");
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  RC(copy_dense(s, s->A.d_chol, chol));
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return STK_OK;
}

int stk_sampler_iterations(stk_sampler* s, int32_t* iters) {
  ARG_CHECK(s && iters, "stk_sampler_iterations: bad arguments");
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  STK_HIP_CHECK(hipMemcpy2DAsync(iters, sizeof(int32_t), s->A.iv + I_ITER, sizeof(int) * I_COUNT, sizeof(int32_t),
                                 s->A.nchains, hipMemcpyDefault, ctx->stream));
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return STK_OK;
}

}  // extern "C"
