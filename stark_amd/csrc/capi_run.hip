// C ABI of libstark_hip.so: whole runs written on the sampler's public calls -- stk_sample and the
// one-transition parity hooks.
#include "capi_internal.h"

static int transition_impl(stk_model* m, int shard, double* q, int32_t C, uint64_t seed, int32_t iteration, double eps,
                           const double* inv_metric, const double* inv_metric_dense, int32_t max_depth, double* lp,
                           double* stats) {
  ARG_CHECK(m && q && C > 0 && shard >= 0 && shard < m->nshards, "stk_transition: bad arguments");
  const int D = m->sh[shard].D;
  stk_config cfg;
  stk_config_default(&cfg);
  cfg.num_warmup = 0;
  cfg.num_samples = 1;
  cfg.chains = C;
  cfg.max_depth = max_depth;
  cfg.adapt_engaged = 0;
  cfg.stepsize = eps;
  cfg.seed = seed;
  cfg.skip_init_stepsize = 1;
  cfg.iter_offset = iteration;
  if (inv_metric_dense) {
    cfg.metric = 1;
    cfg.inv_metric_dense = inv_metric_dense;
  }
  std::vector<double> qh((size_t)C * D);
  if (hipMemcpy(qh.data(), q, sizeof(double) * qh.size(), hipMemcpyDefault) != hipSuccess) {
    stk_set_error("stk_transition: cannot read q");
    return STK_E_ARG;
  }
  std::vector<double> init;
  for (int sh = 0; sh < m->nshards; ++sh) {
    const int Ds = m->sh[sh].D;
    for (int c = 0; c < C; ++c)
      for (int e = 0; e < Ds; ++e) init.push_back(e < D ? qh[(size_t)c * D + e] : 0.0);
  }
  cfg.init = init.data();
  std::vector<double> im;
  if (inv_metric) {
    im.assign(m->Dmax, 1.0);
    std::vector<double> tmp(D);
    if (hipMemcpy(tmp.data(), inv_metric, sizeof(double) * D, hipMemcpyDefault) != hipSuccess) return STK_E_ARG;
    std::copy(tmp.begin(), tmp.end(), im.begin());
    cfg.inv_metric = im.data();
  }
  stk_sampler* s = nullptr;
  RC(stk_sampler_create(m, &cfg, &s));
  int rc = stk_sampler_run(s, 1, 0);
  if (rc == STK_OK) rc = stk_sampler_draws_unconstrained(s, shard, qh.data());
  if (rc == STK_OK) {
    const int P = m->sh[shard].P;
    std::vector<double> dr((size_t)P * C), stv((size_t)C * N_STATS);
    rc = stk_sampler_draws(s, shard, dr.data(), stv.data());
    if (rc == STK_OK) {
      if (lp)
        for (int c = 0; c < C; ++c) lp[c] = dr[(size_t)(P - 1) * C + c];
      if (stats) memcpy(stats, stv.data(), sizeof(double) * stv.size());
      if (hipMemcpy(q, qh.data(), sizeof(double) * qh.size(), hipMemcpyDefault) != hipSuccess) rc = STK_E_HIP;
    }
  }
  stk_sampler_destroy(s);
  return rc;
}

extern "C" {

int stk_sample(stk_model* m, const stk_config* cfg, double* draws, double* stats, stk_run_info* info) {
  stk_sampler* s = nullptr;
  RC(stk_sampler_create(m, cfg, &s));
  int rc = stk_sampler_run(s, cfg->num_warmup + cfg->num_samples, 0);
  stk_run_info inf{};
  if (rc == STK_OK) rc = stk_sampler_info(s, &inf);
  if (rc == STK_OK && inf.errors) {
    stk_set_error("%d chain(s) stopped: step size left (0, 1e7] during init_stepsize", inf.errors);
    rc = STK_E_NUMERIC;
  }
  const size_t S = (size_t)cfg->chains * cfg->num_samples;
  for (int sh = 0; rc == STK_OK && sh < m->nshards; ++sh)
    rc = stk_sampler_draws(s, sh, draws ? draws + (size_t)sh * m->Pmax * S : nullptr,
                           stats ? stats + (size_t)sh * S * N_STATS : nullptr);
  if (info) *info = inf;
  stk_sampler_destroy(s);
  return rc;
}

int stk_transition(stk_model* m, int shard, double* q, int32_t C, uint64_t seed, int32_t iteration, double eps,
                   const double* inv_metric, int32_t max_depth, double* lp, double* stats) {
  return transition_impl(m, shard, q, C, seed, iteration, eps, inv_metric, nullptr, max_depth, lp, stats);
}

int stk_transition_dense(stk_model* m, int shard, double* q, int32_t C, uint64_t seed, int32_t iteration, double eps,
                         const double* inv_metric, int32_t max_depth, double* lp, double* stats) {
  ARG_CHECK(inv_metric, "stk_transition_dense: inv_metric (D x D) is NULL");
  return transition_impl(m, shard, q, C, seed, iteration, eps, nullptr, inv_metric, max_depth, lp, stats);
}

}  // extern "C"
