// C ABI of libstark_hip.so: the semiparametric density-product combiner (dpe.hip, dpe_math.h).
//   stk_dpe_prepare      draws -> the prepared arrays (the combine's moments, then the whitened image)
//   stk_dpe_sample       prepared arrays -> P x T draws of the density product
//   stk_dpe_sample_host  the same on host arrays without a device (the twin)
//   stk_consensus_dpe    both in one call
// The Cholesky factor of Sigma_M, its inverse and mu_M are small host work between the two device
// stages (p x p, fixed order), where the prepare has to wait for the shard flags anyway.
#include "capi_internal.h"
#include "dpe_math.h"

namespace {

struct DpePrep {            // device pointers
  double *mu, *L, *lpw, *Y, *nrm, *g, *lpv;
};

size_t r64(size_t bytes) { return (bytes + 63) & ~(size_t)63; }

size_t prep_doubles(int ns, int p, int S) {
  return (size_t)p + (size_t)p * p + ns + (size_t)ns * S * (dpe_ldp(p) + 3) + 64;
}
void prep_carve(double* base, int ns, int p, int S, DpePrep* d) {
  d->mu = base;
  d->L = d->mu + p;
  d->lpw = d->L + (size_t)p * p;
  d->Y = d->lpw + ns + (8 - (p + (size_t)p * p + ns) % 8) % 8;    // rows of the image on 64-B lines
  d->nrm = d->Y + (size_t)ns * S * dpe_ldp(p);
  d->g = d->nrm + (size_t)ns * S;
  d->lpv = d->g + (size_t)ns * S;
}
size_t prepare_ws_bytes(int ns, int p, int S) { return sizeof(double) * (size_t)ns * S * dpe_ldp(p); }
size_t sample_ws_bytes(int M, int P, int p, int T, int sweeps, int K, bool trace) {
  size_t b = r64(sizeof(double) * (size_t)T * dpe_ldp(p)) + r64(sizeof(double) * (size_t)P * T) +
             r64(sizeof(DpeCoef) * (size_t)sweeps) + r64(sizeof(unsigned long long) * (size_t)M);
  if (trace) b += r64(sizeof(int32_t) * (size_t)K * sweeps * M) + r64(sizeof(double) * (size_t)K * sweeps);
  return b;
}

int check_shape(const char* who, int ns, int P, int lp_row, int* p_out) {
  ARG_CHECK(ns >= 1 && ns <= DPE_MAX_SHARDS, "%s: %d shards; the sampler takes 1 .. %d", who, ns, DPE_MAX_SHARDS);
  const int p = lp_row ? P - 1 : P;
  ARG_CHECK(p >= 1, "%s: P = %d rows%s leave no parameter row", who, P, lp_row ? " (the last is lp__)" : "");
  ARG_CHECK(p <= DPE_MAX_P, "%s: p = %d parameter rows; the chain kernel holds 16 coordinates per lane, p <= %d", who, p,
            DPE_MAX_P);
  *p_out = p;
  return STK_OK;
}

int check_chain_args(const char* who, int T, int K, int burn, int thin, uint32_t stream) {
  ARG_CHECK(T >= 1, "%s: T = %d draws; need T >= 1", who, T);
  ARG_CHECK(K >= 1, "%s: K = %d chains; need K >= 1", who, K);
  ARG_CHECK(thin >= 1, "%s: thin = %d; need thin >= 1", who, thin);
  ARG_CHECK(burn >= 0, "%s: burn = %d; need burn >= 0", who, burn);
  ARG_CHECK(stream < DPE_MAX_STREAM, "%s: stream = %u; a stream is below 2^24 = %u", who, stream, DPE_MAX_STREAM);
  const long long sweeps = (long long)burn + (long long)thin * ((T + K - 1) / K);
  ARG_CHECK(sweeps <= 0x7fffffffLL, "%s: burn + thin ceil(T / K) = %lld sweeps; need below 2^31", who, sweeps);
  return STK_OK;
}
int n_sweeps(int T, int K, int burn, int thin) { return burn + thin * ((T + K - 1) / K); }

int make_coef(const char* who, const double* h, int sweeps, int M, std::vector<DpeCoef>* out) {
  ARG_CHECK(h, "%s: the bandwidth table h is NULL", who);
  out->resize(sweeps);
  for (int r = 0; r < sweeps; ++r) {
    ARG_CHECK(std::isfinite(h[r]) && h[r] > 0.0, "%s: h[%d] = %g; a bandwidth is positive and finite", who, r, h[r]);
    (*out)[r] = dpe_coef(h[r], M);
  }
  return STK_OK;
}

// draws X (device) -> the prepared arrays at d (device); shard_used (host, or null), M
int prepare_dev(stk_ctx* ctx, const double* X, int ns, int P, int S, int p, const DpePrep& d, int32_t* shard_used,
                int* M_out) {
  hipStream_t st = ctx->stream;
  const bool lp_row = p < P;
  const size_t pp = (size_t)P * P, per = (size_t)P * S;
  const size_t wk = std::max(stk_spd_inverse_work_bytes(P, ns), stk_spd_inverse_work_bytes(P, 1));
  const size_t nd = (size_t)ns * P + 2 * pp * ns + 2 * pp + per + (size_t)p * p;
  const size_t ni = (size_t)ns * P + 3 * (size_t)ns + 1 + P;
  DevBuf& Mo = ctx->scratch[SCR_DPE_MOM];
  RC(Mo.ensure(r64(sizeof(double) * nd) + r64(wk) + sizeof(int32_t) * ni + 64));
  double* mean = Mo.as<double>();
  double* cov = mean + (size_t)ns * P;
  double* W = cov + pp * ns;
  double* sw = W + pp * ns;
  double* inv = sw + pp;
  double* swt = inv + pp;
  double* Linv = swt + per;
  double* work = reinterpret_cast<double*>(reinterpret_cast<char*>(mean) + r64(sizeof(double) * nd));
  int32_t* rowbad = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(work) + r64(wk));
  int32_t* used = rowbad + (size_t)ns * P;
  int32_t* status = used + ns;            // ns + 1: the last is Sigma_M's inverse
  int32_t* blk = status + ns + 1;
  int32_t* zmap = blk + P;
  RC(ctx->scratch[SCR_DPE_WS].ensure(prepare_ws_bytes(ns, p, S)));
  double* Z = ctx->scratch[SCR_DPE_WS].as<double>();

  std::vector<int32_t> hb(P, 0);
  if (lp_row) {
    hb[P - 1] = 1;
    STK_HIP_CHECK(hipMemcpyAsync(blk, hb.data(), sizeof(int32_t) * P, hipMemcpyHostToDevice, st));
  }
  STK_HIP_CHECK(stk_launch_consensus_products(X, ns, P, S, lp_row ? blk : nullptr, mean, rowbad, used, status, cov, W, work,
                                              sw, swt, st));
  STK_HIP_CHECK(stk_launch_spd_inverse(sw, inv, work, P, 1, nullptr, status + ns, st));
  std::vector<int32_t> hf(2 * ns + 1);
  STK_HIP_CHECK(hipMemcpyAsync(hf.data(), used, sizeof(int32_t) * (2 * ns + 1), hipMemcpyDeviceToHost, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  std::vector<int32_t> hz;
  for (int s = 0; s < ns; ++s) {
    if (hf[s] && hf[ns + s]) {
      stk_set_error("shard %d: singular sample covariance (LinAlgError)", s);
      return STK_E_LINALG;
    }
    if (hf[s]) hz.push_back(s);
    if (shard_used) shard_used[s] = hf[s];
  }
  const int M = (int)hz.size();
  if (M == 0) {
    stk_set_error("every shard holds NaN draws");
    return STK_E_NAN;
  }
  if (hf[2 * ns]) {
    stk_set_error("singular sum of weights (LinAlgError)");
    return STK_E_LINALG;
  }
  std::vector<double> hinv(pp), hW(pp * ns), hmean((size_t)ns * P);
  STK_HIP_CHECK(hipMemcpyAsync(hinv.data(), inv, sizeof(double) * pp, hipMemcpyDeviceToHost, st));
  STK_HIP_CHECK(hipMemcpyAsync(hW.data(), W, sizeof(double) * pp * ns, hipMemcpyDeviceToHost, st));
  STK_HIP_CHECK(hipMemcpyAsync(hmean.data(), mean, sizeof(double) * ns * P, hipMemcpyDeviceToHost, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));

  // mu_M = Sigma_M sum_m W_m mu_m (usable shards in order), Sigma_M = L L^T, Linv = inv(L): all p x p, fixed order
  std::vector<double> b(p, 0.0), mu(p), L((size_t)p * p, 0.0), Li((size_t)p * p, 0.0), lpw(ns, 0.0);
  for (int m : hz)
    for (int i = 0; i < p; ++i) {
      double v = 0.0;
      for (int j = 0; j < p; ++j) v = fma(hW[((size_t)m * P + i) * P + j], hmean[(size_t)m * P + j], v);
      b[i] = b[i] + v;
    }
  for (int i = 0; i < p; ++i) {
    double v = 0.0;
    for (int j = 0; j < p; ++j) v = fma(hinv[(size_t)i * P + j], b[j], v);
    mu[i] = v;
  }
  for (int j = 0; j < p; ++j) {
    double dj = hinv[(size_t)j * P + j];
    for (int k = 0; k < j; ++k) dj = fma(-L[(size_t)j * p + k], L[(size_t)j * p + k], dj);
    if (!(dj > 0.0)) {
      stk_set_error("the product covariance is not positive definite at row %d (LinAlgError)", j);
      return STK_E_LINALG;
    }
    const double ljj = sqrt(dj);
    L[(size_t)j * p + j] = ljj;
    for (int i = j + 1; i < p; ++i) {
      double v = hinv[(size_t)i * P + j];
      for (int k = 0; k < j; ++k) v = fma(-L[(size_t)i * p + k], L[(size_t)j * p + k], v);
      L[(size_t)i * p + j] = v / ljj;
    }
  }
  for (int c = 0; c < p; ++c) {            // column c of inv(L) by forward substitution
    Li[(size_t)c * p + c] = 1.0 / L[(size_t)c * p + c];
    for (int i = c + 1; i < p; ++i) {
      double v = 0.0;
      for (int k = c; k < i; ++k) v = fma(-L[(size_t)i * p + k], Li[(size_t)k * p + c], v);
      Li[(size_t)i * p + c] = v / L[(size_t)i * p + i];
    }
  }
  if (lp_row) {                            // omega_m ~ 1 / var(lp^m): the 1 x 1 block of the blocked combine
    double tot = 0.0;
    for (int m : hz) tot = tot + hW[((size_t)m * P + p) * P + p];
    for (int z = 0; z < M; ++z) lpw[z] = hW[((size_t)hz[z] * P + p) * P + p] / tot;
  }
  STK_HIP_CHECK(hipMemcpyAsync(d.mu, mu.data(), sizeof(double) * p, hipMemcpyHostToDevice, st));
  STK_HIP_CHECK(hipMemcpyAsync(d.L, L.data(), sizeof(double) * p * p, hipMemcpyHostToDevice, st));
  STK_HIP_CHECK(hipMemcpyAsync(Linv, Li.data(), sizeof(double) * p * p, hipMemcpyHostToDevice, st));
  STK_HIP_CHECK(hipMemcpyAsync(d.lpw, lpw.data(), sizeof(double) * ns, hipMemcpyHostToDevice, st));
  STK_HIP_CHECK(hipMemcpyAsync(zmap, hz.data(), sizeof(int32_t) * M, hipMemcpyHostToDevice, st));
  STK_HIP_CHECK(stk_launch_dpe_image(X, mean, W, zmap, M, P, p, S, d.mu, Linv, d.Y, Z, d.nrm, d.g,
                                     lp_row ? d.lpv : nullptr, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));   // the host vectors above are the copies' sources
  *M_out = M;
  return STK_OK;
}

// prepared arrays at d (device) -> out [P][T] (host or device), accept [M] (host), trace (host or device, or null)
int sample_dev(stk_ctx* ctx, const DpePrep& d, int M, int P, int p, int S, uint64_t seed, uint32_t stream, int T, int K,
               int burn, int thin, const std::vector<DpeCoef>& coef, double* out, int64_t* accept, int32_t* tidx,
               double* tlogw) {
  hipStream_t st = ctx->stream;
  const int sweeps = (int)coef.size(), ldp = dpe_ldp(p);
  const bool lp_row = p < P, trace = tidx || tlogw;
  const bool dev_out = is_device_ptr(out, ctx->device);
  const bool dev_ti = tidx && is_device_ptr(tidx, ctx->device), dev_tl = tlogw && is_device_ptr(tlogw, ctx->device);
  DevBuf& Wb = ctx->scratch[SCR_DPE_WS];
  RC(Wb.ensure(sample_ws_bytes(M, P, p, T, sweeps, K, trace)));
  char* base = Wb.as<char>();
  double* ydraw = reinterpret_cast<double*>(base);
  base += r64(sizeof(double) * (size_t)T * ldp);
  double* ostage = reinterpret_cast<double*>(base);
  base += r64(sizeof(double) * (size_t)P * T);
  DpeCoef* dcoef = reinterpret_cast<DpeCoef*>(base);
  base += r64(sizeof(DpeCoef) * (size_t)sweeps);
  unsigned long long* dacc = reinterpret_cast<unsigned long long*>(base);
  base += r64(sizeof(unsigned long long) * (size_t)M);
  int32_t* ti_stage = reinterpret_cast<int32_t*>(base);
  double* tl_stage = reinterpret_cast<double*>(base + r64(sizeof(int32_t) * (size_t)K * sweeps * M));
  double* o = dev_out ? out : ostage;
  STK_HIP_CHECK(hipMemcpyAsync(dcoef, coef.data(), sizeof(DpeCoef) * sweeps, hipMemcpyHostToDevice, st));
  STK_HIP_CHECK(hipMemsetAsync(dacc, 0, sizeof(unsigned long long) * M, st));
  StkDpeChains c{d.Y, d.nrm, d.g, lp_row ? d.lpv : nullptr, lp_row ? d.lpw : nullptr, dcoef, ydraw,
                 lp_row ? o + (size_t)p * T : nullptr, dacc, tidx ? (dev_ti ? tidx : ti_stage) : nullptr,
                 tlogw ? (dev_tl ? tlogw : tl_stage) : nullptr, seed, stream, M, p, S, T, K, burn, thin, sweeps};
  STK_HIP_CHECK(stk_launch_dpe_chains(c, st));
  STK_HIP_CHECK(stk_launch_dpe_map(ydraw, d.L, d.mu, M, p, T, o, st));
  std::vector<unsigned long long> hacc(M);
  STK_HIP_CHECK(hipMemcpyAsync(hacc.data(), dacc, sizeof(unsigned long long) * M, hipMemcpyDeviceToHost, st));
  if (!dev_out) STK_HIP_CHECK(hipMemcpyAsync(out, ostage, sizeof(double) * P * T, hipMemcpyDeviceToHost, st));
  if (tidx && !dev_ti)
    STK_HIP_CHECK(hipMemcpyAsync(tidx, ti_stage, sizeof(int32_t) * (size_t)K * sweeps * M, hipMemcpyDeviceToHost, st));
  if (tlogw && !dev_tl)
    STK_HIP_CHECK(hipMemcpyAsync(tlogw, tl_stage, sizeof(double) * (size_t)K * sweeps, hipMemcpyDeviceToHost, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  if (accept)
    for (int m = 0; m < M; ++m) accept[m] = (int64_t)hacc[m];
  return STK_OK;
}

}  // namespace

extern "C" {

int stk_dpe_launch_info(int32_t nshards, int32_t P, int32_t S, int32_t T, int32_t K, int32_t lp_row, int64_t out[8]) {
  ARG_CHECK(out, "stk_dpe_launch_info: out is NULL");
  int p = 0;
  RC(check_shape("stk_dpe_launch_info", nshards, P, lp_row, &p));
  ARG_CHECK(S >= 1, "stk_dpe_launch_info: S = %d draws per shard; need S >= 1", S);
  RC(check_chain_args("stk_dpe_launch_info", T, K, 0, 1, 0));
  const int64_t v[8] = {p, dpe_ldp(p), stk_dpe_coords_per_lane(p), (T + K - 1) / K, (int64_t)stk_dpe_lds_bytes(nshards),
                        (int64_t)prepare_ws_bytes(nshards, p, S),
                        (int64_t)sample_ws_bytes(nshards, P, p, T, 0, K, false), K};
  memcpy(out, v, sizeof(v));
  return STK_OK;
}

int stk_dpe_prepare(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S, int32_t lp_row,
                    int32_t* shard_used, int32_t* n_used, double* mu, double* L, double* lp_w, double* Y, double* nrm,
                    double* g, double* lpv) {
  ARG_CHECK(ctx && draws && n_used && mu && L && Y && nrm && g, "stk_dpe_prepare: a NULL argument");
  int p = 0;
  RC(check_shape("stk_dpe_prepare", nshards, P, lp_row, &p));
  ARG_CHECK(!lp_row || (lp_w && lpv), "stk_dpe_prepare: lp_row needs lp_w and lpv");
  ARG_CHECK(S >= 1, "stk_dpe_prepare: S = %d draws per shard; need S >= 1", S);
  if (S <= p) {
    stk_set_error("%d draws give a singular sample covariance for %d parameter rows (rank <= S - 1; LinAlgError)", S, p);
    return STK_E_LINALG;
  }
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t per = (size_t)P * S;
  const double* X = draws;
  if (!is_device_ptr(draws, ctx->device)) {
    RC(ctx->scratch[SCR_DPE_IN].ensure(sizeof(double) * per * nshards));
    STK_HIP_CHECK(hipMemcpyAsync(ctx->scratch[SCR_DPE_IN].p, draws, sizeof(double) * per * nshards, hipMemcpyDefault, st));
    X = ctx->scratch[SCR_DPE_IN].as<double>();
  }
  RC(ctx->scratch[SCR_DPE_PREP].ensure(sizeof(double) * prep_doubles(nshards, p, S)));
  DpePrep s, d;
  prep_carve(ctx->scratch[SCR_DPE_PREP].as<double>(), nshards, p, S, &s);
  const int dev = ctx->device;
  d.mu = is_device_ptr(mu, dev) ? mu : s.mu;
  d.L = is_device_ptr(L, dev) ? L : s.L;
  d.lpw = lp_w && is_device_ptr(lp_w, dev) ? lp_w : s.lpw;
  d.Y = is_device_ptr(Y, dev) ? Y : s.Y;
  d.nrm = is_device_ptr(nrm, dev) ? nrm : s.nrm;
  d.g = is_device_ptr(g, dev) ? g : s.g;
  d.lpv = lpv && is_device_ptr(lpv, dev) ? lpv : s.lpv;
  int M = 0;
  RC(prepare_dev(ctx, X, nshards, P, S, p, d, shard_used, &M));
  *n_used = M;
  const size_t ldp = dpe_ldp(p);
  if (d.mu != mu) STK_HIP_CHECK(hipMemcpyAsync(mu, d.mu, sizeof(double) * p, hipMemcpyDeviceToHost, st));
  if (d.L != L) STK_HIP_CHECK(hipMemcpyAsync(L, d.L, sizeof(double) * p * p, hipMemcpyDeviceToHost, st));
  if (lp_w && d.lpw != lp_w) STK_HIP_CHECK(hipMemcpyAsync(lp_w, d.lpw, sizeof(double) * nshards, hipMemcpyDeviceToHost, st));
  if (d.Y != Y) STK_HIP_CHECK(hipMemcpyAsync(Y, d.Y, sizeof(double) * (size_t)M * S * ldp, hipMemcpyDeviceToHost, st));
  if (d.nrm != nrm) STK_HIP_CHECK(hipMemcpyAsync(nrm, d.nrm, sizeof(double) * (size_t)M * S, hipMemcpyDeviceToHost, st));
  if (d.g != g) STK_HIP_CHECK(hipMemcpyAsync(g, d.g, sizeof(double) * (size_t)M * S, hipMemcpyDeviceToHost, st));
  if (lp_row && d.lpv != lpv)
    STK_HIP_CHECK(hipMemcpyAsync(lpv, d.lpv, sizeof(double) * (size_t)M * S, hipMemcpyDeviceToHost, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  return STK_OK;
}

int stk_dpe_sample(stk_ctx* ctx, int32_t M, int32_t p, int32_t S, const double* mu, const double* L, const double* lp_w,
                   const double* Y, const double* nrm, const double* g, const double* lpv, uint64_t seed, uint32_t stream,
                   int32_t T, int32_t K, int32_t burn, int32_t thin, const double* h, double* out, int64_t* accept,
                   int32_t* trace_idx, double* trace_logw) {
  ARG_CHECK(ctx && mu && L && Y && nrm && g && out, "stk_dpe_sample: a NULL argument");
  int pc = 0;
  RC(check_shape("stk_dpe_sample", M, p, 0, &pc));
  ARG_CHECK(S >= 1, "stk_dpe_sample: S = %d draws per shard; need S >= 1", S);
  ARG_CHECK(!lpv == !lp_w, "stk_dpe_sample: lpv and lp_w come together (the lp__ row) or not at all");
  RC(check_chain_args("stk_dpe_sample", T, K, burn, thin, stream));
  std::vector<DpeCoef> coef;
  RC(make_coef("stk_dpe_sample", h, n_sweeps(T, K, burn, thin), M, &coef));
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int P = p + (lpv ? 1 : 0), dev = ctx->device;
  const size_t ldp = dpe_ldp(p), rows = (size_t)M * S;
  // host arrays are staged; device arrays are read where they lie
  const void* src[7] = {mu, L, lp_w, Y, nrm, g, lpv};
  const size_t bytes[7] = {sizeof(double) * p, sizeof(double) * p * p, sizeof(double) * M, sizeof(double) * rows * ldp,
                           sizeof(double) * rows, sizeof(double) * rows, sizeof(double) * rows};
  RC(ctx->scratch[SCR_DPE_PREP].ensure(sizeof(double) * prep_doubles(M, p, S)));
  DpePrep s;
  prep_carve(ctx->scratch[SCR_DPE_PREP].as<double>(), M, p, S, &s);
  double* slot[7] = {s.mu, s.L, s.lpw, s.Y, s.nrm, s.g, s.lpv};
  const double* use[7];
  for (int i = 0; i < 7; ++i) {
    use[i] = (const double*)src[i];
    if (src[i] && !is_device_ptr(src[i], dev)) {
      STK_HIP_CHECK(hipMemcpyAsync(slot[i], src[i], bytes[i], hipMemcpyDefault, st));
      use[i] = slot[i];
    }
  }
  const DpePrep d{(double*)use[0], (double*)use[1], (double*)use[2], (double*)use[3], (double*)use[4], (double*)use[5],
                  (double*)use[6]};
  return sample_dev(ctx, d, M, P, p, S, seed, stream, T, K, burn, thin, coef, out, accept, trace_idx, trace_logw);
}

int stk_dpe_sample_host(int32_t M, int32_t p, int32_t S, const double* mu, const double* L, const double* lp_w,
                        const double* Y, const double* nrm, const double* g, const double* lpv, uint64_t seed,
                        uint32_t stream, int32_t T, int32_t K, int32_t burn, int32_t thin, const double* h, double* out,
                        int64_t* accept, int32_t* trace_idx, double* trace_logw) {
  ARG_CHECK(mu && L && Y && nrm && g && out, "stk_dpe_sample_host: a NULL argument");
  int pc = 0;
  RC(check_shape("stk_dpe_sample_host", M, p, 0, &pc));
  ARG_CHECK(S >= 1, "stk_dpe_sample_host: S = %d draws per shard; need S >= 1", S);
  ARG_CHECK(!lpv == !lp_w, "stk_dpe_sample_host: lpv and lp_w come together (the lp__ row) or not at all");
  RC(check_chain_args("stk_dpe_sample_host", T, K, burn, thin, stream));
  std::vector<DpeCoef> coef;
  RC(make_coef("stk_dpe_sample_host", h, n_sweeps(T, K, burn, thin), M, &coef));
  std::vector<unsigned long long> acc(M, 0);
  StkDpeChains c{Y, nrm, g, lpv, lp_w, coef.data(), nullptr, nullptr, acc.data(), trace_idx, trace_logw, seed, stream,
                 M, p, S, T, K, burn, thin, (int)coef.size()};
  stk_dpe_chains_host(c, mu, L, out);
  if (accept)
    for (int m = 0; m < M; ++m) accept[m] = (int64_t)acc[m];
  return STK_OK;
}

int stk_consensus_dpe(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S, int32_t lp_row,
                      uint64_t seed, uint32_t stream, int32_t T, int32_t K, int32_t burn, int32_t thin, const double* h,
                      double* out, int32_t* shard_used, int64_t* accept) {
  ARG_CHECK(ctx && draws && out, "stk_consensus_dpe: a NULL argument");
  int p = 0;
  RC(check_shape("stk_consensus_dpe", nshards, P, lp_row, &p));
  ARG_CHECK(S >= 1, "stk_consensus_dpe: S = %d draws per shard; need S >= 1", S);
  RC(check_chain_args("stk_consensus_dpe", T, K, burn, thin, stream));
  std::vector<DpeCoef> coef;
  RC(make_coef("stk_consensus_dpe", h, n_sweeps(T, K, burn, thin), 1, &coef));   // checks h; M is not known yet
  if (S <= p) {
    stk_set_error("%d draws give a singular sample covariance for %d parameter rows (rank <= S - 1; LinAlgError)", S, p);
    return STK_E_LINALG;
  }
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t per = (size_t)P * S;
  const double* X = draws;
  if (!is_device_ptr(draws, ctx->device)) {
    RC(ctx->scratch[SCR_DPE_IN].ensure(sizeof(double) * per * nshards));
    STK_HIP_CHECK(hipMemcpyAsync(ctx->scratch[SCR_DPE_IN].p, draws, sizeof(double) * per * nshards, hipMemcpyDefault, st));
    X = ctx->scratch[SCR_DPE_IN].as<double>();
  }
  RC(ctx->scratch[SCR_DPE_PREP].ensure(sizeof(double) * prep_doubles(nshards, p, S)));
  DpePrep d;
  prep_carve(ctx->scratch[SCR_DPE_PREP].as<double>(), nshards, p, S, &d);
  int M = 0;
  RC(prepare_dev(ctx, X, nshards, P, S, p, d, shard_used, &M));
  RC(make_coef("stk_consensus_dpe", h, (int)coef.size(), M, &coef));
  if (accept)
    for (int m = 0; m < nshards; ++m) accept[m] = 0;
  return sample_dev(ctx, d, M, P, p, S, seed, stream, T, K, burn, thin, coef, out, accept, nullptr, nullptr);
}

}  // extern "C"
