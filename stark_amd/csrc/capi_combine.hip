// C ABI of libstark_hip.so: the consensus combine.  The whole chain of a combine runs on the
// context's stream with one host synchronisation at the end (combine.hip header).
#include "capi_internal.h"

namespace {
// Device buffers of one combine, carved from the context's three combine scratch buffers.
struct CombineBufs {
  double *X, *mean, *cov, *W, *work, *sw, *swt, *inv, *out;
  int32_t *rowbad, *used, *status, *blk;
};
int combine_bufs(stk_ctx* ctx, int nshards, int P, int S, CombineBufs* b, bool general = false) {
  DevBuf &F = ctx->scratch[SCR_COMB_F64], &M = ctx->scratch[SCR_COMB_MAT], &I = ctx->scratch[SCR_COMB_I32];
  const size_t per = (size_t)P * S, pp = (size_t)P * P;
  const size_t wk = std::max(stk_spd_inverse_work_bytes(P, nshards), general ? stk_general_inverse_work_bytes(P) : 0);
  RC(F.ensure(sizeof(double) * (per * nshards + per * 2 + (size_t)P * nshards)));
  RC(M.ensure(sizeof(double) * (pp * nshards * 2 + pp * 2) + wk + 16));
  RC(I.ensure(sizeof(int32_t) * ((size_t)P * nshards + 2 * (size_t)nshards + 2 + (size_t)P) + 64));
  b->X = F.as<double>();
  b->swt = b->X + per * nshards;
  b->out = b->swt + per;
  b->mean = b->out + per;
  b->cov = M.as<double>();
  b->W = b->cov + pp * nshards;
  b->sw = b->W + pp * nshards;
  b->inv = b->sw + pp;
  b->work = b->inv + pp;
  b->rowbad = I.as<int32_t>();
  b->used = b->rowbad + (size_t)P * nshards;
  b->status = b->used + nshards;               // nshards + 1 (the last: the final solve)
  b->blk = b->status + nshards + 1;
  return STK_OK;
}

// The end of a combine whose launches are on the stream: every shard's used / status flags come
// back (and the final solve's when `out`), a used shard with a bad status is the error rc_shard with
// the caller's message (one %d: the shard), then all-NaN and the singular sum; `out` is copied out
// unless the solve wrote it in place.
int combine_finish(stk_ctx* ctx, const CombineBufs& b, int nshards, size_t per, int rc_shard, const char* shard_msg,
                   double* out, bool dev_out, int32_t* shard_used) {
  hipStream_t st = ctx->stream;
  std::vector<int32_t> h(2 * nshards + 1, 0);
  STK_HIP_CHECK(hipMemcpyAsync(h.data(), b.used, sizeof(int32_t) * (2 * nshards + (out ? 1 : 0)), hipMemcpyDeviceToHost, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  int nused = 0;
  for (int s = 0; s < nshards; ++s) {
    if (h[s] && h[nshards + s]) {
      stk_set_error(shard_msg, s);
      return rc_shard;
    }
    nused += h[s];
    if (shard_used) shard_used[s] = h[s];
  }
  if (nused == 0) {
    stk_set_error("every shard holds NaN draws");
    return STK_E_NAN;
  }
  if (out && h[2 * nshards]) {
    stk_set_error("singular sum of weights (LinAlgError)");
    return STK_E_LINALG;
  }
  if (out && !dev_out) {
    STK_HIP_CHECK(hipMemcpyAsync(out, b.out, sizeof(double) * per, hipMemcpyDefault, st));
    STK_HIP_CHECK(hipStreamSynchronize(st));
  }
  return STK_OK;
}

int consensus_run(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S, const int32_t* row_block,
                  double* sum_w, double* sum_wtheta, double* out, int32_t* shard_used) {
  ARG_CHECK(ctx && draws && nshards > 0 && P > 0 && S > 1, "stk_consensus: bad arguments");
  ARG_CHECK(P <= 4096, "P = %d too large", P);
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t per = (size_t)P * S;
  // A sample covariance of S draws has rank <= S - 1: with S <= p (p = the largest weight block)
  // every shard's covariance is singular.  numpy's inv then returns rounding noise of order 1/eps
  // (or raises when a pivot happens to round to exactly zero) and the reference's combine is
  // meaningless; here it is a LinAlgError, independent of rounding.
  int pmax = P;
  if (row_block) {
    std::vector<int32_t> rb(P), cnt(P, 0);
    STK_HIP_CHECK(hipMemcpy(rb.data(), row_block, sizeof(int32_t) * P, hipMemcpyDefault));
    for (int i = 0; i < P; ++i) {
      ARG_CHECK(rb[i] >= 0 && rb[i] < P, "row_block[%d] = %d out of [0, P)", i, rb[i]);
      ++cnt[rb[i]];
    }
    pmax = *std::max_element(cnt.begin(), cnt.end());
  }
  if (S <= pmax) {
    stk_set_error("%d draws give a singular sample covariance for a %d-parameter weight block (rank <= S - 1; "
                  "LinAlgError)", S, pmax);
    return STK_E_LINALG;
  }
  CombineBufs b;
  RC(combine_bufs(ctx, nshards, P, S, &b));
  const bool dev_in = is_device_ptr(draws, ctx->device), dev_out = out && is_device_ptr(out, ctx->device);
  const double* X = dev_in ? draws : b.X;
  if (!dev_in) STK_HIP_CHECK(hipMemcpyAsync(b.X, draws, sizeof(double) * per * nshards, hipMemcpyDefault, st));
  if (row_block) STK_HIP_CHECK(hipMemcpyAsync(b.blk, row_block, sizeof(int32_t) * P, hipMemcpyDefault, st));
  STK_HIP_CHECK(stk_launch_consensus_products(X, nshards, P, S, row_block ? b.blk : nullptr, b.mean, b.rowbad,
                                              b.used, b.status, b.cov, b.W, b.work, b.sw, b.swt, st));
  if (out)
    STK_HIP_CHECK(stk_launch_consensus_solve(b.sw, b.swt, P, S, b.inv, b.work, b.status + nshards,
                                             dev_out ? out : b.out, st, false));
  RC(combine_finish(ctx, b, nshards, per, STK_E_LINALG, "shard %d: singular sample covariance (LinAlgError)", out, dev_out,
                    shard_used));
  if (sum_w) STK_HIP_CHECK(hipMemcpyAsync(sum_w, b.sw, sizeof(double) * P * P, hipMemcpyDefault, st));
  if (sum_wtheta) STK_HIP_CHECK(hipMemcpyAsync(sum_wtheta, b.swt, sizeof(double) * per, hipMemcpyDefault, st));
  if (sum_w || sum_wtheta) STK_HIP_CHECK(hipStreamSynchronize(st));
  return STK_OK;
}
}  // namespace

extern "C" {

int stk_consensus_products(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S, double* sum_w,
                           double* sum_wtheta, int32_t* shard_used) {
  return consensus_run(ctx, draws, nshards, P, S, nullptr, sum_w, sum_wtheta, nullptr, shard_used);
}

int stk_consensus_solve(stk_ctx* ctx, const double* sum_w, const double* sum_wtheta, int32_t P, int32_t S,
                        double* out) {
  ARG_CHECK(ctx && sum_w && sum_wtheta && out && P > 0 && S > 0, "stk_consensus_solve: bad arguments");
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t per = (size_t)P * S;
  CombineBufs b;
  RC(combine_bufs(ctx, 1, P, S, &b, true));
  STK_HIP_CHECK(hipMemcpyAsync(b.sw, sum_w, sizeof(double) * P * P, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipMemcpyAsync(b.swt, sum_wtheta, sizeof(double) * per, hipMemcpyDefault, st));
  // the caller's sum W: any invertible matrix, inverted by partial pivoting as np.linalg.inv
  STK_HIP_CHECK(stk_launch_consensus_solve(b.sw, b.swt, P, S, b.inv, b.work, b.status, b.out, st, true));
  int32_t hs = 0;
  STK_HIP_CHECK(hipMemcpyAsync(&hs, b.status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  STK_HIP_CHECK(hipMemcpyAsync(out, b.out, sizeof(double) * per, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  if (hs) {
    stk_set_error("singular sum of weights (LinAlgError)");
    return STK_E_LINALG;
  }
  return STK_OK;
}

int stk_consensus(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S, double* out,
                  int32_t* shard_used) {
  ARG_CHECK(out, "stk_consensus: out is NULL");
  return consensus_run(ctx, draws, nshards, P, S, nullptr, nullptr, nullptr, out, shard_used);
}

int stk_consensus_blocked(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S,
                          const int32_t* row_block, double* out, int32_t* shard_used) {
  ARG_CHECK(out && row_block, "stk_consensus_blocked: out / row_block is NULL");
  return consensus_run(ctx, draws, nshards, P, S, row_block, nullptr, nullptr, out, shard_used);
}

// The combine with the caller's weights: the NaN mask, sum W, sum W theta and the final solve of
// stk_consensus; no covariance, no per-shard inverse (so S may be any count >= 1).
int stk_consensus_weighted(stk_ctx* ctx, const double* draws, const double* weights, int32_t nshards, int32_t P,
                           int32_t S, double* out, int32_t* shard_used) {
  ARG_CHECK(ctx && draws && weights && out && nshards > 0 && P > 0 && S > 0, "stk_consensus_weighted: bad arguments");
  ARG_CHECK(P <= 4096, "P = %d too large", P);
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t per = (size_t)P * S, pp = (size_t)P * P;
  CombineBufs b;
  RC(combine_bufs(ctx, nshards, P, S, &b));
  const bool dev_in = is_device_ptr(draws, ctx->device), dev_out = is_device_ptr(out, ctx->device);
  const double* X = dev_in ? draws : b.X;
  if (!dev_in) STK_HIP_CHECK(hipMemcpyAsync(b.X, draws, sizeof(double) * per * nshards, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipMemcpyAsync(b.W, weights, sizeof(double) * pp * nshards, hipMemcpyDefault, st));   // masked in place
  STK_HIP_CHECK(stk_launch_consensus_weighted(X, nshards, P, S, b.mean, b.rowbad, b.used, b.status, b.W, b.sw, b.swt, st));
  STK_HIP_CHECK(stk_launch_consensus_solve(b.sw, b.swt, P, S, b.inv, b.work, b.status + nshards, dev_out ? out : b.out,
                                           st, false));
  return combine_finish(ctx, b, nshards, per, STK_E_ARG, "shard %d: non-finite weight", out, dev_out, shard_used);
}

}  // extern "C"
