// C ABI of libstark_hip.so: models -- creation from host rows or the generator, info, priors, data
// copy-out -- and the data fingerprints.
#include "capi_internal.h"
#include "gamma_math.h"

const char* family_name(int family) {
  switch (family) {
    case STK_SCHOOLS: return "schools";
    case STK_LINREG: return "linear";
    case STK_LOGREG: return "logistic";
    case STK_POISSON: return "poisson";
    case STK_NEGBIN: return "neg_binomial";
    case STK_STUDENT: return "student_t";
    case STK_GAMMA: return "gamma";
    case STK_CATEGORICAL: return "categorical";
  }
  return "unknown";
}

// The families every regression entry point serves (the analysis sweeps among them)...
bool is_regression(int family) { return family == STK_LINREG || family == STK_LOGREG || family == STK_POISSON; }
// ...and those the gradient sweeps, the sampler and the priors serve: the negative binomial, Student-t and gamma too.
bool is_sweep_family(int family) {
  return is_regression(family) || family == STK_NEGBIN || family == STK_STUDENT || family == STK_GAMMA;
}

// ...and categorical, which has a sweep of its own (sweep_cat.hip) and none of the sparse or analysis forms.
bool is_density_family(int family) { return is_sweep_family(family) || family == STK_CATEGORICAL; }

int model_ready(const stk_model* m) {
  ARG_CHECK(m->family != STK_STUDENT || m->nu > 0.0,
            "the student_t model's nu has not been set: call stk_model_set_student_nu first (there is no default)");
  ARG_CHECK(m->family != STK_CATEGORICAL || m->ncat >= 2,
            "the categorical model's classes have not been set: call stk_model_set_categories first (there is no default)");
  return STK_OK;
}

ShardRange shard_range(const stk_model* m, int shard, int (*chunks)(int64_t n)) {
  ShardRange r{shard < 0 ? 0 : shard, shard < 0 ? m->nshards : 1, 1};
  for (int s = r.shard0; s < r.shard0 + r.nsh; ++s) r.Gs = std::max(r.Gs, chunks(m->sh[s].n));
  return r;
}

static int family_dims(int family, int64_t n, int d, int* D, int* P) {
  switch (family) {
    case STK_SCHOOLS: *D = (int)n + 2; *P = 2 * (int)n + 3; return STK_OK;
    case STK_LINREG: *D = d + 2; *P = d + 3; return STK_OK;
    case STK_LOGREG: *D = d + 1; *P = d + 2; return STK_OK;
    case STK_POISSON: *D = d + 1; *P = d + 2; return STK_OK;   // the logistic layout: alpha, beta, lp__
    case STK_NEGBIN: *D = d + 2; *P = d + 3; return STK_OK;    // the linear layout: alpha, beta, phi (v = log phi), lp__
    case STK_STUDENT: *D = d + 2; *P = d + 3; return STK_OK;   // the linear layout itself: alpha, beta, sigma (s = log sigma), lp__
    case STK_GAMMA: *D = d + 2; *P = d + 3; return STK_OK;     // the linear layout: alpha, beta, shape (u = log shape), lp__
    case STK_CATEGORICAL: *D = 0; *P = 0; return STK_OK;       // (K - 1)(d + 1) and + 1, once stk_model_set_categories has said K
  }
  stk_set_error("unknown model family %d", family);
  return STK_E_ARG;
}

// ---------------------------------------------------------------- creation
// A model of `family` on ctx (which it holds) with no shard yet.
static stk_model* model_new(stk_ctx* ctx, int family, int nshards, int d) {
  stk_model* m = new stk_model();
  m->ctx = ctx;
  ctx->refs++;
  m->family = family;
  m->nshards = nshards;
  m->d = d;
  return m;
}

static int upload_nb_table(stk_model* m);
static int upload_shard_table(stk_model* m) {
  for (auto& s : m->sh) {
    m->Dmax = std::max(m->Dmax, s.D);
    m->Pmax = std::max(m->Pmax, s.P);
  }
  if (m->family == STK_NEGBIN || m->family == STK_GAMMA) RC(upload_nb_table(m));
  RC(m->sh_dev.ensure(sizeof(ShardDev) * m->sh.size()));
  STK_HIP_CHECK(hipMemcpyAsync(m->sh_dev.p, m->sh.data(), sizeof(ShardDev) * m->sh.size(), hipMemcpyHostToDevice,
                               m->ctx->stream));
  STK_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  return STK_OK;
}

// The model's [nshards] NbShardDev (count tables and phi priors; gamma: sum log y and the shape prior) to the
// device; again after a prior changes.
static int upload_nb_table(stk_model* m) {
  RC(m->nb_dev.ensure(sizeof(NbShardDev) * m->nb.size()));
  STK_HIP_CHECK(hipMemcpyAsync(m->nb_dev.p, m->nb.data(), sizeof(NbShardDev) * m->nb.size(), hipMemcpyHostToDevice,
                               m->ctx->stream));
  STK_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  return STK_OK;
}

// The end of both constructors.  rc: the outcome of the shards; a partly built model is destroyed.
static int model_finish(stk_model* m, int rc, stk_model** out) {
  if (rc == STK_OK) rc = upload_shard_table(m);
  if (rc != STK_OK) {
    stk_model_destroy(m);
    return rc;
  }
  *out = m;
  return STK_OK;
}

template <class T>
static int upload(stk_model* m, const T* src, size_t count, const T** dst) {
  m->bufs.emplace_back();
  DevBuf& b = m->bufs.back();
  RC(b.ensure(sizeof(T) * count));
  STK_HIP_CHECK(hipMemcpyAsync(b.p, src, sizeof(T) * count, hipMemcpyDefault, m->ctx->stream));
  *dst = b.as<T>();
  m->bytes += (int64_t)(sizeof(T) * count);
  return STK_OK;
}

// bernoulli_logit: y in {0, 1} (the sweeps read y as a sign bit); poisson_log: y >= 0.  Checked on the
// device copy by a reduction that returns the first bad row (8 bytes back, not the shard).
static int check_y_int(stk_model* m, int s, const int32_t* yi, int64_t n, bool pois, const char* pois_rule) {
  hipStream_t st = m->ctx->stream;
  DevBuf flag;
  RC(flag.ensure(sizeof(int64_t)));
  int64_t bad = -1;
  int32_t v = 0;
  hipError_t e = pois ? stk_launch_check_ynonneg(yi, n, flag.as<int64_t>(), st) : stk_launch_check_y01(yi, n, flag.as<int64_t>(), st);
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, flag.p, sizeof(int64_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess && bad >= 0 && bad < n) e = hipMemcpy(&v, yi + bad, sizeof(int32_t), hipMemcpyDeviceToHost);
  flag.release();
  if (e != hipSuccess) {
    stk_set_error("shard %d: y_int check failed: %s", s, hipGetErrorString(e));
    return STK_E_HIP;
  }
  ARG_CHECK(bad < 0 || bad >= n, "shard %d: y_int[%lld] = %d; %s", s, (long long)bad, v,
            pois ? pois_rule : "bernoulli_logit needs 0 or 1");
  return STK_OK;
}

// The count table of a negative-binomial shard (negbin_math.h) from its n counts, all >= 0: the tail
// counts T_j = #{i : y_i > j} for j < ncap = min(max y, NB_CAP), then (value, multiplicity) of every
// distinct count past NB_CAP, ascending.
static void nb_build_table(const int32_t* y, int64_t n, std::vector<double>* tab, int* ncap, int* nbig) {
  std::vector<int64_t> hist(NB_CAP + 1, 0);   // hist[k] = #{y_i = k}, k <= NB_CAP; the rest in `big`
  std::vector<int32_t> big;
  int32_t ymax = 0;
  for (int64_t i = 0; i < n; ++i) {
    ymax = std::max(ymax, y[i]);
    if (y[i] <= NB_CAP) hist[y[i]]++;
    else big.push_back(y[i]);
  }
  *ncap = std::min<int32_t>(ymax, NB_CAP);
  tab->assign(*ncap, 0.0);
  int64_t above = (int64_t)big.size();        // #{y_i > j}, from j = ncap - 1 down
  for (int j = *ncap - 1; j >= 0; --j) {
    above += hist[j + 1];
    (*tab)[j] = (double)above;
  }
  std::sort(big.begin(), big.end());
  *nbig = 0;
  for (size_t i = 0; i < big.size();) {
    size_t k = i;
    while (k < big.size() && big[k] == big[i]) ++k;
    tab->push_back((double)big[i]);
    tab->push_back((double)(k - i));
    ++*nbig;
    i = k;
  }
}

// Build shard s's table from its device copy of y_int (checked >= 0) and keep it next to the shard.
static int attach_nb_table(stk_model* m, const int32_t* yi_dev, int64_t n) {
  std::vector<int32_t> y((size_t)n);
  STK_HIP_CHECK(hipMemcpyAsync(y.data(), yi_dev, sizeof(int32_t) * n, hipMemcpyDeviceToHost, m->ctx->stream));
  STK_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  std::vector<double> tab;
  NbShardDev nb{};
  nb_build_table(y.data(), n, &tab, &nb.ncap, &nb.nbig);
  if (tab.empty()) tab.push_back(0.0);   // all counts zero: an empty table (ncap = nbig = 0)
  RC(upload(m, tab.data(), tab.size(), &nb.tab));
  STK_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));   // tab is a local: the copy must have read it
  m->nb.push_back(nb);
  return STK_OK;
}

// Sum of x[0 .. n) by halves down to runs of 8: a fixed order, the same bits on every run, error O(log n) ulp.
static double pairwise_sum(const double* x, int64_t n) {
  if (n <= 8) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += x[i];
    return s;
  }
  const int64_t h = n / 2;
  return pairwise_sum(x, h) + pairwise_sum(x + h, n - h);
}

// A gamma shard's derived data from its device copy of y: every y finite and > 0 (the first bad row is named),
// ly = log y as the array the sweeps read (*ly_dev; the shard keeps y itself for copy-out and the fingerprint)
// and L = sum ly in the shard's NbShardDev entry.
static int attach_gamma_data(stk_model* m, int s, const double* y_dev, int64_t n, const double** ly_dev) {
  std::vector<double> y((size_t)n);
  STK_HIP_CHECK(hipMemcpyAsync(y.data(), y_dev, sizeof(double) * n, hipMemcpyDeviceToHost, m->ctx->stream));
  STK_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  for (int64_t i = 0; i < n; ++i) {
    ARG_CHECK(std::isfinite(y[i]) && y[i] > 0.0, "shard %d: y[%lld] = %g; gamma needs y finite and > 0", s, (long long)i, y[i]);
    y[i] = log(y[i]);
  }
  const double L = pairwise_sum(y.data(), n);
  NbShardDev gm{};
  int rc = upload(m, y.data(), (size_t)n, ly_dev);
  if (rc == STK_OK) rc = upload(m, &L, 1, &gm.tab);
  // y and L are locals: whatever the uploads' outcome, a copy that was started must have read them before they go
  const hipError_t e = hipStreamSynchronize(m->ctx->stream);
  RC(rc);
  STK_HIP_CHECK(e);
  m->nb.push_back(gm);
  return STK_OK;
}

// A regression shard's y, dense or sparse: validated for the family, copied to the device, with the family's derived
// data (the negative binomial's count table, the gamma family's log y).  `in` is read for n_rows, y, y_int and sigma.
static int upload_regression_y(stk_model* m, int s, const stk_shard& in, ShardDev* out) {
  const int family = m->family;
  const size_t n = (size_t)in.n_rows;
  ShardDev& sd = *out;
  if (family == STK_CATEGORICAL) {   // y_int in [1, K] as given; checked once K is known (stk_model_set_categories)
    ARG_CHECK(in.y_int, "shard %d: categorical needs y_int", s);
    ARG_CHECK(!in.y && !in.sigma, "shard %d: categorical takes its classes in y_int alone; y and sigma must be NULL", s);
    RC(upload(m, in.y_int, n, &sd.yi));
  } else if (family == STK_LOGREG || family == STK_POISSON || family == STK_NEGBIN) {
    const bool pois = family != STK_LOGREG;   // a count family
    const char* fam = family == STK_NEGBIN ? "neg_binomial" : pois ? "poisson" : "logreg";
    ARG_CHECK(in.y_int, "shard %d: %s needs y_int", s, fam);
    // counts handed over as doubles too: say so, do not pick one of the two
    ARG_CHECK(!pois || (!in.y && !in.sigma), "shard %d: %s takes its counts in y_int alone; y and sigma must be NULL", s, fam);
    RC(upload(m, in.y_int, n, &sd.yi));
    RC(check_y_int(m, s, sd.yi, in.n_rows, pois, family == STK_NEGBIN ? "neg_binomial_2_log needs y >= 0" : "poisson_log needs y >= 0"));
    if (family == STK_NEGBIN) RC(attach_nb_table(m, sd.yi, in.n_rows));
  } else {   // family_dims knows every family: a new one must say here which y it takes
    ARG_CHECK(family == STK_LINREG || family == STK_STUDENT || family == STK_GAMMA, "shard %d: model family %d has no data layout", s,
              family);
    ARG_CHECK(in.y, "shard %d: %s needs y", s, family == STK_STUDENT ? "student_t" : family == STK_GAMMA ? "gamma" : "linreg");
    RC(upload(m, in.y, n, &sd.y));
    if (family == STK_GAMMA) RC(attach_gamma_data(m, s, sd.y, in.n_rows, &sd.sigma));   // sigma carries ly = log y (common.h)
  }
  return STK_OK;
}

// Shard s of a model from the caller's rows: validated, copied to the device, appended to m->sh.
static int upload_shard(stk_model* m, int s, const stk_shard& in) {
  const int family = m->family;
  const size_t n = (size_t)in.n_rows;
  ShardDev sd{};
  sd.n = in.n_rows;
  sd.d = family == STK_SCHOOLS ? 0 : in.n_cols;
  ARG_CHECK(in.n_rows > 0, "shard %d: n_rows must be positive", s);
  ARG_CHECK(family == STK_SCHOOLS || in.n_cols == m->d, "shard %d: n_cols %d differs from shard 0 (%d)", s, in.n_cols, m->d);
  RC(family_dims(family, in.n_rows, sd.d, &sd.D, &sd.P));
  if (family == STK_SCHOOLS) {
    ARG_CHECK(in.y && in.sigma, "shard %d: schools needs y and sigma", s);
    RC(upload(m, in.y, n, &sd.y));
    RC(upload(m, in.sigma, n, &sd.sigma));
  } else {
    ARG_CHECK(in.x && in.n_cols > 0, "shard %d: regression needs x", s);
    ARG_CHECK(stk_sweep_supported(1, in.n_cols), "n_cols %d unsupported (1..1024)", in.n_cols);
    RC(upload(m, in.x, n * in.n_cols, &sd.x));
    RC(upload_regression_y(m, s, in, &sd));
  }
  m->sh.push_back(sd);
  return STK_OK;
}

// ---------------------------------------------------------------- sparse shards
// A sparse shard's three CSR arrays as host memory: the caller's own, or copies of its device arrays.
struct CsrHost {
  std::vector<int64_t> ip;
  std::vector<int32_t> ix;
  std::vector<double> vv;
  const int64_t* indptr = nullptr;
  const int32_t* indices = nullptr;
  const double* values = nullptr;
};
static int csr_host(int s, const stk_shard_sparse& in, int device, CsrHost* h) {
  ARG_CHECK(in.n_rows > 0, "shard %d: n_rows must be positive", s);
  ARG_CHECK(in.indptr, "shard %d: a sparse shard needs indptr", s);
  h->indptr = in.indptr;
  if (device >= 0 && is_device_ptr(in.indptr, device)) {
    h->ip.resize((size_t)in.n_rows + 1);
    STK_HIP_CHECK(hipMemcpy(h->ip.data(), in.indptr, sizeof(int64_t) * h->ip.size(), hipMemcpyDefault));
    h->indptr = h->ip.data();
  }
  const int64_t nnz = h->indptr[in.n_rows];
  ARG_CHECK(nnz >= 0, "shard %d: row %lld: indptr ends at %lld; it runs from 0 to the number of entries", s,
            (long long)in.n_rows - 1, (long long)nnz);
  ARG_CHECK(nnz == 0 || (in.indices && in.values), "shard %d: a sparse shard with entries needs indices and values", s);
  h->indices = in.indices;
  h->values = in.values;
  if (nnz > 0 && device >= 0 && is_device_ptr(in.indices, device)) {
    h->ix.resize((size_t)nnz);
    STK_HIP_CHECK(hipMemcpy(h->ix.data(), in.indices, sizeof(int32_t) * h->ix.size(), hipMemcpyDefault));
    h->indices = h->ix.data();
  }
  if (nnz > 0 && device >= 0 && is_device_ptr(in.values, device)) {
    h->vv.resize((size_t)nnz);
    STK_HIP_CHECK(hipMemcpy(h->vv.data(), in.values, sizeof(double) * h->vv.size(), hipMemcpyDefault));
    h->values = h->vv.data();
  }
  return STK_OK;
}

// The checks of include/stark_hip.h (stk_shard_sparse), each naming the shard and the row, then the padded rows:
// K = the longest row, idx / val [n_rows][K], a short row filled up with (0, 0.0).  Nothing reaches the device
// before every index is known to lie in [0, d).
static int csr_pad_rows(int s, const stk_shard_sparse& in, const CsrHost& h, std::vector<int32_t>* idx, std::vector<double>* val,
                        int* K) {
  const int d = in.n_cols;
  const int64_t n = in.n_rows;
  ARG_CHECK(h.indptr[0] == 0, "shard %d: row 0: indptr[0] = %lld; indptr runs from 0 to the number of entries", s,
            (long long)h.indptr[0]);
  int64_t kmax = 0;
  for (int64_t r = 0; r < n; ++r) {
    const int64_t e0 = h.indptr[r], e1 = h.indptr[r + 1];
    ARG_CHECK(e1 >= e0, "shard %d: row %lld: indptr decreases (%lld after %lld)", s, (long long)r, (long long)e1, (long long)e0);
    ARG_CHECK(e1 <= h.indptr[n], "shard %d: row %lld: indptr %lld passes the number of entries %lld", s, (long long)r, (long long)e1,
              (long long)h.indptr[n]);
    for (int64_t e = e0; e < e1; ++e) {
      const int32_t j = h.indices[e];
      ARG_CHECK(j >= 0 && j < d, "shard %d: row %lld: index %d is outside [0, %d)", s, (long long)r, j, d);
      ARG_CHECK(e == e0 || j > h.indices[e - 1],
                "shard %d: row %lld: indices must be strictly increasing within a row (%d after %d): sort them and sum duplicates", s,
                (long long)r, j, h.indices[e - 1]);
      ARG_CHECK(std::isfinite(h.values[e]), "shard %d: row %lld: the value at column %d is not finite (%g)", s, (long long)r, j,
                h.values[e]);
    }
    kmax = std::max(kmax, e1 - e0);
  }
  *K = (int)kmax;   // <= d: a row's indices are distinct and in range
  idx->assign((size_t)n * kmax, 0);
  val->assign((size_t)n * kmax, 0.0);
  for (int64_t r = 0; r < n; ++r)
    for (int64_t e = h.indptr[r]; e < h.indptr[r + 1]; ++e) {
      (*idx)[(size_t)(r * kmax + (e - h.indptr[r]))] = h.indices[e];
      (*val)[(size_t)(r * kmax + (e - h.indptr[r]))] = h.values[e];
    }
  return STK_OK;
}

static int sparse_shard_dims(int s, int family, const stk_shard_sparse& in, int d0) {
  ARG_CHECK(is_sweep_family(family), "a sparse model is one of the six regression families, not the %s family (%d)", family_name(family),
            family);
  ARG_CHECK(in.n_cols > 0 && in.n_cols <= 1024, "shard %d: n_cols %d unsupported (1..1024)", s, in.n_cols);
  ARG_CHECK(in.n_cols == d0, "shard %d: n_cols %d differs from shard 0 (%d)", s, in.n_cols, d0);
  return STK_OK;
}

// Shard s of a sparse model: validated on the host, padded, copied to the device, appended to m->sh and m->sp.
static int upload_shard_sparse(stk_model* m, int s, const stk_shard_sparse& in) {
  RC(sparse_shard_dims(s, m->family, in, m->d));
  CsrHost h;
  RC(csr_host(s, in, m->ctx->device, &h));
  std::vector<int32_t> idx;
  std::vector<double> val;
  SpShardDev sp{};
  int K = 0;
  RC(csr_pad_rows(s, in, h, &idx, &val, &K));
  sp.K = K;
  ShardDev sd{};
  sd.n = in.n_rows;
  sd.d = in.n_cols;
  RC(family_dims(m->family, in.n_rows, sd.d, &sd.D, &sd.P));
  if (idx.empty()) {   // K = 0: nothing to read, but a pointer to hand over
    idx.push_back(0);
    val.push_back(0.0);
  }
  const int64_t before = m->bytes;
  int rc = upload(m, idx.data(), idx.size(), &sp.idx);
  if (rc == STK_OK) rc = upload(m, val.data(), val.size(), &sp.val);
  const hipError_t e = hipStreamSynchronize(m->ctx->stream);   // idx and val are locals: a started copy must have read them
  RC(rc);
  STK_HIP_CHECK(e);
  m->bytes = before + 12 * (int64_t)K * in.n_rows;
  const stk_shard ys{in.n_rows, in.n_cols, nullptr, in.y, in.y_int, nullptr};
  RC(upload_regression_y(m, s, ys, &sd));
  m->sh.push_back(sd);
  m->sp.push_back(sp);
  m->sp_nnz.push_back(h.indptr[in.n_rows]);
  return STK_OK;
}

static int upload_sp_table(stk_model* m) {
  RC(m->sp_dev.ensure(sizeof(SpShardDev) * m->sp.size()));
  STK_HIP_CHECK(hipMemcpyAsync(m->sp_dev.p, m->sp.data(), sizeof(SpShardDev) * m->sp.size(), hipMemcpyHostToDevice, m->ctx->stream));
  STK_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  return STK_OK;
}

// Every shard of a synthetic model, generated in place.  beta_dev is the caller's: released by it
// once the stream has drained.
static int gen_shards(stk_model* m, DevBuf* beta_dev, const std::vector<double>& beta, int64_t rows, int64_t row_offset,
                      uint64_t data_seed, double alpha, double noise_sigma) {
  const int family = m->family, d = m->d;
  RC(beta_dev->ensure(sizeof(double) * d));
  if (hipMemcpy(beta_dev->p, beta.data(), sizeof(double) * d, hipMemcpyHostToDevice) != hipSuccess) {
    stk_set_error("beta upload failed");
    return STK_E_HIP;
  }
  for (int s = 0; s < m->nshards; ++s) {
    ShardDev sd{};
    sd.n = rows;
    sd.d = d;
    family_dims(family, rows, d, &sd.D, &sd.P);
    m->bufs.emplace_back();
    RC(m->bufs.back().ensure(sizeof(double) * rows * d));
    double* X = m->bufs.back().as<double>();
    m->bufs.emplace_back();
    const size_t ybytes = family == STK_LOGREG ? sizeof(int32_t) * rows : sizeof(double) * rows;
    RC(m->bufs.back().ensure(ybytes));
    void* y = m->bufs.back().p;
    m->bytes += (int64_t)(sizeof(double) * rows * d + ybytes);
    const hipError_t e = stk_launch_gen_shard(X, family == STK_LINREG ? (double*)y : nullptr,
                                              family == STK_LOGREG ? (int32_t*)y : nullptr, rows, d,
                                              row_offset + (int64_t)s * rows, data_seed, alpha, beta_dev->as<double>(),
                                              noise_sigma, family, m->ctx->stream);
    if (e != hipSuccess) {
      stk_set_error("gen_shard launch: %s", hipGetErrorString(e));
      return STK_E_HIP;
    }
    sd.x = X;
    if (family == STK_LOGREG) sd.yi = (const int32_t*)y;
    else sd.y = (const double*)y;
    m->sh.push_back(sd);
  }
  return STK_OK;
}

void model_release(stk_model* m) {
  if (--m->refs > 0) return;
  stk_ctx* c = m->ctx;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  for (auto& b : m->bufs) b.release();
  m->sh_dev.release();
  m->nb_dev.release();
  m->sp_dev.release();
  delete m;
  ctx_release(c);
}

// ---------------------------------------------------------------- data fingerprint
// words() of the header: words([family, n_rows, n_cols], 0, 0).
static uint64_t fp_shard_header(int family, int64_t n_rows, int n_cols) {
  const uint64_t h[3] = {(uint64_t)family, (uint64_t)n_rows, (uint64_t)(family == STK_SCHOOLS ? 0 : n_cols)};
  return stk_fp_words_host(h, 3, 8, 0, 0);
}

// A sparse shard's header: four words, the longest row K among them.
static uint64_t fp_sparse_header(int family, int64_t n_rows, int n_cols, int K) {
  const uint64_t h[4] = {(uint64_t)family, (uint64_t)n_rows, (uint64_t)n_cols, (uint64_t)K};
  return stk_fp_words_host(h, 4, 8, 0, 0);
}

// One kernel per data array of the shard, all adding into one zeroed device word; cached.
int model_fingerprint(stk_model* m, int shard, uint64_t* out) {
  if (m->fp_ok.size() != (size_t)m->nshards) {
    m->fp.assign(m->nshards, 0);
    m->fp_ok.assign(m->nshards, 0);
  }
  if (!m->fp_ok[shard]) {
    stk_ctx* ctx = m->ctx;
    STK_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const ShardDev& s = m->sh[shard];
    RC(ctx->scratch[SCR_FP_SUM].ensure(sizeof(unsigned long long)));
    unsigned long long* sum = ctx->scratch[SCR_FP_SUM].as<unsigned long long>();
    STK_HIP_CHECK(hipMemsetAsync(sum, 0, sizeof(*sum), st));
    if (s.x) STK_HIP_CHECK(stk_launch_fp_words(s.x, s.n * s.d, 8, 1, 0, sum, st));
    if (m->sparse) {   // the padded rows, under tags of their own
      const SpShardDev& sp = m->sp[shard];
      STK_HIP_CHECK(stk_launch_fp_words(sp.idx, s.n * sp.K, 4, 5, 0, sum, st));
      STK_HIP_CHECK(stk_launch_fp_words(sp.val, s.n * sp.K, 8, 6, 0, sum, st));
    }
    if (s.y) STK_HIP_CHECK(stk_launch_fp_words(s.y, s.n, 8, 2, 0, sum, st));
    if (s.yi) STK_HIP_CHECK(stk_launch_fp_words(s.yi, s.n, 4, 3, 0, sum, st));
    if (m->family == STK_SCHOOLS) STK_HIP_CHECK(stk_launch_fp_words(s.sigma, s.n, 8, 4, 0, sum, st));   // the only family with a sigma array
    unsigned long long v = 0;
    STK_HIP_CHECK(hipMemcpyAsync(&v, sum, sizeof(v), hipMemcpyDeviceToHost, st));
    STK_HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t head = m->sparse ? fp_sparse_header(m->family, s.n, s.d, m->sp[shard].K) : fp_shard_header(m->family, s.n, s.d);
    m->fp[shard] = stk_fp_fmix(head + (uint64_t)v);
    m->fp_ok[shard] = 1;
  }
  *out = m->fp[shard];
  return STK_OK;
}

extern "C" {

int stk_model_create(stk_ctx* ctx, int family, const stk_shard* shards, int nshards, stk_model** out) {
  ARG_CHECK(ctx && shards && out && nshards > 0, "stk_model_create: bad arguments");
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  stk_model* m = model_new(ctx, family, nshards, family == STK_SCHOOLS ? 0 : shards[0].n_cols);
  int rc = STK_OK;
  for (int s = 0; s < nshards && rc == STK_OK; ++s) rc = upload_shard(m, s, shards[s]);
  return model_finish(m, rc, out);
}

int stk_model_create_sparse(stk_ctx* ctx, int family, const stk_shard_sparse* shards, int nshards, stk_model** out) {
  ARG_CHECK(ctx && shards && out && nshards > 0, "stk_model_create_sparse: bad arguments");
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  stk_model* m = model_new(ctx, family, nshards, shards[0].n_cols);
  m->sparse = true;
  int rc = STK_OK;
  for (int s = 0; s < nshards && rc == STK_OK; ++s) rc = upload_shard_sparse(m, s, shards[s]);
  if (rc == STK_OK) rc = upload_sp_table(m);
  return model_finish(m, rc, out);
}

int stk_model_sparse_info(const stk_model* m, int shard, int64_t out[3]) {
  ARG_CHECK(m && out && shard >= 0 && shard < m->nshards, "stk_model_sparse_info: bad arguments");
  ARG_CHECK(m->sparse, "stk_model_sparse_info: the model is dense (stk_model_create)");
  out[0] = m->sp[shard].K;
  out[1] = m->sp_nnz[shard];
  out[2] = 12 * (int64_t)m->sp[shard].K * m->sh[shard].n;
  return STK_OK;
}

int stk_shard_fingerprint_sparse_host(int family, const stk_shard_sparse* sh, uint64_t* out) {
  ARG_CHECK(sh && out, "stk_shard_fingerprint_sparse_host: bad arguments");
  RC(sparse_shard_dims(0, family, *sh, sh->n_cols));
  CsrHost h;
  RC(csr_host(0, *sh, -1, &h));
  std::vector<int32_t> idx;
  std::vector<double> val;
  int K = 0;
  RC(csr_pad_rows(0, *sh, h, &idx, &val, &K));
  uint64_t acc = fp_sparse_header(family, sh->n_rows, sh->n_cols, K);
  acc += stk_fp_words_host(idx.data(), sh->n_rows * K, 4, 5, 0) + stk_fp_words_host(val.data(), sh->n_rows * K, 8, 6, 0);
  if (family == STK_LOGREG || family == STK_POISSON || family == STK_NEGBIN) {
    ARG_CHECK(sh->y_int, "stk_shard_fingerprint_sparse_host: the %s family needs y_int", family_name(family));
    ARG_CHECK(family == STK_LOGREG || !sh->y, "stk_shard_fingerprint_sparse_host: the %s family takes its counts in y_int alone; y must be NULL",
              family_name(family));
    acc += stk_fp_words_host(sh->y_int, sh->n_rows, 4, 3, 0);
  } else {
    ARG_CHECK(sh->y, "stk_shard_fingerprint_sparse_host: the %s family needs y", family_name(family));
    acc += stk_fp_words_host(sh->y, sh->n_rows, 8, 2, 0);
  }
  *out = stk_fp_fmix(acc);
  return STK_OK;
}

int stk_gen_beta(uint64_t seed, int32_t d, double* beta) {
  ARG_CHECK(beta && d > 0, "stk_gen_beta: bad arguments");
  const double s = 1.0 / sqrt((double)d);
  for (int j = 0; j < d; ++j) beta[j] = normal_at(seed, (uint32_t)(j >> 1) & ~0u, 0u, 0u, (uint32_t)(j & 1), TAG_BETA) * s;
  return STK_OK;
}

int stk_model_create_synthetic(stk_ctx* ctx, int family, int nshards, int64_t rows_per_shard, int64_t row_offset,
                               int32_t n_cols, uint64_t data_seed, double alpha, const double* beta,
                               double noise_sigma, stk_model** out) {
  ARG_CHECK(ctx && out && nshards > 0 && rows_per_shard > 0 && n_cols > 0, "stk_model_create_synthetic: bad arguments");
  ARG_CHECK(family == STK_LOGREG || family == STK_LINREG,
            "synthetic shards exist for linreg/logreg only, not for the %s family (%d): the generator draws nothing "
            "else, build such shards from host rows with stk_model_create", family_name(family), family);
  ARG_CHECK(stk_sweep_supported(1, n_cols), "n_cols %d unsupported (1..1024)", n_cols);
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  std::vector<double> b(n_cols);
  if (beta) memcpy(b.data(), beta, sizeof(double) * n_cols);
  else stk_gen_beta(data_seed, n_cols, b.data());
  stk_model* m = model_new(ctx, family, nshards, n_cols);
  DevBuf beta_dev;
  const int rc = model_finish(m, gen_shards(m, &beta_dev, b, rows_per_shard, row_offset, data_seed, alpha, noise_sigma), out);
  beta_dev.release();
  return rc;
}

int stk_model_destroy(stk_model* m) {
  if (m) model_release(m);
  return STK_OK;
}

int stk_model_info(const stk_model* m, int shard, int32_t* D, int32_t* P, int64_t* n_rows) {
  ARG_CHECK(m && shard >= 0 && shard < m->nshards, "stk_model_info: bad shard");
  if (D) *D = m->sh[shard].D;
  if (P) *P = m->sh[shard].P;
  if (n_rows) *n_rows = m->sh[shard].n;
  return STK_OK;
}

int stk_model_device_bytes(const stk_model* m, int64_t* bytes) {
  ARG_CHECK(m && bytes, "bad arguments");
  *bytes = m->bytes;
  return STK_OK;
}

int stk_model_copy_data(stk_model* m, int shard, double* x, double* y, int32_t* y_int) {
  ARG_CHECK(m && shard >= 0 && shard < m->nshards, "stk_model_copy_data: bad shard");
  STK_HIP_CHECK(hipSetDevice(m->ctx->device));
  const ShardDev& s = m->sh[shard];
  hipStream_t st = m->ctx->stream;
  if (x && s.x) STK_HIP_CHECK(hipMemcpyAsync(x, s.x, sizeof(double) * s.n * s.d, hipMemcpyDefault, st));
  if (y && s.y) STK_HIP_CHECK(hipMemcpyAsync(y, s.y, sizeof(double) * s.n, hipMemcpyDefault, st));
  if (y_int && s.yi) STK_HIP_CHECK(hipMemcpyAsync(y_int, s.yi, sizeof(int32_t) * s.n, hipMemcpyDefault, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  return STK_OK;
}

int stk_model_set_prior(stk_model* m, double alpha_scale, double beta_scale) {
  ARG_CHECK(m, "stk_model_set_prior: NULL model");
  ARG_CHECK(is_density_family(m->family), "priors apply to the regression families");
  ARG_CHECK(alpha_scale >= 0.0 && beta_scale >= 0.0, "prior scales must be >= 0 (0 or inf: flat)");
  auto prec = [](double sc) { return (sc == 0.0 || std::isinf(sc)) ? 0.0 : 1.0 / (sc * sc); };
  for (auto& sd : m->sh) {
    sd.pa = prec(alpha_scale);
    sd.pb = prec(beta_scale);
  }
  STK_HIP_CHECK(hipSetDevice(m->ctx->device));
  STK_HIP_CHECK(hipMemcpy(m->sh_dev.p, m->sh.data(), sizeof(ShardDev) * m->sh.size(), hipMemcpyHostToDevice));
  return STK_OK;
}

int stk_model_set_prior_phi(stk_model* m, double shape, double rate) {
  ARG_CHECK(m, "stk_model_set_prior_phi: NULL model");
  ARG_CHECK(m->family == STK_NEGBIN, "stk_model_set_prior_phi: a prior on phi is for the neg_binomial family, not for the %s family (%d)",
            family_name(m->family), m->family);
  ARG_CHECK(shape > 0.0 && std::isfinite(shape) && rate >= 0.0 && std::isfinite(rate),
            "stk_model_set_prior_phi: phi ~ gamma(shape, rate) needs shape > 0 and rate >= 0 (1, 0: flat), got (%g, %g)", shape, rate);
  for (auto& nb : m->nb) {
    nb.pr_a1 = shape - 1.0;
    nb.pr_b = rate;
  }
  STK_HIP_CHECK(hipSetDevice(m->ctx->device));
  return upload_nb_table(m);
}

int stk_model_set_prior_shape(stk_model* m, double shape, double rate) {
  ARG_CHECK(m, "stk_model_set_prior_shape: NULL model");
  ARG_CHECK(m->family == STK_GAMMA, "stk_model_set_prior_shape: a prior on shape is for the gamma family, not for the %s family (%d)",
            family_name(m->family), m->family);
  ARG_CHECK(shape > 0.0 && std::isfinite(shape) && rate >= 0.0 && std::isfinite(rate),
            "stk_model_set_prior_shape: shape ~ gamma(shape, rate) needs shape > 0 and rate >= 0 (1, 0: flat), got (%g, %g)", shape, rate);
  for (auto& gm : m->nb) {
    gm.pr_a1 = shape - 1.0;
    gm.pr_b = rate;
  }
  STK_HIP_CHECK(hipSetDevice(m->ctx->device));
  return upload_nb_table(m);
}

int stk_gamma_shape_terms_host(double a, double* out2) {
  ARG_CHECK(out2, "stk_gamma_shape_terms_host: out2 is NULL");
  gamma_shape_terms(a, out2);
  return STK_OK;
}

int stk_model_set_student_nu(stk_model* m, double nu) {
  ARG_CHECK(m, "stk_model_set_student_nu: NULL model");
  ARG_CHECK(m->family == STK_STUDENT, "stk_model_set_student_nu: nu is for the student_t family, not for the %s family (%d)",
            family_name(m->family), m->family);
  ARG_CHECK(std::isfinite(nu) && nu > 0.0, "stk_model_set_student_nu: nu must be finite and > 0, got %g", nu);
  m->nu = nu;
  for (auto& sd : m->sh) shard_set_nu(sd, nu);
  STK_HIP_CHECK(hipSetDevice(m->ctx->device));
  return upload_shard_table(m);
}

int stk_model_set_categories(stk_model* m, int32_t ncat) {
  ARG_CHECK(m, "stk_model_set_categories: NULL model");
  ARG_CHECK(m->family == STK_CATEGORICAL, "stk_model_set_categories: classes are for the categorical family, not for the %s family (%d)",
            family_name(m->family), m->family);
  ARG_CHECK(m->ncat == 0, "stk_model_set_categories: the model's classes are set already (K = %d): they are set once", m->ncat);
  ARG_CHECK(ncat >= 2, "stk_model_set_categories: K = %d classes; categorical_logit needs K >= 2 (d = %d)", ncat, m->d);
  const int G = ncat - 1, d = m->d;
  ARG_CHECK(stk_sweep_cat_supported(G, d) && (int64_t)G * (d + 1) <= 1024,
            "stk_model_set_categories: K = %d classes at d = %d covariates are outside the categorical sweep's envelope: it needs "
            "K - 1 <= 16, (K - 1) ceil(d / 16) <= 16 and (K - 1)(d + 1) <= 1024", ncat, d);
  stk_ctx* ctx = m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf flag;
  RC(flag.ensure(sizeof(int64_t)));
  for (int s = 0; s < m->nshards; ++s) {   // the kernel never sees a class outside [1, K]
    const ShardDev& sd = m->sh[s];
    int64_t bad = -1;
    int32_t v = 0;
    hipError_t e = stk_launch_check_ycat(sd.yi, sd.n, ncat, flag.as<int64_t>(), st);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, flag.p, sizeof(int64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && bad >= 0 && bad < sd.n) e = hipMemcpy(&v, sd.yi + bad, sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
      flag.release();
      stk_set_error("shard %d: y_int check failed: %s", s, hipGetErrorString(e));
      return STK_E_HIP;
    }
    if (bad >= 0 && bad < sd.n) {
      flag.release();
      stk_set_error("shard %d: y_int[%lld] = %d; categorical_logit with K = %d classes needs 1 .. %d", s, (long long)bad, v, ncat, ncat);
      return STK_E_ARG;
    }
  }
  flag.release();
  m->ncat = ncat;
  for (auto& sd : m->sh) {
    sd.D = G * (d + 1);
    sd.P = sd.D + 1;
  }
  return upload_shard_table(m);
}

int stk_negbin_phi_terms_host(const int32_t* y_int, int64_t n, double phi, double* out) {
  ARG_CHECK(y_int && out && n > 0, "stk_negbin_phi_terms_host: bad arguments");
  ARG_CHECK(phi > 0.0 && std::isfinite(phi), "stk_negbin_phi_terms_host: phi must be positive and finite, got %g", phi);
  for (int64_t i = 0; i < n; ++i)
    ARG_CHECK(y_int[i] >= 0, "stk_negbin_phi_terms_host: y_int[%lld] = %d; neg_binomial_2_log needs y >= 0", (long long)i, y_int[i]);
  std::vector<double> tab;
  int ncap = 0, nbig = 0;
  nb_build_table(y_int, n, &tab, &ncap, &nbig);
  const double v = log(phi);
  double a1 = 0.0, a2 = 0.0;
  for (int e = 0; e < ncap + nbig; ++e) {
    double t1, t2;
    nb_entry_term(tab.data(), ncap, e, phi, v, &t1, &t2);
    a1 += t1;
    a2 += t2;
  }
  out[0] = a1;
  out[1] = a2 / phi;   // the device keeps phi sum [psi(y + phi) - psi(phi)], what d lp / d v takes
  return STK_OK;
}

int stk_model_shard_arrays(const stk_model* m, int shard, stk_shard* out) {
  ARG_CHECK(m && out && shard >= 0 && shard < m->nshards, "stk_model_shard_arrays: bad arguments");
  const ShardDev& s = m->sh[shard];
  *out = stk_shard{s.n, s.d, s.x, s.y, s.yi, m->family == STK_SCHOOLS ? s.sigma : nullptr};
  return STK_OK;
}

int stk_model_fingerprint(stk_model* m, int shard, uint64_t* out) {
  ARG_CHECK(m && out && shard >= 0 && shard < m->nshards, "stk_model_fingerprint: bad arguments");
  return model_fingerprint(m, shard, out);
}

int stk_fingerprint_words(stk_ctx* ctx, const void* buf, int64_t count, int32_t word_bytes, int32_t tag,
                          uint64_t index0, uint64_t* sum) {
  ARG_CHECK(sum, "stk_fingerprint_words: sum is NULL");
  ARG_CHECK(word_bytes == 4 || word_bytes == 8, "stk_fingerprint_words: word_bytes must be 4 or 8, got %d", word_bytes);
  ARG_CHECK(tag >= 0 && tag <= 4, "stk_fingerprint_words: tag must be in 0..4, got %d", tag);
  ARG_CHECK(count >= 0, "stk_fingerprint_words: count must be >= 0");
  ARG_CHECK(buf || count == 0, "stk_fingerprint_words: buf is NULL");
  ARG_CHECK(((uintptr_t)buf & (uintptr_t)(word_bytes - 1)) == 0, "stk_fingerprint_words: buf is not aligned to %d bytes",
            word_bytes);
  *sum = 0;
  if (count == 0) return STK_OK;
  if (!ctx) {   // the caller asked for the host twin: no device is touched
    *sum = stk_fp_words_host(buf, count, word_bytes, tag, index0);
    return STK_OK;
  }
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  RC(ctx->scratch[SCR_FP_SUM].ensure(sizeof(unsigned long long)));
  unsigned long long* acc = ctx->scratch[SCR_FP_SUM].as<unsigned long long>();
  STK_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(*acc), st));
  if (is_device_ptr(buf, ctx->device)) {
    STK_HIP_CHECK(stk_launch_fp_words(buf, count, word_bytes, tag, index0, acc, st));
  } else {   // host (or another device's) memory: staged in pieces, words() is additive over index ranges
    const int64_t piece = ((int64_t)64 << 20) / word_bytes;
    DevBuf& stage = ctx->scratch[SCR_FP_STAGE];
    RC(stage.ensure((size_t)std::min(count, piece) * word_bytes));
    const char* src = static_cast<const char*>(buf);
    for (int64_t i0 = 0; i0 < count; i0 += piece) {
      const int64_t n = std::min(piece, count - i0);
      STK_HIP_CHECK(hipMemcpyAsync(stage.p, src + i0 * word_bytes, (size_t)n * word_bytes, hipMemcpyDefault, st));
      STK_HIP_CHECK(stk_launch_fp_words(stage.p, n, word_bytes, tag, index0 + (uint64_t)i0, acc, st));
    }
  }
  unsigned long long v = 0;
  STK_HIP_CHECK(hipMemcpyAsync(&v, acc, sizeof(v), hipMemcpyDeviceToHost, st));
  STK_HIP_CHECK(hipStreamSynchronize(st));
  *sum = v;
  return STK_OK;
}

int stk_shard_fingerprint_host(int family, const stk_shard* sh, uint64_t* out) {
  ARG_CHECK(sh && out, "stk_shard_fingerprint_host: bad arguments");
  ARG_CHECK(family == STK_SCHOOLS || family == STK_LINREG || family == STK_LOGREG || family == STK_POISSON || family == STK_NEGBIN ||
                family == STK_STUDENT || family == STK_GAMMA || family == STK_CATEGORICAL,
            "unknown model family %d", family);
  ARG_CHECK(sh->n_rows > 0, "stk_shard_fingerprint_host: n_rows must be positive");
  uint64_t acc = fp_shard_header(family, sh->n_rows, sh->n_cols);
  if (family == STK_SCHOOLS) {
    ARG_CHECK(sh->y && sh->sigma, "stk_shard_fingerprint_host: schools needs y and sigma");
    acc += stk_fp_words_host(sh->y, sh->n_rows, 8, 2, 0) + stk_fp_words_host(sh->sigma, sh->n_rows, 8, 4, 0);
  } else {
    ARG_CHECK(sh->x && sh->n_cols > 0, "stk_shard_fingerprint_host: regression needs x");
    acc += stk_fp_words_host(sh->x, sh->n_rows * sh->n_cols, 8, 1, 0);
    if (family == STK_LOGREG || family == STK_POISSON || family == STK_NEGBIN || family == STK_CATEGORICAL) {
      const char* fam = family == STK_CATEGORICAL ? "categorical" : family == STK_NEGBIN ? "neg_binomial" : family == STK_POISSON ? "poisson" : "logreg";
      ARG_CHECK(sh->y_int, "stk_shard_fingerprint_host: %s needs y_int", fam);
      ARG_CHECK(family == STK_LOGREG || (!sh->y && !sh->sigma),
                "stk_shard_fingerprint_host: %s takes its counts in y_int alone; y and sigma must be NULL", fam);
      acc += stk_fp_words_host(sh->y_int, sh->n_rows, 4, 3, 0);
    } else {
      ARG_CHECK(sh->y, "stk_shard_fingerprint_host: %s needs y",
                family == STK_STUDENT ? "student_t" : family == STK_GAMMA ? "gamma" : "linreg");
      acc += stk_fp_words_host(sh->y, sh->n_rows, 8, 2, 0);
    }
  }
  *out = stk_fp_fmix(acc);
  return STK_OK;
}

}  // extern "C"
