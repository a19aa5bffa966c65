// What the units of the C ABI layer (capi*.hip) share: the error macros, the handle types and the
// helpers that more than one unit calls.  Host-side orchestration only: every numeric result comes
// from a gfx950 kernel; there is no CPU fallback.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "launchers.h"

using namespace stk;

#define ARG_CHECK(cond, ...)          \
  do {                                \
    if (!(cond)) {                    \
      stk_set_error(__VA_ARGS__);     \
      return STK_E_ARG;               \
    }                                 \
  } while (0)
#define RC(expr)                      \
  do {                                \
    int _rc = (expr);                 \
    if (_rc != STK_OK) return _rc;    \
  } while (0)

// ---------------------------------------------------------------- device buffers
struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  int ensure(size_t bytes) {
    if (bytes <= n && p) return STK_OK;
    if (p) hipFree(p);
    p = nullptr;
    n = 0;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
      p = nullptr;
      stk_set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
      return STK_E_NOMEM;
    }
    n = bytes;
    return STK_OK;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    n = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// The context's grow-only scratch buffers, each named after the one entry-point family that owns
// it: an entry point may call another family's while it holds its own (the Hessian calls the hooks).
// The three sweeps over a draw image (predictive, PSIS-LOO, per-draw log density) are one family:
// they never call one another, and each synchronises before it returns.
enum Scratch : int {
  SCR_HOOK_Q, SCR_HOOK_LP, SCR_HOOK_GRAD,   // parity hooks (regression and schools): points, lp, grad
  SCR_HOOK_PARTIAL, SCR_HOOK_WS,            // regression hooks: partial sums, 64-chain workspace
  SCR_FP_SUM, SCR_FP_STAGE,                 // fingerprints: the device sum, staging of host words
  SCR_HESS_WS, SCR_HESS_QH,                 // Hessian: chunk-partial workspace, points and result
  SCR_COMB_F64, SCR_COMB_MAT, SCR_COMB_I32, // combine: draws-sized doubles, P x P matrices, ints
  SCR_DRAW_IMG, SCR_DRAW_PARTIAL, SCR_DRAW_ROWS,   // draw-image sweeps: image + draws (+ lp), partials, per-row staging
  SCR_LAPLACE,                                     // Laplace proposal: mode, factor, draws, log_q
  SCR_BOOT_IO, SCR_BOOT_PARTIAL,                   // bootstrap sweep: points + streams + lp, grad, wsum; partials
  SCR_DPE_IN, SCR_DPE_MOM, SCR_DPE_PREP, SCR_DPE_WS,   // density-product combiner: staged draws; the combine's moments;
                                                       // prepared arrays (one-call path, host callers); Z, draws, trace
  SCR_COUNT
};

// Handles are reference counted (a model holds its context, a sampler its model), so the
// caller may destroy them in any order -- e.g. a garbage collector finalising a cycle.
struct stk_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;     // false: a caller's stream (stk_ctx_create_on_stream), not destroyed here
  int profiling = 0;
  int refs = 1;
  DevBuf scratch[SCR_COUNT];
};

struct stk_model {
  int refs = 1;
  stk_ctx* ctx = nullptr;
  int family = 0;
  int nshards = 0;
  int d = 0;
  int Dmax = 0, Pmax = 0;
  std::vector<ShardDev> sh;
  std::vector<DevBuf> bufs;
  DevBuf sh_dev;
  std::vector<NbShardDev> nb;   // STK_NEGBIN: per shard, the count table (in bufs) and the phi prior; derived data
                                // (STK_GAMMA: per shard, L = sum log y (in bufs) and the shape prior)
  DevBuf nb_dev;                // its device copy, what the reduce reads
  bool sparse = false;          // every shard's design matrix is kept as padded rows (stk_model_create_sparse): sh[s].x is null
  std::vector<SpShardDev> sp;   // its side table, per shard (idx and val live in bufs), and the entries handed over
  std::vector<int64_t> sp_nnz;
  DevBuf sp_dev;                // the side table's device copy, what k_sweep_sp reads
  double nu = 0.0;              // STK_STUDENT: the degrees of freedom (0: not set yet); every shard's ShardDev carries a copy
  int ncat = 0;                 // STK_CATEGORICAL: the classes K (0: not set yet; stk_model_set_categories); likewise
  int64_t bytes = 0;
  std::vector<uint64_t> fp;   // shard fingerprints, computed on first use (the data never changes)
  std::vector<char> fp_ok;
};

// A run's sweeps over shards [first, first + count) at Ct chains per shard, the one construction
// for the sampler and the parity hooks.  Every chain batch has its first chain c0, its own region
// of the partial-sum buffer and its grouped launches: consecutive shards of equal n share one
// launch of nsh * G blocks (stk_sweep_plan decides the kernel and its shape), and every shard's
// partial sums lie Gs = the batch's largest G chunks apart.  The 64-chain workspace is one, reused
// by successive 64-batches on the stream.
struct SweepGroup { int shard0, nsh; SweepLaunch launch; };
struct ChainBatch {
  int c0 = 0, Gs = 1;
  size_t part_off = 0;        // doubles into the partial-sum buffer
  std::vector<SweepGroup> groups;
};
struct ChainPlan {
  std::vector<ChainBatch> batches;
  int Ct = 0;
  size_t partial_bytes = 0;   // every batch's [nshards][Gs][C][sweep_pw] doubles
  SweepLaunch ws_at{};        // the 64-batch launch of the shard with the most rows (kind 0: no workspace)
  size_t ws_bytes = 0;        // its workspace for every shard of the model
};

struct stk_sampler {
  stk_model* m = nullptr;
  stk_config cfg{};
  NutsArgs A{};
  int nch = 1;
  int step = 0;
  int64_t steps = 0;
  int64_t sweeps = 0;
  int64_t shard_sweeps = 0;
  double sweep_ms = 0.0;
  std::vector<DevBuf> bufs;
  DevBuf partial, ran, ws;
  SweepWs sws{};
  stk_allreduce_fn ar_fn = nullptr;   // full-data mode: rank-sum of [grad | lp] after every reduce
  void* ar_user = nullptr;
  ChainPlan plan;
  std::vector<hipEvent_t> ev;
  std::vector<int> iv_host;
  std::vector<unsigned long long> cnt_host;
};

// One device buffer that a sampler's NutsArgs points to.  sampler_buffers() is the one description
// of them: allocation, creation-time zeroing and the checkpoint's segments all iterate it.
struct SamplerBuf {
  void* field;    // the address of the NutsArgs pointer the buffer fills: the pointer itself is read
                  // when the buffer is used (stk_sampler_set_allreduce may redirect g_in after creation)
  size_t bytes;
  bool saved;     // a checkpoint segment (zeroed at creation), in the table's order
  void* get() const {
    void* p;
    memcpy(&p, field, sizeof(p));
    return p;
  }
  void set(void* p) const { memcpy(field, &p, sizeof(p)); }
};
std::vector<SamplerBuf> sampler_buffers(stk_sampler* s);   // capi_sampler.hip; needs s->A's counts filled

// ---- capi.hip
void ctx_release(stk_ctx* c);
// device memory ON THE CONTEXT'S DEVICE (hipMalloc / a torch cuda tensor): an entry point reads or
// writes it in place instead of staging it through the context's scratch buffers.  Memory of
// another device is not used in place (the kernels would dereference it without peer access): it
// takes the staged hipMemcpyAsync(Default) path, which copies across devices.
bool is_device_ptr(const void* p, int device);

// ---- capi_model.hip
const char* family_name(int family);
bool is_regression(int family);     // linear, logistic, poisson: every regression entry point
bool is_sweep_family(int family);   // those, neg_binomial, student_t and gamma: the gradient sweeps, the sampler, the priors
bool is_density_family(int family); // those and categorical, whose sweep is its own (sweep_cat.hip): the hooks, the sampler, the priors
int model_ready(const stk_model* m);   // STK_E_ARG for a student_t model whose nu, or a categorical one whose K, has not been set (no hidden default)
void model_release(stk_model* m);
int model_fingerprint(stk_model* m, int shard, uint64_t* out);   // cached
// shard == -1 means every shard: the first shard, how many, and the largest per-shard chunk count.
struct ShardRange { int shard0, nsh, Gs; };
ShardRange shard_range(const stk_model* m, int shard, int (*chunks)(int64_t n));

// ---- capi_density.hip: the chain plan (its construction comment is at ChainPlan above)
std::vector<int> chain_batches(int C, int d);
std::vector<int> chain_batches_sparse(int C, int d);
std::vector<int> chain_batches_cat(int C, int ncat, int d);
std::vector<int> model_chain_batches(const stk_model* m, int C);   // the model's family and storage decide which of the three
int model_sweep_pw(const stk_model* m);                            // columns of a chunk's partial row per chain
// An entry point without a sparse form: STK_E_ARG, before anything is launched, with a message that names the
// entry point and says that the model is sparse.
#define REFUSE_SPARSE(m, what)                                                                                      \
  ARG_CHECK(!(m)->sparse, "%s: the model is sparse (stk_model_create_sparse); the sparse storage serves the density " \
                          "hooks and the sampler only: build a dense model for this", what)
int chain_plan(const stk_model* m, const std::vector<int>& sizes, int first, int count, ChainPlan* cp);
hipError_t plan_sweeps(const stk_model* m, const ChainPlan& cp, const SweepCall& run, hipStream_t st);
hipError_t plan_reduces(const stk_model* m, const ChainPlan& cp, const SweepCall& run, double* lp, double* g,
                        hipStream_t st);
