// C ABI of libstark_hip.so: checkpoint / resume of a sampler.  The blob's layout and the checks of
// a blob's header are in state_blob.h (host only); here are the device copies around them.
#include "capi_internal.h"
#include "state_blob.h"

namespace {
// The sampler's checkpoint segments, in the blob's order.
std::vector<SamplerBuf> state_segments(stk_sampler* s) {
  std::vector<SamplerBuf> segs;
  for (const SamplerBuf& b : sampler_buffers(s))
    if (b.saved) segs.push_back(b);
  return segs;
}

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  template <class T>
  void add(const T& v) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&v);
    for (size_t i = 0; i < sizeof(T); ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
};

int state_geometry(const stk_sampler* s, uint64_t* out) {
  const NutsArgs& A = s->A;
  const stk_model* m = s->m;
  Fnv f;
  f.add(m->family), f.add(m->nshards), f.add(m->d), f.add(m->Dmax), f.add(m->Pmax);
  for (const auto& sd : m->sh) f.add(sd.n), f.add(sd.D), f.add(sd.P), f.add(sd.pa), f.add(sd.pb);
  for (const auto& nb : m->nb) f.add(nb.pr_a1), f.add(nb.pr_b);   // negative binomial: the phi prior; gamma: the shape prior (no other family has entries)
  if (m->family == STK_STUDENT) f.add(m->nu);                       // student_t alone: a state saved at nu = 4 is not one for nu = 5
  if (m->family == STK_CATEGORICAL) f.add(m->ncat);                 // categorical alone: (K = 3, d = 5) and (K = 4, d = 3) share D = 12
  f.add(A.nchains), f.add(A.C), f.add(A.Dp), f.add(A.max_depth), f.add(A.num_warmup), f.add(A.num_samples);
  f.add(A.adapt), f.add(A.var_on), f.add(A.skip_ss), f.add(A.iter_offset);
  f.add(A.init_buffer), f.add(A.term_buffer), f.add(A.base_window);
  f.add(A.delta), f.add(A.gamma), f.add(A.kappa), f.add(A.t0), f.add(A.seed), f.add(A.jitter);
  f.add(A.uturn_ext), f.add(A.cpw_cap), f.add(A.ud_first), f.add(A.ud_iters), f.add(s->nch);
  if (A.metric) f.add(A.metric);   // diag_e blobs keep the hash they always had
  f.add((int)(s->ar_fn != nullptr));   // full-data mode: its [grad | lp] block holds sums over ranks
  std::vector<int32_t> ids(m->nshards);
  for (int i = 0; i < m->nshards; ++i) ids[i] = i;
  if (A.shard_ids)
    STK_HIP_CHECK(hipMemcpy(ids.data(), A.shard_ids, sizeof(int32_t) * ids.size(), hipMemcpyDeviceToHost));
  for (int v : ids) f.add(v);
  *out = f.h;
  return STK_OK;
}

// What a blob of this sampler holds besides the segments themselves: their sizes, the geometry
// hash and the model's fingerprints.  `e` points into the two vectors.
struct Expected {
  std::vector<uint64_t> seg_bytes, fps;
  StateExpect e{};
};
int state_expect(stk_sampler* s, const std::vector<SamplerBuf>& segs, Expected* x) {
  ARG_CHECK(segs.size() <= (size_t)kStateMaxSegs, "sampler state: %zu segments, the header holds %d", segs.size(), kStateMaxSegs);
  for (const SamplerBuf& g : segs) x->seg_bytes.push_back(g.bytes);
  x->fps.resize(s->m->nshards);
  for (int sh = 0; sh < s->m->nshards; ++sh) RC(model_fingerprint(s->m, sh, &x->fps[sh]));
  x->e = StateExpect{x->seg_bytes.data(), segs.size(), 0, x->fps.data(), s->m->nshards};
  return state_geometry(s, &x->e.geometry);
}
}  // namespace

extern "C" {

int stk_sampler_state_bytes(stk_sampler* s, int64_t* bytes) {
  ARG_CHECK(s && bytes, "stk_sampler_state_bytes: bad arguments");
  size_t n = sizeof(StateHeader) + sizeof(uint64_t) * (size_t)s->m->nshards;
  for (const SamplerBuf& g : state_segments(s)) n += g.bytes;
  *bytes = (int64_t)n;
  return STK_OK;
}

int stk_sampler_save_state(stk_sampler* s, void* buf, int64_t bytes) {
  ARG_CHECK(s && buf, "stk_sampler_save_state: bad arguments");
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  const auto segs = state_segments(s);
  Expected x;
  RC(state_expect(s, segs, &x));
  const int64_t need = (int64_t)x.e.blob_bytes();
  ARG_CHECK(bytes >= need, "stk_sampler_save_state: buffer of %lld bytes, the state needs %lld", (long long)bytes,
            (long long)need);
  StateHeader h{};
  memcpy(h.magic, kStateMagic, 8);
  h.version = kStateVersion;
  h.nsegs = (uint32_t)segs.size();
  h.geometry = x.e.geometry;
  h.step = s->step;
  h.steps = s->steps;
  h.sweeps = s->sweeps;
  h.shard_sweeps = s->shard_sweeps;
  h.sweep_ms = s->sweep_ms;
  std::copy(x.seg_bytes.begin(), x.seg_bytes.end(), h.seg_bytes);
  char* out = static_cast<char*>(buf);
  memcpy(out, &h, sizeof(h));
  memcpy(out + sizeof(h), x.fps.data(), sizeof(uint64_t) * x.fps.size());
  size_t off = sizeof(h) + sizeof(uint64_t) * x.fps.size();
  for (const SamplerBuf& g : segs) {
    STK_HIP_CHECK(hipMemcpyAsync(out + off, g.get(), g.bytes, hipMemcpyDefault, ctx->stream));
    off += g.bytes;
  }
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return STK_OK;
}

int stk_sampler_load_state(stk_sampler* s, const void* buf, int64_t bytes) {
  ARG_CHECK(s && buf, "stk_sampler_load_state: bad arguments");
  stk_ctx* ctx = s->m->ctx;
  STK_HIP_CHECK(hipSetDevice(ctx->device));
  const auto segs = state_segments(s);
  Expected x;
  RC(state_expect(s, segs, &x));
  StateHeader h;
  char msg[512];
  if (const int rc = state_blob_check(buf, bytes, x.e, &h, msg, sizeof(msg))) {
    stk_set_error("%s", msg);
    return rc;
  }
  const char* in = static_cast<const char*>(buf) + sizeof(h) + sizeof(uint64_t) * x.fps.size();
  for (const SamplerBuf& g : segs) {
    STK_HIP_CHECK(hipMemcpyAsync(g.get(), in, g.bytes, hipMemcpyDefault, ctx->stream));
    in += g.bytes;
  }
  STK_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  s->step = (int)h.step;
  s->steps = h.steps;
  s->sweeps = h.sweeps;
  s->shard_sweeps = h.shard_sweeps;
  s->sweep_ms = h.sweep_ms;
  return STK_OK;
}

}  // extern "C"
