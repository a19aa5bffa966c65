// C ABI of libstark_hip.so (declared in include/stark_hip.h): errors, version, config defaults and
// the context.  The other entry points are in capi_model.hip, capi_density.hip, capi_sampler.hip,
// capi_run.hip, capi_state.hip and capi_combine.hip; what they share is in capi_internal.h.
#include <stdarg.h>

#include "capi_internal.h"

// ---------------------------------------------------------------- errors
static thread_local char g_err[1024] = "";
void stk_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

bool is_device_ptr(const void* p, int device) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();   // a plain host pointer is no error here
    return false;
  }
  return a.type == hipMemoryTypeDevice && a.device == device;
}

void ctx_release(stk_ctx* c) {
  if (--c->refs > 0) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  for (auto& b : c->scratch) b.release();
  if (c->own_stream) hipStreamDestroy(c->stream);
  delete c;
}

extern "C" {

const char* stk_last_error(void) { return g_err; }
int stk_version(void) { return 1; }

void stk_config_default(stk_config* c) {
  memset(c, 0, sizeof(*c));
  c->num_warmup = 1000;
  c->num_samples = 1000;
  c->chains = 1;
  c->max_depth = 10;
  c->adapt_delta = 0.8;
  c->adapt_gamma = 0.05;
  c->adapt_kappa = 0.75;
  c->adapt_t0 = 10.0;
  c->stepsize = 1.0;
  c->init_radius = 2.0;
  c->adapt_init_buffer = 75;
  c->adapt_term_buffer = 50;
  c->adapt_window = 25;
  c->adapt_engaged = 1;
  c->seed = 1234;
}

// ---------------------------------------------------------------- context
// A context on `device` with no stream yet; `who` names the entry point in the messages.
static int ctx_new(const char* who, int device, stk_ctx** out) {
  ARG_CHECK(out, "%s: out is NULL", who);
  int n = 0;
  STK_HIP_CHECK(hipGetDeviceCount(&n));
  ARG_CHECK(device >= 0 && device < n, "%s: device %d not in [0, %d)", who, device, n);
  STK_HIP_CHECK(hipSetDevice(device));
  *out = new stk_ctx();
  (*out)->device = device;
  return STK_OK;
}

int stk_ctx_create(int device, stk_ctx** out) {
  RC(ctx_new("stk_ctx_create", device, out));
  const hipError_t e = hipStreamCreateWithFlags(&(*out)->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete *out;
    *out = nullptr;
    stk_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
    return STK_E_HIP;
  }
  return STK_OK;
}

int stk_ctx_create_on_stream(int device, void* stream, stk_ctx** out) {
  RC(ctx_new("stk_ctx_create_on_stream", device, out));
  (*out)->stream = (hipStream_t)stream;   // NULL = the device's null stream
  (*out)->own_stream = false;
  return STK_OK;
}

int stk_ctx_destroy(stk_ctx* c) {
  if (c) ctx_release(c);
  return STK_OK;
}

int stk_ctx_sync(stk_ctx* c) {
  ARG_CHECK(c, "stk_ctx_sync: NULL context");
  STK_HIP_CHECK(hipSetDevice(c->device));
  STK_HIP_CHECK(hipStreamSynchronize(c->stream));
  return STK_OK;
}

int stk_ctx_set_profiling(stk_ctx* c, int on) {
  ARG_CHECK(c, "NULL context");
  ARG_CHECK(on >= 0, "stk_ctx_set_profiling: on must be >= 0");
  c->profiling = on;
  return STK_OK;
}

void* stk_ctx_stream(stk_ctx* c) { return c ? (void*)c->stream : nullptr; }

}  // extern "C"
