// The sampler checkpoint blob's header and its checks: host only, no HIP header, so the parsing of
// bytes that come from a file is tested (and sanitized) without a device (tools/state_blob_check.cpp).
//
// Blob (version 2): StateHeader, one uint64 data fingerprint per shard (stk_model_fingerprint),
// then the device segments in sampler_buffers() order.  The header's geometry hash covers
// everything that shapes the state or its evolution (model family and shard geometry, priors,
// every sampler setting, the RNG seed and shard ids, full-data mode) and the fingerprints cover
// the rows, so a blob only loads into a sampler that continues the same run on the same data.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/stark_hip.h"

namespace stk {

constexpr int kStateMaxSegs = 16;
struct StateHeader {
  char magic[8];
  uint32_t version, nsegs;
  uint64_t geometry;
  int64_t step, steps, sweeps, shard_sweeps;
  double sweep_ms;
  uint64_t seg_bytes[kStateMaxSegs];
};
constexpr char kStateMagic[8] = {'S', 'T', 'K', 'S', 'T', 'A', 'T', 'E'};
constexpr uint32_t kStateVersion = 2;   // 1: no fingerprints after the header

// What the loading sampler expects of a blob.
struct StateExpect {
  const uint64_t* seg_bytes;   // nsegs <= kStateMaxSegs segment sizes
  size_t nsegs;
  uint64_t geometry;
  const uint64_t* fps;         // this model's fingerprint of each of its nshards shards
  int nshards;
  size_t blob_bytes() const {
    size_t n = sizeof(StateHeader) + sizeof(uint64_t) * (size_t)nshards;
    for (size_t i = 0; i < nsegs; ++i) n += seg_bytes[i];
    return n;
  }
};

// STK_OK when the `bytes` bytes at buf are a blob this sampler can load; else STK_E_ARG with the
// reason in msg.  Nothing of buf past `bytes` is read, and nothing of the header's tables past what `e`
// has: a foreign metric is named before the sizes are compared, the total size is settled before
// the fingerprints are read.  *h receives the header when it could be read.
inline int state_blob_check(const void* buf, int64_t bytes, const StateExpect& e, StateHeader* h, char* msg, size_t cap) {
#define STK_BLOB_FAIL(...) return snprintf(msg, cap, "stk_sampler_load_state: " __VA_ARGS__), STK_E_ARG
  const size_t need = e.blob_bytes();
  if (e.nsegs > (size_t)kStateMaxSegs) STK_BLOB_FAIL("%zu segments, the header holds %d", e.nsegs, kStateMaxSegs);
  memset(h, 0, sizeof(*h));
  if (bytes >= (int64_t)sizeof(*h)) memcpy(h, buf, sizeof(*h));
  const bool magic = !memcmp(h->magic, kStateMagic, 8);
  if (magic && h->version != kStateVersion)
    STK_BLOB_FAIL("the blob is a version %u sampler state, this library reads version %u (version 1 carries no data "
                  "fingerprints): save the state again with this library", h->version, kStateVersion);
  if (magic && h->nsegs != e.nsegs)   // another metric: said so, before the sizes are compared
    STK_BLOB_FAIL("the state was saved with another metric (%u segments, this sampler has %zu)", h->nsegs, e.nsegs);
  if (bytes < 0 || (size_t)bytes != need)
    STK_BLOB_FAIL("blob of %lld bytes, this sampler's state has %lld", (long long)bytes, (long long)need);
  if (!magic) STK_BLOB_FAIL("not a sampler state blob");
  if (h->geometry != e.geometry) STK_BLOB_FAIL("the state belongs to another model geometry or sampler config");
  for (size_t i = 0; i < e.nsegs; ++i)
    if (h->seg_bytes[i] != e.seg_bytes[i]) STK_BLOB_FAIL("segment %zu size mismatch", i);
  const char* in = static_cast<const char*>(buf) + sizeof(*h);
  for (int sh = 0; sh < e.nshards; ++sh) {   // the rows, not only their shape
    uint64_t saved;
    memcpy(&saved, in + sizeof(saved) * (size_t)sh, sizeof(saved));
    if (saved != e.fps[sh]) STK_BLOB_FAIL("the state was saved against other data (shard %d)", sh);
  }
#undef STK_BLOB_FAIL
  return STK_OK;
}

}  // namespace stk
