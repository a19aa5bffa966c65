// Host check of stark_amd/csrc/state_blob.h: blobs built in memory -- a valid one and one per way a
// blob from a file can be wrong -- against state_blob_check's verdict and message.  Meant for a
// sanitizer, since the header's tables are indexed by counts that come from the blob:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o state_blob_check tools/state_blob_check.cpp
//   ./state_blob_check
// Exits non-zero on any miss (tests/test_host_state_blob.py runs it).
#include <cstdio>
#include <cstring>
#include <vector>
#include "../stark_amd/csrc/state_blob.h"

using namespace stk;

static const uint64_t kSegs[3] = {64, 24, 8};            // the loading sampler: three segments,
static const uint64_t kFps[3] = {0x1111, 0x2222, 0x3333};   // three shards
static const StateExpect kExpect{kSegs, 3, 0xfeedbeefull, kFps, 3};

// A blob that kExpect accepts, in a heap block of exactly its size (so an overread is a report).
static std::vector<unsigned char> valid_blob() {
  StateHeader h{};
  memcpy(h.magic, kStateMagic, 8);
  h.version = kStateVersion;
  h.nsegs = 3;
  h.geometry = kExpect.geometry;
  h.step = 7;
  memcpy(h.seg_bytes, kSegs, sizeof(kSegs));
  std::vector<unsigned char> b(kExpect.blob_bytes(), 0xab);
  memcpy(b.data(), &h, sizeof(h));
  memcpy(b.data() + sizeof(h), kFps, sizeof(kFps));
  return b;
}

static int misses = 0;
// want: nullptr for a blob that must load, else words the message must contain.
static void expect(const char* name, const std::vector<unsigned char>& blob, const char* want) {
  // the bytes in a block of their own size: reading past a truncated blob is a heap overflow
  std::vector<unsigned char> exact(blob.begin(), blob.end());
  StateHeader h;
  char msg[512] = "";
  const int rc = state_blob_check(exact.data(), (int64_t)exact.size(), kExpect, &h, msg, sizeof(msg));
  const bool ok = want ? (rc == STK_E_ARG && strstr(msg, want) && strstr(msg, "stk_sampler_load_state: ") == msg)
                       : (rc == STK_OK && h.step == 7);
  printf("%-28s rc %d  %s%s\n", name, rc, msg, ok ? "" : "   <-- MISS");
  misses += !ok;
}

template <class F>
static std::vector<unsigned char> with(F edit) {
  std::vector<unsigned char> b = valid_blob();
  StateHeader h;
  memcpy(&h, b.data(), sizeof(h));
  edit(h, b);
  if (b.size() >= sizeof(h)) memcpy(b.data(), &h, sizeof(h));
  return b;
}
using Blob = std::vector<unsigned char>;

int main() {
  expect("valid", valid_blob(), nullptr);
  expect("empty", Blob(), "blob of 0 bytes, this sampler's state has 312");
  expect("shorter than the header", with([](StateHeader&, Blob& b) { b.resize(sizeof(StateHeader) - 1); }), "blob of 191 bytes");
  expect("header alone", with([](StateHeader&, Blob& b) { b.resize(sizeof(StateHeader)); }), "blob of 192 bytes");
  expect("cut inside the fingerprints", with([](StateHeader&, Blob& b) { b.resize(sizeof(StateHeader) + 12); }), "blob of 204 bytes");
  expect("one byte short", with([](StateHeader&, Blob& b) { b.pop_back(); }), "blob of 311 bytes");
  expect("one byte long", with([](StateHeader&, Blob& b) { b.push_back(0); }), "blob of 313 bytes");
  expect("wrong magic", with([](StateHeader& h, Blob&) { h.magic[0] ^= 1; }), "not a sampler state blob");
  expect("wrong magic, other size", with([](StateHeader& h, Blob& b) { h.magic[0] ^= 1; b.push_back(0); }), "blob of 313 bytes");
  expect("version 1", with([](StateHeader& h, Blob&) { h.version = 1; }), "version 1 ");
  expect("version 1, other size", with([](StateHeader& h, Blob& b) { h.version = 1; b.resize(200); }), "version 1 ");
  expect("other segment count", with([](StateHeader& h, Blob&) { h.nsegs = 2; }), "saved with another metric (2 segments, this sampler has 3)");
  // a foreign-metric blob hears about the metric before it hears about its size
  expect("other segment count and size", with([](StateHeader& h, Blob& b) { h.nsegs = 6; b.resize(b.size() + 3 * 64); }),
         "saved with another metric");
  expect("nsegs above the table", with([](StateHeader& h, Blob&) { h.nsegs = kStateMaxSegs + 1; }), "saved with another metric (17 segments");
  expect("nsegs 2^32 - 1", with([](StateHeader& h, Blob&) { h.nsegs = 0xffffffffu; }), "saved with another metric");
  expect("other geometry", with([](StateHeader& h, Blob&) { h.geometry ^= 1; }), "another model geometry or sampler config");
  expect("segment 0 size", with([](StateHeader& h, Blob&) { h.seg_bytes[0] = 56; }), "segment 0 size mismatch");
  expect("segment 2 size", with([](StateHeader& h, Blob&) { h.seg_bytes[2] = 16; }), "segment 2 size mismatch");
  expect("geometry before segment size", with([](StateHeader& h, Blob&) { h.geometry ^= 1; h.seg_bytes[0] = 0; }), "another model geometry");
  expect("other data, shard 0", with([](StateHeader&, Blob& b) { b[sizeof(StateHeader)] ^= 1; }), "saved against other data (shard 0)");
  expect("other data, shard 2", with([](StateHeader&, Blob& b) { b[sizeof(StateHeader) + 16] ^= 1; }), "saved against other data (shard 2)");
  expect("other data, shards 1 and 2", with([](StateHeader&, Blob& b) { b[sizeof(StateHeader) + 8] ^= 1; b[sizeof(StateHeader) + 23] ^= 0x80; }),
         "saved against other data (shard 1)");
  expect("segment size before data", with([](StateHeader& h, Blob& b) { h.seg_bytes[1] = 0; b[sizeof(StateHeader)] ^= 1; }), "segment 1 size mismatch");

  // a sampler that claims more segments than the header holds is refused, not indexed
  std::vector<uint64_t> many(kStateMaxSegs + 1, 8);
  const StateExpect big{many.data(), many.size(), kExpect.geometry, kFps, 3};
  const Blob b = valid_blob();
  StateHeader h;
  char msg[512] = "";
  const bool ok = state_blob_check(b.data(), (int64_t)b.size(), big, &h, msg, sizeof(msg)) == STK_E_ARG && strstr(msg, "17 segments");
  printf("%-28s %s%s\n", "17 expected segments", msg, ok ? "" : "   <-- MISS");
  misses += !ok;

  printf("%d miss(es)\n", misses);
  return misses ? 1 : 0;
}
