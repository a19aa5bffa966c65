// Shard fingerprint (include/stark_hip.h, "data fingerprint"): a position-sensitive 64-bit sum over
// a stream of 8- or 4-byte words, computed where the rows lie.  All arithmetic is modulo 2^64:
//   fmix(a):  a ^= a >> 32;  a *= M;  a ^= a >> 29
//   words(w[0..m), tag, index0) = sum_i fmix(w[i] + (index0 + i + 1) * K + T[tag])
// The sum is an integer sum, so the kernel's reduction order (lanes, waves, one atomic per block)
// and the host twin's left-to-right loop give the same bits.  fmix has ONE 64 x 64 multiply: the
// kernel has to stay under the HBM time of the read at gfx950's 32-bit integer multiply rate
// (DESIGN.md "Data fingerprint").
#include "launchers.h"
#include <string.h>
#include <algorithm>
#include <type_traits>

namespace stk {

constexpr uint64_t FP_K = 0x9E3779B97F4A7C15ull, FP_M = 0xD6E8FEB86659FD93ull;
// A block reads FP_UNROLL consecutive 4 KiB segments per trip (one 16-byte load per lane and segment,
// all in flight together), nontemporal: 6.50 TB/s on one 10 GB shard against 5.74 for plain loads
// one grid stride apart, and the same time with fmix removed -- HBM-bound (DESIGN.md "Data fingerprint").
constexpr int FP_BLOCK = 256, FP_UNROLL = 8, FP_BLOCKS_PER_CU = 8;

__host__ __device__ __forceinline__ uint64_t fp_fmix(uint64_t a) {
  a ^= a >> 32;
  a *= FP_M;
  a ^= a >> 29;
  return a;
}

typedef uint32_t fp_u32x4 __attribute__((ext_vector_type(4)));

// The terms of one 16-byte vector whose first word has key `key` = index * K + T (index 1-based).
template <int WB>
__device__ __forceinline__ uint64_t fp_vec_terms(const fp_u32x4 v, uint64_t key) {
  if constexpr (WB == 8) {
    const uint64_t w0 = (uint64_t)v.x | ((uint64_t)v.y << 32), w1 = (uint64_t)v.z | ((uint64_t)v.w << 32);
    return fp_fmix(w0 + key) + fp_fmix(w1 + key + FP_K);
  } else {   // int32 patterns, zero-extended
    return fp_fmix((uint64_t)v.x + key) + fp_fmix((uint64_t)v.y + key + FP_K) +
           fp_fmix((uint64_t)v.z + key + 2 * FP_K) + fp_fmix((uint64_t)v.w + key + 3 * FP_K);
  }
}

// words() over `count` WB-byte words at buf, added into *sum.  base = (index0 + 1) * K + T[tag], so
// element e contributes fmix(w[e] + base + e * K).  The first `head` (< 16 / WB) words bring the
// address to a 16-byte boundary; `nvec` 16-byte vectors follow, read grid-stride in chunks of
// FP_UNROLL * FP_BLOCK vectors per block, each lane's key advanced by adds alone; the < 16 / WB words
// after them and the head go scalar, on lanes of block 0.  Every index is 64-bit: a headline shard
// has 1.25e9 words.
template <int WB>
__global__ __launch_bounds__(FP_BLOCK) void k_fp_words(const void* buf, int64_t count, int head, int64_t nvec,
                                                       uint64_t base, unsigned long long* sum) {
  constexpr int N = 16 / WB;
  typedef typename std::conditional<WB == 8, uint64_t, uint32_t>::type word_t;
  const word_t* w = static_cast<const word_t*>(buf);
  const fp_u32x4* p = reinterpret_cast<const fp_u32x4*>(w + head);
  const int64_t stride = (int64_t)gridDim.x * (FP_BLOCK * FP_UNROLL);
  int64_t v = (int64_t)blockIdx.x * (FP_BLOCK * FP_UNROLL) + threadIdx.x;
  uint64_t key = base + (uint64_t)(head + v * N) * FP_K;
  const uint64_t dk = (uint64_t)stride * N * FP_K;          // one trip of the grid
  constexpr uint64_t dj = (uint64_t)FP_BLOCK * N * FP_K;    // one segment
  uint64_t acc = 0;
  for (; v + (FP_UNROLL - 1) * FP_BLOCK < nvec; v += stride, key += dk) {
    fp_u32x4 r[FP_UNROLL];
#pragma unroll
    for (int j = 0; j < FP_UNROLL; ++j) r[j] = __builtin_nontemporal_load(p + v + j * FP_BLOCK);
#pragma unroll
    for (int j = 0; j < FP_UNROLL; ++j) acc += fp_vec_terms<WB>(r[j], key + j * dj);
  }
  // the ragged last chunk: this lane's v now lies in it, or past the end
  for (int j = 0; j < FP_UNROLL; ++j)
    if (v + j * FP_BLOCK < nvec) acc += fp_vec_terms<WB>(__builtin_nontemporal_load(p + v + j * FP_BLOCK), key + j * dj);
  if (blockIdx.x == 0) {
    const int64_t tail0 = head + nvec * N;          // first word after the vectors
    const int t = threadIdx.x;
    if (t < head + (int)(count - tail0)) {
      const int64_t e = t < head ? t : tail0 + (t - head);
      acc += fp_fmix((uint64_t)w[e] + base + (uint64_t)e * FP_K);
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor((unsigned long long)acc, o);
  __shared__ unsigned long long part[FP_BLOCK / WAVE];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int i = 0; i < FP_BLOCK / WAVE; ++i) s += part[i];
    atomicAdd(sum, s);
  }
}

// (5, 6: a sparse shard's padded columns and values -- the library's own; stk_fingerprint_words takes 0..4)
static const uint64_t kFpTag[7] = {0x243F6A8885A308D3ull, 0x13198A2E03707344ull, 0xA4093822299F31D0ull,
                                   0x082EFA98EC4E6C89ull, 0x452821E638D01377ull, 0xBE5466CF34E90C6Cull,
                                   0xC0AC29B7C97C50DDull};

}  // namespace stk

using namespace stk;

uint64_t stk_fp_fmix(uint64_t a) { return fp_fmix(a); }

// The host twin: the definition, left to right.
uint64_t stk_fp_words_host(const void* buf, int64_t count, int word_bytes, int tag, uint64_t index0) {
  const unsigned char* b = static_cast<const unsigned char*>(buf);
  uint64_t key = (index0 + 1) * FP_K + kFpTag[tag], acc = 0;
  for (int64_t i = 0; i < count; ++i, key += FP_K) {
    uint64_t w = 0;
    if (word_bytes == 8) {
      memcpy(&w, b + 8 * i, 8);
    } else {
      uint32_t w32;
      memcpy(&w32, b + 4 * i, 4);
      w = w32;
    }
    acc += fp_fmix(w + key);
  }
  return acc;
}

// Adds words(buf[0..count), tag, index0) into *sum (device memory, zeroed by the caller) on `st`.
// buf: device memory aligned to word_bytes.  The grid is sized to the device, not to the buffer.
hipError_t stk_launch_fp_words(const void* buf, int64_t count, int word_bytes, int tag, uint64_t index0,
                               unsigned long long* sum, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  const int N = 16 / word_bytes;
  int head = (int)(((16 - ((uintptr_t)buf & 15)) & 15) / word_bytes);
  if (head > count) head = (int)count;
  const int64_t nvec = (count - head) / N;
  int dev = 0, cus = 0;
  if (const hipError_t e = hipGetDevice(&dev)) return e;
  if (const hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) return e;
  int64_t blocks = (nvec + FP_BLOCK * FP_UNROLL - 1) / (FP_BLOCK * FP_UNROLL);
  blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)std::max(cus, 1) * FP_BLOCKS_PER_CU));
  const uint64_t base = (index0 + 1) * FP_K + kFpTag[tag];
  if (word_bytes == 8)
    hipLaunchKernelGGL(k_fp_words<8>, dim3((unsigned)blocks), dim3(FP_BLOCK), 0, st, buf, count, head, nvec, base, sum);
  else
    hipLaunchKernelGGL(k_fp_words<4>, dim3((unsigned)blocks), dim3(FP_BLOCK), 0, st, buf, count, head, nvec, base, sum);
  return hipGetLastError();
}
