// Access-pattern A/B of the data fingerprint's streaming read (stark_amd/csrc/fingerprint.hip) on one
// headline shard's X (1.25e7 x 100 doubles, 10 GB): loads one grid stride apart against a block
// taking U consecutive 4 KiB segments, plain against nontemporal loads, blocks per CU, and each form
// with fmix replaced by an xor ("novalu": is the kernel bound by the integer multiplies or by HBM?).
// Every variant with fmix must print the same sum.  DESIGN.md "Data fingerprint" quotes the result
// (profiles/r12a_fingerprint_micro.log).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/fingerprint_micro.hip -o tools/_bin/fingerprint_micro
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

constexpr uint64_t FP_K = 0x9E3779B97F4A7C15ull, FP_M = 0xD6E8FEB86659FD93ull;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t fmix(uint64_t a) {
  a ^= a >> 32;
  a *= FP_M;
  a ^= a >> 29;
  return a;
}
template <bool NOVALU>
__device__ __forceinline__ uint64_t terms(const u32x4 v, uint64_t key) {
  const uint64_t w0 = (uint64_t)v.x | ((uint64_t)v.y << 32), w1 = (uint64_t)v.z | ((uint64_t)v.w << 32);
  if constexpr (NOVALU) return (w0 ^ w1) + key;
  return fmix(w0 + key) + fmix(w1 + key + FP_K);
}
template <bool NT>
__device__ __forceinline__ u32x4 ld(const u32x4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  return *p;
}

// MODE 0: grid-stride, U loads one grid stride apart.  MODE 1: a block takes U consecutive 4 KiB
// segments per trip (the grid strides by U segments per block).
template <int MODE, int U, bool NT, bool NOVALU>
__global__ __launch_bounds__(256) void k(const u32x4* p, int64_t nvec, uint64_t base, unsigned long long* sum) {
  uint64_t acc = 0;
  if constexpr (MODE == 0) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t key = base + (uint64_t)(v * 2) * FP_K;
    const uint64_t dk = (uint64_t)stride * 2 * FP_K;
    for (; v + (U - 1) * stride < nvec; v += U * stride) {
      u32x4 r[U];
#pragma unroll
      for (int j = 0; j < U; ++j) r[j] = ld<NT>(p + v + j * stride);
#pragma unroll
      for (int j = 0; j < U; ++j) acc += terms<NOVALU>(r[j], key + j * dk);
      key += U * dk;
    }
    for (; v < nvec; v += stride) {
      acc += terms<NOVALU>(ld<NT>(p + v), key);
      key += dk;
    }
  } else {
    const int64_t stride = (int64_t)gridDim.x * 256 * U;
    int64_t v = (int64_t)blockIdx.x * 256 * U + threadIdx.x;
    uint64_t key = base + (uint64_t)(v * 2) * FP_K;
    const uint64_t dk = (uint64_t)stride * 2 * FP_K, dj = (uint64_t)256 * 2 * FP_K;
    for (; v + (U - 1) * 256 < nvec; v += stride) {
      u32x4 r[U];
#pragma unroll
      for (int j = 0; j < U; ++j) r[j] = ld<NT>(p + v + j * 256);
#pragma unroll
      for (int j = 0; j < U; ++j) acc += terms<NOVALU>(r[j], key + j * dj);
      key += dk;
    }
    for (int j = 0; j < U; ++j)
      if (v + j * 256 < nvec) acc += terms<NOVALU>(ld<NT>(p + v + j * 256), key + j * dj);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor((unsigned long long)acc, o);
  __shared__ unsigned long long part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(sum, part[0] + part[1] + part[2] + part[3]);
}

#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(_e), __LINE__); return 1; } } while (0)

template <int MODE, int U, bool NT, bool NOVALU>
int run(const char* name, const u32x4* p, int64_t nvec, int bpc, int cus, unsigned long long* sum) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int blocks = cus * bpc;
  std::vector<float> ms;
  unsigned long long h = 0;
  for (int r = 0; r < 7; ++r) {
    CK(hipMemset(sum, 0, 8));
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL((k<MODE, U, NT, NOVALU>), dim3(blocks), dim3(256), 0, 0, p, nvec, FP_K + 1, sum);
    CK(hipGetLastError());
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float t;
    CK(hipEventElapsedTime(&t, e0, e1));
    if (r >= 2) ms.push_back(t);
    CK(hipMemcpy(&h, sum, 8, hipMemcpyDeviceToHost));
  }
  std::sort(ms.begin(), ms.end());
  const double med = ms[ms.size() / 2];
  printf("%-34s bpc %2d  median %.3f ms  min %.3f  %.3f TB/s  sum %016llx\n", name, bpc, med, ms[0],
         (double)nvec * 16 / (med * 1e-3) / 1e12, h);
  fflush(stdout);
  return 0;
}

int main() {
  int cus = 0;
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  const int64_t nvec = (int64_t)12500000 * 100 / 2;   // one headline shard's X
  u32x4* p;
  unsigned long long* sum;
  CK(hipMalloc(&p, nvec * 16));
  CK(hipMalloc(&sum, 8));
  CK(hipMemset(p, 0x5a, nvec * 16));
  CK(hipDeviceSynchronize());
  printf("CUs %d, %.2f GB\n", cus, nvec * 16 / 1e9);
  for (int round = 0; round < 2; ++round) {
    if (run<0, 4, false, false>("gridstride U4", p, nvec, 8, cus, sum)) return 1;
    if (run<0, 4, false, true>("gridstride U4 novalu", p, nvec, 8, cus, sum)) return 1;
    if (run<0, 4, true, false>("gridstride U4 nt", p, nvec, 8, cus, sum)) return 1;
    if (run<0, 4, false, false>("gridstride U4", p, nvec, 16, cus, sum)) return 1;
    if (run<0, 4, false, false>("gridstride U4", p, nvec, 4, cus, sum)) return 1;
    if (run<0, 8, false, false>("gridstride U8", p, nvec, 8, cus, sum)) return 1;
    if (run<0, 8, true, false>("gridstride U8 nt", p, nvec, 8, cus, sum)) return 1;
    if (run<0, 2, false, false>("gridstride U2", p, nvec, 16, cus, sum)) return 1;
    if (run<1, 4, false, false>("blockchunk U4", p, nvec, 8, cus, sum)) return 1;
    if (run<1, 4, false, true>("blockchunk U4 novalu", p, nvec, 8, cus, sum)) return 1;
    if (run<1, 4, true, false>("blockchunk U4 nt", p, nvec, 8, cus, sum)) return 1;
    if (run<1, 8, false, false>("blockchunk U8", p, nvec, 8, cus, sum)) return 1;
    if (run<1, 8, true, false>("blockchunk U8 nt", p, nvec, 8, cus, sum)) return 1;
    if (run<1, 4, false, false>("blockchunk U4", p, nvec, 16, cus, sum)) return 1;
    if (run<1, 8, true, true>("blockchunk U8 nt novalu", p, nvec, 8, cus, sum)) return 1;
  }
  CK(hipFree(p));
  CK(hipFree(sum));
  return 0;
}
