// 16-byte pieces of a weight row, as the row gathers (ocf_sparse.hip) and the per-entry predictions
// (ocf_predict.hip) read them: row-major [rows][ldw] or the 16-bit 64x64-blocked layout (ocf.h b_blocked).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ocf {

template <typename WT> struct EPc { static constexpr int v = 16 / (int)sizeof(WT); };

// piece p (16 bytes) of row n of a weight array: row-major [rows][ldw] or 64x64-blocked (16-bit)
template <typename WT>
__device__ __forceinline__ void load_piece(const WT* W, int64_t ldw, int blocked, int n, int p,
                                           float (&out)[EPc<WT>::v]) {
  constexpr int E = EPc<WT>::v;
  const char* base;
  if (blocked) {
    const int h = p * 8;
    base = reinterpret_cast<const char*>(W) + ((((int64_t)(n >> 6) * (ldw >> 6)) + (h >> 6)) << 13) + (n & 63) * 128 +
           (h & 63) * 2;
  } else {
    base = reinterpret_cast<const char*>(W + (int64_t)n * ldw) + p * 16;
  }
  const uint4 u = *reinterpret_cast<const uint4*>(base);
  if constexpr (sizeof(WT) == 4) {
    __builtin_memcpy(out, &u, 16);
  } else {
    WT e[E];
    __builtin_memcpy(e, &u, 16);
#pragma unroll
    for (int k = 0; k < E; ++k) out[k] = (float)e[k];
  }
}

// raw 16-byte piece (kept packed in registers until used: half the VGPRs for 16-bit weights)
template <typename WT>
__device__ __forceinline__ uint4 load_piece_raw(const WT* W, int64_t ldw, int blocked, int n, int p) {
  const char* base;
  if (blocked) {
    const int h = p * 8;
    base = reinterpret_cast<const char*>(W) + ((((int64_t)(n >> 6) * (ldw >> 6)) + (h >> 6)) << 13) + (n & 63) * 128 +
           (h & 63) * 2;
  } else {
    base = reinterpret_cast<const char*>(W + (int64_t)n * ldw) + p * 16;
  }
  return *reinterpret_cast<const uint4*>(base);
}
template <typename WT>
__device__ __forceinline__ void unpack_piece(const uint4& u, float (&out)[EPc<WT>::v]) {
  if constexpr (sizeof(WT) == 4) {
    __builtin_memcpy(out, &u, 16);
  } else {
    WT e[EPc<WT>::v];
    __builtin_memcpy(e, &u, 16);
#pragma unroll
    for (int k = 0; k < EPc<WT>::v; ++k) out[k] = (float)e[k];
  }
}

}  // namespace ocf
