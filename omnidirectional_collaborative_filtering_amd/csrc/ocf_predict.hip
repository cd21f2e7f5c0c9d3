// ocf_predict_entries: the decoder's prediction at listed entries only (ocf.h) -- no decoder GEMM over all columns,
// no [B][N] array.
//
//   y[lboff[b] + j] = clip( aux * ( h[b] . W[col_j] + bias[col_j] ) )          for every entry j of batch row b
//
// Launch 1, predict_entries_kernel: the forward half of ocf_sparse.hip's decoder_chunk.  A workgroup owns one chunk
// of one batch row; a group of G lanes owns an entry at a time and each lane holds PPL 16-byte pieces of the entry's
// weight row (pieces l, l + G, ...: every load instruction of a group reads G x 16 contiguous bytes, and the
// blocked shadow is read as it lies).  Column, target, flag and bias of the next entries load one iteration ahead.
// What the training kernel carries beyond that -- the d * W_out[n] sums (acc[V]), their reduction through LDS, the
// [n_chunks][H] partials and the arrival counters -- is not here, and the registers they held go to entries in
// flight: U = 8 / PPL entries per group (the decoder keeps RG_UD at 133 - 163 VGPRs).
//   H <= 512: h[b] sits in registers (the lane's own PPL pieces).
//   H  > 512: h[b] is staged once per workgroup in LDS (fp32) and the row is walked in 512-wide slabs, a lane
//             accumulating its share of every slab before the one group reduction.
// fp32 accumulation everywhere.  Every entry is independent: y does not depend on the chunk tables.
// Statistics: lane 0 of a group sums its entries' (y - t)^2, |y - t| and t + y != 0 on the stored y; the groups'
// sums are added in group order into chunk_stats[c].
// Launch 2, predict_rows_kernel (statistics only, one workgroup): thread b adds the chunk rows of batch row b in chunk
// order (its first chunk by a search of the non-decreasing ch_row), zeros for rows without chunks and padding rows,
// then the rows are added in a fixed order into total[4].
// No atomics, no wait between workgroups, every loop bounded by the tables.
#include <algorithm>

#include "ocf_internal.h"
#include "ocf_pieces.h"

using namespace ocf;

namespace {

constexpr int PE_THREADS = 256;
constexpr int PE_SLAB = 512;          // elements of a row a group holds at a time
constexpr int PE_MAX_H = 2048;
constexpr int PE_ROW_THREADS = 256;

__device__ __forceinline__ float load_h(const void* h, int dtype, int64_t i) {
  if (dtype == OCF_F16) return (float)reinterpret_cast<const _Float16*>(h)[i];
  if (dtype == OCF_BF16) return (float)reinterpret_cast<const __bf16*>(h)[i];
  return reinterpret_cast<const float*>(h)[i];
}

// SLAB = false: H = G * PPL * E, the hidden row in registers.  SLAB = true: any H, 512 elements (G * PPL * E) of
// the row at a time against the hidden row in LDS; the last slab may be short (its missing pieces are not loaded).
template <typename WT, int G, int PPL, bool SLAB>
__global__ void __launch_bounds__(PE_THREADS) predict_entries_kernel(OcfPredictArgs a) {
  constexpr int E = EPc<WT>::v;
  constexpr int V = PPL * E;
  constexpr int NG = PE_THREADS / G;
  constexpr int U = 8 / PPL;                    // entries per group in flight (8 pieces = 32 VGPRs per lane)
  static_assert(!SLAB || G * V == PE_SLAB, "a slab is 512 elements");
  __shared__ float st[NG][4];
  __shared__ float h_sh[SLAB ? PE_MAX_H : 1];
  const int c = blockIdx.x;
  const int b = a.ch_row[c], j0 = a.ch_j0[c];
  const int grp = threadIdx.x / G, l = threadIdx.x % G;
  const int r = a.rows[b];
  const int j1 = r >= 0 ? a.ch_j1[c] : j0;      // a batch row without a CSR row has no entries
  const int64_t s = r >= 0 ? a.rp[r] : 0;
  const int64_t lb = a.lboff[b];
  const WT* W = reinterpret_cast<const WT*>(a.W);
  const bool stats = a.val != nullptr && a.row_stats != nullptr;
  const int pieces = a.H / E;

  int n[U];
  float t[U];
  bool fl[U];
  auto idx = [&](int j) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ju = j + u * NG;
      const bool ok = ju < j1;
      n[u] = ok ? a.col[s + ju] : -1;
      t[u] = ok && stats ? a.val[s + ju] : 0.f;
      fl[u] = ok && stats && (a.flag == nullptr || a.flag[lb + ju] != 0);
    }
  };
  idx(j0 + grp);

  float hv[V];
  if constexpr (SLAB) {
    for (int x = threadIdx.x; x < a.H; x += PE_THREADS) h_sh[x] = load_h(a.h, a.h_dtype, (int64_t)b * a.ldh + x);
    __syncthreads();
  } else {
#pragma unroll
    for (int i = 0; i < PPL; ++i)
#pragma unroll
      for (int k = 0; k < E; ++k) hv[i * E + k] = load_h(a.h, a.h_dtype, (int64_t)b * a.ldh + (l + G * i) * E + k);
  }

  float sse = 0.f, sae = 0.f, cnt = 0.f;
  for (int j = j0 + grp; j < j1; j += NG * U) {
    int nc[U];
    float tc[U], bn[U], dot[U];
    bool fc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      nc[u] = n[u];
      tc[u] = t[u];
      fc[u] = fl[u];
      bn[u] = nc[u] >= 0 ? a.bias[nc[u]] : 0.f;
      dot[u] = 0.f;
    }
    const int nslab = SLAB ? (a.H + PE_SLAB - 1) / PE_SLAB : 1;
    for (int sl = 0; sl < nslab; ++sl) {
      const int p0 = sl * (G * PPL);            // first piece of the slab
      uint4 w[U][PPL];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < PPL; ++i) {
          const int p = p0 + l + G * i;
          w[u][i] = nc[u] >= 0 && (!SLAB || p < pieces) ? load_piece_raw<WT>(W, a.ldw, a.w_blocked, nc[u], p)
                                                        : make_uint4(0, 0, 0, 0);
        }
      if (sl == 0) idx(j + NG * U);
      if constexpr (SLAB) {
#pragma unroll
        for (int i = 0; i < PPL; ++i) {
          const int p = p0 + l + G * i;
#pragma unroll
          for (int k = 0; k < E; ++k) hv[i * E + k] = p < pieces ? h_sh[p * E + k] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float d0 = dot[u];
#pragma unroll
        for (int i = 0; i < PPL; ++i) {
          float f[E];
          unpack_piece<WT>(w[u][i], f);
#pragma unroll
          for (int k = 0; k < E; ++k) d0 += hv[i * E + k] * f[k];
        }
        dot[u] = d0;
      }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1)
#pragma unroll
      for (int u = 0; u < U; ++u) dot[u] += __shfl_xor(dot[u], off, G);
    if (l == 0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ju = j + u * NG;
        if (ju >= j1) break;
        float yh = a.aux * (dot[u] + bn[u]);
        if (a.clip) yh = fminf(fmaxf(yh, a.clip_lo), a.clip_hi);
        a.y[lb + ju] = yh;
        if (fc[u]) {
          const float err = yh - tc[u];
          sse += err * err;
          sae += fabsf(err);
          cnt += (tc[u] + yh != 0.f) ? 1.f : 0.f;
        }
      }
    }
  }
  if (!stats) return;
  if (l == 0) {
    st[grp][0] = sse;
    st[grp][1] = sae;
    st[grp][2] = cnt;
    st[grp][3] = 0.f;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float v = 0.f;
    for (int g = 0; g < NG; ++g) v += st[g][threadIdx.x];
    a.chunk_stats[(int64_t)c * 4 + threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(PE_ROW_THREADS) predict_rows_kernel(OcfPredictArgs a) {
  __shared__ float red[PE_ROW_THREADS][4];
  float tot[4] = {0.f, 0.f, 0.f, 0.f};
  for (int b = threadIdx.x; b < a.Bp; b += PE_ROW_THREADS) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (b < a.B) {
      int lo = 0, hi = a.n_chunks;              // the first chunk with ch_row >= b
      while (lo < hi) {
        const int md = (lo + hi) >> 1;
        if (a.ch_row[md] < b) lo = md + 1; else hi = md;
      }
      for (int c = lo; c < a.n_chunks && a.ch_row[c] == b; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += a.chunk_stats[(int64_t)c * 4 + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a.row_stats[(int64_t)b * 4 + k] = v[k];
      tot[k] += v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[threadIdx.x][k] = tot[k];
  __syncthreads();
  for (int off = PE_ROW_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
#pragma unroll
      for (int k = 0; k < 4; ++k) red[threadIdx.x][k] += red[threadIdx.x + off][k];
    __syncthreads();
  }
  if (threadIdx.x < 4) a.total[threadIdx.x] = red[0][threadIdx.x];
}

template <typename WT, int G, int PPL, bool SLAB>
void launch(const OcfPredictArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((predict_entries_kernel<WT, G, PPL, SLAB>), dim3(a.n_chunks), dim3(PE_THREADS), 0, s, a);
}

// the widest group of <= 32 lanes the row's pieces fill (gather_shape's rule); beyond 512 the slab form, whose
// 32 lanes hold 512 elements
template <typename WT>
void launch_by_shape(const OcfPredictArgs& a, hipStream_t s) {
  if constexpr (sizeof(WT) == 4) {
    if (a.H > PE_SLAB) launch<WT, 32, 4, true>(a, s);
    else if (a.H == 128) launch<WT, 32, 1, false>(a, s);
    else if (a.H == 256) launch<WT, 32, 2, false>(a, s);
    else if (a.H == 384) launch<WT, 32, 3, false>(a, s);
    else launch<WT, 32, 4, false>(a, s);
  } else {
    if (a.H > PE_SLAB) launch<WT, 32, 2, true>(a, s);
    else if (a.H == 128) launch<WT, 16, 1, false>(a, s);
    else if (a.H == 256) launch<WT, 32, 1, false>(a, s);
    else if (a.H == 384) launch<WT, 16, 3, false>(a, s);
    else launch<WT, 32, 2, false>(a, s);
  }
}

bool is_dtype(int d) { return d == OCF_F32 || d == OCF_F16 || d == OCF_BF16; }

}  // namespace

extern "C" int ocf_predict_entries(const OcfPredictArgs* args, void* stream) {
  OCF_TRY_BEGIN
  OCF_CHECK(args != nullptr, "ocf_predict_entries: null arguments");
  const OcfPredictArgs& a = *args;
  OCF_CHECK(a.h != nullptr, "ocf_predict_entries: null h");
  OCF_CHECK(a.W != nullptr, "ocf_predict_entries: null W");
  OCF_CHECK(a.bias != nullptr, "ocf_predict_entries: null bias");
  OCF_CHECK(a.y != nullptr, "ocf_predict_entries: null y");
  OCF_CHECK(a.lboff != nullptr, "ocf_predict_entries: null lboff");
  OCF_CHECK(a.H >= 128 && a.H <= PE_MAX_H && a.H % 128 == 0,
            "ocf_predict_entries: H must be a multiple of 128 in [128, 2048]");
  OCF_CHECK(is_dtype(a.h_dtype) && is_dtype(a.w_dtype), "ocf_predict_entries: h_dtype and w_dtype are OCF_DT_*");
  OCF_CHECK(!a.w_blocked || a.w_dtype != OCF_F32,
            "ocf_predict_entries: the blocked flag needs a 16-bit weight (w_dtype f16 / bf16)");
  OCF_CHECK(!a.w_blocked || a.ldw % 64 == 0, "ocf_predict_entries: blocked W needs ldw % 64 == 0");
  OCF_CHECK(a.ldw >= a.H && a.ldw % 8 == 0 && a.ldh >= a.H, "ocf_predict_entries: ldw (a multiple of 8) and ldh must be >= H");
  OCF_CHECK(!a.clip || a.clip_lo <= a.clip_hi, "ocf_predict_entries: clip needs clip_lo <= clip_hi");
  OCF_CHECK(!a.row_stats || (a.val && a.chunk_stats && a.total),
            "ocf_predict_entries: row_stats given without val, chunk_stats or total");
  OCF_CHECK(a.n_chunks >= 0 && a.B >= 0 && a.Bp >= a.B, "ocf_predict_entries: n_chunks >= 0, 0 <= B <= Bp");
  OCF_CHECK(a.n_chunks == 0 || (a.rows && a.rp && a.col && a.ch_row && a.ch_j0 && a.ch_j1),
            "ocf_predict_entries: chunks given without rows, rp, col, ch_row, ch_j0 or ch_j1");
  hipStream_t s = (hipStream_t)stream;
  if (a.n_chunks > 0) {
    if (a.w_dtype == OCF_F32) launch_by_shape<float>(a, s);
    else if (a.w_dtype == OCF_F16) launch_by_shape<_Float16>(a, s);
    else launch_by_shape<__bf16>(a, s);
    OCF_HIP(hipGetLastError());
  }
  if (a.row_stats) {
    hipLaunchKernelGGL(predict_rows_kernel, dim3(1), dim3(PE_ROW_THREADS), 0, s, a);
    OCF_HIP(hipGetLastError());
  }
  OCF_TRY_END
}
