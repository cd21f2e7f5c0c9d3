// ocf_topk: the k best decoder scores of every batch row without a [B][N] score array (ocf.h).
//
// Launch 1, topk_select_kernel: a workgroup owns a 128-row tile and a contiguous run of 128-column tiles.  Per
// tile it runs gemm_kernel's K-loop (same stagers, same MFMA order: every score is bit-identical to
// OCF_EPI_PREDICT's), stages y = acc + b in LDS over the operand buffers, writes -inf at padding and excluded
// columns, and compares the tile against each row's current k-th value: one compare per value (256 threads, a
// row half each, one 64-bit pass mask per thread), then the row's owner thread puts the few that pass into the
// row's list: k unordered slots, the scores in LDS (the owner's working copy) and (score, column) pairs in the
// workspace (stores only).  A value that passes replaces the current minimum and the owner rescans its k LDS
// values for the new one -- k pipelined reads, no moves.  Columns arrive in ascending order, so "strictly greater
// than the k-th" keeps the (descending score, ascending column) order; among equal minima the largest column
// leaves (read back from the workspace, rare).
// Launch 2, topk_merge_kernel: a wave per batch row stages the groups' lists in LDS, drops what lies below the
// largest minimum of a full list (k candidates are at least that good), selects k times the best of the rest and,
// given held-out entries, counts hits / DCG / relevant columns of the final list.
// The transposed call (OcfTopkArgs bias_by_row / h_dtype1 / h_blocked) ranks along the other axis with the same two
// launches: the decoder weight rows as the M operand (fp32 master, row-major or 64x64-blocked shadow), a table of
// hidden codes as the N operand, the bias along M.  It has select variants of its own (TR = true).
#include <algorithm>
#include <climits>
#include <cmath>

#include "ocf_gemm.h"
#include "ocf_internal.h"

using namespace ocf;

namespace {

constexpr int YS = GT_BN + 4;          // LDS row stride (floats) of the staged tile (EpiMaskedMSE's)
constexpr int Y_BYTES = GT_BM * YS * 4;
constexpr int SEL_WGS = 256;           // workgroups the default group count aims for (one per CU)
constexpr int64_t WORK_HEADER = 256;
constexpr int MERGE_LDS_CAND = 128 * 1024;   // the merge stages a row's candidates in LDS up to this many bytes

struct SelParams {
  const void* h; int64_t ldh;
  const void* W; int64_t ldw; int w_blk;
  const float* bias;
  int N, K, m_real, n_real, k, groups, n_tiles, ks;
  const int32_t* ex_rows; const int64_t* ex_rp; const int32_t* ex_tptr; const int32_t* ex_col; int ex_ntiles;
  const float* ex_mask; int64_t ld_ex; const int64_t* ex_mrows;
  uint2* cand;              // [M][groups][k]: (score bits, column), unordered; (-inf, -1) = empty
  int h_blk, bias_m;        // TR variants only: h stored 64x64-blocked; bias indexed by M row
};

// LDS row stride (floats) of the per-row score lists: k rounded up to 16 plus one 16-B slot (an odd number of
// slots: the owners' ds_read_b128 hit distinct banks)
inline int list_stride(int k) { return ((k + 15) & ~15) + 4; }

__host__ __device__ __forceinline__ uint2 none_entry() { return make_uint2(0xFF800000u, 0xFFFFFFFFu); }   // (-inf, -1)

// AGT: the M operand's element type in memory (CT, or float = the fp32 master rounded while staging, as WGT is
// on the N side).  TR: the transposed call's variants -- the M operand may be 64x64-blocked (p.h_blk) and the bias
// may run along M (p.bias_m; the tile's 128 values sit in LDS behind the lists).  With AGT = CT and TR = false
// every line below compiles to what it was before these parameters existed.
template <typename CT, typename WGT, typename AGT = CT, bool TR = false>
__global__ void __launch_bounds__(GT_THREADS) topk_select_kernel(SelParams p) {
  using Cfg = GemmCfg<CT, false, false, CT, WGT>;
  constexpr int BK = Cfg::BK;
  static_assert(Cfg::OPER_LDS >= Y_BYTES, "the staged tile overlays the operand buffers");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* Y = reinterpret_cast<float*>(lds);
  float* thr = reinterpret_cast<float*>(lds + Cfg::OPER_LDS);                   // [128] k-th value (-inf: list not full)
  unsigned long long* pm = reinterpret_cast<unsigned long long*>(lds + Cfg::OPER_LDS + GT_BM * 8);   // [256]
  float* lists = reinterpret_cast<float*>(lds + Cfg::OPER_LDS + GT_BM * 8 + GT_THREADS * 8);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile_m = blockIdx.x / p.groups, g = blockIdx.x % p.groups;
  const int t0 = (int)((int64_t)g * p.n_tiles / p.groups), t1 = (int)((int64_t)(g + 1) * p.n_tiles / p.groups);
  const int m0 = tile_m * GT_BM;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int ml = tid & (GT_BM - 1), half = tid >> 7;
  const int k = p.k;
  const float NEG_INF = -INFINITY;

  uint2* G = p.cand + ((int64_t)(m0 + ml) * p.groups + g) * k;      // this row's candidate list of the group
  float* V = lists + ml * p.ks;                                     // its scores (owner thread only)
  const int kp = (k + 15) & ~15;
  float th = NEG_INF;       // owner thread: the list's minimum once it is full, its slot, the entries held
  int mslot = 0, c = 0;
  if (tid < GT_BM) {
    thr[tid] = NEG_INF;
    for (int j = k; j < kp; ++j) V[j] = INFINITY;                   // padding up to 16 values: never the minimum
  }
  // the new minimum of a full list; among equal minima the largest column (the last in the order) leaves
  auto rescan = [&]() {
    float mv = INFINITY;
    int ms = 0, ties = 0;
    for (int j = 0; j < kp; j += 16) {       // 16 values per round: four reads in flight, then the compares
      float x[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 t4 = *reinterpret_cast<const float4*>(V + j + 4 * q);
        x[4 * q] = t4.x; x[4 * q + 1] = t4.y; x[4 * q + 2] = t4.z; x[4 * q + 3] = t4.w;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const bool lt = x[u] < mv;
        ties = lt ? 1 : ties + (x[u] == mv ? 1 : 0);
        ms = lt ? j + u : ms;
        mv = lt ? x[u] : mv;
      }
    }
    if (ties > 1) {
      int bc = -1;
      for (int j = 0; j < k; ++j)
        if (V[j] == mv) {
          const int cj = (int)G[j].y;
          if (cj > bc) { bc = cj; ms = j; }
        }
    }
    th = mv;
    mslot = ms;
  };

  const AGT* Ag = reinterpret_cast<const AGT*>(p.h);
  const WGT* Bg = reinterpret_cast<const WGT*>(p.W);
  const bool bblk = sizeof(WGT) == 2 && p.w_blk;
  const bool ablk = TR && sizeof(AGT) == 2 && p.h_blk;
  const __amdgpu_buffer_rsrc_t ra =
      ablk ? tile_rsrc(reinterpret_cast<const char*>(Ag) + Stager<AGT, CT, GT_BM, false>::blocked_origin(p.ldh, m0, 0))
           : tile_rsrc(Ag + (int64_t)m0 * p.ldh);
  const bool bias_m = TR && p.bias_m;
  float* brow = lists + GT_BM * p.ks;                               // [128] the tile's biases (TR, bias by M row)
  if constexpr (TR) {
    if (tid < GT_BM) brow[tid] = bias_m ? p.bias[m0 + tid] : 0.f;   // read from step 1 on, after the K-loop's barriers
  }
  const int nk = p.K / BK;
  char* buf0 = lds;
  char* buf1 = lds + Cfg::BUF;

  for (int t = t0; t < t1; ++t) {
    const int n0 = t * GT_BN;
    const __amdgpu_buffer_rsrc_t rb =
        bblk ? tile_rsrc(reinterpret_cast<const char*>(Bg) + Stager<WGT, CT, GT_BN, false>::blocked_origin(p.ldw, n0, 0))
             : tile_rsrc(Bg + (int64_t)n0 * p.ldw);
    // ---- gemm_kernel's K-loop (one split, A [M][K] x B [N][K])
    ocf_f16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    {
      Stager<AGT, CT, GT_BM, false> sa;
      Stager<WGT, CT, GT_BN, false> sb;
      const uint32_t sta = decltype(sa)::step_bytes(p.ldh, ablk), stb = decltype(sb)::step_bytes(p.ldw, bblk);
      sa.load(ra, p.ldh, 0, tid, false, ablk);
      sb.load(rb, p.ldw, 0, tid, false, bblk);
      sa.store(buf0, tid);
      sb.store(buf0 + Cfg::ImgA::BYTES, tid);
      __syncthreads();
      for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) {
          sa.load(ra, p.ldh, (kt + 1) * sta, tid, false, ablk);
          sb.load(rb, p.ldw, (kt + 1) * stb, tid, false, bblk);
        }
        const char* cb = (kt & 1) ? buf1 : buf0;
        mfma_kstep<CT, false, false>(cb, cb + Cfg::ImgA::BYTES, wm, wn, lane, acc);
        if (more) {
          char* nb = ((kt + 1) & 1) ? buf1 : buf0;
          sa.store(nb, tid);
          sb.store(nb + Cfg::ImgA::BYTES, tid);
        }
        __syncthreads();
      }
    }
    // ---- 1. stage y = acc + b; padding columns are not eligible
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const int n = n0 + wn + acc_col(bj, lane);
      const bool pad = n >= p.n_real;
      if constexpr (TR) {
        const float bias_n = bias_m ? 0.f : p.bias[n];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = wm + acc_row(bi, r, lane);
            Y[row * YS + wn + acc_col(bj, lane)] = pad ? NEG_INF : acc[bi][bj][r] + (bias_m ? brow[row] : bias_n);
          }
      } else {
        const float bias = p.bias[n];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            Y[(wm + acc_row(bi, r, lane)) * YS + wn + acc_col(bj, lane)] = pad ? NEG_INF : acc[bi][bj][r] + bias;
      }
    }
    __syncthreads();
    // ---- 2. exclusions of this tile
    if (p.ex_rows) {
      // thread tid: half (tid >> 7) of row (tid & 127)'s entries in this column tile
      const int b = m0 + ml;
      const int r = b < p.m_real ? p.ex_rows[b] : -1;
      if (r >= 0) {
        const int64_t base = p.ex_rp[r];
        const int32_t* tp = p.ex_tptr + (int64_t)r * (p.ex_ntiles + 1) + t;
        const int64_t lo = base + tp[0], hi = base + tp[1];
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        for (int64_t e = half ? mid : lo; e < (half ? hi : mid); ++e) Y[ml * YS + (p.ex_col[e] & (GT_BN - 1))] = NEG_INF;
      }
    } else if (p.ex_mask) {
      for (int i = tid; i < GT_BM * GT_BN; i += GT_THREADS) {
        const int rl = i >> 7, nl = i & (GT_BN - 1);
        const int b = m0 + rl, n = n0 + nl;
        if (b < p.m_real && n < p.n_real) {
          const int64_t row = p.ex_mrows ? p.ex_mrows[b] : (int64_t)b;
          if (p.ex_mask[row * p.ld_ex + n] != 0.f) Y[rl * YS + nl] = NEG_INF;
        }
      }
    }
    __syncthreads();
    // ---- 3. compare the row half against the row's k-th value
    {
      const float th = thr[ml];
      const float* yr = Y + ml * YS + half * (GT_BN / 2);
      unsigned long long mask = 0ull;
#pragma unroll
      for (int j4 = 0; j4 < GT_BN / 8; ++j4) {
        const float4 v = *reinterpret_cast<const float4*>(yr + 4 * j4);
        mask |= (unsigned long long)(v.x > th) << (4 * j4);
        mask |= (unsigned long long)(v.y > th) << (4 * j4 + 1);
        mask |= (unsigned long long)(v.z > th) << (4 * j4 + 2);
        mask |= (unsigned long long)(v.w > th) << (4 * j4 + 3);
      }
      pm[half * GT_BM + ml] = mask;
    }
    __syncthreads();
    // ---- 4. the row's owner takes what passed, in ascending column order
    if (tid < GT_BM) {
      for (int hf = 0; hf < 2; ++hf) {
        unsigned long long mask = pm[hf * GT_BM + ml];
        while (mask) {
          const int j = __builtin_ctzll(mask);
          mask &= mask - 1;
          const int nl = hf * (GT_BN / 2) + j;
          const float v = Y[ml * YS + nl];
          if (!(v > th)) continue;
          const int slot = c < k ? c : mslot;       // a free slot, or the minimum's
          V[slot] = v;
          G[slot] = make_uint2(__float_as_uint(v), (uint32_t)(n0 + nl));
          if (c < k) ++c;
          if (c == k) rescan();
        }
      }
      thr[ml] = th;
    }
    __syncthreads();
  }
  // ---- the slots never filled
  if (tid < GT_BM)
    for (int j = c; j < k; ++j) G[j] = none_entry();
}

struct MergeParams {
  uint2* cand;
  int k, groups, cand_lds;
  int32_t* out_idx; float* out_val; int64_t ld_out;
  const int32_t* rel_rows; const int64_t* rel_rp; const int32_t* rel_col; const float* rel_val;
  float rel_min;
  float* row_rank;
};

__device__ __forceinline__ bool beats(float v, int c, float v2, int c2) { return v > v2 || (v == v2 && c < c2); }

__global__ void __launch_bounds__(64) topk_merge_kernel(MergeParams p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint2* outl = reinterpret_cast<uint2*>(lds);                         // [128] the final list
  int* relf = reinterpret_cast<int*>(lds + OCF_TOPK_MAX_K * 8);        // [128] list position holds a relevant column
  uint2* cl = reinterpret_cast<uint2*>(lds + OCF_TOPK_MAX_K * 12);
  const int m = blockIdx.x, lane = threadIdx.x;
  const int k = p.k, C = p.groups * k;
  uint2* src = p.cand + (int64_t)m * C;      // the row's candidates, unordered; lane l owns entries l, l + 64, ...
  if (p.cand_lds) {
    for (int i = lane; i < C; i += 64) cl[i] = src[i];
    src = cl;
  }
  __syncthreads();
  // 1. a lower bound of the k-th best score: the largest minimum of a full group list (k entries are >= it)
  float lb = -INFINITY;
  for (int g = lane; g < p.groups; g += 64) {
    const uint2* gl = src + g * k;
    float mn = INFINITY;
    bool full = true;
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
      const uint2 e = gl[j];
      full &= (int)e.y >= 0;
      mn = fminf(mn, __uint_as_float(e.x));
    }
    if (full) lb = fmaxf(lb, mn);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lb = fmaxf(lb, __shfl_xor(lb, off));
  // 2. keep what can still make the list: compacted in place, in order (a round reads its 64 entries before it
  //    writes, and writes at or below where it read)
  int n = 0;
  for (int base = 0; base < C; base += 64) {
    const int i = base + lane;
    uint2 e = none_entry();
    if (i < C) e = src[i];
    const bool keep = (int)e.y >= 0 && __uint_as_float(e.x) >= lb;
    const unsigned long long bal = __ballot(keep);
    const int pos = n + __popcll(bal & ((1ull << lane) - 1ull));
    if (keep) src[pos] = e;
    n += __popcll(bal);
  }
  __syncthreads();
  // 3. k times the best of what is left; lane l owns entries l, l + 64, ... and marks the one it gave
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY;
    int bc = INT_MAX, bi = -1;
#pragma unroll 4
    for (int i = lane; i < n; i += 64) {
      const uint2 e = src[i];
      const int c = (int)e.y;
      const float v = __uint_as_float(e.x);
      const bool better = c >= 0 && (bi < 0 || beats(v, c, bv, bc));
      bv = better ? v : bv;
      bc = better ? c : bc;
      bi = better ? i : bi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oc = __shfl_xor(bc, off), oi = __shfl_xor(bi, off);
      if (oi >= 0 && (bi < 0 || beats(ov, oc, bv, bc))) { bv = ov; bc = oc; bi = oi; }
    }
    if (lane == 0) outl[j] = bi < 0 ? none_entry() : make_uint2(__float_as_uint(bv), (uint32_t)bc);
    if (bi >= 0 && (bi & 63) == lane) src[bi].y = 0xFFFFFFFFu;
  }
  __syncthreads();
  for (int j = lane; j < k; j += 64) {
    const uint2 e = outl[j];
    p.out_val[(int64_t)m * p.ld_out + j] = __uint_as_float(e.x);
    p.out_idx[(int64_t)m * p.ld_out + j] = (int32_t)e.y;
  }
  if (!p.rel_rows) return;
  // ---- hits / DCG of the list and the row's relevant columns
  const int r = p.rel_rows[m];
  const int64_t lo = r >= 0 ? p.rel_rp[r] : 0, hi = r >= 0 ? p.rel_rp[r + 1] : 0;
  for (int j = lane; j < k; j += 64) {
    const int c = (int)outl[j].y;
    int f = 0;
    if (c >= 0) {
      int64_t a = lo, b = hi;
      while (a < b) {
        const int64_t md = (a + b) >> 1;
        if (p.rel_col[md] < c) a = md + 1; else b = md;
      }
      for (; a < hi && p.rel_col[a] == c; ++a) f |= p.rel_val[a] >= p.rel_min ? 1 : 0;
    }
    relf[j] = f;
  }
  int nrel = 0;
  for (int64_t e = lo + lane; e < hi; e += 64) {
    if (!(p.rel_val[e] >= p.rel_min)) continue;
    bool first = true;       // a column counts once: at its first relevant entry
    for (int64_t d = e - 1; d >= lo && p.rel_col[d] == p.rel_col[e]; --d)
      if (p.rel_val[d] >= p.rel_min) { first = false; break; }
    nrel += first ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nrel += __shfl_xor(nrel, off);
  __syncthreads();
  if (lane == 0) {
    int hits = 0;
    double dcg = 0.0;
    for (int j = 0; j < k; ++j)
      if (relf[j]) { ++hits; dcg += 1.0 / log2((double)(j + 2)); }
    float* rr = p.row_rank + (int64_t)m * 4;
    rr[0] = (float)hits; rr[1] = (float)dcg; rr[2] = (float)nrel; rr[3] = 0.f;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------
int groups_of(const OcfTopkArgs& a) {
  const int n_tiles = a.N / GT_BN, gm = a.M / GT_BM;
  int g = a.groups > 0 ? a.groups : std::max(1, SEL_WGS / gm);
  return std::min(g, n_tiles);
}

// everything that can be judged without the workspace or a device
void check_shape(const OcfTopkArgs& a) {
  OCF_CHECK(a.k >= 1 && a.k <= OCF_TOPK_MAX_K, "ocf_topk: k must be in 1 .. OCF_TOPK_MAX_K (128)");
  OCF_CHECK(a.M > 0 && a.N > 0 && a.K > 0 && a.M % GT_BM == 0 && a.N % GT_BN == 0 && a.K % 128 == 0,
            "ocf_topk: M, N and K must be padded to multiples of 128");
  OCF_CHECK(a.n_real >= 0 && a.n_real <= a.N, "ocf_topk: n_real > N");
  OCF_CHECK(a.m_real >= 0 && a.m_real <= a.M, "ocf_topk: m_real > M");
  OCF_CHECK(a.groups >= 0, "ocf_topk: groups >= 0 (0 = the library's choice)");
}

template <typename CT, typename WGT, typename AGT = CT, bool TR = false>
void launch_select(const SelParams& p, int gm, hipStream_t s) {
  using Cfg = GemmCfg<CT, false, false, CT, WGT>;
  const int lds = Cfg::OPER_LDS + GT_BM * 8 + GT_THREADS * 8 + GT_BM * p.ks * 4 + (TR ? GT_BM * 4 : 0);
  OCF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&topk_select_kernel<CT, WGT, AGT, TR>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL((topk_select_kernel<CT, WGT, AGT, TR>), dim3(gm * p.groups), dim3(GT_THREADS), lds, s, p);
  OCF_HIP(hipGetLastError());
}

// the transposed call's variants: the N side as before, the M side in the compute dtype or fp32
template <typename CT>
void launch_select_tr(const SelParams& p, int gm, bool w32, bool h32, hipStream_t s) {
  if (w32) {
    if (h32) launch_select<CT, float, float, true>(p, gm, s); else launch_select<CT, float, CT, true>(p, gm, s);
  } else {
    if (h32) launch_select<CT, CT, float, true>(p, gm, s); else launch_select<CT, CT, CT, true>(p, gm, s);
  }
}

}  // namespace

extern "C" int64_t ocf_topk_workspace(const OcfTopkArgs* a) {
  try {
    OCF_CHECK(a != nullptr, "ocf_topk_workspace: null arguments");
    check_shape(*a);
    return WORK_HEADER + (int64_t)a->M * groups_of(*a) * a->k * 8;
  } catch (const std::exception& e) {
    set_error(e.what());
    return -1;
  }
}

extern "C" int ocf_topk(const OcfTopkArgs* args, void* stream) {
  OCF_TRY_BEGIN
  OCF_CHECK(args != nullptr, "ocf_topk: null arguments");
  const OcfTopkArgs& a = *args;
  check_shape(a);
  OCF_CHECK(a.ld_out >= a.k, "ocf_topk: ld_out < k");
  OCF_CHECK(!a.bias_by_row || a.bias, "ocf_topk: bias_by_row needs a bias of M values (null bias)");
  OCF_CHECK(a.h && a.W && a.bias && a.out_idx && a.out_val, "ocf_topk: null h, W, bias, out_idx or out_val");
  OCF_CHECK(!(a.ex_rows && a.ex_mask), "ocf_topk: both exclusion forms given (row-segment and dense)");
  OCF_CHECK(!a.ex_rows || (a.ex_rp && a.ex_tptr && a.ex_col && a.ex_ntiles * GT_BN >= a.N),
            "ocf_topk: row-segment exclusion needs ex_rp, ex_tptr, ex_col and ex_ntiles * 128 >= N");
  OCF_CHECK(!a.ex_mask || a.ld_ex >= a.n_real, "ocf_topk: dense exclusion needs ld_ex >= n_real");
  OCF_CHECK(a.compute_dtype == OCF_F32 || a.compute_dtype == OCF_F16 || a.compute_dtype == OCF_BF16,
            "ocf_topk: bad compute dtype");
  OCF_CHECK(a.w_dtype == OCF_F32 || a.w_dtype == a.compute_dtype, "ocf_topk: W must be fp32 or the compute dtype");
  OCF_CHECK(!a.w_blocked || a.w_dtype != OCF_F32, "ocf_topk: the blocked flag needs a 16-bit weight (w_dtype f16 / bf16)");
  OCF_CHECK(!a.w_blocked || a.ldw % 64 == 0, "ocf_topk: blocked W needs ldw % 64 == 0");
  OCF_CHECK(a.h_dtype1 == 0 || a.h_dtype1 == OCF_F32 + 1 || a.h_dtype1 == a.compute_dtype + 1,
            "ocf_topk: h must be fp32 or the compute dtype (h_dtype1 = 0, or OCF_DT_* + 1)");
  const bool h32 = a.h_dtype1 ? a.h_dtype1 == OCF_F32 + 1 : a.compute_dtype == OCF_F32;
  OCF_CHECK(!a.h_blocked || !h32, "ocf_topk: a blocked h needs a 16-bit operand (h in fp32 is row-major)");
  OCF_CHECK(!a.h_blocked || a.ldh % 64 == 0, "ocf_topk: blocked h needs ldh % 64 == 0");
  OCF_CHECK(a.ldh % 8 == 0 && a.ldw % 8 == 0 && a.ldh >= a.K && a.ldw >= a.K,
            "ocf_topk: ldh and ldw must be multiples of 8 and >= K");
  OCF_CHECK(!a.rel_rows || a.row_rank, "ocf_topk: relevance given without row_rank");
  OCF_CHECK(!a.rel_rows || (a.rel_rp && a.rel_col && a.rel_val), "ocf_topk: relevance needs rel_rp, rel_col and rel_val");
  const int64_t need = ocf_topk_workspace(&a);
  OCF_CHECK(a.work && a.work_bytes >= need, "ocf_topk: work_bytes too small (ocf_topk_workspace)");
  if (a.m_real == 0) return 0;
  hipStream_t s = (hipStream_t)stream;

  SelParams p;
  p.h = a.h; p.ldh = a.ldh; p.W = a.W; p.ldw = a.ldw; p.w_blk = a.w_blocked != 0; p.bias = a.bias;
  p.N = a.N; p.K = a.K; p.m_real = a.m_real; p.n_real = a.n_real; p.k = a.k;
  p.groups = groups_of(a); p.n_tiles = a.N / GT_BN; p.ks = list_stride(a.k);
  p.ex_rows = a.ex_rows; p.ex_rp = a.ex_rp; p.ex_tptr = a.ex_tptr; p.ex_col = a.ex_col; p.ex_ntiles = a.ex_ntiles;
  p.ex_mask = a.ex_mask; p.ld_ex = a.ld_ex; p.ex_mrows = a.ex_mrows;
  p.cand = reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.work) + WORK_HEADER);
  p.h_blk = a.h_blocked != 0; p.bias_m = a.bias_by_row != 0;
  const int gm = a.M / GT_BM;
  const bool w32 = a.w_dtype == OCF_F32;
  if (a.bias_by_row || a.h_dtype1 || a.h_blocked) {      // any new field set: the transposed call's variants
    switch (a.compute_dtype) {
      case OCF_F16: launch_select_tr<_Float16>(p, gm, w32, h32, s); break;
      case OCF_BF16: launch_select_tr<__bf16>(p, gm, w32, h32, s); break;
      default: launch_select<float, float, float, true>(p, gm, s);
    }
  } else switch (a.compute_dtype) {
    case OCF_F16:
      if (w32) launch_select<_Float16, float>(p, gm, s); else launch_select<_Float16, _Float16>(p, gm, s);
      break;
    case OCF_BF16:
      if (w32) launch_select<__bf16, float>(p, gm, s); else launch_select<__bf16, __bf16>(p, gm, s);
      break;
    default:
      launch_select<float, float>(p, gm, s);
  }

  MergeParams q;
  q.cand = p.cand; q.k = a.k; q.groups = p.groups;
  const int64_t cbytes = (int64_t)p.groups * a.k * 8;
  q.cand_lds = cbytes <= MERGE_LDS_CAND;
  q.out_idx = a.out_idx; q.out_val = a.out_val; q.ld_out = a.ld_out;
  q.rel_rows = a.rel_rows; q.rel_rp = a.rel_rp; q.rel_col = a.rel_col; q.rel_val = a.rel_val; q.rel_min = a.rel_min;
  q.row_rank = a.row_rank;
  const int mlds = OCF_TOPK_MAX_K * 12 + (q.cand_lds ? (int)cbytes : 0);
  OCF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&topk_merge_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, mlds));
  hipLaunchKernelGGL(topk_merge_kernel, dim3(a.m_real), dim3(64), mlds, s, q);
  OCF_HIP(hipGetLastError());
  OCF_TRY_END
}
