// ocf_mlp_step (ocf.h): a small dense model's whole training step in one persistent launch.
//
// The dense path's step (split-K encoder, hidden-layer GEMMs, the masked-MSE decoder, the backward GEMMs
// with the fused optimizer, bias kernels, stats) is ~14 launches of 2-33 us on a model of 0.14 M
// parameters (train_jester.py's 200 -> 256 -> 256 -> 100, batch 128): every launch is a handful of
// workgroups waiting on latency, and the host spends longer issuing them than the GPU running them.
// Here a grid of up to 128 workgroups stays resident and walks the step's phases, each a set of 32 x 32
// output tiles (one per workgroup, the reduction dimension split over its four waves, MFMA from LDS;
// operands from the L2 / MALL-resident weights and activations), separated by grid barriers:
//   F_0 .. F_{L-1}  h_i = act(h_{i-1} W_i + b_i)                     (model.py:64-71)
//   OUT             y = M * (h_{L-1} W_L + b_L), e = y - T, delta_L = e * M, the step's statistics, the
//                   column sums of delta_L (model.py:81-86, train.py:49, 102-121)
//   BACK_L          stats; b_L's update; delta_{L-1} = (delta_L W_L^T) * act' (+ column sums); dW_L -> scratch
//   BACK_i          W_{i+1} updated from its scratch gradient (nothing reads it any more); b_i's update;
//                   delta_{i-1}; dW_i -> scratch
//   BACK_0          W_1 updated; b_0's update; dW_0 tiles update W_0 directly
// (Keras computes every gradient from the weights before the step, train.py:50-51: a layer's weights
// change only after the phase that last reads them.)  Gradients are carried unscaled (e * M) and the
// MSE's 2 / (B N) applied in fp32 at the update, as on the other paths.
#include "ocf_mlp_kernel.h"

namespace ocf {
namespace mlp {

struct Layout {
  size_t h[MAXL], d[MAXL + 1], g[MAXL], colp[MAXL + 1], am[MAXL], dm[MAXL], rowp, totp, rhop, total;
};
Layout layout(const OcfMlpStepArgs& a, int* dim) {
  Layout w{};
  size_t off = 0;
  auto take = [&](size_t floats) {
    const size_t o = off;
    off += (floats * 4 + 255) / 256 * 256;
    return o;
  };
  const int L = a.n_hidden;
  for (int i = 0; i < L; ++i) w.h[i] = take((size_t)a.Bp * dim[i + 1]);
  for (int i = 0; i <= L; ++i) w.d[i] = take((size_t)a.Bp * dim[i + 1]);
  for (int i = 1; i <= L; ++i) w.g[i] = take((size_t)dim[i] * dim[i + 1]);
  for (int i = 0; i <= L; ++i) w.colp[i] = take((size_t)(a.Bp / TT) * dim[i + 1]);
  for (int i = 0; i < L; ++i) {
    const size_t n = a.keep < 1.f ? (size_t)a.Bp * dim[i + 1] : 0;
    w.am[i] = take(n);
    w.dm[i] = take(n);
  }
  w.rowp = take((size_t)(a.Np / TT) * a.Bp);
  w.totp = take((size_t)(a.Bp / TT) * (a.Np / TT) * WAVES * 3);
  w.rhop = take((size_t)(a.Bp / TT) * (a.Np / TT) * WAVES);
  w.total = off;
  return w;
}

void dims_of(const OcfMlpStepArgs& a, int* dim, int* real) {
  const int L = a.n_hidden;
  dim[0] = a.k_blocks * a.Np;
  real[0] = a.k_blocks * a.N;
  for (int i = 0; i < L; ++i) {
    dim[i + 1] = a.hidden_p[i];
    real[i + 1] = a.hidden[i];
  }
  dim[L + 1] = a.Np;
  real[L + 1] = a.N;
}

void check(const OcfMlpStepArgs& a) {
  OCF_CHECK(a.n_hidden >= 1 && a.n_hidden <= OCF_MAX_HIDDEN, "ocf_mlp_step: n_hidden 1..OCF_MAX_HIDDEN");
  OCF_CHECK(a.Bp % 64 == 0 && a.Bp >= 64 && a.Bp <= 512 && a.B >= 1 && a.B <= a.Bp, "ocf_mlp_step: B <= Bp, Bp % 64 == 0, <= 512");
  OCF_CHECK(a.N >= 1 && a.Np % 64 == 0 && a.N <= a.Np, "ocf_mlp_step: N <= Np, Np % 64 == 0");
  OCF_CHECK(a.k_blocks >= 1 && a.k_blocks <= 3, "ocf_mlp_step: k_blocks 1..3");
  for (int i = 0; i < a.n_hidden; ++i)
    OCF_CHECK(a.hidden_p[i] % 64 == 0 && a.hidden[i] >= 1 && a.hidden[i] <= a.hidden_p[i],
              "ocf_mlp_step: hidden widths padded to multiples of 64");
  for (int j = 0; j < a.k_blocks; ++j) OCF_CHECK(a.x[j] != nullptr, "ocf_mlp_step: null input block");
  OCF_CHECK(a.rows && a.out_mask && a.targets && a.ld_x >= a.N && a.ld_t >= a.N, "ocf_mlp_step: batch arrays");
  OCF_CHECK(a.keep > 0.f && a.keep <= 1.f, "ocf_mlp_step: keep in (0, 1]");
  if (a.keep < 1.f)
    for (int i = 0; i < a.n_hidden; ++i) OCF_CHECK(a.mask[i] != nullptr, "ocf_mlp_step: dropout masks");
  for (int i = 0; i <= a.n_hidden; ++i) OCF_CHECK(a.W[i] && a.b[i], "ocf_mlp_step: null parameter");
  OCF_CHECK(a.opt.l2 == 0.f, "ocf_mlp_step: l2 must be 0 (the regulariser is not fused)");
  const int slots = opt_slots(a.opt.kind);
  OCF_CHECK(slots >= 0, "ocf_mlp_step: unknown optimizer kind (OCF_OPTK_* 0..5)");
  if (slots)
    for (int i = 0; i <= a.n_hidden; ++i)
      OCF_CHECK(a.sW1[i] && a.sb1[i] && (slots != 2 || (a.sW2[i] && a.sb2[i])), "ocf_mlp_step: optimizer slots");
  OCF_CHECK(a.stats && a.work && a.barrier, "ocf_mlp_step: stats / work / barrier");
  check_loss(a.loss, a.loss_param, "ocf_mlp_step");
}

template <typename CT, int LOSS>
void launch_loss(const OcfMlpStepArgs& a, const P& p, int wgs, hipStream_t s) {
  switch (a.opt.kind) {
    case OCF_OPT_ADAGRAD: hipLaunchKernelGGL((mlp_step_kernel<CT, OCF_OPT_ADAGRAD, LOSS>), dim3(wgs), dim3(THREADS), 0, s, p); break;
    case OCF_OPT_RMSPROP: hipLaunchKernelGGL((mlp_step_kernel<CT, OCF_OPT_RMSPROP, LOSS>), dim3(wgs), dim3(THREADS), 0, s, p); break;
    case OCF_OPT_ADAM: hipLaunchKernelGGL((mlp_step_kernel<CT, OCF_OPT_ADAM, LOSS>), dim3(wgs), dim3(THREADS), 0, s, p); break;
    case OCF_OPT_ADADELTA:
    case OCF_OPT_ADAMAX: launch_loss_x<CT, LOSS>(a.opt.kind, p, wgs, s); break;
    case OCF_OPT_SGD: hipLaunchKernelGGL((mlp_step_kernel<CT, OCF_OPT_SGD, LOSS>), dim3(wgs), dim3(THREADS), 0, s, p); break;
    default: throw std::runtime_error("ocf_mlp_step: unknown optimizer kind");
  }
  OCF_HIP(hipGetLastError());
}
template <typename CT>
void launch(const OcfMlpStepArgs& a, const P& p, int wgs, hipStream_t s) {
  OCF_LOSS_SWITCH(a.loss, (launch_loss<CT, LK>(a, p, wgs, s)));
}

}  // namespace mlp
}  // namespace ocf

using namespace ocf;

namespace ocf {
int g_mlp_max_polls = 1 << 22;   // ocf_mlp_step's bounded barrier wait (ocf_set_tuning "mlp_max_polls"; < 0: fault injection)
}

extern "C" int64_t ocf_mlp_step_workspace(const OcfMlpStepArgs* a) {
  try {
    OCF_CHECK(a != nullptr, "ocf_mlp_step_workspace: null arguments");
    int dim[mlp::MAXL + 1], real[mlp::MAXL + 1];
    OCF_CHECK(a->n_hidden >= 1 && a->n_hidden <= OCF_MAX_HIDDEN, "ocf_mlp_step: n_hidden 1..OCF_MAX_HIDDEN");
    mlp::dims_of(*a, dim, real);
    return (int64_t)mlp::layout(*a, dim).total;
  } catch (const std::exception& e) {
    set_error(e.what());
    return -1;
  }
}

extern "C" int ocf_mlp_step(const OcfMlpStepArgs* a, void* stream) {
  OCF_TRY_BEGIN
  OCF_CHECK(a != nullptr, "ocf_mlp_step: null arguments");
  mlp::check(*a);
  mlp::P p{};
  p.L = a->n_hidden; p.B = a->B; p.Bp = a->Bp; p.N = a->N; p.Np = a->Np; p.k = a->k_blocks; p.act = a->act;
  mlp::dims_of(*a, p.dim, p.real);
  const mlp::Layout w = mlp::layout(*a, p.dim);
  OCF_CHECK(a->work_bytes >= (int64_t)w.total, "ocf_mlp_step: workspace too small");
  char* ws = reinterpret_cast<char*>(a->work);
  for (int i = 0; i < p.L; ++i) p.h[i] = reinterpret_cast<float*>(ws + w.h[i]);
  for (int i = 0; i <= p.L; ++i) p.d[i] = reinterpret_cast<float*>(ws + w.d[i]);
  for (int i = 1; i <= p.L; ++i) p.g[i] = reinterpret_cast<float*>(ws + w.g[i]);
  for (int i = 0; i <= p.L; ++i) p.colp[i] = reinterpret_cast<float*>(ws + w.colp[i]);
  for (int i = 0; i < p.L; ++i) {
    p.am[i] = reinterpret_cast<float*>(ws + w.am[i]);
    p.dm[i] = reinterpret_cast<float*>(ws + w.dm[i]);
    p.mask[i] = a->mask[i];
  }
  p.keep = a->keep; p.seed = a->seed; p.stream = a->stream;
  p.rowp = reinterpret_cast<float*>(ws + w.rowp);
  p.totp = reinterpret_cast<float*>(ws + w.totp);
  p.rhop = reinterpret_cast<float*>(ws + w.rhop);
  p.loss_param = a->loss_param;
  for (int j = 0; j < 3; ++j) p.x[j] = a->x[j];
  p.ld_x = a->ld_x; p.rows = a->rows; p.om = a->out_mask; p.tg = a->targets; p.ld_t = a->ld_t;
  for (int i = 0; i <= p.L; ++i) {
    p.W[i] = a->W[i]; p.b[i] = a->b[i]; p.sW1[i] = a->sW1[i]; p.sW2[i] = a->sW2[i]; p.sb1[i] = a->sb1[i];
    p.sb2[i] = a->sb2[i]; p.sh[i] = a->shadow[i];
  }
  p.sh_blk = a->shadow_blocked;
  p.op = a->opt;
  p.stats = a->stats;
  p.bar = a->barrier;
  p.err = async_error_word();
  p.max_polls = g_mlp_max_polls;
  p.trace = a->trace;
  // every workgroup must be resident for the grid barriers; by default one per 32 x 32 tile of the busiest
  // phase, at most 128 (the barriers' arrivals grow with the grid) -- or one per CU (at most 256) when a phase
  // has more than 256 tiles (the wide output layers of the I-AutoRec models on the opt-in generator path)
  int tiles = 0;
  {
    const int bt = p.Bp / mlp::TT;
    for (int i = 0; i <= p.L; ++i) tiles = std::max(tiles, bt * (p.dim[i + 1] / mlp::TT));
    for (int i = p.L; i >= 0; --i)
      tiles = std::max(tiles, (i > 0 ? bt * (p.dim[i] / mlp::TT) : 0) + (p.dim[i] / mlp::TT) * (p.dim[i + 1] / mlp::TT));
  }
  int cus = 0, dev = 0;
  OCF_HIP(hipGetDevice(&dev));
  OCF_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  // (the default never exceeds the CU count: a partitioned device may have fewer CUs than tiles)
  int wgs = tiles > 256 ? std::min(cus, 256) : std::min({tiles, 128, cus});
  if (a->wgs > 0) {
    OCF_CHECK(a->wgs <= cus, "ocf_mlp_step: wgs must not exceed the CU count (grid barriers)");
    wgs = a->wgs;
  }
  hipStream_t s = (hipStream_t)stream;
  switch (a->compute_dtype) {
    case OCF_F16: mlp::launch<_Float16>(*a, p, wgs, s); break;
    case OCF_BF16: mlp::launch<__bf16>(*a, p, wgs, s); break;
    case OCF_F32: mlp::launch<float>(*a, p, wgs, s); break;
    default: throw std::runtime_error("ocf_mlp_step: bad compute dtype");
  }
  OCF_TRY_END
}
