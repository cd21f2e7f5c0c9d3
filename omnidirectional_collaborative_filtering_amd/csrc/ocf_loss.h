// The training losses (ocf.h OCF_LOSS_*): rho and rho' of the residual e = m * y - t, as compile-time
// specialisations of the kernels that compute the masked loss.  The MSE instance of every kernel keeps the
// statements it had before the other losses existed (err * m, sse += err * err): the templates below are used
// under `if constexpr (LOSS != OCF_LOSS_MSE)` only.
#pragma once
#include <stdexcept>
#include <string>

#include "../../include/ocf.h"

namespace ocf {

// rho'(e); d = Huber's delta
template <int LOSS>
__device__ __forceinline__ float loss_grad(float e, float d) {
  if constexpr (LOSS == OCF_LOSS_MAE) {
    return (e > 0.f ? 1.f : 0.f) - (e < 0.f ? 1.f : 0.f);      // exactly 0 at e = 0
  } else if constexpr (LOSS == OCF_LOSS_HUBER) {
    return fminf(fmaxf(e, -d), d);
  } else if constexpr (LOSS == OCF_LOSS_LOGCOSH) {
    // tanh e = -expm1(-2 |e|) / (expm1(-2 |e|) + 2) with e's sign: the denominator stays in [1, 2], so no
    // Inf / Inf at large |e| (-> +-1), and expm1 keeps the small residuals' digits
    const float em = expm1f(-2.f * fabsf(e));
    return copysignf(-em / (em + 2.f), e);
  } else {
    return 2.f * e;
  }
}

// rho(e)
template <int LOSS>
__device__ __forceinline__ float loss_value(float e, float d) {
  const float a = fabsf(e);
  if constexpr (LOSS == OCF_LOSS_MAE) {
    return a;
  } else if constexpr (LOSS == OCF_LOSS_HUBER) {
    return a <= d ? 0.5f * (e * e) : d * (a - 0.5f * d);
  } else if constexpr (LOSS == OCF_LOSS_LOGCOSH) {
    // |e| + log1p(exp(-2 |e|)) - ln 2: cosh itself overflows fp32 at |e| ~ 89.  Below |e| = 0.5 the two terms
    // cancel against ln 2 (absolute error ~1e-7 on values down to 0), so the even Taylor polynomial of log cosh
    // through e^12 is used there (truncation < 2e-8 at 0.5)
    if (a < 0.5f) {
      const float x = e * e;
      float p = -691.f / 935550.f;
      p = p * x + 31.f / 14175.f;
      p = p * x - 17.f / 2520.f;
      p = p * x + 1.f / 45.f;
      p = p * x - 1.f / 12.f;
      p = p * x + 0.5f;
      return p * x;
    }
    return (a + log1pf(expf(-2.f * a))) - 0.69314718055994531f;
  } else {
    return e * e;
  }
}

// stats values a loss partial carries: SSE, SAE, count (MSE) + the sum of rho (the others)
template <int LOSS> struct LossStats { static constexpr int N = LOSS == OCF_LOSS_MSE ? 3 : 4; };

inline void check_loss(int loss, float param, const char* who) {
  if (loss < OCF_LOSS_MSE || loss > OCF_LOSS_LOGCOSH)
    throw std::runtime_error(std::string(who) + ": unknown loss code " + std::to_string(loss) + " (OCF_LOSS_* 0..3)");
  if (loss == OCF_LOSS_HUBER && !(param > 0.f))
    throw std::runtime_error(std::string(who) + ": OCF_LOSS_HUBER needs loss_param (delta) > 0");
}

}  // namespace ocf

// run `stmt` with the constant LK bound to the runtime loss code (checked before)
#define OCF_LOSS_SWITCH(loss, stmt)                                              \
  do {                                                                           \
    switch (loss) {                                                              \
      case OCF_LOSS_MAE: { constexpr int LK = OCF_LOSS_MAE; stmt; } break;        \
      case OCF_LOSS_HUBER: { constexpr int LK = OCF_LOSS_HUBER; stmt; } break;    \
      case OCF_LOSS_LOGCOSH: { constexpr int LK = OCF_LOSS_LOGCOSH; stmt; } break; \
      default: { constexpr int LK = OCF_LOSS_MSE; stmt; }                         \
    }                                                                            \
  } while (0)
