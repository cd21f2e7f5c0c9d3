// fused small-model step (ocf_mlp_kernel.h): the kernel's Adadelta / Adamax instances (4 losses x 3 dtypes x 2 kinds)
#include "ocf_mlp_kernel.h"

namespace ocf {
namespace mlp {

template <typename CT, int LOSS>
void launch_loss_x(int kind, const P& p, int wgs, hipStream_t s) {
  if (kind == OCF_OPT_ADADELTA)
    hipLaunchKernelGGL((mlp_step_kernel<CT, OCF_OPT_ADADELTA, LOSS>), dim3(wgs), dim3(THREADS), 0, s, p);
  else if (kind == OCF_OPT_ADAMAX)
    hipLaunchKernelGGL((mlp_step_kernel<CT, OCF_OPT_ADAMAX, LOSS>), dim3(wgs), dim3(THREADS), 0, s, p);
  else
    throw std::runtime_error("ocf_mlp_step: kind " + std::to_string(kind) + " is not Adadelta / Adamax");
}
#define OCF_MLP_X_INST(CT)                                                                     \
  template void launch_loss_x<CT, OCF_LOSS_MSE>(int, const P&, int, hipStream_t);               \
  template void launch_loss_x<CT, OCF_LOSS_MAE>(int, const P&, int, hipStream_t);               \
  template void launch_loss_x<CT, OCF_LOSS_HUBER>(int, const P&, int, hipStream_t);             \
  template void launch_loss_x<CT, OCF_LOSS_LOGCOSH>(int, const P&, int, hipStream_t);
OCF_MLP_X_INST(float)
OCF_MLP_X_INST(_Float16)
OCF_MLP_X_INST(__bf16)

}  // namespace mlp
}  // namespace ocf
