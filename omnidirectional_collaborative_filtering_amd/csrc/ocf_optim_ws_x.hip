// Role-split weight-gradient + optimizer kernel (ocf_optim_ws.h): the Adadelta / Adamax instances, in a
// translation unit of their own so that ocf_gemm.hip compiles what it compiled before.
#include "ocf_internal.h"
#include "ocf_optim_ws.h"

namespace ocf {

template <typename CT>
void launch_ws_x(int kind, int G, const GemmShape& sh, const EpiOptim::Params& ep, const WsJobs& jb, hipStream_t s) {
  switch (kind) {
    case OCF_OPT_ADADELTA:
      hipLaunchKernelGGL((optim_ws_kernel<CT, false, OCF_OPT_ADADELTA>), dim3(G), dim3(WS_THREADS), 0, s, sh, ep, jb);
      break;
    case OCF_OPT_ADAMAX:
      hipLaunchKernelGGL((optim_ws_kernel<CT, false, OCF_OPT_ADAMAX>), dim3(G), dim3(WS_THREADS), 0, s, sh, ep, jb);
      break;
    default:
      throw std::runtime_error("optim_ws: kind " + std::to_string(kind) + " is not Adadelta / Adamax");
  }
}

template void launch_ws_x<_Float16>(int, int, const GemmShape&, const EpiOptim::Params&, const WsJobs&, hipStream_t);
template void launch_ws_x<__bf16>(int, int, const GemmShape&, const EpiOptim::Params&, const WsJobs&, hipStream_t);

}  // namespace ocf
