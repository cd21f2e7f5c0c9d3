// The row-stream launches of the Adadelta / Adamax kernel instances (ocf_rows_impl.h rows_x_*), instantiated
// once per compute dtype in ocf_rows_x_f16.hip / ocf_rows_x_bf16.hip / ocf_rows_x_f32.hip: the same kernels and
// launch forms as for the other kinds, in translation units of their own so that the build's longest units
// (ocf_rows_{f16,bf16,f32}.hip) stay as they were.
#pragma once
#include "ocf_rows_impl.h"

namespace ocf {

template <typename CT>
void rows_x_one(const RowsLaunch& L, hipStream_t s) {
  rows_dispatch<CT, true>(L, RowsOne{L, s});
}
template <typename CT>
void rows_x_pair(const RowsLaunch& A, const RowsLaunch& B, const RsPair& ps, hipStream_t s) {
  rows_dispatch<CT, true>(A, RowsPair{A, B, ps, s});
}
template <typename CT>
void rows_x_dual(const RowsLaunch& A, const RowsLaunch& B, const RsPair& ps, int grid, hipStream_t s) {
  rows_dispatch<CT, true>(A, RowsDual{A, B, ps, grid, s});
}

#define OCF_ROWS_X_INSTANTIATE(CT)                                                                          \
  template void rows_x_one<CT>(const RowsLaunch&, hipStream_t);                                             \
  template void rows_x_pair<CT>(const RowsLaunch&, const RowsLaunch&, const RsPair&, hipStream_t);          \
  template void rows_x_dual<CT>(const RowsLaunch&, const RowsLaunch&, const RsPair&, int, hipStream_t);

}  // namespace ocf
