// row-stream kernel instances of Adadelta / Adamax for _Float16 compute (ocf_rows_x.h)
#include "ocf_rows_x.h"

namespace ocf {
OCF_ROWS_X_INSTANTIATE(_Float16)
}  // namespace ocf
