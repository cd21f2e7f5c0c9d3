// row-stream kernel instances of Adadelta / Adamax for float compute (ocf_rows_x.h)
#include "ocf_rows_x.h"

namespace ocf {
OCF_ROWS_X_INSTANTIATE(float)
}  // namespace ocf
