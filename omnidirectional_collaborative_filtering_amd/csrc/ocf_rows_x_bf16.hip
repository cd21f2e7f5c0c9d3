// row-stream kernel instances of Adadelta / Adamax for __bf16 compute (ocf_rows_x.h)
#include "ocf_rows_x.h"

namespace ocf {
OCF_ROWS_X_INSTANTIATE(__bf16)
}  // namespace ocf
