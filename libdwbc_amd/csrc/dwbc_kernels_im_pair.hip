// dwbc_kernels_im_pair.hip -- per-instance body table (dwbc_kernels_im.h): the two-wave cycle kernels.
#include "dwbc_kernels_im.h"
DWBC_IM_TABLE(dwbc_im_rows_pair, DWBC_ROW_PAIR(1) DWBC_ROW_PAIR(2))
