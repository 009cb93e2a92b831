// dwbc_kernels_im_l1.hip -- per-instance body table (dwbc_kernels_im.h): the one-wave cycle kernels of 1 task level.
#include "dwbc_kernels_im.h"
DWBC_IM_LEVEL(dwbc_im_rows_l1, 1)
