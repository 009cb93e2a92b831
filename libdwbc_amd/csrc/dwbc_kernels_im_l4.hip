// dwbc_kernels_im_l4.hip -- per-instance body table (dwbc_kernels_im.h): the one-wave cycle kernels of 4 task levels.
#include "dwbc_kernels_im.h"
DWBC_IM_LEVEL(dwbc_im_rows_l4, 4)
