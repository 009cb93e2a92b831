// dwbc_kernels_im_l3.hip -- per-instance body table (dwbc_kernels_im.h): the one-wave cycle kernels of 3 task levels.
#include "dwbc_kernels_im.h"
DWBC_IM_LEVEL(dwbc_im_rows_l3, 3)
