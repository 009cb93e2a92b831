// dwbc_kernels_im_lean.hip -- per-instance body table (dwbc_kernels_im.h): the six lean launches.
#include "dwbc_kernels_im.h"
DWBC_IM_TABLE(dwbc_im_rows_lean, DWBC_ROW_REDIST(39, 34, TopoTocabi, 1) DWBC_ROW_GRAVCOMP(39, 34, TopoTocabi, 1) DWBC_ROW_LINK_QUERY(39, 34)
                  DWBC_ROW_DYNAMICS(39, 34, TopoTocabi, 1) DWBC_ROW_CONTACT_SPACE(39, 34, TopoTocabi, 1) DWBC_ROW_TASK_SPACE(39, 34, TopoTocabi, 1))
