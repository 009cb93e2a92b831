// dwbc_kernels_im.h -- the build of the kernels that reads one body table per instance (DWBC_BODY of dwbc_types.h under DWBC_INST_MODEL):
// the same source as the product kernels (dwbc_kernels.h) with the namespace renamed to dwbc_im, so that both builds link into
// libdwbc_hip.so and no code object of the default build depends on this one.  Included by the dwbc_kernels_im_*.hip translation units
// alone, which split the instantiations so that they compile side by side; each emits its rows through DWBC_IM_TABLE, every row marked
// dwbc_plan::kInstModel (DWBC_ROW), and dwbc_capi.hip joins them into one table.  fp64, TOCABI's constant tree: the full-model cycle of one to
// four task levels on every launch route and the six lean launches; no reduced path, no general-contact kernel, no generic tree.
#pragma once
#define DWBC_INST_MODEL
#define DWBC_NO_BUILTIN_ROWS
#define dwbc dwbc_im  // (stays defined to the end of the translation unit: the row macros spell dwbc:: into kernel and tree names)
#include "dwbc_kernels.h"

using namespace dwbc;

#define DWBC_IM_TABLE(FN, ...)                                      \
    extern "C" const dwbc_plan::Row *FN(int *count) {               \
        static const dwbc_plan::Row rows[] = {__VA_ARGS__};         \
        *count = (int)(sizeof(rows) / sizeof(rows[0]));             \
        return rows;                                                \
    }
// capped extras, wide extras, wide lean and compact lean build of one level count
#define DWBC_IM_LEVEL(FN, NLV) DWBC_IM_TABLE(FN, DWBC_ROWS_V2(39, 34, NLV, TopoTocabi, 1) DWBC_ROW_LEAN_COMPACT(39, 34, NLV, TopoTocabi, 1))
