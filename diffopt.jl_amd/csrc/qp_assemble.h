// What qp_assemble.hip defines for the other files (qp.hip, nlp.hip); it
// includes this header itself, so a changed signature fails to compile.
#pragma once

#include "dopt_internal.h"

namespace dopt {

template <int RPT>
__global__ void qp_prep_kernel(QPIn, double*, int32_t*, int32_t*, double*, double*, int64_t, QPMeta*,
                               const int32_t*, double*, int, QPSummary*, unsigned*, unsigned);
__global__ void qp_asm_tile_kernel(QPIn, const int32_t*, const double*, const double*, int64_t, QPMeta*, double*,
                                   int, int, const int32_t*, int, double*);
__global__ void qp_qsym_kernel(QPIn, double*, int32_t*, const int32_t*);
int qsym_pairs(int n);
int prep_rows_per_thread(int m);
int prep_threads(int m);
size_t prep_lds(int n);

}  // namespace dopt
