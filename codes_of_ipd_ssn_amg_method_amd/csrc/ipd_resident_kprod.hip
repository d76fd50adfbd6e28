// The production forms of the column-slice kernels (DIAG == false: no stamps, no skip-publish hook) and the full-shape
// forms of the composed instantiation (FULL): the rows of RESIDENT_VARIANTS (ipd_resident_host.hip), nothing else.
#include "ipd_amg_internal.h"

#include "ipd_resident.h"

template __global__ void k_resident<16, 16, 0, true, false, true>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<16, 16, 0, true, true, true>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<16, 16, 0, true, false, false>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<16, 16, 0, false, false, false>(const ResDesc, const double* __restrict__, double*, double*, int);
