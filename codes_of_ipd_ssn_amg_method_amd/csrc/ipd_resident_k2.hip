// The two-level forms of k_resident (KE3 == 0): four rows of RESIDENT_KERNELS (ipd_resident_host.hip), nothing else.
#include "ipd_amg_internal.h"

#include "ipd_resident.h"

template __global__ void k_resident<16, 16, 0, true>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<4, 4, 0, false>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<8, 8, 0, false>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<16, 16, 0, false>(const ResDesc, const double* __restrict__, double*, double*, int);
