// The three-level forms of k_resident (KE3 != 0): six rows of RESIDENT_KERNELS (ipd_resident_host.hip), nothing else.
#include "ipd_amg_internal.h"

#include "ipd_resident.h"

template __global__ void k_resident<4, 4, 1, false>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<8, 8, 1, false>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<4, 4, 4, false>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<4, 4, 8, false>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<8, 8, 4, false>(const ResDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident<8, 8, 8, false>(const ResDesc, const double* __restrict__, double*, double*, int);
