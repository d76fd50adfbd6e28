// The mask-form kernel k_resident_big: four rows of RESIDENT_KERNELS (ipd_resident_host.hip), nothing else.
#include "ipd_amg_internal.h"

#include "ipd_resident_big.h"

template __global__ void k_resident_big<4, 2, true>(const ResBigDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident_big<8, 2, true>(const ResBigDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident_big<16, 1, false>(const ResBigDesc, const double* __restrict__, double*, double*, int);
template __global__ void k_resident_big<32, 1, false>(const ResBigDesc, const double* __restrict__, double*, double*, int);
