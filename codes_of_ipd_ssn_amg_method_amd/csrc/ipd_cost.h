// What ipd_cost.hip (the cost matrix built on the device from point clouds) sees of a driver handle, and the one
// body ipd_apd_create and ipd_apd_create_points share.  struct ipd_apd itself stays private to ipd_driver.hip;
// host code only.
#pragma once

#include <functional>

#include "ipd_internal.h"

struct ipd_apd;

struct ApdCostView {
    ipd_ctx* ctx = nullptr;
    int m = 0, n = 0;
    size_t mn = 0;
    const double* c = nullptr;          // mn
    ipd_cost_stats* stats = nullptr;    // of c, valid once *have_stats (c never changes after the create)
    bool* have_stats = nullptr;
};

// Fills the device arrays of a workspace under construction: c (mn), phi_ones (mn, to be set to ones; nullptr
// when the workspace has no phi or the caller gave one), *st the statistics of c.  A throw abandons the create.
using ApdCostFill = std::function<void(double* c_dev, double* phi_ones_dev, ipd_cost_stats* st)>;

// ipd_driver.hip
ApdCostView apd_cost_view(ipd_apd* h);
// Allocates and uploads everything but c: fill == nullptr uploads d->c (and needs d->phi for class 2),
// otherwise fill makes c (and the phi the caller left out).
void apd_create_common(ipd_ctx* ctx, const ipd_apd_data* d, const ApdCostFill* fill, ipd_apd** out);
