// What ipd_plan.hip (the sparse transport plan out of and into the workspace) sees of a driver
// handle.  struct ipd_apd itself stays private to ipd_driver.hip; host code only.
#pragma once

#include "ipd_internal.h"

struct ipd_apd;

struct ApdPlanView {
    ipd_ctx* ctx = nullptr;
    int m = 0, n = 0;
    size_t mn = 0;
    const double* c = nullptr;   // mn
    const double* p = nullptr;   // m
    const double* q = nullptr;   // n
    double* u = nullptr;         // the x block is the first mn entries (class 2: of uk = [xk;yk;zk])
    double* v = nullptr;
};

// ipd_driver.hip
ApdPlanView apd_plan_view(ipd_apd* h);
// the script variables after a new state went in: what ipd_apd_set_state does besides the uploads
// (k, the KKT reference, the records and the AMG counters start over; bk, lk, histories stay)
void apd_restart_script(ipd_apd* h);
