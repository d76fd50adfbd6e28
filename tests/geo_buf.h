// A buffer as the geometry drivers see it (tests/walk_geo_driver.cpp, plan_apply_geo_driver.cpp, dual_geo_driver.cpp,
// round_geo_driver.cpp): which entries the walking kernels write, which the finishing kernels read.
#pragma once

#include <cstddef>
#include <vector>

struct Buf {
    std::vector<unsigned char> written;
    size_t wmax = 0, rmax = 0, dup = 0, unwritten = 0;   // largest index written / read, entries written twice / read unwritten
    bool outside = false;                                // an index at or beyond the length
    explicit Buf(size_t len) : written(len, 0) {}
    size_t len() const { return written.size(); }
    void write(size_t idx) {
        wmax = idx > wmax ? idx : wmax;
        if (idx >= written.size()) {
            outside = true;
            return;
        }
        dup += written[idx];
        written[idx] = 1;
    }
    void read(size_t idx) {
        rmax = idx > rmax ? idx : rmax;
        if (idx >= written.size())
            outside = true;
        else if (!written[idx])
            ++unwritten;
    }
};
