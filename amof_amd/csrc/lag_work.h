// The lag/origin work list of the dynamics family (vanhove_distinct.hip, isf.hip, current.hip, bond.hip), host side (no HIP
// dependency: the CPU test suite compiles it with g++, tests/test_lag_work_cpu.py).  Included by amof_internal.h.
//
// Lag m = windows[w] has the origins k = 1 + stride o, o = 0 .. n(m) - 1, i.e. every stride-th frame from 1 up to
// F - m - 1.  The work list is every (lag, origin) pair in lag-major order, origins ascending; a call takes the entries
// [wb, we) of it, so ranks and halves split it by index.  amof_amd/lags.py states the same rule for the Python side.
#pragma once

#include <stdint.h>

#include <algorithm>

namespace amof {

// origins of lag m in a trajectory of F frames
inline int64_t lag_origin_count(int64_t F, int64_t m, int64_t stride)
{
    return F - m - 2 >= 0 ? (F - m - 2) / stride + 1 : 0;
}

// frame of origin o
inline int64_t lag_origin_frame(int64_t o, int64_t stride) { return 1 + stride * o; }

// length of the work list
inline int64_t lag_work_total(const int32_t *windows, int W, int64_t F, int64_t stride)
{
    int64_t total = 0;
    for (int w = 0; w < W; w++) total += lag_origin_count(F, windows[w], stride);
    return total;
}

// origin indices [o0, o1) of one lag: the layout of HIP's int2, which the F(q, t) kernel reads the table as
struct LagRange {
    int32_t o0, o1;
};

// out[w] = the origins of lag w among the entries [wb, we) of the work list ({0, 0} where there are none); returns the
// length of the whole list (the caller checks 0 <= wb <= we <= that)
inline int64_t lag_work_ranges(const int32_t *windows, int W, int64_t F, int64_t stride, int64_t wb, int64_t we, LagRange *out)
{
    int64_t first = 0;
    for (int w = 0; w < W; w++) {
        const int64_t n = lag_origin_count(F, windows[w], stride);
        const int64_t o0 = std::max<int64_t>(wb - first, 0), o1 = std::min<int64_t>(we - first, n);
        out[w] = o0 < o1 ? LagRange{(int32_t)o0, (int32_t)o1} : LagRange{0, 0};
        first += n;
    }
    return first;
}

}  // namespace amof
