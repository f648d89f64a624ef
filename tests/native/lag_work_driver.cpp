// Prints what amof_amd/csrc/lag_work.h computes for the inputs on stdin (tests/test_lag_work_cpu.py compares with
// amof_amd/lags.py).
//   line "F stride W m0 .. m(W-1)"  -> "T total" (lag_work_total), then for every 0 <= wb <= we <= total one line
//                                      "wb we o0 o1 .. " with the W intervals of lag_work_ranges, whose return value must
//                                      be the same total (exit status 3 otherwise)
#include <stdio.h>

#include <vector>

#include "../../amof_amd/csrc/lag_work.h"

int main()
{
    long long F, stride;
    int W;
    while (scanf("%lld %lld %d", &F, &stride, &W) == 3) {
        if (W < 0) return 1;
        std::vector<int32_t> windows((size_t)W);
        for (auto &m : windows)
            if (scanf("%d", &m) != 1) return 1;
        const int64_t total = amof::lag_work_total(windows.data(), W, F, stride);
        printf("T %lld\n", (long long)total);
        std::vector<amof::LagRange> iv((size_t)W);
        for (int64_t wb = 0; wb <= total; wb++)
            for (int64_t we = wb; we <= total; we++) {
                if (amof::lag_work_ranges(windows.data(), W, F, stride, wb, we, iv.data()) != total) return 3;
                printf("%lld %lld", (long long)wb, (long long)we);
                for (const amof::LagRange &r : iv) printf(" %d %d", r.o0, r.o1);
                printf("\n");
            }
    }
    return 0;
}
