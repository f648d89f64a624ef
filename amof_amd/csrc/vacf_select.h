// Which kernel answers a velocity-autocorrelation call (vacf.hip: vacf_lds on LDS-resident columns, vacf_general on the
// columns in device memory), the constants that decision shares with the kernels, the lag tiles and the LDS bytes.
// Host only (no HIP dependency: the CPU test suite compiles it with g++, tests/test_vacf_select_cpu.py through
// tests/native/vacf_select_driver.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "msd_select.h"

namespace amof {

constexpr int VACF_GROUP = 8;       // atoms per block of the fixed summation order (one accumulator per block and lag)
// vacf_lds: consecutive lags per lane.  Odd: the lanes' partner reads lie R doubles apart, and 2 R i mod 64, i = 0 .. 31, then
// names 32 different even banks -- a ds_read_b64 of a half wave is conflict-free.  11: the 2500 lags of the headline are one
// tile of 228 lanes (four waves), and a lane keeps 2 R doubles in 44 registers.
constexpr int VACF_R = 11;
constexpr int VACF_MAX_LANES = 256; // threads of a vacf_lds workgroup: a multiple of 64, at most this
constexpr int VACF_GEN_THREADS = 256;
constexpr size_t VACF_LDS_BUDGET = MSD_LDS_SERIES;      // series plus zero tail, once or twice
// The LDS of a CU.  A second column buffer is taken only where two workgroups with two buffers each still fit a CU: at the
// headline shape (5000 frames, 2500 lags: 62 624 bytes per buffer) one workgroup per CU with the load-ahead took 19.6 ms, two
// workgroups per CU with one buffer each 14.6 ms (profiles/vacf/vacf_timing.md) -- the second workgroup hides the loads, the
// LDS latency and the early end of the waves that own the long lags.
constexpr size_t VACF_LDS_CU = 160 * 1024;

// ---- the AMOF_VACF_* switches (tests / measurements), read once per call ----
struct VacfSwitches {
    bool general = false;           // AMOF_VACF_GENERAL: never vacf_lds
    bool nodb = false;              // AMOF_VACF_NODB: vacf_lds with one column buffer
    bool db = false;                // AMOF_VACF_DB: two column buffers wherever they fit the budget (measurements)

    static VacfSwitches from_env()
    {
        VacfSwitches s;
        s.general = getenv("AMOF_VACF_GENERAL") != nullptr;
        s.nodb = getenv("AMOF_VACF_NODB") != nullptr;
        s.db = getenv("AMOF_VACF_DB") != nullptr;
        return s;
    }
};

// windows[w] == w, w = 0 .. W - 1 (every lag from 0: what VelocityAutocorrelation asks for by default)
inline bool consecutive_lags(const int32_t *windows, int W)
{
    if (W < 1) return false;
    for (int w = 0; w < W; w++)
        if (windows[w] != w) return false;
    return true;
}

enum VacfKernel { VACF_LDS, VACF_GENERAL };
struct VacfPlan {
    VacfKernel kernel = VACF_GENERAL;
    // vacf_lds: tile t owns the lags [t tile_lags, min(W, (t + 1) tile_lags)), lane l of it the R lags from t tile_lags + l R
    int n_tiles = 0, lanes = 0, tile_lags = 0;
    int tail = 0;               // zeros behind a column in LDS: a lane reads at most F + 65 R - 2 <= F + tail - 1
    int64_t series = 0;         // F + tail doubles
    bool db = false;            // two column buffers: the next column streams in behind the arithmetic (VACF_LDS_CU)
    size_t lds = 0;             // dynamic LDS of the launch
    const char *path = "vacf_general";
};

inline VacfPlan vacf_select(int64_t F, int W, const int32_t *windows, int64_t origin_stride, const VacfSwitches &sw)
{
    VacfPlan p;
    if (sw.general || origin_stride != 1 || F < 2 || !consecutive_lags(windows, W)) return p;
    const int lane_windows = (W + VACF_R - 1) / VACF_R;
    // as many lanes as the lags ask for, spread evenly over the tiles; fewer (a shorter zero tail) while the series does not fit
    int tiles = (lane_windows + VACF_MAX_LANES - 1) / VACF_MAX_LANES;
    int lanes = ((lane_windows + tiles - 1) / tiles + 63) / 64 * 64;
    for (; lanes >= 64; lanes -= 64) {
        const int tail = (lanes * VACF_R + VACF_R + 1) / 2 * 2;
        const size_t bytes = (size_t)(F + tail) * sizeof(double);
        if (bytes > VACF_LDS_BUDGET) continue;
        p.kernel = VACF_LDS;
        p.lanes = lanes;
        p.tile_lags = lanes * VACF_R;
        p.n_tiles = (W + p.tile_lags - 1) / p.tile_lags;
        p.tail = tail;
        p.series = F + tail;
        p.db = !sw.nodb && 2 * bytes <= VACF_LDS_BUDGET && (sw.db || 4 * bytes <= VACF_LDS_CU);
        p.lds = p.db ? 2 * bytes : bytes;
        p.path = "vacf_lds";
        break;
    }
    return p;
}

}  // namespace amof
