// CPU driver of amof_amd/csrc/ring_search.h (tests/test_ring_native_cpu.py): the text the GPU kernels compile, on tables the
// test writes.  stdin: "N nmax cap", then N rows of 16 neighbour indices, N degrees, N x N distances (255 = farther than
// nmax / 2).  stdout: "ok <candidates> <candidates with a ring>" and N rows of c[v][0 .. nmax], or "capacity" where an end node
// has more than cap shortest paths.
#include <cstdio>
#include <vector>

#include "../../amof_amd/csrc/ring_search.h"

int main()
{
    int N = 0, nmax = 0, cap = 0;
    if (scanf("%d %d %d", &N, &nmax, &cap) != 3 || N < 0 || N > RING_MAX_ATOMS || nmax < RING_MIN_SIZE || nmax > RING_MAX_SIZE || cap < 1) return 2;
    std::vector<int32_t> adj((size_t)N * RING_MAX_DEGREE), deg((size_t)N);
    std::vector<uint8_t> D((size_t)N * N);
    for (int32_t &x : adj)
        if (scanf("%d", &x) != 1) return 2;
    for (int32_t &x : deg)
        if (scanf("%d", &x) != 1 || x < 0 || x > RING_MAX_DEGREE) return 2;
    for (uint8_t &x : D) {
        int v;
        if (scanf("%d", &v) != 1 || v < 0 || v > 255) return 2;
        x = (uint8_t)v;
    }
    for (int i = 0; i < N; i++)
        for (int q = 0; q < deg[(size_t)i]; q++)
            if (adj[(size_t)i * RING_MAX_DEGREE + q] < 0 || adj[(size_t)i * RING_MAX_DEGREE + q] >= N) return 2;
    const ring::Graph g{adj.data(), deg.data(), D.data(), N};
    std::vector<uint32_t> c((size_t)N * (nmax + 1), 0u);
    unsigned long long stats[2] = {0, 0};
    uint16_t P1[RING_MAX_K], P2[RING_MAX_K];
    bool over = false;
    for (int v = 0; v < N; v++)
        if (ring::search_source(g, v, nmax, cap, P1, P2, 1, c.data() + (size_t)v * (nmax + 1), stats) < 0) over = true;
    if (over) {
        printf("capacity\n");
        return 0;
    }
    printf("ok %llu %llu\n", stats[0], stats[1]);
    for (int v = 0; v < N; v++) {
        for (int n = 0; n <= nmax; n++) printf("%u%c", c[(size_t)v * (nmax + 1) + n], n == nmax ? '\n' : ' ');
    }
    return 0;
}
