// Driver for tests/test_pore_access_host.py: the winding resolver of amof_amd/csrc/pore_access_math.h on the CPU.
// stdin, one job per line:
//   links L  lo hi axis  lo hi axis ...           a list of wrap links between open labels
//   mask nx ny nz px py pz  0/1 x (nx ny nz)      a mask: labelled here WITHOUT the links through the faces (a sequential
//                                                 flood fill, label = smallest linear index), the wrap links between its void
//                                                 points emitted as the library's kernels emit them, then resolved
// stdout, one line per job:
//   links: "label dimension" of every periodic component that has a wrap link, in label order
//   mask:  "label size dimension" of EVERY periodic component, in label order
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <vector>

#include "../../amof_amd/csrc/pore_access_math.h"

using amof::PeriodicComponent;
using amof::WrapLink;

static void job_links()
{
    int L = 0;
    if (scanf("%d", &L) != 1) return;
    std::vector<WrapLink> links((size_t)L);
    for (WrapLink &l : links)
        if (scanf("%d %d %d", &l.lo, &l.hi, &l.axis) != 3) return;
    amof::WindingResolver res;
    for (const PeriodicComponent &c : res.resolve(links)) printf("%d %d  ", c.label, c.dimension);
    printf("\n");
}

static void job_mask()
{
    int n[3], pbc[3];
    if (scanf("%d %d %d %d %d %d", &n[0], &n[1], &n[2], &pbc[0], &pbc[1], &pbc[2]) != 6) return;
    const int G = n[0] * n[1] * n[2];
    std::vector<int> mask((size_t)G), label((size_t)G, -1);
    for (int &m : mask)
        if (scanf("%d", &m) != 1) return;
    const int stride[3] = {n[1] * n[2], n[2], 1};
    auto coord = [&](int p, int ax) { return ax == 0 ? p / stride[0] : ax == 1 ? (p / stride[1]) % n[1] : p % n[2]; };
    std::map<int, int> open_size;
    for (int seed = 0; seed < G; seed++) {
        if (!mask[(size_t)seed] || label[(size_t)seed] >= 0) continue;
        std::vector<int> todo(1, seed);
        label[(size_t)seed] = seed;
        int size = 0;
        while (!todo.empty()) {
            const int p = todo.back();
            todo.pop_back();
            size++;
            for (int ax = 0; ax < 3; ax++)
                for (int d = -1; d <= 1; d += 2) {
                    const int c = coord(p, ax) + d;
                    if (c < 0 || c >= n[ax]) continue;          // (no link through a face)
                    const int q = p + d * stride[ax];
                    if (mask[(size_t)q] && label[(size_t)q] < 0) {
                        label[(size_t)q] = seed;
                        todo.push_back(q);
                    }
                }
        }
        open_size[seed] = size;
    }
    std::vector<WrapLink> links;
    for (int ax = 0; ax < 3; ax++) {
        if (!pbc[ax]) continue;
        for (int p = 0; p < G; p++) {
            if (coord(p, ax) != n[ax] - 1) continue;
            const int q = p - (n[ax] - 1) * stride[ax];
            if (mask[(size_t)p] && mask[(size_t)q]) links.push_back(WrapLink{label[(size_t)p], label[(size_t)q], ax});
        }
    }
    amof::WindingResolver res;
    const std::vector<PeriodicComponent> comps = res.resolve(links);
    // the periodic component of an open label: the trees of the link graph, found again here by a plain union-find
    std::map<int, int> up;
    for (const auto &kv : open_size) up[kv.first] = kv.first;
    auto root = [&](int x) {
        while (up[x] != x) x = up[x];
        return x;
    };
    for (const WrapLink &l : links) {
        const int a = root(l.lo), b = root(l.hi);
        if (a != b) up[a > b ? a : b] = a > b ? b : a;          // (towards the smaller label: the root is the tree's smallest)
    }
    std::map<int, int> size;
    for (const auto &kv : open_size) size[root(kv.first)] += kv.second;
    for (const auto &kv : size) {
        int dim = 0;
        for (const PeriodicComponent &c : comps)
            if (c.label == kv.first) dim = c.dimension;
        printf("%d %d %d  ", kv.first, kv.second, dim);
    }
    printf("\n");
}

int main()
{
    char word[16];
    while (scanf("%15s", word) == 1) {
        if (word[0] == 'l') job_links();
        else if (word[0] == 'm') job_mask();
        else return 2;
    }
    return 0;
}
