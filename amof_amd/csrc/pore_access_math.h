// Winding of the periodic components of a labelled grid (pore_access.hip): the host side of the accessibility test.  No HIP
// dependency: the CPU test suite compiles it with g++ (tests/native/pore_access_driver.cpp).
//
// The device labels the void WITHOUT the links through the periodic faces ("open" components; label = smallest linear index)
// and hands over the wrap links between void points as (label below the face, label above the face, axis).  A closed path
// inside one open component crosses no face, so its winding is zero; every winding comes from the graph whose nodes are the
// open components and whose edges are the wrap links.  A union-find over that graph that carries, per node, the image offset
// relative to its root yields, for every link that closes a cycle, the cycle's winding vector offset(lo) + e_axis - offset(hi).
// The fundamental cycles of a spanning forest generate the cycle space, so the vectors collected per tree span the winding
// lattice of that periodic component: its rank is the component's dimension.  Work: O(links log links).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace amof {

// up to three independent integer vectors: the rank of everything added so far.  Offsets are sums of at most `links` unit
// steps (< 2^21 for a grid of 2^31 points), cross products stay below 2^43 in int64, the determinant is taken in 128 bits.
struct WindingBasis {
    int rank = 0;
    int64_t b[2][3] = {{0, 0, 0}, {0, 0, 0}};
    void add(const int64_t v[3])
    {
        if (rank == 3 || (v[0] == 0 && v[1] == 0 && v[2] == 0)) return;
        if (rank == 0) {
            for (int c = 0; c < 3; c++) b[0][c] = v[c];
            rank = 1;
            return;
        }
        const int64_t cx = b[0][1] * v[2] - b[0][2] * v[1], cy = b[0][2] * v[0] - b[0][0] * v[2], cz = b[0][0] * v[1] - b[0][1] * v[0];
        if (rank == 1) {
            if (cx == 0 && cy == 0 && cz == 0) return;
            for (int c = 0; c < 3; c++) b[1][c] = v[c];
            rank = 2;
            return;
        }
        // rank 2: det(b0, b1, v) = b1 . (v x b0) = -b1 . (b0 x v)
        const __int128 det = (__int128)b[1][0] * cx + (__int128)b[1][1] * cy + (__int128)b[1][2] * cz;
        if (det != 0) rank = 3;
    }
    void merge(const WindingBasis &o)
    {
        if (o.rank == 3) rank = 3;
        for (int k = 0; k < o.rank && k < 2; k++) add(o.b[k]);
    }
};

struct WrapLink {
    int32_t lo, hi;     // open labels of the void points below and above the face
    int32_t axis;       // the face's axis: the step from lo to hi adds e_axis to the image
};

struct PeriodicComponent {
    int32_t label;      // the smallest open label of the tree = the periodic component's label
    int32_t dimension;  // rank of its winding lattice
};

class WindingResolver {
public:
    // the periodic components that contain a wrap link, sorted by label (every other component has dimension 0)
    std::vector<PeriodicComponent> resolve(const std::vector<WrapLink> &links)
    {
        ids_.clear();
        ids_.reserve(links.size() * 2);
        for (const WrapLink &l : links) {
            ids_.push_back(l.lo);
            ids_.push_back(l.hi);
        }
        std::sort(ids_.begin(), ids_.end());
        ids_.erase(std::unique(ids_.begin(), ids_.end()), ids_.end());
        const size_t n = ids_.size();
        parent_.resize(n);
        size_.assign(n, 1);
        off_.assign(n * 3, 0);
        basis_.assign(n, WindingBasis());
        least_.resize(n);
        for (size_t k = 0; k < n; k++) {
            parent_[k] = (int32_t)k;
            least_[k] = ids_[k];
        }
        for (const WrapLink &l : links) {
            int64_t oa[3], ob[3], w[3];
            const int32_t ra = find(node(l.lo), oa), rb = find(node(l.hi), ob);
            for (int c = 0; c < 3; c++) w[c] = oa[c] + (c == l.axis ? 1 : 0) - ob[c];
            if (ra == rb) {
                basis_[ra].add(w);
                continue;
            }
            // image(hi's root) = image(lo's root) + w; the smaller tree goes under the larger
            int32_t top = ra, sub = rb;
            if (size_[ra] < size_[rb]) {
                top = rb;
                sub = ra;
                for (int c = 0; c < 3; c++) w[c] = -w[c];
            }
            parent_[sub] = top;
            for (int c = 0; c < 3; c++) off_[(size_t)sub * 3 + c] = w[c];
            size_[top] += size_[sub];
            least_[top] = std::min(least_[top], least_[sub]);
            basis_[top].merge(basis_[sub]);
        }
        std::vector<PeriodicComponent> out;
        for (size_t k = 0; k < n; k++)
            if (parent_[k] == (int32_t)k) out.push_back(PeriodicComponent{least_[k], basis_[k].rank});
        std::sort(out.begin(), out.end(), [](const PeriodicComponent &x, const PeriodicComponent &y) { return x.label < y.label; });
        return out;
    }

private:
    int32_t node(int32_t label) const { return (int32_t)(std::lower_bound(ids_.begin(), ids_.end(), label) - ids_.begin()); }
    // root of x and the image offset of x relative to it; the path is compressed (no recursion: chains can be long)
    int32_t find(int32_t x, int64_t o[3])
    {
        path_.clear();
        int32_t r = x;
        while (parent_[r] != r) {
            path_.push_back(r);
            r = parent_[r];
        }
        int64_t acc[3] = {0, 0, 0};
        for (size_t k = path_.size(); k-- > 0;) {
            const int32_t y = path_[k];
            for (int c = 0; c < 3; c++) {
                acc[c] += off_[(size_t)y * 3 + c];
                off_[(size_t)y * 3 + c] = acc[c];
            }
            parent_[y] = r;
        }
        for (int c = 0; c < 3; c++) o[c] = acc[c];
        return r;
    }
    std::vector<int32_t> ids_, parent_, size_, least_, path_;
    std::vector<int64_t> off_;
    std::vector<WindingBasis> basis_;
};

}  // namespace amof
