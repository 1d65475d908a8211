// The host lists of the boundary pass (csrc/sns_host.cpp: build_facet_lists) under the address and undefined-behaviour
// sanitizers, for tests/test_host_boundary.py::test_facet_lists_under_sanitizers: every boundary facet of a Kuhn box mesh with
// shuffled windings, the checks of the lists, and the three refusals (which must leave the output as it was).
#include <algorithm>
#include <array>
#include <cstdio>
#include <map>
#include <random>
#include <stdexcept>
#include <vector>

#include "sns_internal.h"
namespace sns { void set_error(const std::string&) {} }
using namespace sns;

int main() {
    const int nx = 5, ny = 4, nz = 3;
    const int sy = nz + 1, sx = (ny + 1) * (nz + 1), n = (nx + 1) * sx;
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    std::vector<int32_t> tets;
    std::vector<double> pts((size_t)3 * n);
    for (int i = 0; i <= nx; ++i) for (int j = 0; j <= ny; ++j) for (int k = 0; k <= nz; ++k) {
        double* p = pts.data() + 3 * (size_t)(i * sx + j * sy + k);
        p[0] = i * 0.7; p[1] = j * 1.1; p[2] = k * 0.9;
    }
    for (int i = 0; i < nx; ++i) for (int j = 0; j < ny; ++j) for (int k = 0; k < nz; ++k) {
        const int base = i * sx + j * sy + k;
        for (auto& p : perm) {
            int off[3] = {0, 0, 0};
            tets.push_back(base);
            for (int s = 0; s < 3; ++s) { off[p[s]] = 1; tets.push_back(base + off[0] * sx + off[1] * sy + off[2]); }
        }
    }
    const int64_t E = (int64_t)tets.size() / 4;
    // boundary facets: faces that belong to one tet
    std::map<std::array<int32_t, 3>, std::pair<int, int64_t>> faces;
    for (int64_t t = 0; t < E; ++t)
        for (int o = 0; o < 4; ++o) {
            std::array<int32_t, 3> f;
            for (int a = 0, m = 0; a < 4; ++a) if (a != o) f[m++] = tets[4 * t + a];
            std::sort(f.begin(), f.end());
            auto& e = faces[f];
            ++e.first;
            e.second = t;
        }
    std::vector<int32_t> facets;
    std::vector<int64_t> own;
    std::mt19937 rng(5);
    for (auto& kv : faces)
        if (kv.second.first == 1) {
            std::array<int32_t, 3> f = kv.first;
            std::shuffle(f.begin(), f.end(), rng);
            facets.insert(facets.end(), f.begin(), f.end());
            own.push_back(kv.second.second);
        }
    const int32_t nf = (int32_t)own.size();
    HostFacetLists L;
    build_facet_lists(n, E, tets.data(), pts.data(), nf, facets.data(), own.data(), L);
    if ((int32_t)L.facets.size() != 3 * nf || L.row_ptr.size() != L.rows.size() + 1 || L.row_ptr.back() != 3 * nf) { std::printf("ERROR sizes\n"); return 1; }
    std::vector<char> seen((size_t)3 * nf, 0);
    for (size_t r = 0; r < L.rows.size(); ++r)
        for (int32_t e = L.row_ptr[r]; e < L.row_ptr[r + 1]; ++e) {
            const int32_t fv = L.row_fv[e], k = fv >> 2, a = fv & 3;
            if (k < 0 || k >= nf || a > 2 || L.facets[3 * k + a] != L.rows[r] || seen[3 * k + a]++) { std::printf("ERROR row list\n"); return 1; }
            if (e > L.row_ptr[r] && (L.row_fv[e - 1] >> 2) >= k) { std::printf("ERROR facet order\n"); return 1; }
        }
    std::printf("%d boundary facets, %zu boundary rows\n", nf, L.rows.size());
    // the refusals leave L as it is
    const HostFacetLists keep = L;
    auto refused = [&](const std::vector<int32_t>& f, const std::vector<int64_t>& o, const std::vector<double>& x) {
        try {
            build_facet_lists(n, E, tets.data(), x.data(), (int32_t)o.size(), f.data(), o.data(), L);
        } catch (const std::runtime_error&) {
            return L.facets == keep.facets && L.rows == keep.rows && L.row_ptr == keep.row_ptr && L.row_fv == keep.row_fv;
        }
        return false;
    };
    std::vector<int64_t> wrong = own;
    wrong[1] = (own[1] + E / 2) % E;
    std::vector<int32_t> twice = facets;
    twice.insert(twice.end(), facets.begin(), facets.begin() + 3);
    std::vector<int64_t> own2 = own;
    own2.push_back(own[0]);
    std::vector<double> flat = pts;
    for (int d = 0; d < 3; ++d) flat[3 * (size_t)facets[1] + d] = 0.5 * (pts[3 * (size_t)facets[0] + d] + pts[3 * (size_t)facets[2] + d]);
    if (!refused(facets, wrong, pts) || !refused(twice, own2, pts) || !refused(facets, own, flat)) { std::printf("ERROR refusal\n"); return 1; }
    std::printf("facet lists ok\n");
    return 0;
}
