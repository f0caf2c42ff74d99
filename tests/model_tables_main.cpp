// model_tables_main.cpp - build_model_tables (csrc/pmx_model_tables.cpp) as a program of its own, for a run under the address and
// undefined-behaviour sanitizers (tests/test_model_tables_cpu.py compiles and starts it): the shapes at which a table is empty or tiny, a
// model at the limits (256 nodes, 128 clusters) drawn from a fixed seed, and the refused descriptions.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pmx.h"
#include "pmx_model_tables.h"

namespace {

struct Model {
    std::vector<uint8_t> node_type, typemask;
    std::vector<float> mean, std;
    std::vector<uint64_t> cluster_nodes;
    std::vector<double> center, size;
    pmx_model_desc desc() const {
        const int nm = (int)node_type.size(), k = (int)typemask.size();
        return pmx_model_desc{nm, k, node_type.data(), mean.data(), std.data(), cluster_nodes.data(), typemask.data(), center.data(), size.data()};
    }
};

// Nodes with the given types, edge (m, n) = {mean(m, n), sd(m, n)}, clusters as node lists.
template <class FM, class FS>
Model make(const std::vector<int> &types, const std::vector<std::vector<int>> &clusters, FM mean, FS sd) {
    Model m;
    const int nm = (int)types.size(), words = nm > 64 ? (nm + 63) / 64 : 1;
    for (int t : types) m.node_type.push_back((uint8_t)t);
    for (int a = 0; a < nm; ++a)
        for (int b = 0; b < nm; ++b) m.mean.push_back(mean(a, b)), m.std.push_back(sd(a, b));
    m.cluster_nodes.assign(clusters.size() * words, 0);
    for (size_t c = 0; c < clusters.size(); ++c) {
        uint8_t tm = 0;
        for (int x : clusters[c]) m.cluster_nodes[c * words + x / 64] |= 1ull << (x % 64), tm |= (uint8_t)(1u << types[x]);
        m.typemask.push_back(tm);
        m.center.insert(m.center.end(), {1.5 * c, 0.25 * c, -1.0 * c});
        m.size.push_back(1.0 + 0.5 * c);
    }
    return m;
}

int g_failed = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

// Builds the tables through the hook, reads every array from end to end (the sanitizer sees a size that is wrong) and frees them.
const pmxt_tables_view *g_view = nullptr;
int build(const Model &m, int expect_rc, void (*check)() = nullptr) {
    const pmx_model_desc d = m.desc();
    pmxt_tables *t = nullptr;
    const int rc = pmxt_tables_create(&d, &t);
    EXPECT(rc == expect_rc);
    if (rc != PMX_OK) {
        EXPECT(t == nullptr && pmx_last_error()[0] != 0);
        return rc;
    }
    pmxt_tables_view v;
    EXPECT(pmxt_tables_view_get(t, &v) == PMX_OK);
    double sum = 0;
    uint64_t nan = 0;
    for (uint64_t i = 0; i < 4 * v.n_edge; ++i) sum += v.edge[i];
    for (uint64_t i = 0; i < 2 * v.n_cpair; ++i) sum += v.cpair[i] + (std::isfinite(v.cwin[i]) ? v.cwin[i] : 0.f);
    for (uint64_t i = 0; i < v.n_win; ++i) {
        nan += std::isnan(v.win[2 * i]) ? 1 : 0;
        EXPECT(std::isnan(v.win[2 * i]) == std::isnan(v.win[2 * i + 1]));
    }
    for (uint64_t i = 0; i < v.n_edge; ++i) sum += v.wok[i] ? v.wlo[i] + v.whi[i] : 0.f;
    for (uint64_t i = 0; i < v.n_node_type; ++i) sum += v.node_type[i];
    for (uint64_t i = 0; i < v.n_tclus; ++i) sum += (double)v.tclus[i];
    for (uint64_t i = 0; i < v.n_sidtab; ++i) EXPECT(v.sidtab[i] < v.NS);
    for (uint64_t i = 0; i + 1 < v.n_sub_off; ++i) EXPECT(v.sub_off[i] <= v.sub_off[i + 1]);
    EXPECT(v.n_sub_off == (uint64_t)v.NS + 1 && v.n_sub_nodes >= v.sub_off[v.NS] && v.n_sub_nodes >= 1);
    for (uint64_t i = 0; i < v.n_sub_nodes; ++i) EXPECT((int)v.sub_nodes[i] < (v.Nm > 0 ? v.Nm : 1));
    EXPECT(nan == v.n_complex_cells && v.n_win == (uint64_t)v.NF * v.ncell && std::isfinite(sum));
    EXPECT(v.NF == (v.symmetric ? v.NS * (v.NS + 1) / 2 : v.NS * v.NS));
    g_view = &v;
    if (check) check();
    g_view = nullptr;
    EXPECT(pmxt_tables_destroy(t) == PMX_OK);
    return rc;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull; // fixed seed (xorshift64)
double uniform() {
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return (double)(g_rng >> 11) / 9007199254740992.0;
}

} // namespace

int main() {
    auto flat = [](float v) { return [v](int, int) { return v; }; };
    // no node, no cluster
    build(make({}, {}, flat(0.f), flat(1.f)), PMX_OK, [] { EXPECT(g_view->NS == 1 && g_view->NF == 1 && g_view->n_edge == 0 && g_view->n_cpair == 0); });
    // one node in one cluster
    build(make({3}, {{0}}, flat(0.f), flat(0.8f)), PMX_OK, [] { EXPECT(g_view->NS == 2 && g_view->NF == 3); });
    // two nodes, no cluster
    build(make({0, 4}, {}, [](int a, int b) { return a == b ? 0.f : 4.f; }, [](int a, int b) { return a == b ? 0.5f : 0.7f; }), PMX_OK,
          [] { EXPECT(g_view->NS == 1 && g_view->K == 0 && g_view->n_sidtab == 128); });
    // three nodes, asymmetric edges
    {
        const float mean[9] = {0.f, 3.f, 5.5f, 3.4f, 0.f, 4.25f, 6.f, 4.f, 0.f}, sd[9] = {0.5f, 0.6f, 0.9f, 0.7f, 0.5f, 0.55f, 0.8f, 0.6f, 0.5f};
        build(make({0, 0, 4}, {{0, 1}, {2}, {0, 2}}, [&](int a, int b) { return mean[3 * a + b]; }, [&](int a, int b) { return sd[3 * a + b]; }), PMX_OK,
              [] { EXPECT(g_view->symmetric == 0 && g_view->NF == g_view->NS * g_view->NS); });
    }
    // two windows with a gap inside one cell: a NaN cell
    {
        const float mean[9] = {0.f, 3.05f, 5.07f, 3.05f, 0.f, 2.f, 5.07f, 2.f, 0.f};
        build(make({0, 0, 0}, {{0}, {1, 2}}, [&](int a, int b) { return mean[3 * a + b]; }, flat(0.5f)), PMX_OK,
              [] { EXPECT(g_view->symmetric == 1 && g_view->n_complex_cells >= 1); });
    }
    // an edge no distance >= 0 can pass (mean far below zero): no window, nothing read out of it
    build(make({1, 1}, {{0, 1}}, [](int a, int b) { return a == b ? 0.f : -5.f; }, flat(0.5f)), PMX_OK);
    // the limits: 256 nodes in 128 clusters, drawn from the seed; nodes in several clusters, every type
    {
        const int nm = PMX_MAX_MODEL_NODES, k = PMX_MAX_MODEL_CLUSTERS;
        std::vector<int> types(nm);
        std::vector<double> x(3 * nm);
        for (int i = 0; i < nm; ++i) {
            types[i] = (int)(uniform() * PMX_NUM_TYPES) % PMX_NUM_TYPES;
            for (int c = 0; c < 3; ++c) x[3 * i + c] = 20.0 * uniform();
        }
        std::vector<std::vector<int>> clusters(k);
        for (int i = 0; i < nm; ++i) clusters[i % k].push_back(i);
        for (int c = 0; c < k; ++c)
            if (uniform() < 0.25) clusters[c].push_back((int)(uniform() * nm) % nm);
        std::vector<float> sd(nm * nm);
        for (int a = 0; a < nm; ++a)
            for (int b = 0; b <= a; ++b) sd[a * nm + b] = sd[b * nm + a] = (float)(0.6 + 0.9 * uniform());
        auto mean = [&](int a, int b) {
            const double dx = x[3 * a] - x[3 * b], dy = x[3 * a + 1] - x[3 * b + 1], dz = x[3 * a + 2] - x[3 * b + 2];
            return (float)std::sqrt(dx * dx + dy * dy + dz * dz);
        };
        build(make(types, clusters, mean, [&](int a, int b) { return sd[a * nm + b]; }), PMX_OK,
              [] { EXPECT(g_view->Nm == 256 && g_view->K == 128 && g_view->symmetric == 1 && g_view->NS > 128); });
    }
    // refused descriptions
    build(make({0, 0}, {{0, 1}}, flat(1.f), [](int a, int b) { return a == 1 && b == 0 ? 0.f : 0.5f; }), PMX_ERR_INVALID);
    build(make({7}, {{0}}, flat(0.f), flat(0.5f)), PMX_ERR_INVALID);
    {
        pmx_model_desc d = {};
        pmxt_tables *t = nullptr;
        d.n_nodes = PMX_MAX_MODEL_NODES + 1;
        EXPECT(pmxt_tables_create(&d, &t) == PMX_ERR_INVALID && !t);
        d.n_nodes = 0, d.n_clusters = PMX_MAX_MODEL_CLUSTERS + 1;
        EXPECT(pmxt_tables_create(&d, &t) == PMX_ERR_INVALID && !t);
        EXPECT(pmxt_tables_create(nullptr, &t) == PMX_ERR_INVALID && pmxt_tables_create(&d, nullptr) == PMX_ERR_INVALID);
        EXPECT(pmxt_tables_destroy(nullptr) == PMX_OK);
    }
    std::printf("model_tables_main: %d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
