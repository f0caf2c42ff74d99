// pmx_model_tables.cpp - the host arithmetic behind a device model (pmx_model_tables.h). It decides, bit for bit, whether the engine
// agrees with the reference's float32 test abs((d - mean) / std) < 2 (match_utils.py:55-57): the kernels compare against the threshold,
// the windows and the per-cell majority windows computed here and never divide. Host only; compiled with -ffp-contract=off.
#include "pmx_model_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "pmx_error.h"

namespace pmx {
namespace {

// A set of model nodes (PMX_MAX_MODEL_NODES bits).
struct NodeSet {
    static constexpr int W = PMX_MAX_MODEL_NODES / 64;
    uint64_t w[W] = {};
    bool any() const { for (int i = 0; i < W; ++i) if (w[i]) return true; return false; }
    void set(int m) { w[m >> 6] |= 1ull << (m & 63); }
    bool operator==(const NodeSet &o) const { return std::memcmp(w, o.w, sizeof(w)) == 0; }
    NodeSet operator&(const NodeSet &o) const { NodeSet r; for (int i = 0; i < W; ++i) r.w[i] = w[i] & o.w[i]; return r; }
    std::vector<int> list() const { // ascending
        std::vector<int> v;
        for (int i = 0; i < W; ++i)
            for (uint64_t x = w[i]; x; x &= x - 1) v.push_back(i * 64 + __builtin_ctzll(x));
        return v;
    }
};

// Largest float T with fl(T / std) < 2 under round-to-nearest-even float32 division: the quotient
// rounds below 2 exactly when T / std < 2 - 2^-24, and std * (2 - 2^-24) is exact in double.
float pass_threshold(float std) {
    const double bound = (double)std * (2.0 - std::ldexp(1.0, -24));
    float t = (float)bound;
    if ((double)t >= bound) t = std::nextafterf(t, -INFINITY);
    return t;
}

// The floats d >= 0 with |fl(d - mean)| <= T, i.e. abs((d - mean) / std) < 2 in the reference's float32 arithmetic
// (match_utils.py:55-57; T = pass_threshold(std)). fl(d - mean) is monotonic in d, so the set is an interval of floats;
// its ends are found by bisection on the bit patterns (non-negative floats order like their bits).
bool edge_window(float mean, float T, float &lo, float &hi) {
    auto f32 = [](uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; };
    auto ge = [&](uint32_t b) { volatile float x = f32(b) - mean; return x >= -T; };
    auto le = [&](uint32_t b) { volatile float x = f32(b) - mean; return x <= T; };
    const uint32_t top = 0x7f7fffffu;
    if (!le(0u) || !ge(top)) return false;
    uint32_t a = 0, b = top; // smallest b with ge
    if (ge(0u)) b = 0;
    else {
        while (b - a > 1) {
            const uint32_t m = a + (b - a) / 2;
            if (ge(m)) b = m; else a = m;
        }
    }
    const uint32_t lo_b = b;
    a = 0, b = top; // largest a with le
    if (le(top)) a = top;
    else {
        while (b - a > 1) {
            const uint32_t m = a + (b - a) / 2;
            if (le(m)) a = m; else b = m;
        }
    }
    const uint32_t hi_b = a;
    if (lo_b > hi_b) return false;
    lo = f32(lo_b);
    hi = f32(hi_b);
    return true;
}

// The majority windows of one pair of node subsets A, B on the grid: out[ncell]. Returns the number of NaN cells.
uint64_t cell_windows(const ModelTables &t, const std::vector<int> &A, const std::vector<int> &B, F2 *out) {
    const float INF = INFINITY;
    if (A.empty() || B.empty()) { // no item: never a fail
        for (uint32_t i = 0; i < t.ncell; ++i) out[i] = F2{-INF, INF};
        return 0;
    }
    const int mn = (int)(A.size() * B.size());
    std::vector<std::pair<float, int>> ev;
    for (const int am : A)
        for (const int bm : B) {
            const int e = am * t.Nm + bm;
            if (!t.wok[e]) continue;
            ev.emplace_back(t.wlo[e], +1);
            ev.emplace_back(std::nextafterf(t.whi[e], INF), -1); // first float after the window
        }
    std::sort(ev.begin(), ev.end());
    std::vector<std::pair<float, float>> pass; // the runs of floats at which at least half of the node pairs pass
    int cnt = 0;
    bool in = false;
    float start = 0.f;
    for (size_t i = 0; i < ev.size();) {
        const float x = ev[i].first;
        for (; i < ev.size() && ev[i].first == x; ++i) cnt += ev[i].second;
        const bool ok = 2 * cnt >= mn; // num_pass >= num_match * 0.5 (match_utils.py:61)
        if (ok && !in) { in = true; start = x; }
        else if (!ok && in) { in = false; pass.emplace_back(start, std::nextafterf(x, -INF)); }
    }
    if (in) pass.emplace_back(start, INF);
    uint64_t n_complex = 0;
    for (uint32_t i = 0; i < t.ncell; ++i) {
        const float x0 = (float)i * t.h, x1 = (i + 1 == t.ncell) ? INF : (float)(i + 1) * t.h;
        int hits = 0;
        F2 w{INF, INF}; // never passes (no distance is >= INF; written so that lo <= hi holds for every window: the device's median-of-three test)
        for (const auto &pr : pass)
            if (pr.first < x1 && pr.second >= x0) {
                ++hits;
                w = F2{pr.first, pr.second};
            }
        if (hits > 1) {
            w = F2{NAN, NAN};
            ++n_complex;
        }
        out[i] = w;
    }
    return n_complex;
}

} // namespace

int build_model_tables(const pmx_model_desc *d, ModelTables *out) {
    if (!d || !out) return pmx_fail(PMX_ERR_INVALID, "null argument");
    const int Nm = d->n_nodes, K = d->n_clusters;
    if (Nm < 0 || Nm > PMX_MAX_MODEL_NODES) return pmx_fail(PMX_ERR_INVALID, "model has %d nodes (max %d)", Nm, PMX_MAX_MODEL_NODES);
    if (K < 0 || K > PMX_MAX_MODEL_CLUSTERS) return pmx_fail(PMX_ERR_INVALID, "model has %d clusters (max %d)", K, PMX_MAX_MODEL_CLUSTERS);
    for (int i = 0; i < Nm; ++i)
        if (d->node_type[i] >= PMX_NUM_TYPES) return pmx_fail(PMX_ERR_INVALID, "node %d has type id %d", i, d->node_type[i]);
    ModelTables t;
    t.Nm = Nm;
    t.K = K;
    const size_t n_edge = (size_t)Nm * Nm, n_pair = (size_t)K * K;

    // edges: the Gaussian's scale, the pass threshold and the exact pass window
    t.edge.resize(n_edge);
    t.wlo.resize(n_edge);
    t.whi.resize(n_edge);
    t.wok.resize(n_edge);
    const double s_const = std::sqrt(0.5 * 1.4426950408889634074); // sqrt(0.5 * log2(e))
    for (size_t i = 0; i < n_edge; ++i) {
        const float mean = d->edge_mean[i], sd = d->edge_std[i];
        if (!(sd > 0.f)) return pmx_fail(PMX_ERR_INVALID, "edge %zu has distance_std %g", i, (double)sd);
        const float T = pass_threshold(sd);
        t.edge[i] = F4{mean, (float)(s_const / (double)sd), T, sd};
        t.wok[i] = edge_window(mean, T, t.wlo[i], t.whi[i]) ? 1 : 0;
    }
    for (int a = 0; a < Nm && t.symmetric; ++a)
        for (int b = 0; b < a; ++b)
            if (std::memcmp(&d->edge_mean[a * Nm + b], &d->edge_mean[b * Nm + a], 4) || std::memcmp(&d->edge_std[a * Nm + b], &d->edge_std[b * Nm + a], 4)) {
                t.symmetric = 0;
                break;
            }

    // nodes by type and by cluster; the model clusters that share a type with a ligand type mask
    t.node_type.assign(PMX_MAX_MODEL_NODES, 0);
    NodeSet type_nodes[PMX_NUM_TYPES];
    for (int m = 0; m < Nm; ++m) {
        t.node_type[m] = d->node_type[m];
        type_nodes[d->node_type[m]].set(m);
    }
    std::vector<NodeSet> cnodes((size_t)std::max(K, 1));
    const int NW = std::max(1, (Nm + 63) / 64); // words per cluster in cluster_nodes
    for (int a = 0; a < K; ++a)
        for (int m = 0; m < Nm; ++m)
            if (d->cluster_nodes[(size_t)a * NW + (m >> 6)] >> (m & 63) & 1) cnodes[a].set(m);
    NodeSet tnodes[128];
    t.tclus.assign(2 * 128, 0);
    for (int mask = 0; mask < 128; ++mask) {
        for (int ty = 0; ty < PMX_NUM_TYPES; ++ty)
            if (mask >> ty & 1)
                for (int i = 0; i < NodeSet::W; ++i) tnodes[mask].w[i] |= type_nodes[ty].w[i];
        for (int a = 0; a < K; ++a)
            if (d->cluster_typemask[a] & mask) t.tclus[2 * mask + (a >> 6)] |= 1ull << (a & 63);
    }

    // cluster pairs: centre distance and size sum; the hull of the node pairs' windows (the dead-entry test of build_tables)
    t.cpair.resize(n_pair);
    t.cwin.resize(n_pair);
    std::vector<std::vector<int>> clist((size_t)K);
    for (int a = 0; a < K; ++a) clist[a] = cnodes[a].list();
    for (int a = 0; a < K; ++a)
        for (int b = 0; b < K; ++b) {
            const double *ca = d->cluster_center + 3 * a, *cb = d->cluster_center + 3 * b;
            const double dist = std::sqrt((ca[0] - cb[0]) * (ca[0] - cb[0]) + (ca[1] - cb[1]) * (ca[1] - cb[1]) +
                                          (ca[2] - cb[2]) * (ca[2] - cb[2])); // graph_match.py:263-264
            t.cpair[a * K + b] = F2{(float)dist, (float)(d->cluster_size[a] + d->cluster_size[b])}; // :265
            float lo = INFINITY, hi = -INFINITY;
            for (const int am : clist[a])
                for (const int bm : clist[b]) {
                    const size_t e = (size_t)am * Nm + bm;
                    if (!t.wok[e]) continue;
                    lo = std::min(lo, t.wlo[e]);
                    hi = std::max(hi, t.whi[e]);
                }
            t.cwin[a * K + b] = F2{lo, hi};
        }

    // node subsets
    std::vector<NodeSet> subs(1);
    t.sidtab.assign((size_t)std::max(K, 1) * 128, 0);
    for (int a = 0; a < K; ++a)
        for (int mask = 0; mask < 128; ++mask) {
            const NodeSet nodes = cnodes[a] & tnodes[mask];
            if (!nodes.any()) continue;
            size_t id = 1;
            for (; id < subs.size(); ++id)
                if (subs[id] == nodes) break;
            if (id == subs.size()) subs.push_back(nodes);
            t.sidtab[(size_t)a * 128 + mask] = (uint16_t)id;
        }
    const uint32_t NS = (uint32_t)subs.size();
    if (NS > 65535u) return pmx_fail(PMX_ERR_INVALID, "model has %u distinct node subsets (max 65535)", NS);
    std::vector<std::vector<int>> sublist(NS);
    t.sub_off.assign(NS + 1, 0);
    for (uint32_t s = 0; s < NS; ++s) {
        sublist[s] = subs[s].list();
        t.sub_off[s] = (uint32_t)t.sub_nodes.size();
        for (int x : sublist[s]) t.sub_nodes.push_back((uint8_t)x);
    }
    t.sub_off[NS] = (uint32_t)t.sub_nodes.size();
    if (t.sub_nodes.empty()) t.sub_nodes.push_back(0);

    // grid: h = the largest power of two <= std_min / 4 (quintic Hermite error < 6e-8 of the peak, measured), range to mean + 7 std
    float std_min = 1e30f, dmax = 1.f;
    for (size_t i = 0; i < n_edge; ++i) {
        std_min = std::min(std_min, d->edge_std[i]);
        dmax = std::max(dmax, d->edge_mean[i] + 7.0f * d->edge_std[i]);
    }
    if (Nm == 0) std_min = 1.f;
    float h = 0.5f;
    while (h > std_min / 4.f && h > 1.f / 64.f) h *= 0.5f;
    const uint32_t ncell = (uint32_t)std::ceil((double)dmax / (double)h) + 1;
    if (ncell > 16384 || (uint64_t)NS * NS * ncell * kFnCellBytes >= (4ull << 30)) // (the kernels address the table with 32-bit byte offsets)
        return pmx_fail(PMX_ERR_INVALID, "pair-function tables of this model would take %llu cells x %u x %u subsets", (unsigned long long)ncell, NS, NS);
    t.NS = NS;
    t.ncell = ncell;
    t.h = h;

    // a symmetric model (edge[m][n] == edge[n][m]: distances are) has F_(A,B) == F_(B,A): the pair (lo, hi) is stored once
    const bool tri = t.symmetric != 0;
    t.NF = tri ? NS * (NS + 1) / 2 : NS * NS;
    t.win.resize((size_t)t.NF * ncell);
    for (uint32_t sa = 0; sa < NS; ++sa)
        for (uint32_t sb = 0; sb < (tri ? sa + 1 : NS); ++sb)
            t.n_complex_cells += cell_windows(t, sublist[sa], sublist[sb], t.win.data() + (size_t)(tri ? sa * (sa + 1) / 2 + sb : sa * NS + sb) * ncell);
    *out = std::move(t);
    return PMX_OK;
}

} // namespace pmx

// ------------------------------------------------------------------------------------------ test hook
struct pmxt_tables {
    pmx::ModelTables t;
};

extern "C" int pmxt_tables_create(const pmx_model_desc *desc, pmxt_tables **out) {
    if (!out) return pmx_fail(PMX_ERR_INVALID, "null argument");
    pmxt_tables *p = new pmxt_tables();
    const int rc = pmx::build_model_tables(desc, &p->t);
    if (rc != PMX_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return PMX_OK;
}

extern "C" int pmxt_tables_view_get(const pmxt_tables *p, pmxt_tables_view *v) {
    if (!p || !v) return pmx_fail(PMX_ERR_INVALID, "null argument");
    const pmx::ModelTables &t = p->t;
    v->Nm = t.Nm, v->K = t.K, v->symmetric = t.symmetric;
    v->NS = t.NS, v->NF = t.NF, v->ncell = t.ncell;
    v->h = t.h;
    v->n_complex_cells = t.n_complex_cells;
    auto floats = [](const auto &vec) { return reinterpret_cast<const float *>(vec.data()); };
    v->edge = floats(t.edge), v->cpair = floats(t.cpair), v->cwin = floats(t.cwin), v->win = floats(t.win);
    v->wlo = t.wlo.data(), v->whi = t.whi.data();
    v->node_type = t.node_type.data(), v->sub_nodes = t.sub_nodes.data(), v->wok = t.wok.data();
    v->tclus = t.tclus.data();
    v->sidtab = t.sidtab.data();
    v->sub_off = t.sub_off.data();
    v->n_edge = t.edge.size(), v->n_cpair = t.cpair.size(), v->n_cwin = t.cwin.size(), v->n_win = t.win.size();
    v->n_node_type = t.node_type.size(), v->n_sub_nodes = t.sub_nodes.size(), v->n_tclus = t.tclus.size(), v->n_sidtab = t.sidtab.size(), v->n_sub_off = t.sub_off.size();
    return PMX_OK;
}

extern "C" int pmxt_tables_destroy(pmxt_tables *p) {
    delete p;
    return PMX_OK;
}
