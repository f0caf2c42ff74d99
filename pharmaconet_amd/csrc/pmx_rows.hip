// pmx_rows.hip - the kernels that answer a question about listed (ligand, conformer, key) rows, on gfx950: pmx_attribute, pmx_hotspots and
// pmx_align (include/pmx.h). One wavefront handles one row, and all kernels open a row the same way (open_row, pmx_rows_front.h - shared with pmx_pose_fit.hip): the ligand's record, its type masks,
// its tree levels with the candidates of each (the level rule of pmx_screen_tables.h), and the key checked against them.
//
// pmx_screen_tables.h is compiled here once more, as namespace pmx_r, for parse_record, the level rule, the wavefront helpers, center_size
// and exact_value. Nothing else of the screening path is part of this translation unit: no score table is built, no tabulated pair function
// is read, no slice or arena is used.
//
// attribute_row - which ligand nodes carry a leaf's total: the matrix of self and pair entries the reference's tree adds up for that leaf
// (match_utils.py:9-122 behind graph_match.py:139-172, :263-268), the number of failing node pairs per pair entry, the leaf's total in the
// product walker's order, and the share of every ligand node. Every node-pair term is evaluated one by one in the reference's float32
// operations (exact_value), so the answer does not depend on PMX_TAILS_RATIO or on the rough-cell flags of the tabulated functions. Five
// steps after open_row, which hand over through the wavefront's LDS (all but `nodes` are leaf_steps, which hotspots_row runs too):
//   centres   lane c = conformer c: centre and size of every matched level's cluster, then the cluster-distance prefilter of every
//             pair of matched levels (it fails only when it fails for every conformer: one ballot)
//   terms     lane u = node u: term(u, v) and fail(u, v) for every later listed node v, into term[u][v] and one fail mask per node
//   entries   lane e = entry (l1, l2): the float32 sum in the reference's order (itertools.combinations / product), the fails, -1
//             where the reference says no match, and the float64 sum of the same terms
//   nodes     lane u = node u: half of every term the node is part of, in ascending order of the other node, in float64
//   total     the entries in the product walker's order
// The shares add up to the total: an entry is a float32 accumulation, so the float64 sum of its terms differs from it by float32
// rounding (relative 1e-7). Each term is therefore weighted by entry / (float64 sum of the entry's terms) - 1 to within that rounding -
// which spreads the entry's rounding residual over its terms in proportion: sum_u node[u] = sum of the entries = total to float64 rounding.
//
// align_row - where a binding mode sits in the pocket: the proper rotation R and translation t that bring the matched ligand nodes onto
// the pharmacophore points of the model nodes they are matched to, in the weighted least-squares sense, with the residuals of that fit.
// The reference scores distances only and has no counterpart; the correspondence is the match list of graph_match.py:139-172.
//   pairs     lane u = ligand node u: the node subset of (matched model cluster, type mask of u) is exactly the model nodes m that pair with
//             u, in ascending order (sidtab / sub_nodes: the cluster's node words and the type's node words, intersected when the model was
//             created - any number of node words, so models above 64 nodes need nothing special). The lane adds up W_u = sum w and sum w y_m.
//   sums      W, the centroids and S = sum_u (x_u - xbar) (sum_m w y_m - W_u ybar)^T by xor butterflies: lanes i and i ^ k add the same two
//             numbers, so every lane ends with the same bits and everything after it is wave-uniform
//   fit       Horn's 4x4 matrix of S, cyclic Jacobi (at most kSweeps sweeps; the exit test reads wave-uniform numbers), R from the unit quaternion
//   residuals lane u walks its model nodes again: sum w |R x_u + t - y_m|^2 and sum w |y_m - ybar|^2 from the points themselves (sum w |y_m|^2
//             minus the centroid's square would lose |y|^2 / E0 of the precision: pocket coordinates are tens of Angstrom from the origin)
// Several targets per node: sum_m w |p - y_m|^2 = W_u |p - ybar_u|^2 + sum_m w |y_m - ybar_u|^2 for any point p, so the fit sees node u
// as one point ybar_u of weight W_u and the second sum is a constant of the row (sse - rmsd_nodes^2 W).
//
// hotspots_row - which model nodes carry the same total: attribute_row's steps up to the entries and the total (leaf_steps, shared), then
// the model-side step described where it stands.
//
// In no kernel does a lane add to another lane's sum, and there is no floating-point atomic: the same call gives the same bits.
#include <hip/hip_runtime.h>

#define PMX_NS pmx_r
#include "pmx_screen_tables.h"
#include "pmx_rows.h"
#include "pmx_rows_front.h" // RowLds, open_row, row_node_subset, row_status: the row front end

namespace pmx_r {

__device__ __forceinline__ void write_row_header(const Rows &rows, const RowLds &L, uint32_t li, int status) {
    const int lane = lane_id();
    if (lane < kL) rows.levels[(size_t)li * kL + lane] = L.lev[lane];
    if (lane == 0) rows.status[li] = status;
}

// Persistent wavefronts over the call's rows: f(li) for the rows this one draws.
template <class F>
__device__ __forceinline__ void for_each_row(const Rows &rows, F f) {
    for (;;) {
        const int lane = lane_id();
        uint32_t next = 0;
        if (lane == 0) next = atomicAdd(rows.cursor, 1u);
        next = (uint32_t)uni((int)next);
        if (next >= rows.n) break;
        f(next);
    }
}

// ------------------------------------------------------------------------------------------------ attribution
constexpr int kTS = kN + 1; // row stride of the term matrix: lane u writes term[u][v] for a uniform v, and 65 floats apart they land in 64 banks

// LDS of the wavefront (static)
constexpr uint32_t kAtR = 0;                                // float4 ctr[kL][64] {centre, size} per level and conformer; then float term[kN][kTS]
constexpr uint32_t kRBytes = kL * 64 * 16 > kN * kTS * 4 ? kL * 64 * 16 : kN * kTS * 4;
constexpr uint32_t kAtPos = kAtR + kRBytes;                // float4 [kN]: the nodes' positions in the row's conformer
constexpr uint32_t kAtScale = kAtPos + kN * 16;            // double [kL][kL]: entry / float64 sum of its terms
constexpr uint32_t kAtFailm = kAtScale + kL * kL * 8;      // u64 [kN]: bit v of word u = fail(u, v), v > u
constexpr uint32_t kAtRow = kAtFailm + kN * 8;             // RowLds
constexpr uint32_t kAtEnt = kAtRow + sizeof(RowLds);       // float [kL][kL]: the entries as they are written
constexpr uint32_t kAtPf = kAtEnt + kL * kL * 4;           // u32 [kL]: bit l2 of word l1 = the prefilter lets (l1, l2) pass
constexpr uint32_t kAtFc = kAtPf + kL * 4;                 // u16 [kL][kL]: failing node pairs
constexpr uint32_t kAtSid = kAtFc + kL * kL * 2;           // u16 [kN]: node subset of the node under its level's match (0: not in the match list)
constexpr uint32_t kAtNlv = kAtSid + kN * 2;               // u8 [kN]: the node's level (kNoMatch: not in a match list)
constexpr uint32_t kAttributeLds = kAtNlv + kN;
static_assert(kAtScale % 8 == 0 && kAtFailm % 8 == 0 && kAtRow % 8 == 0 && kAtEnt % 4 == 0 && kAtPf % 4 == 0 && kAtFc % 2 == 0 && kAtSid % 2 == 0, "LDS alignment");
static_assert(kAttributeLds <= 64 * 1024, "LDS of a work-group");

// The wavefront's LDS as the steps below see it.
struct LeafLds {
    float4 *ctr;
    float *term;
    float4 *pos;
    double *scale;
    unsigned long long *failm;
    RowLds &L;
    float *ent;
    uint32_t *pf;
    uint16_t *fc, *sid;
    uint8_t *nlv;
    __device__ explicit LeafLds(unsigned char *lds)
        : ctr(reinterpret_cast<float4 *>(lds + kAtR)), term(reinterpret_cast<float *>(lds + kAtR)), pos(reinterpret_cast<float4 *>(lds + kAtPos)),
          scale(reinterpret_cast<double *>(lds + kAtScale)), failm(reinterpret_cast<unsigned long long *>(lds + kAtFailm)),
          L(*reinterpret_cast<RowLds *>(lds + kAtRow)), ent(reinterpret_cast<float *>(lds + kAtEnt)), pf(reinterpret_cast<uint32_t *>(lds + kAtPf)),
          fc(reinterpret_cast<uint16_t *>(lds + kAtFc)), sid(reinterpret_cast<uint16_t *>(lds + kAtSid)), nlv(lds + kAtNlv) {}
};

// What the shared steps leave behind them, next to the LDS: the row, the lane's own node, and the leaf's verdict and total.
struct Leaf {
    Row w;
    int mylev;      // tree level of node `lane`
    uint32_t mysid; // its node subset under its level's match (0: not in a match list)
    bool dead;      // some pair entry between matched levels is not > 0
    double total;
};

// Index of (u, v), u < v < kN, in a triangular array of kN (kN - 1) / 2.
__device__ __forceinline__ int tri_index(int u, int v) { return ((u * (2 * kN - u - 1)) >> 1) + (v - u - 1); }

// G(u, v) of pmx_hotspots: the float64 sum, in the order of itertools.product, of the float32 addends exact_value forms for the node pair.
__device__ __forceinline__ double inner_sum(const ScreenParams &p, uint32_t sidu, uint32_t sidv, float d) {
    const uint8_t *A = p.sub_nodes + p.sub_off[sidu], *B = p.sub_nodes + p.sub_off[sidv];
    const int nA = (int)(p.sub_off[sidu + 1] - p.sub_off[sidu]), nB = (int)(p.sub_off[sidv + 1] - p.sub_off[sidv]);
    double G = 0.0;
    for (int ia = 0; ia < nA; ++ia) {
        const int m = A[ia];
        const float wa = p.W.w[p.M.node_type[m]];
        for (int ib = 0; ib < nB; ++ib) {
            const int n = B[ib];
            const float4 e = p.M.edge[m * p.M.Nm + n]; // {mean, s, T, std}
            const float z = (d - e.x) / e.w;
            const float wos = (wa * p.W.w[p.M.node_type[n]]) / e.w;
            const float g = wos * expf(-0.5f * (z * z));
            G = G + (double)g;
        }
    }
    return G;
}

// Row li of the call through open_row and the steps centres, terms, entries and total: what pmx_attribute and pmx_hotspots share. With
// `gsum` (pmx_hotspots) the terms step also leaves G(u, v) of every evaluated node pair in gsum[tri_index(u, v)].
template <bool WITH_G>
__device__ __forceinline__ Leaf leaf_steps(const ScreenParams &p, const Rows &rows, const LeafLds &S, double *gsum, uint32_t li) {
    const int lane = lane_id();
    float4 *ctr = S.ctr;
    float *term = S.term;
    float4 *pos = S.pos;
    double *scale = S.scale;
    unsigned long long *failm = S.failm;
    RowLds &L = S.L;
    float *ent = S.ent;
    uint32_t *pf = S.pf;
    uint16_t *fc = S.fc;
    uint16_t *sid = S.sid;
    uint8_t *nlv = S.nlv;
    const uint8_t *ls = L.ls, *le = L.le, *keyl = L.key;

    // ---- the row as for a ligand without levels
    for (int e = lane; e < kL * kL; e += 64) {
        ent[e] = 0.f;
        fc[e] = 0;
    }
    sid[lane] = 0;
    nlv[lane] = kNoMatch;
    Leaf f;
    f.w = open_row(p, rows, L, li);
    f.mylev = -1, f.mysid = 0u, f.dead = false, f.total = 0.0;
    const Row &w = f.w;
    const Record &r = w.r;
    const int n = w.n, C = w.C, nl = w.nl, c = w.c;

    // (entries are reported for a key with a match that is no candidate, too: that match counts as None; the row is invalid)
    if (w.compute) {
        GlobalFloats xyz = (GlobalFloats)uniptr(r.xyz);
        // ---- nodes: level, subset under the level's match, position in conformer c
        const NodeSubset me = row_node_subset(p, w, L, lane);
        const int mylev = me.lev;
        const uint32_t mysid = me.sid;
        f.mylev = mylev, f.mysid = mysid;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (lane < n) {
            const uint32_t o = (uint32_t)(lane * 3 * C + c);
            px = xyz[o], py = xyz[o + C], pz = xyz[o + 2 * C];
            pos[lane] = make_float4(px, py, pz, 0.f);
        }
        sid[lane] = (uint16_t)mysid;
        nlv[lane] = mysid != 0u ? (uint8_t)mylev : kNoMatch;

        // ---- centres (lane = conformer; lanes past C hold copies of conformer C - 1) and the prefilter of graph_match.py:263-268
        const int cc = lane < C ? lane : C - 1;
        for (int l = 0; l < nl; ++l) {
            if (uni((int)keyl[l]) == kNoMatch) continue;
            Pos3 ct;
            float size;
            center_size(xyz, C, uni((int)ls[l]), uni((int)le[l]), cc, ct, size);
            ctr[l * 64 + lane] = make_float4(ct.x, ct.y, ct.z, size);
        }
        wave_sync();
        const int K = p.M.K;
        for (int l1 = 0; l1 < nl; ++l1) {
            const int a1 = uni((int)keyl[l1]);
            uint32_t bits = 0;
            if (a1 != kNoMatch) {
                const float4 A = ctr[l1 * 64 + lane];
                for (int l2 = l1 + 1; l2 < nl; ++l2) {
                    const int a2 = uni((int)keyl[l2]);
                    if (a2 == kNoMatch) continue;
                    const float4 B = ctr[l2 * 64 + lane];
                    const float ldist = norm3f(A.x - B.x, A.y - B.y, A.z - B.z); // graph_match.py:240
                    const float lsize = A.w + B.w;                               // :241
                    const float2 mp = p.M.cpair[a1 * K + a2];
                    const bool pass = lane < C && !((fabsf(ldist - mp.x) - lsize) > mp.y);
                    bits |= __ballot(pass) != 0ull ? 1u << l2 : 0u;
                }
            }
            if (lane == 0) pf[l1] = bits;
        }
        wave_sync(); // (the centres are read: their room becomes the term matrix)

        // ---- terms: lane u evaluates (u, v) for the listed nodes v behind it - record order is level order, so u is the first node of the pair
        unsigned long long fm = 0ull;
        for (int v = 1; v < n; ++v) {
            const uint32_t sv = (uint32_t)uni((int)sid[v]);
            if (sv == 0u) continue;
            if (mysid != 0u && lane < v) {
                const float4 Q = pos[v];
                const float d = norm3f(px - Q.x, py - Q.y, pz - Q.z);
                int np, mn;
                term[lane * kTS + v] = exact_value(p, mysid, sv, d, np, mn);
                fm |= 2 * np < mn ? 1ull << v : 0ull; // match_utils.py:56-61
                if (WITH_G) gsum[tri_index(lane, v)] = inner_sum(p, mysid, sv, d);
            }
        }
        failm[lane] = fm;
        wave_sync();

        // ---- entries: lane e = (l1, l2), l1 <= l2, both matched
        bool dead_pair = false;
        for (int e0 = 0; e0 < kL * kL; e0 += 64) {
            const int e = e0 + lane;
            const int l1 = e / kL, l2 = e - l1 * kL;
            if (!(e < kL * kL && l1 <= l2 && l2 < nl)) continue;
            if (keyl[l1] == kNoMatch || keyl[l2] == kNoMatch) continue;
            const int s1 = ls[l1], e1 = le[l1], s2 = ls[l2], e2 = le[l2];
            float acc = 0.f;
            double accd = 0.0;
            int fails = 0, n1 = 0, n2 = 0;
            for (int v = s2; v < e2; ++v) n2 += sid[v] != 0 ? 1 : 0;
            for (int u = s1; u < e1; ++u) {
                if (sid[u] == 0) continue;
                ++n1;
                const unsigned long long fu = failm[u];
                for (int v = l1 == l2 ? u + 1 : s2; v < e2; ++v) {
                    if (sid[v] == 0) continue;
                    const float t = term[u * kTS + v];
                    acc = acc + t; // float32, in the order of itertools.combinations / product (match_utils.py:26-28, :87)
                    accd += (double)t;
                    fails += (int)((fu >> v) & 1ull);
                }
            }
            float value = acc;
            if (l1 != l2) { // (a self entry has no majority test)
                if (!((pf[l1] >> l2) & 1u) || 2 * fails > n1 * n2) value = -1.f; // graph_match.py:263-268 | match_utils.py:71-74
                dead_pair = dead_pair || !(value > 0.f);                          // tree.py:81 (NaN: not > 0)
                fc[e] = (uint16_t)fails;
            }
            ent[e] = value;
            scale[e] = accd != 0.0 ? (double)value / accd : 0.0;
        }
        f.dead = __ballot(dead_pair) != 0ull;
        wave_sync();

        // ---- the total as the product walker sums it: (running + self) + (pair entries with the matched ancestors, shallowest first)
        double total = 0.0;
        for (int l = 0; l < nl; ++l) {
            if (uni((int)keyl[l]) == kNoMatch) continue;
            double sum = 0.0;
            for (int l0 = 0; l0 < l; ++l0)
                if (uni((int)keyl[l0]) != kNoMatch) sum += (double)ent[l0 * kL + l];
            total = (total + (double)ent[l * kL + l]) + sum;
        }
        f.total = total;
    }
    return f;
}

// Row li of the call.
__device__ void attribute_row(const ScreenParams &p, const pmx_rows::AttributeArgs &a, unsigned char *lds, uint32_t li) {
    const int lane = lane_id();
    const LeafLds S(lds);
    const Leaf f = leaf_steps<false>(p, a.rows, S, nullptr, li);
    const float *term = S.term, *ent = S.ent;
    const double *scale = S.scale;

    // ---- node shares
    double share = 0.0;
    if (f.w.compute && f.mysid != 0u) {
        for (int v = 0; v < f.w.n; ++v) {
            const int lv = uni((int)S.nlv[v]);
            if (lv == kNoMatch) continue;
            if (v != lane) {
                const float t = v > lane ? term[lane * kTS + v] : term[v * kTS + lane];
                share += (double)t * scale[min(f.mylev, lv) * kL + max(f.mylev, lv)];
            }
        }
        share *= 0.5;
    }

    // ---- the row
    const int status = row_status(f.w, f.dead);
    const double nan = __builtin_nan("");
    a.node[(size_t)li * kN + lane] = status == PMX_LIGAND_OK ? share : nan;
    for (int e = lane; e < kL * kL; e += 64) {
        a.entry[(size_t)li * kL * kL + e] = ent[e];
        a.fails[(size_t)li * kL * kL + e] = S.fc[e];
    }
    if (lane == 0) a.total[li] = status == PMX_LIGAND_OK ? f.total : nan;
    write_row_header(a.rows, S.L, li, status);
    wave_sync(); // (the next row starts by clearing this LDS)
}

__global__ __launch_bounds__(64) void attribute_kernel(const ScreenParams p, const pmx_rows::AttributeArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kAttributeLds];
    for_each_row(a.rows, [&](uint32_t li) { attribute_row(p, a, lds, li); });
}

// ------------------------------------------------------------------------------------------------ hotspots
// hotspots_row - which model nodes carry a leaf's total: leaf_steps as above, with G(u, v) kept per node pair, then the model-side step.
//   masks     lane u = node u: its node subset as a bit per model node, PMX_FINGERPRINT_WORDS words
//   hotspots  lane = model node m = lane + 64 j (a register set per node word j): the listed node pairs (u, v) are walked wave-uniformly, in
//             ascending (u, v); a lane whose m is in u's subset walks v's subset in ascending order and adds up the pair's inner terms
//             (m, m') in float64, a lane whose m is in v's subset walks u's; the sums are weighted by term(u, v) scale[e] / (2 G(u, v)).
//             Every inner term is evaluated once from each side, and no lane adds to another lane's sum.
constexpr int kW = PMX_FINGERPRINT_WORDS;
static_assert(kW * 64 == PMX_MAX_MODEL_NODES && kW == 4, "a lane per model node and node word");
constexpr uint32_t kHsG = (kAttributeLds + 7u) & ~7u;             // double [kN (kN - 1) / 2]: G(u, v), tri_index
constexpr uint32_t kHsMask = kHsG + (kN * (kN - 1) / 2) * 8;      // u64 [kN][kW]: the model nodes of each listed node's subset
constexpr uint32_t kHotspotsLds = kHsMask + kN * kW * 8;
static_assert(kHotspotsLds <= 64 * 1024, "LDS of a work-group");

// The inner terms of one side: model node m (in one node's subset) against the other node's subset `other` (ascending). SWAP: m is the
// second index of the model edge (m is on v's side). Adds the float32 addends to `sum` in float64 and counts terms and passes.
template <bool SWAP>
__device__ __forceinline__ void inner_side(const ScreenParams &p, int m, const unsigned long long *other, int nw, float d, double &sum, uint32_t &terms, uint32_t &pass) {
    const float wm = p.W.w[p.M.node_type[m]];
    for (int j = 0; j < nw; ++j) {
        unsigned long long bits = other[j];
        while (bits != 0ull) {
            const int o = 64 * j + (int)__builtin_ctzll(bits);
            bits &= bits - 1ull;
            const float wo = p.W.w[p.M.node_type[o]];
            const float4 e = SWAP ? p.M.edge[o * p.M.Nm + m] : p.M.edge[m * p.M.Nm + o]; // {mean, s, T, std}
            const float t = d - e.x, z = t / e.w;
            const float wos = (SWAP ? wo * wm : wm * wo) / e.w;
            const float g = wos * expf(-0.5f * (z * z));
            sum = sum + (double)g;
            terms += 1u;
            pass += fabsf(t) <= e.z ? 1u : 0u; // == abs(z) < 2 (pmx_device.h)
        }
    }
}

// Row li of the call.
__device__ void hotspots_row(const ScreenParams &p, const pmx_rows::HotspotArgs &a, unsigned char *lds, uint32_t li) {
    const int lane = lane_id();
    const LeafLds S(lds);
    double *gsum = reinterpret_cast<double *>(lds + kHsG);
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(lds + kHsMask);
    const Leaf f = leaf_steps<true>(p, a.rows, S, gsum, li);
    const int status = row_status(f.w, f.dead);
    const int Nm = p.M.Nm, nw = (Nm + 63) >> 6; // (a model has at most PMX_MAX_MODEL_NODES nodes: nw <= kW)

    double hs[kW] = {0.0, 0.0, 0.0, 0.0};
    uint32_t tc[kW] = {0u, 0u, 0u, 0u}, pc[kW] = {0u, 0u, 0u, 0u};
    if (status == PMX_LIGAND_OK) {
        // ---- masks
        unsigned long long mw[kW] = {0ull, 0ull, 0ull, 0ull};
        if (f.mysid != 0u) {
            for (uint32_t k = p.sub_off[f.mysid]; k < p.sub_off[f.mysid + 1u]; ++k) {
                const int m = p.sub_nodes[k];
#pragma unroll
                for (int j = 0; j < kW; ++j) mw[j] |= (m >> 6) == j ? 1ull << (m & 63) : 0ull;
            }
        }
#pragma unroll
        for (int j = 0; j < kW; ++j) mask[lane * kW + j] = mw[j];
        wave_sync();

        // ---- hotspots
        const int n = f.w.n;
        for (int u = 0; u + 1 < n; ++u) {
            const int lu = uni((int)S.nlv[u]);
            if (lu == kNoMatch) continue;
            const float4 P = S.pos[u];
            const unsigned long long *mu = mask + u * kW;
            for (int v = u + 1; v < n; ++v) {
                const int lv = uni((int)S.nlv[v]);
                if (lv == kNoMatch) continue;
                const float4 Q = S.pos[v];
                const float d = norm3f(P.x - Q.x, P.y - Q.y, P.z - Q.z); // (the operands and the operations of the terms step)
                const double G = gsum[tri_index(u, v)];
                const double coef = G != 0.0 ? (0.5 * ((double)S.term[u * kTS + v] * S.scale[min(lu, lv) * kL + max(lu, lv)])) / G : 0.0;
                const unsigned long long *mv = mask + v * kW;
#pragma unroll
                for (int j = 0; j < kW; ++j) {
                    if (j >= nw) continue;
                    const int m = lane + 64 * j;
                    if ((mu[j] >> lane) & 1ull) {
                        double sum = 0.0;
                        inner_side<false>(p, m, mv, nw, d, sum, tc[j], pc[j]);
                        hs[j] = hs[j] + coef * sum;
                    }
                    if ((mv[j] >> lane) & 1ull) {
                        double sum = 0.0;
                        inner_side<true>(p, m, mu, nw, d, sum, tc[j], pc[j]);
                        hs[j] = hs[j] + coef * sum;
                    }
                }
            }
        }
    }

    // ---- the row
    const double nan = __builtin_nan("");
    unsigned long long fp[kW];
#pragma unroll
    for (int j = 0; j < kW; ++j) {
        const size_t o = (size_t)li * PMX_MAX_MODEL_NODES + (size_t)(lane + 64 * j);
        a.hotspot[o] = status == PMX_LIGAND_OK ? hs[j] : nan;
        a.terms[o] = tc[j];
        a.pass[o] = pc[j];
        fp[j] = __ballot(tc[j] > 0u && 2u * pc[j] >= tc[j]); // match_utils.py:56-61, per hotspot
    }
    if (lane == 0) {
        a.total[li] = status == PMX_LIGAND_OK ? f.total : nan;
#pragma unroll
        for (int j = 0; j < kW; ++j) a.fingerprint[(size_t)li * kW + j] = fp[j];
    }
    write_row_header(a.rows, S.L, li, status);
    wave_sync(); // (the next row starts by clearing this LDS)
}

__global__ __launch_bounds__(64) void hotspots_kernel(const ScreenParams p, const pmx_rows::HotspotArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kHotspotsLds];
    for_each_row(a.rows, [&](uint32_t li) { hotspots_row(p, a, lds, li); });
}

// ------------------------------------------------------------------------------------------------ rigid fit
constexpr int kSweeps = 32; // a 4x4 symmetric matrix is diagonal to the last bit after 6 to 8 sweeps

// The wavefront's sum in every lane, the same bits in each: at step k lanes i and i ^ k both form v_i + v_(i ^ k).
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) v = v + __shfl_xor(v, k);
    return v;
}
__device__ inline int wave_sum(int v) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) v = v + __shfl_xor(v, k);
    return v;
}

// Eigenvalues d and eigenvectors (columns of v) of the symmetric 4x4 matrix a (upper triangle read, destroyed): cyclic Jacobi with the
// threshold and the negligible-element rule of Rutishauser's procedure. Every index is a constant after unrolling: registers only.
__device__ inline void jacobi4(double (&a)[4][4], double (&d)[4], double (&v)[4][4]) {
    double b[4], z[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
        b[i] = d[i] = a[i][i];
        z[i] = 0.0;
    }
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        double sm = 0.0;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) sm = sm + fabs(a[p][q]);
        if (sm == 0.0) break;
        const double tresh = sweep < 3 ? 0.2 * sm / 16.0 : 0.0;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double g = 100.0 * fabs(a[p][q]);
                if (sweep > 3 && fabs(d[p]) + g == fabs(d[p]) && fabs(d[q]) + g == fabs(d[q])) {
                    a[p][q] = 0.0;
                } else if (fabs(a[p][q]) > tresh) {
                    double h = d[q] - d[p], t;
                    if (fabs(h) + g == fabs(h)) {
                        t = a[p][q] / h;
                    } else {
                        const double theta = 0.5 * h / a[p][q];
                        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
                        t = theta < 0.0 ? -t : t;
                    }
                    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
                    h = t * a[p][q];
                    z[p] = z[p] - h, z[q] = z[q] + h;
                    d[p] = d[p] - h, d[q] = d[q] + h;
                    a[p][q] = 0.0;
                    const auto rot = [s, tau](double &x, double &y) {
                        const double gx = x, hy = y;
                        x = gx - s * (hy + gx * tau);
                        y = hy + s * (gx - hy * tau);
                    };
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (j < p) rot(a[j][p], a[j][q]);
                        else if (j > p && j < q) rot(a[p][j], a[j][q]);
                        else if (j > q) rot(a[p][j], a[q][j]);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) rot(v[j][p], v[j][q]);
                }
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            b[i] = b[i] + z[i];
            d[i] = b[i];
            z[i] = 0.0;
        }
    }
}

// Row li of the call.
__device__ void align_row(const ScreenParams &p, const pmx_rows::AlignArgs &a, RowLds &L, uint32_t li) {
    const int lane = lane_id();
    const Row w = open_row(p, a.rows, L, li); // (the key need not be a leaf of the tree: nothing is scored)
    const Record &r = w.r;
    const int n = w.n, C = w.C, c = w.c;
    const int status = row_status(w, false);

    double R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}}, t[3] = {0.0, 0.0, 0.0};
    double W = 0.0, sse = 0.0, rn = 0.0, e0 = 0.0, gap = 0.0, dev = -1.0;
    int nfit = 0, npairs = 0;
    if (status == PMX_LIGAND_OK) {
        // ---- pairs: the lane's node against the model nodes of its level's match that share a type with it, in model-node order
        uint32_t k0 = 0, k1 = 0;
        double x[3] = {0.0, 0.0, 0.0}, wu = 0.0, sy[3] = {0.0, 0.0, 0.0};
        int np = 0;
        if (lane < n) {
            const uint32_t sid = row_node_subset(p, w, L, lane).sid;
            if (sid != 0u) k0 = p.sub_off[sid], k1 = p.sub_off[sid + 1u];
            const uint32_t o = (uint32_t)(lane * 3 * C + c);
            x[0] = (double)r.xyz[o], x[1] = (double)r.xyz[o + C], x[2] = (double)r.xyz[o + 2 * C];
        }
        for (uint32_t k = k0; k < k1; ++k) {
            const uint32_t m = p.sub_nodes[k];
            const double w = (double)p.W.w[p.M.node_type[m]];
            if (!(w > 0.0)) continue;
            wu = wu + w;
#pragma unroll
            for (int j = 0; j < 3; ++j) sy[j] = sy[j] + w * a.center[3u * m + j];
            ++np;
        }
        const bool fitted = np > 0;
        nfit = (int)__popcll(__ballot(fitted));
        npairs = wave_sum(np);
        W = wave_sum(wu);
        if (npairs > 0) {
            // ---- centroids and the cross-covariance (an unfitted lane adds exact zeros whatever its position holds)
            double xb[3], yb[3], dx[3], ty[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                xb[j] = wave_sum(fitted ? wu * x[j] : 0.0) / W;
                yb[j] = wave_sum(sy[j]) / W;
                dx[j] = x[j] - xb[j];
                ty[j] = sy[j] - wu * yb[j];
            }
            double S[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double s = wave_sum(fitted ? dx[i] * ty[j] : 0.0);
                    S[i][j] = nfit >= 2 ? s : 0.0; // (one node: its own centroid, S is rounding noise; R = I exactly)
                }
            // ---- Horn's matrix, its eigenvalues, the quaternion of the largest (lowest index on equal eigenvalues: N = 0 gives (1, 0, 0, 0))
            double N[4][4], d[4], v[4][4];
            N[0][0] = (S[0][0] + S[1][1]) + S[2][2];
            N[1][1] = (S[0][0] - S[1][1]) - S[2][2];
            N[2][2] = (S[1][1] - S[0][0]) - S[2][2];
            N[3][3] = (S[2][2] - S[0][0]) - S[1][1];
            N[0][1] = S[1][2] - S[2][1];
            N[0][2] = S[2][0] - S[0][2];
            N[0][3] = S[0][1] - S[1][0];
            N[1][2] = S[0][1] + S[1][0];
            N[1][3] = S[2][0] + S[0][2];
            N[2][3] = S[1][2] + S[2][1];
            N[1][0] = N[2][0] = N[2][1] = N[3][0] = N[3][1] = N[3][2] = 0.0;
            jacobi4(N, d, v);
            int im = 0;
            double l1 = d[0];
#pragma unroll
            for (int i = 1; i < 4; ++i)
                if (d[i] > l1) l1 = d[i], im = i;
            double l2 = -__builtin_inf(), q[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) l2 = (i != im && d[i] > l2) ? d[i] : l2;
            gap = l1 - l2;
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = im == 0 ? v[j][0] : (im == 1 ? v[j][1] : (im == 2 ? v[j][2] : v[j][3]));
            const double qn = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = q[j] / qn;
            const double q00 = q[0] * q[0], q11 = q[1] * q[1], q22 = q[2] * q[2], q33 = q[3] * q[3];
            R[0][0] = ((q00 + q11) - q22) - q33;
            R[1][1] = ((q00 - q11) + q22) - q33;
            R[2][2] = ((q00 - q11) - q22) + q33;
            R[0][1] = 2.0 * (q[1] * q[2] - q[0] * q[3]);
            R[1][0] = 2.0 * (q[1] * q[2] + q[0] * q[3]);
            R[0][2] = 2.0 * (q[1] * q[3] + q[0] * q[2]);
            R[2][0] = 2.0 * (q[1] * q[3] - q[0] * q[2]);
            R[1][2] = 2.0 * (q[2] * q[3] - q[0] * q[1]);
            R[2][1] = 2.0 * (q[2] * q[3] + q[0] * q[1]);
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = yb[i] - ((R[i][0] * xb[0] + R[i][1] * xb[1]) + R[i][2] * xb[2]);
            // ---- residuals, from the posed points
            double px[3], su = 0.0, ey = 0.0, d2 = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) px[i] = ((R[i][0] * x[0] + R[i][1] * x[1]) + R[i][2] * x[2]) + t[i];
            for (uint32_t k = k0; k < k1; ++k) {
                const uint32_t m = p.sub_nodes[k];
                const double w = (double)p.W.w[p.M.node_type[m]];
                if (!(w > 0.0)) continue;
                double r2 = 0.0, y2 = 0.0;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double y = a.center[3u * m + j];
                    r2 = r2 + (px[j] - y) * (px[j] - y);
                    y2 = y2 + (y - yb[j]) * (y - yb[j]);
                }
                su = su + w * r2;
                ey = ey + w * y2;
            }
            if (fitted) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double e = px[j] - sy[j] / wu;
                    d2 = d2 + e * e;
                }
                dev = sqrt(d2);
            }
            sse = wave_sum(su);
            rn = wave_sum(fitted ? wu * d2 : 0.0);
            e0 = wave_sum(fitted ? wu * ((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]) + ey : 0.0);
        }
    }

    // ---- the row
    const double nan = __builtin_nan("");
    a.node[(size_t)li * kN + lane] = status == PMX_LIGAND_OK ? dev : nan;
    if (lane == 0) {
        const bool ok = status == PMX_LIGAND_OK;
        double *rot = a.rot + (size_t)li * 9, *tr = a.trans + (size_t)li * 3, *fit = a.fit + (size_t)li * 8;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) rot[3 * i + j] = ok ? R[i][j] : nan;
            tr[i] = ok ? t[i] : nan;
        }
        const bool any = npairs > 0;
        fit[0] = ok ? W : nan;
        fit[1] = ok ? sse : nan;
        fit[2] = ok ? (any ? sqrt(sse / W) : 0.0) : nan;
        fit[3] = ok ? (any ? sqrt(rn / W) : 0.0) : nan;
        fit[4] = ok ? e0 : nan;
        fit[5] = ok ? gap : nan;
        fit[6] = ok ? 0.0 : nan;
        fit[7] = ok ? 0.0 : nan;
        a.count[(size_t)li * 2] = nfit;
        a.count[(size_t)li * 2 + 1] = npairs;
    }
    write_row_header(a.rows, L, li, status);
    wave_sync(); // (the next row starts by clearing this LDS)
}

__global__ __launch_bounds__(64) void align_kernel(const ScreenParams p, const pmx_rows::AlignArgs a) {
    __shared__ RowLds L;
    for_each_row(a.rows, [&](uint32_t li) { align_row(p, a, L, li); });
}

} // namespace pmx_r

namespace pmx_rows {

size_t lds_bytes(Kind kind) { return kind == kAttribute ? (size_t)pmx_r::kAttributeLds : (kind == kHotspots ? (size_t)pmx_r::kHotspotsLds : sizeof(pmx_r::RowLds)); }

void launch(unsigned blocks, hipStream_t stream, const pmx::ScreenParams &p, const AttributeArgs &a) { pmx_r::attribute_kernel<<<dim3(blocks), dim3(64), 0, stream>>>(p, a); }
void launch(unsigned blocks, hipStream_t stream, const pmx::ScreenParams &p, const AlignArgs &a) { pmx_r::align_kernel<<<dim3(blocks), dim3(64), 0, stream>>>(p, a); }
void launch(unsigned blocks, hipStream_t stream, const pmx::ScreenParams &p, const HotspotArgs &a) { pmx_r::hotspots_kernel<<<dim3(blocks), dim3(64), 0, stream>>>(p, a); }

} // namespace pmx_rows
