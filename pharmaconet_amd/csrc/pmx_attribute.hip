// pmx_attribute.hip - which ligand nodes carry a leaf's total, on gfx950: for listed (ligand, conformer, key) rows the matrix of self
// and pair entries the reference's tree adds up for that leaf (match_utils.py:9-122 behind graph_match.py:139-172, :263-268), the
// number of failing node pairs per pair entry, the leaf's total in the product walker's order, and the share of every ligand node.
//
// pmx_screen_tables.h is compiled here once more, as namespace pmx_a, for parse_record, the level scan's rules, center_size and
// exact_value. Nothing else of the screening path is part of this translation unit: no score table is built, no tabulated pair function
// is read, no slice or arena is used. Every node-pair term is evaluated one by one in the reference's float32 operations
// (exact_value), so the answer does not depend on PMX_TAILS_RATIO or on the rough-cell flags of the tabulated functions.
//
// One wavefront handles one row, in five steps that hand over through its LDS:
//   levels    lane q = ligand cluster q: candidates, tree levels (as scan_ligand / explain_walk find them); lane l = level l: the key is checked
//   centres   lane c = conformer c: centre and size of every matched level's cluster, then the cluster-distance prefilter of every
//             pair of matched levels (it fails only when it fails for every conformer: one ballot)
//   terms     lane u = node u: term(u, v) and fail(u, v) for every later listed node v, into term[u][v] and one fail mask per node
//   entries   lane e = entry (l1, l2): the float32 sum in the reference's order (itertools.combinations / product), the fails, -1
//             where the reference says no match, and the float64 sum of the same terms
//   nodes     lane u = node u: half of every term the node is part of, in ascending order of the other node, in float64
// No lane adds to another lane's sum and there is no floating-point atomic: the same call gives the same bits.
//
// The shares add up to the total: an entry is a float32 accumulation, so the float64 sum of its terms differs from it by float32
// rounding (relative 1e-7). Each term is therefore weighted by entry / (float64 sum of the entry's terms) - 1 to within that rounding -
// which spreads the entry's rounding residual over its terms in proportion: sum_u node[u] = sum of the entries = total to float64 rounding.
#include <hip/hip_runtime.h>
#include <cstring>

#define PMX_NS pmx_a
#include "pmx_screen_tables.h"
#include "pmx_attribute.h"

namespace pmx_a {

constexpr uint8_t kNoMatch = 0xFF, kNoLevel = 0xFE;
constexpr int kL = PMX_MAX_LEVELS, kN = PMX_MAX_LIGAND_NODES;
constexpr int kTS = kN + 1; // row stride of the term matrix: lane u writes term[u][v] for a uniform v, and 65 floats apart they land in 64 banks
static_assert(kN == 64 && PMX_MAX_LIGAND_CLUSTERS <= 64 && PMX_MAX_CONFORMERS <= 64 && kL <= 32, "one wavefront: a lane per node, cluster, conformer; a bit per level");

// LDS of the wavefront (static)
constexpr uint32_t kAtR = 0;                                // float4 ctr[kL][64] {centre, size} per level and conformer; then float term[kN][kTS]
constexpr uint32_t kRBytes = kL * 64 * 16 > kN * kTS * 4 ? kL * 64 * 16 : kN * kTS * 4;
constexpr uint32_t kAtPos = kAtR + kRBytes;                // float4 [kN]: the nodes' positions in the row's conformer
constexpr uint32_t kAtScale = kAtPos + kN * 16;            // double [kL][kL]: entry / float64 sum of its terms
constexpr uint32_t kAtFailm = kAtScale + kL * kL * 8;      // u64 [kN]: bit v of word u = fail(u, v), v > u
constexpr uint32_t kAtCb = kAtFailm + kN * 8;              // u64 [kL][2]: candidate model clusters of each level
constexpr uint32_t kAtEnt = kAtCb + kL * 16;               // float [kL][kL]: the entries as they are written
constexpr uint32_t kAtPf = kAtEnt + kL * kL * 4;           // u32 [kL]: bit l2 of word l1 = the prefilter lets (l1, l2) pass
constexpr uint32_t kAtFc = kAtPf + kL * 4;                 // u16 [kL][kL]: failing node pairs
constexpr uint32_t kAtSid = kAtFc + kL * kL * 2;           // u16 [kN]: node subset of the node under its level's match (0: not in the match list)
constexpr uint32_t kAtNlv = kAtSid + kN * 2;               // u8 [kN]: the node's level (kNoMatch: not in a match list)
constexpr uint32_t kAtTm = kAtNlv + kN;                    // u8 [kN]: type masks
constexpr uint32_t kAtLs = kAtTm + kN;                     // u8 [32]: first node of each level's cluster
constexpr uint32_t kAtLe = kAtLs + 32;                     // u8 [32]: one past its last node
constexpr uint32_t kAtKey = kAtLe + 32;                    // u8 [32]: the key as it counts (kNoMatch for None and for what is not a candidate)
constexpr uint32_t kAtLev = kAtKey + 32;                   // u8 [32]: ligand cluster of each level (kNoLevel past nl)
constexpr uint32_t kLdsBytes = kAtLev + 32;
static_assert(kAtScale % 8 == 0 && kAtFailm % 8 == 0 && kAtCb % 8 == 0 && kAtEnt % 4 == 0 && kAtPf % 4 == 0 && kAtFc % 2 == 0 && kAtSid % 2 == 0, "LDS alignment");
static_assert(kLdsBytes <= 64 * 1024, "LDS of a work-group");

// Row li of the call.
__device__ void attribute_row(const ScreenParams &p, const pmx_attr::Args &a, unsigned char *lds, uint32_t li) {
    const int lane = lane_id();
    float4 *ctr = reinterpret_cast<float4 *>(lds + kAtR);
    float *term = reinterpret_cast<float *>(lds + kAtR);
    float4 *pos = reinterpret_cast<float4 *>(lds + kAtPos);
    double *scale = reinterpret_cast<double *>(lds + kAtScale);
    unsigned long long *failm = reinterpret_cast<unsigned long long *>(lds + kAtFailm);
    unsigned long long *cbl = reinterpret_cast<unsigned long long *>(lds + kAtCb);
    float *ent = reinterpret_cast<float *>(lds + kAtEnt);
    uint32_t *pf = reinterpret_cast<uint32_t *>(lds + kAtPf);
    uint16_t *fc = reinterpret_cast<uint16_t *>(lds + kAtFc);
    uint16_t *sid = reinterpret_cast<uint16_t *>(lds + kAtSid);
    uint8_t *nlv = lds + kAtNlv, *tm = lds + kAtTm, *ls = lds + kAtLs, *le = lds + kAtLe, *keyl = lds + kAtKey, *lev = lds + kAtLev;

    const uint64_t lig = uni64(a.ligands[li]);
    const int c = uni((int)a.conformer[li]);

    // ---- the row as for a ligand without levels
    for (int e = lane; e < kL * kL; e += 64) {
        ent[e] = 0.f;
        fc[e] = 0;
    }
    if (lane < 32) {
        lev[lane] = kNoLevel;
        keyl[lane] = kNoMatch;
    }
    sid[lane] = 0;
    nlv[lane] = kNoMatch;

    bool supported = lig < p.lib.n; // (not a ligand of the library: nothing is read)
    Record r = Record{0, 0, 0, nullptr, nullptr, nullptr};
    int n = 0, C = 0, ncl = 0;
    if (supported) {
        r = parse_record(p.lib.data + p.lib.offsets[lig]);
        n = uni(r.n), C = uni(r.C), ncl = uni(r.ncl);
        supported = record_supported(r); // (a header-only record has no conformer)
    }
    if (supported && lane < n) tm[lane] = r.typemask[lane] & 127u;
    wave_sync();

    // ---- levels: the clusters that have a candidate, in priority order, at most PMX_MAX_LEVELS (scan_ligand's rules)
    int nl = 0;
    if (supported) {
        int cs = 0, ce = 0;
        unsigned long long cb0 = 0, cb1 = 0;
        if (lane < ncl) {
            cs = lane ? r.cluster_end[lane - 1] : 0;
            ce = r.cluster_end[lane];
            unsigned lm = 0;
            for (int u = cs; u < ce; ++u) lm |= tm[u & (kN - 1)];
            cb0 = p.M.tclus[2u * (lm & 127u)];
            cb1 = p.M.tclus[2u * (lm & 127u) + 1u];
        }
        const bool has = (cb0 | cb1) != 0ull;
        const int kc = (int)__popcll(cb0) + (int)__popcll(cb1);
        const unsigned long long bal = __ballot(has);
        const int lq = __popcll(bal & ((1ull << lane) - 1ull));
        nl = min((int)__popcll(bal), kL);
        if (__ballot(has && lq < kL && kc > PMX_MAX_LEVEL_CANDIDATES) != 0ull) {
            supported = false; // (as pmx_score and pmx_explain report such a ligand)
            nl = 0;
        } else if (has && lq < kL) {
            lev[lq] = (uint8_t)lane;
            ls[lq] = (uint8_t)cs;
            le[lq] = (uint8_t)ce;
            cbl[2 * lq] = cb0;
            cbl[2 * lq + 1] = cb1;
        }
    }
    wave_sync();

    // ---- the key: every match has to be a candidate of its level
    bool invalid = false;
    const bool compute = supported && c >= 0 && c < C;
    if (supported) {
        bool bad = false;
        if (lane < kL) {
            const int kk = a.key[(size_t)li * kL + lane];
            if (kk != kNoMatch) {
                bool ok = lane < nl && kk < p.M.K && kk < PMX_MAX_MODEL_CLUSTERS;
                if (ok) ok = ((kk < 64 ? cbl[2 * lane] >> kk : cbl[2 * lane + 1] >> (kk - 64)) & 1ull) != 0ull;
                bad = !ok;
                if (ok) keyl[lane] = (uint8_t)kk; // (a match that is no candidate counts as None in what follows; the row is invalid)
            }
        }
        invalid = __ballot(bad) != 0ull || !compute;
    }
    wave_sync();

    double share = 0.0, total = 0.0;
    if (compute) {
        GlobalFloats xyz = (GlobalFloats)uniptr(r.xyz);
        // ---- nodes: level, subset under the level's match (graph_match.py:145-155), position in conformer c
        int mylev = -1;
        uint32_t mysid = 0;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (lane < n) {
            for (int l = 0; l < nl; ++l) mylev = (lane >= (int)ls[l] && lane < (int)le[l]) ? l : mylev;
            if (mylev >= 0 && keyl[mylev] != kNoMatch) mysid = p.sidtab[(uint32_t)keyl[mylev] * 128u + tm[lane]];
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
        invalid = invalid || __ballot(dead_pair) != 0ull;
        wave_sync();

        // ---- node shares
        if (mysid != 0u) {
            for (int v = 0; v < n; ++v) {
                const int lv = uni((int)nlv[v]);
                if (lv == kNoMatch) continue;
                if (v != lane) {
                    const float t = v > lane ? term[lane * kTS + v] : term[v * kTS + lane];
                    share += (double)t * scale[min(mylev, lv) * kL + max(mylev, lv)];
                }
            }
            share *= 0.5;
        }
        // ---- the total as the product walker sums it: (running + self) + (pair entries with the matched ancestors, shallowest first)
        for (int l = 0; l < nl; ++l) {
            if (uni((int)keyl[l]) == kNoMatch) continue;
            double sum = 0.0;
            for (int l0 = 0; l0 < l; ++l0)
                if (uni((int)keyl[l0]) != kNoMatch) sum += (double)ent[l0 * kL + l];
            total = (total + (double)ent[l * kL + l]) + sum;
        }
    }

    // ---- the row
    const int status = !supported ? PMX_LIGAND_UNSUPPORTED : (invalid ? PMX_LIGAND_KEY_INVALID : PMX_LIGAND_OK);
    const double nan = __builtin_nan("");
    a.node[(size_t)li * kN + lane] = status == PMX_LIGAND_OK ? share : nan;
    for (int e = lane; e < kL * kL; e += 64) {
        a.entry[(size_t)li * kL * kL + e] = ent[e];
        a.fails[(size_t)li * kL * kL + e] = fc[e];
    }
    if (lane < kL) a.levels[(size_t)li * kL + lane] = lev[lane];
    if (lane == 0) {
        a.total[li] = status == PMX_LIGAND_OK ? total : nan;
        a.status[li] = status;
    }
    wave_sync(); // (the next row starts by clearing this LDS)
}

// Persistent wavefronts over the call's rows.
__global__ __launch_bounds__(64) void attribute_kernel(const ScreenParams p, const pmx_attr::Args a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
    for (;;) {
        const int lane = lane_id();
        uint32_t next = 0;
        if (lane == 0) next = atomicAdd(a.cursor, 1u);
        next = (uint32_t)uni((int)next);
        if (next >= a.n) break;
        attribute_row(p, a, lds, next);
    }
}

} // namespace pmx_a

namespace pmx_attr {

size_t lds_bytes() { return pmx_a::kLdsBytes; }

bool launch(unsigned blocks, hipStream_t stream, const void *params, size_t bytes, const Args &a) {
    if (bytes != sizeof(pmx_a::ScreenParams)) return false;
    pmx_a::ScreenParams p;
    std::memcpy(&p, params, sizeof p);
    pmx_a::attribute_kernel<<<dim3(blocks), dim3(64), 0, stream>>>(p, a);
    return true;
}

} // namespace pmx_attr
