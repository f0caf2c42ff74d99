// pmx_rows_front.h - how a row kernel opens a (ligand, conformer, key) row: the ligand's record, its type masks, its tree levels with the
// candidates of each (the level rule of pmx_screen_tables.h), the key checked against them, a node's subset under its level's match, and
// the row's status. One definition for every unit that takes such rows (pmx_rows.hip: pmx_attribute, pmx_align, pmx_hotspots;
// pmx_pose_fit.hip: pmx_pose_fit in key mode), so that their pairs and their statuses cannot drift. Include after pmx_screen_tables.h,
// under the unit's PMX_NS.
#pragma once
#include "pmx_rows.h"

namespace PMX_NS {
using pmx_rows::Rows;

constexpr uint8_t kNoMatch = 0xFF, kNoLevel = 0xFE;
constexpr int kL = PMX_MAX_LEVELS, kN = PMX_MAX_LIGAND_NODES;
static_assert(kN == 64 && PMX_MAX_LIGAND_CLUSTERS <= 64 && PMX_MAX_CONFORMERS <= 64 && kL <= 32, "one wavefront: a lane per node, cluster, conformer; a bit per level");

// ------------------------------------------------------------------------------------------------ a row, opened
// What open_row leaves in the wavefront's LDS.
struct RowLds {
    unsigned long long cbl[kL][2]; // candidate model clusters of each level
    uint8_t tm[kN];                // type masks
    uint8_t ls[32], le[32];        // first node of each level's cluster, one past its last node
    uint8_t key[32];               // the key as it counts (kNoMatch for None and for what is not a candidate)
    uint8_t lev[32];               // ligand cluster of each level (kNoLevel past nl)
};
static_assert(sizeof(RowLds) == 512 && alignof(RowLds) == 8, "RowLds layout");

struct Row {
    Record r;
    int n, C, ncl, nl, c; // nodes, conformers, clusters, tree levels of the ligand; the row's conformer
    bool supported;       // a ligand of the library with a conformer and no level of more than PMX_MAX_LEVEL_CANDIDATES candidates
    bool key_bad;         // some match of the key is no candidate of its level (it counts as None in RowLds::key)
    bool compute;         // supported, and c is a conformer of the ligand
};

// Row li of the call: the record, the levels and the checked key (all wave-uniform).
__device__ __forceinline__ Row open_row(const ScreenParams &p, const Rows &rows, RowLds &L, uint32_t li) {
    const int lane = lane_id();
    const uint64_t lig = uni64(rows.ligands[li]);
    Row w;
    w.c = uni((int)rows.conformer[li]);
    if (lane < 32) {
        L.lev[lane] = kNoLevel;
        L.key[lane] = kNoMatch;
    }
    w.supported = lig < p.lib.n; // (not a ligand of the library: nothing is read)
    w.r = Record{0, 0, 0, nullptr, nullptr, nullptr};
    w.n = w.C = w.ncl = w.nl = 0;
    if (w.supported) {
        w.r = parse_record(p.lib.data + p.lib.offsets[lig]);
        w.n = uni(w.r.n), w.C = uni(w.r.C), w.ncl = uni(w.r.ncl);
        w.supported = record_supported(w.r); // (a header-only record has no conformer)
    }
    if (w.supported && lane < w.n) L.tm[lane] = w.r.typemask[lane] & 127u;
    wave_sync();

    // ---- levels: the clusters that have a candidate, in priority order, at most PMX_MAX_LEVELS
    if (w.supported) {
        const ClusterCand k = cluster_candidates(p, w.r, w.ncl, lane, [&L](int u) { return (unsigned)L.tm[u & (kN - 1)]; });
        const LevelSlot s = level_slot(k, lane);
        if (s.too_many) {
            w.supported = false; // (as pmx_score and pmx_explain report such a ligand)
        } else {
            w.nl = s.nl;
            if (s.has && s.lev < kL) {
                L.lev[s.lev] = (uint8_t)lane;
                L.ls[s.lev] = (uint8_t)k.cs;
                L.le[s.lev] = (uint8_t)k.ce;
                L.cbl[s.lev][0] = k.cb0;
                L.cbl[s.lev][1] = k.cb1;
            }
        }
    }
    wave_sync();

    // ---- the key: every match has to be a candidate of its level
    w.compute = w.supported && w.c >= 0 && w.c < w.C;
    w.key_bad = false;
    if (w.supported) {
        bool bad = false;
        if (lane < kL) {
            const int kk = rows.key[(size_t)li * kL + lane];
            if (kk != kNoMatch) {
                bool ok = lane < w.nl && kk < p.M.K && kk < PMX_MAX_MODEL_CLUSTERS;
                if (ok) ok = ((kk < 64 ? L.cbl[lane][0] >> kk : L.cbl[lane][1] >> (kk - 64)) & 1ull) != 0ull;
                bad = !ok;
                if (ok) L.key[lane] = (uint8_t)kk;
            }
        }
        w.key_bad = __ballot(bad) != 0ull;
    }
    wave_sync();
    return w;
}

// Node `lane` of the row: its tree level (-1: none) and its node subset under its level's match (graph_match.py:145-155), 0 when the
// level has no match or the node is none of the ligand's.
struct NodeSubset {
    int lev;
    uint32_t sid;
};
__device__ __forceinline__ NodeSubset row_node_subset(const ScreenParams &p, const Row &w, const RowLds &L, int lane) {
    NodeSubset s{-1, 0u};
    if (lane < w.n) {
        for (int l = 0; l < w.nl; ++l) s.lev = (lane >= (int)L.ls[l] && lane < (int)L.le[l]) ? l : s.lev;
        if (s.lev >= 0 && L.key[s.lev] != kNoMatch) s.sid = p.sidtab[(uint32_t)L.key[s.lev] * 128u + L.tm[lane]];
    }
    return s;
}

// `invalid`: what the caller itself found wrong with a supported row.
__device__ __forceinline__ int row_status(const Row &w, bool invalid) {
    return !w.supported ? PMX_LIGAND_UNSUPPORTED : (w.key_bad || !w.compute || invalid ? PMX_LIGAND_KEY_INVALID : PMX_LIGAND_OK);
}

} // namespace PMX_NS
