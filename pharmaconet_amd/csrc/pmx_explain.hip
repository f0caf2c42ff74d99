// pmx_explain.hip - what a score is made of, on gfx950: for listed ligands the per-conformer maxima that pmx_score averages
// (graph_match.py:103-109, `scores` inside _run_average) and, per conformer, the leaf of the reference's tree that reaches
// its maximum (ClusterMatchTree.key, tree.py:129-137).
//
// The table phase of the screening path (pmx_screen_tables.h) is compiled here once more, as namespace pmx_x: the explain kernel builds
// a ligand's tables with the product's own prepare_ligand (same slices, large slices and arena passes, same statuses) and walks them with
// a walker of its own. Neither the product walker (pmx_screen_walk.h) nor the product kernels (pmx_screen.hip) are part of this
// translation unit.
//
// The explaining leaf of conformer c is the first leaf in `root_tree.iteration()` order whose score for c equals the maximum -
// the leaf a strict `>` update in _run_average keeps. This walker visits the tree in that order (candidates in ascending
// model-cluster order, the skip child last, tree.py:88-101) and updates with a strict `>`, so the first leaf it records at the
// final maximum IS that leaf. A child is dropped only when no leaf below it can reach the running maximum of any of its
// conformers ((total + R) * kBoundSlack < running maximum, strictly; the running maximum is never above the final one), so
// no leaf that ties the maximum is ever dropped, and only children with >= 5 matches are dropped at all: their existence alone
// settles every skip decision above them (tree.py:98, see walk() in pmx_screen_walk.h). Leaf totals are summed as the product
// walker sums them - (parent + self) + (pair entries of the matched ancestors, shallowest first) in float64 - so the maxima
// are bit for bit the ones pmx_score averages.
//
// Constrained matching (pmx_explain_constrained): the same tree - which children exist and when the skip child exists do not depend on
// the constraint - but only a leaf whose key qualifies (a cluster of every require group, none of the exclude set) may update a
// conformer's maximum. The constrained instantiation keeps, per frame, the 128-bit set of model clusters matched on the path; the
// bound test above holds with the constrained running maximum, and a child with >= 5 matches is also dropped when no leaf below it can
// qualify (an excluded cluster on its path, or a require group with no cluster on the path or among the candidates of the levels
// below). A subtree with fewer matches that cannot qualify is walked for its match count alone.
//
// Modes: there is one walker, and it keeps per conformer the M = n_modes best leaves - the leaves that hold the conformer with a score
// > 0 (and qualify, under a constraint), by descending total, equal totals in iteration order. pmx_explain and pmx_explain_constrained
// are M = 1 (the list is the running maximum and its key, the outputs [n][1][...] are the layouts they document), pmx_explain_modes any M
// up to PMX_MAX_MODES. A lane keeps its M totals, sorted, in LDS and its M keys (as candidate numbers) in the row's own output block,
// turned into model clusters in place at the end. A leaf enters the list iff its total is strictly above the lane's M-th value, behind
// every entry >= it: a later leaf never overtakes an equal earlier one, so the list is the stable order above and its head is the first
// leaf at the maximum, as the strict `>` of _run_average keeps it. The bound follows the M-th value (with M = 1 the running maximum of
// the note above): a child with >= 5 matches is dropped when (total + R) * kBoundSlack < the running M-th value, strictly, for every
// conformer it holds. The running M-th value of a conformer never
// exceeds its final one (entries only rise), so every leaf below a dropped child is strictly below the final M-th value of every conformer
// it holds and belongs to no list; a leaf that ties the M-th value is never dropped, and the walked leaves arrive in iteration order, so the
// lists are those of the full tree. The feasibility drops of the constrained walker do not look at values and are unchanged.
#include <hip/hip_runtime.h>
#include <algorithm>

#define PMX_NS pmx_x
#include "pmx_screen_tables.h"
#include "pmx_explain.h"

namespace pmx_x {

constexpr uint8_t kNoMatch = 0xFF, kNoLevel = 0xFE;

// The explain walker's LDS, behind the product's per-wave layout.
template <int G>
struct ExplainLds {
    uint32_t tot, frame, mrow, path, cb, pm, sfx, bytes;
};
template <int G>
__host__ __device__ inline ExplainLds<G> explain_lds(const WaveShape<G> &ws, bool constrained) {
    ExplainLds<G> e;
    uint32_t o = (ws.bytes + 15u) & ~15u;
    e.tot = o; // double [frame][G]: the total of each frame's tree node (frame f = the node whose children are the candidates of level f)
    o += (PMX_MAX_LEVELS + 1) * G * 8;
    e.frame = o; // int [PMX_MAX_LEVELS + 1]: nb | mx << 8 | any << 16 | matched << 17 | nm << 24
    o += 4 * 24;
    e.mrow = o; // int [PMX_MAX_LEVELS]: pair entry of match q against candidate x = mrow[q] + x
    o += 4 * PMX_MAX_LEVELS;
    e.path = o; // u8 [PMX_MAX_LEVELS]: the candidate taken at each level of the current path (kNoMatch: the skip child)
    o += 32;
    e.cb = o; // u64 [PMX_MAX_LEVELS][2]: model clusters that are candidates of each level
    o += 16 * PMX_MAX_LEVELS;
    e.pm = e.sfx = o;
    if (constrained) {
        e.pm = o; // u64 [PMX_MAX_LEVELS + 1][2]: model clusters matched on the path to each frame's node
        o += 16 * (PMX_MAX_LEVELS + 1);
        e.sfx = o; // u64 [PMX_MAX_LEVELS + 1][2]: model clusters that are candidates of level f or of a level below it
        o += 16 * (PMX_MAX_LEVELS + 1);
    }
    e.bytes = o; // (the mode totals lie behind: double [n_modes][G], conformer c's descending; the keys live in the row's output block)
    return e;
}

// Can a key whose matched model clusters are (m0, m1), and that may still gain clusters of (s0, s1), qualify: no excluded cluster matched,
// and every require group has a cluster matched or still to come. With s = 0: does the key qualify. Wave-uniform.
__device__ inline bool con_feasible(const pmx_match_constraint &k, unsigned long long m0, unsigned long long m1, unsigned long long s0, unsigned long long s1) {
    if (((m0 & k.exclude[0]) | (m1 & k.exclude[1])) != 0ull) return false;
    for (int g = 0; g < k.n_require; ++g)
        if ((((m0 | s0) & k.require[g][0]) | ((m1 | s1) & k.require[g][1])) == 0ull) return false;
    return true;
}

// Candidate b of a level whose candidates are the model clusters (w0, w1), as a one-bit set: candidates are in ascending cluster order.
__device__ inline void candidate_bit(unsigned long long w0, unsigned long long w1, int b, unsigned long long &b0, unsigned long long &b1) {
    const int n0 = __popcll(w0);
    unsigned long long xw = b < n0 ? w0 : w1;
    for (int j = b < n0 ? b : b - n0; j > 0; --j) xw &= xw - 1ull;
    xw &= 0ull - xw;
    b0 = b < n0 ? xw : 0ull;
    b1 = b < n0 ? 0ull : xw;
}

// Candidate b of such a level as a model cluster.
__device__ inline uint8_t candidate_cluster(unsigned long long w0, unsigned long long w1, int b) {
    const int n0 = __popcll(w0);
    unsigned long long xw = b < n0 ? w0 : w1;
    for (int j = b < n0 ? b : b - n0; j > 0; --j) xw &= xw - 1ull;
    return (uint8_t)((b < n0 ? 0 : 64) + __ffsll(xw) - 1);
}

// The tree of one prepared ligand (tables at `rec`): the a.n_modes best leaves per conformer, totals and keys into row li of the output
// (a.conf_max and a.match are [n][n_modes][...]). Lane c < G is conformer c.
// CONSTRAINED: only leaves whose key qualifies under a.con enter a list (see the note at the top).
template <int G, bool CONSTRAINED>
__device__ void explain_walk(const ScreenParams &p, unsigned char *lds, const ExplainLds<G> &E, const unsigned char *rec, uint64_t lig, uint32_t li,
                             const pmx_xpl::Args &a) {
    const int lane = lane_id();
    const int c = lane & (G - 1);
    const bool mine = lane < G; // (lanes >= G idle)
    const RecHeader *H = reinterpret_cast<const RecHeader *>(rec);
    const int nl = uni((int)H->nl), C = uni((int)H->C);
    const uint32_t ksumtot = (uint32_t)uni((int)H->ksumtot), T = (uint32_t)uni((int)H->T);
    const float *S = reinterpret_cast<const float *>(rec + rec_s_off<G>());
    const float *P = reinterpret_cast<const float *>(rec + rec_p_off<G>(ksumtot));
    const double *R = reinterpret_cast<const double *>(rec + rec_r_off<G>(ksumtot, T));
    double *tot = reinterpret_cast<double *>(lds + E.tot);
    int *frame = reinterpret_cast<int *>(lds + E.frame);
    int *mrow = reinterpret_cast<int *>(lds + E.mrow);
    uint8_t *path = lds + E.path;
    unsigned long long *cbl = reinterpret_cast<unsigned long long *>(lds + E.cb);
    unsigned long long *pm = reinterpret_cast<unsigned long long *>(lds + E.pm);
    unsigned long long *sfx = reinterpret_cast<unsigned long long *>(lds + E.sfx);
    // conformer c's totals at mv[m * G + c], mode m's key at mkey + m * kModeKeys
    const int M = uni((int)a.n_modes);
    double *mv = reinterpret_cast<double *>(lds + E.bytes);
    constexpr size_t kModeKeys = (size_t)PMX_MAX_CONFORMERS * PMX_MAX_LEVELS;
    uint8_t *mkey = a.match + ((size_t)li * M * PMX_MAX_CONFORMERS + c) * PMX_MAX_LEVELS;

    // ---- the levels of the row and the model clusters that are candidates of each
    const Record r = parse_record(p.lib.data + p.lib.offsets[lig]);
    {
        const ClusterCand k = cluster_candidates(p, r, r.ncl, lane, [&r](int u) { return (unsigned)r.typemask[u]; });
        const LevelSlot s = level_slot(k, lane);
        if (s.has && s.lev < nl) { // (nl is the record header's: prepare_ligand has refused a ligand with too many candidates at a level)
            a.levels[(size_t)li * PMX_MAX_LEVELS + s.lev] = (uint8_t)lane;
            cbl[2 * s.lev] = k.cb0;
            cbl[2 * s.lev + 1] = k.cb1;
        }
    }
    bool go = true; // (no leaf can qualify when a require group has no cluster among the candidates of any level)
    if constexpr (CONSTRAINED) {
        wave_sync();
        if (lane == 0) {
            unsigned long long s0 = 0, s1 = 0;
            sfx[2 * nl] = sfx[2 * nl + 1] = 0ull;
            for (int l = nl - 1; l >= 0; --l) {
                s0 |= cbl[2 * l];
                s1 |= cbl[2 * l + 1];
                sfx[2 * l] = s0;
                sfx[2 * l + 1] = s1;
            }
            pm[0] = pm[1] = 0ull;
        }
        wave_sync();
        go = con_feasible(a.con, 0ull, 0ull, uni64(sfx[0]), uni64(sfx[1]));
    }

    uint32_t vbits = (mine && c < C) ? 1u : 0u; // bit f: conformer c is in the pair_scores of frame f's node (tree.py:78-84)
    double best = 0.0;                           // running M-th value of conformer c (M = 1: its running maximum, graph_match.py:105-108)
    if (mine) {
        tot[c] = 0.0;
        for (int m = 0; m < M; ++m) mv[m * G + c] = 0.0; // (the keys are the row's: 0xFF throughout, explain_init_kernel)
    }
    if (lane == 0) frame[0] = 0;
    wave_sync();
    const double slack = kBoundSlack;
    int f = 0;
    while (go) {
        if (f == nl) { // a leaf: its pair_scores are the frame's totals over the frame's conformers
            bool qualifies = true;
            if constexpr (CONSTRAINED) qualifies = con_feasible(a.con, uni64(pm[2 * f]), uni64(pm[2 * f + 1]), 0ull, 0ull);
            if (qualifies && mine && ((vbits >> f) & 1u)) {
                const double t = tot[f * G + c];
                if (t > best) { // behind every entry >= t; the entries below move down one place, the last one leaves
                    int at = M - 1;
                    for (; at > 0 && mv[(at - 1) * G + c] < t; --at) {
                        mv[at * G + c] = mv[(at - 1) * G + c];
                        for (int l = 0; l < nl; ++l) mkey[at * kModeKeys + l] = mkey[(at - 1) * kModeKeys + l];
                    }
                    mv[at * G + c] = t;
                    for (int l = 0; l < nl; ++l) mkey[at * kModeKeys + l] = path[l];
                    best = mv[(M - 1) * G + c];
                }
            }
            const int ret = (uni(frame[f]) >> 17) & 1;
            --f;
            const int st = uni(frame[f]);
            const int mx = max((st >> 8) & 255, ret);
            wave_sync();
            if (lane == 0) frame[f] = (st & ~0xff00) | (mx << 8);
            wave_sync();
            continue;
        }
        const int st = uni(frame[f]);
        int nb = st & 255, mx = (st >> 8) & 255, any = (st >> 16) & 1;
        const int matched = (st >> 17) & 1, nm = (st >> 24) & 255;
        const int kf = uni((int)H->k[f]), ksf = uni((int)H->ksum[f]);
        if (nb < kf) { // candidate nb of level f: does the child exist, and what are its totals (tree.py:33-41, 78-84)
            const int b = nb++;
            const uint32_t x = (uint32_t)(ksf + b);
            bool valid = false;
            double t = 0.0;
            if (mine) {
                const float self = S[(size_t)x * G + c];
                float lo = 1.f;
                double sum = 0.0;
                for (int q = 0; q < nm; ++q) {
                    const float v = P[(size_t)(uint32_t)(uni(mrow[q]) + (int)x) * G + c];
                    lo = fminf(lo, v);
                    sum += (double)v;
                }
                valid = ((vbits >> f) & 1u) && lo > 0.f && sum == sum; // (NaN entry: not > 0, see walk())
                t = (tot[f * G + c] + (double)self) + sum;
            }
            if (__ballot(valid) == 0ull) {
                wave_sync();
                if (lane == 0) frame[f] = (st & ~0xff) | nb;
                wave_sync();
                continue;
            }
            any = 1;
            unsigned long long m0 = 0, m1 = 0; // the child's matched model clusters
            if constexpr (CONSTRAINED) {
                candidate_bit(uni64(cbl[2 * f]), uni64(cbl[2 * f + 1]), b, m0, m1);
                m0 |= uni64(pm[2 * f]);
                m1 |= uni64(pm[2 * f + 1]);
            }
            if (nm + 1 >= 5) { // a child whose existence settles every skip decision above it: may be dropped on its bound
                bool drop = false; // (or when no leaf below it can qualify)
                if constexpr (CONSTRAINED) drop = !con_feasible(a.con, m0, m1, uni64(sfx[2 * (f + 1)]), uni64(sfx[2 * (f + 1) + 1]));
                if (!drop) {
                    const double rb = mine ? R[(size_t)(f + 1) * G + c] : 0.0;
                    drop = __ballot(valid && (t + rb) * slack >= best) == 0ull;
                }
                if (drop) {
                    mx = max(mx, 1); // (it returns >= 1 match: all the frames above need to know, see the note at the top)
                    wave_sync();
                    if (lane == 0) frame[f] = nb | (mx << 8) | (any << 16) | (matched << 17) | (nm << 24);
                    wave_sync();
                    continue;
                }
            }
            wave_sync();
            if (lane == 0) {
                frame[f] = nb | (mx << 8) | (any << 16) | (matched << 17) | (nm << 24);
                frame[f + 1] = (1 << 17) | ((nm + 1) << 24);
                path[f] = (uint8_t)b;
                const int k1 = (int)H->ksum[f + 1];
                mrow[nm] = (int)H->rowbase[f] + b * ((int)ksumtot - k1) - k1; // entry((f, b) -> x) = rowbase[f] + b nd_f + (x - ksum[f + 1])
                if constexpr (CONSTRAINED) {
                    pm[2 * (f + 1)] = m0;
                    pm[2 * (f + 1) + 1] = m1;
                }
            }
            if (mine) tot[(f + 1) * G + c] = t;
            vbits = (vbits & ~(1u << (f + 1))) | ((valid ? 1u : 0u) << (f + 1));
            wave_sync();
            ++f;
            continue;
        }
        if (nb == kf) { // the candidates are done: the skip child (tree.py:98-101)
            wave_sync();
            if (lane == 0) frame[f] = (st & ~0xff) | (kf + 1);
            wave_sync();
            if (any && nm + mx >= 5) continue;
            const bool valid = mine && ((vbits >> f) & 1u);
            const double t = mine ? tot[f * G + c] : 0.0;
            if (nm >= 5) {
                bool drop = false;
                if constexpr (CONSTRAINED)
                    drop = !con_feasible(a.con, uni64(pm[2 * f]), uni64(pm[2 * f + 1]), uni64(sfx[2 * (f + 1)]), uni64(sfx[2 * (f + 1) + 1]));
                if (!drop) {
                    const double rb = mine ? R[(size_t)(f + 1) * G + c] : 0.0;
                    drop = __ballot(valid && (t + rb) * slack >= best) == 0ull;
                }
                if (drop) continue;
            }
            if (lane == 0) {
                frame[f + 1] = nm << 24;
                path[f] = kNoMatch;
                if constexpr (CONSTRAINED) {
                    pm[2 * (f + 1)] = pm[2 * f];
                    pm[2 * (f + 1) + 1] = pm[2 * f + 1];
                }
            }
            if (mine) tot[(f + 1) * G + c] = t;
            vbits = (vbits & ~(1u << (f + 1))) | ((valid ? 1u : 0u) << (f + 1));
            wave_sync();
            ++f;
            continue;
        }
        // the frame is done: it returns its own match and the most its children returned (tree.py:102)
        if (f == 0) break;
        const int ret = matched + mx;
        --f;
        const int sp = uni(frame[f]);
        const int mxp = max((sp >> 8) & 255, ret);
        wave_sync();
        if (lane == 0) frame[f] = (sp & ~0xff00) | (mxp << 8);
        wave_sync();
    }

    // ---- the row: maxima, keys as model clusters, best conformer
    wave_sync();
    const bool live = mine && c < C;
    for (int m = 0; m < M; ++m) {
        const double v = live ? mv[m * G + c] : 0.0;
        a.conf_max[((size_t)li * M + m) * PMX_MAX_CONFORMERS + lane] = v;
        if (v > 0.0) // (a place no leaf took keeps its 0xFF)
            for (int l = 0; l < nl; ++l) {
                uint8_t &k = mkey[m * kModeKeys + l];
                if (k != kNoMatch) k = candidate_cluster(cbl[2 * l], cbl[2 * l + 1], k);
            }
    }
    best = live ? mv[c] : 0.0; // (the best conformer is mode 0's)
    // smallest conformer with the largest maximum
    double m = live ? best : -1.0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_xor(m, d);
        m = o > m ? o : m;
    }
    const unsigned long long at = __ballot(live && best == m);
    if (lane == 0) a.best[li] = at ? __ffsll(at) - 1 : 0;
    wave_sync();
}

// Persistent wavefronts over the call's list (mode 0) or over the ligands an earlier pass handed on (modes 1 - 3): the tables
// as the product builds them (prepare_ligand, which also writes the status), then the explain walk.
template <int G, bool TAILS, bool CONSTRAINED>
__global__ __launch_bounds__(64) void explain_kernel(const ScreenParams p, const pmx_xpl::Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane0 = lane_id();
    const uint32_t wave_id = blockIdx.x;
    const WaveShape<G> ws = wave_shape<G>(p.M.K, (int)p.max_nodes);
    const ExplainLds<G> E = explain_lds<G>(ws, CONSTRAINED);
    const uint32_t todo = p.mode == 0 ? a.n
                                      : min(p.mode == 1 ? p.ctl->ovf_count : (p.mode == 2 ? p.ctl->carry_count : p.ctl->retry_count[p.retry_slot ^ 1u]), p.list_cap);
    const uint32_t *list = p.mode == 1 ? p.ovf_list : (p.mode == 2 ? p.carry_list : p.retry_in);
    WaveStats *stat = reinterpret_cast<WaveStats *>(lds + ws.off_stat);
    if (lane0 < (int)(sizeof(WaveStats) / 8)) reinterpret_cast<unsigned long long *>(stat)[lane0] = 0ull;
    wave_sync();
    for (;;) {
        const int lane = lane_id();
        uint32_t next = 0;
        if (lane == 0) next = atomicAdd(&p.ctl->cursor[p.mode], 1u);
        next = (uint32_t)uni((int)next);
        if (next >= todo) break;
        const uint32_t li = p.mode == 0 ? next : (uint32_t)uni((int)list[next]);
        const uint64_t lig = uni64(a.ligands[li]);
        if (lig >= p.lib.n) { // (not a ligand of the library: reported unsupported, nothing is read)
            if (lane == 0) a.status[li] = PMX_LIGAND_UNSUPPORTED;
            continue;
        }
        // row li of the call is library ligand `lig`: prepare_ligand reads record first + li and writes status[li] and scores[li]
        // (a NaN or the 0 of a ligand without levels: written into the row's first maximum, which it is)
        ScreenParams q = p;
        q.first = lig - (uint64_t)li;
        q.status = a.status;
        q.scores = reinterpret_cast<float *>(a.conf_max + (size_t)li * (a.n_modes * PMX_MAX_CONFORMERS - 1));
        q.flags = PMX_SCORES_F64;
        unsigned char *rec = prepare_ligand<G, false, TAILS>(q, lds, ws, li, wave_id, stat);
        if (!rec) continue;
        explain_walk<G, CONSTRAINED>(q, lds, E, rec, lig, li, a);
    }
}

// a.conf_max is [n][n_modes][PMX_MAX_CONFORMERS], a.match [n][n_modes][PMX_MAX_CONFORMERS][PMX_MAX_LEVELS].
__global__ void explain_init_kernel(const pmx_xpl::Args a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = a.n, nm = n * a.n_modes;
    if (i < nm * PMX_MAX_CONFORMERS) a.conf_max[i] = 0.0;
    if (i < n * PMX_MAX_LEVELS) a.levels[i] = kNoLevel;
    if (i < n) a.best[i] = 0;
    for (size_t j = i; j < nm * PMX_MAX_CONFORMERS * PMX_MAX_LEVELS; j += (size_t)gridDim.x * blockDim.x) a.match[j] = kNoMatch;
}

__global__ void explain_fixup_kernel(const pmx_xpl::Args a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t row = (size_t)a.n_modes * PMX_MAX_CONFORMERS;
    if (i >= (size_t)a.n * row) return;
    const size_t li = i / row;
    if (a.status[li] == PMX_LIGAND_OK) return;
    a.conf_max[i] = __builtin_nan("");
    if (i % row == 0) a.best[li] = -1;
}

} // namespace pmx_x

namespace pmx_xpl {

size_t lds_bytes(int G, int K, int max_nodes, bool constrained, int n_modes) {
    size_t bytes = 0;
    pmx::with_lanes(G, [&](auto g) { bytes = pmx_x::explain_lds<decltype(g)::value>(pmx_x::wave_shape<decltype(g)::value>(K, max_nodes), constrained).bytes + (size_t)n_modes * decltype(g)::value * 8; });
    return bytes;
}

template <int G, bool CONSTRAINED>
static void launch_shape(bool tails, unsigned blocks, unsigned lds, hipStream_t stream, const pmx::ScreenParams &p, const Args &a) {
    if (tails) pmx_x::explain_kernel<G, true, CONSTRAINED><<<dim3(blocks), dim3(64), lds, stream>>>(p, a);
    else pmx_x::explain_kernel<G, false, CONSTRAINED><<<dim3(blocks), dim3(64), lds, stream>>>(p, a);
}

bool launch(int G, bool tails, bool constrained, unsigned blocks, unsigned lds, hipStream_t stream, const pmx::ScreenParams &p, const Args &a) {
    return pmx::with_lanes(G, [&](auto g) {
        constexpr int L = decltype(g)::value;
        constrained ? launch_shape<L, true>(tails, blocks, lds, stream, p, a) : launch_shape<L, false>(tails, blocks, lds, stream, p, a);
    });
}

void launch_init(const Args &a, hipStream_t stream) {
    const size_t n = (size_t)a.n * a.n_modes * PMX_MAX_CONFORMERS;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 65535);
    pmx_x::explain_init_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(a);
}

void launch_fixup(const Args &a, hipStream_t stream) {
    const size_t n = (size_t)a.n * a.n_modes * PMX_MAX_CONFORMERS;
    pmx_x::explain_fixup_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(a);
}

} // namespace pmx_xpl
