// pmx_screen_walk.h - the tree phase of the screening path (device): the depth-first walker over a prepared ligand's tables, its
// bound tests (probe, path_bound, path_bound_wide), and the two functions the kernels of pmx_screen.hip call around it - prepare_walk
// (subtree record -> walker state) and run_job (walk, hand-over to the task queue, score). Tables and helpers: pmx_screen_tables.h.
#pragma once
#include "pmx_screen_tables.h"

// ---- tuning constants of this file (-D through PMX_CXXFLAGS or tools/build_variant.py; none changes a layout; [MI355X] ms per bench pass)
#ifndef PMX_ROW_BATCH
#define PMX_ROW_BATCH 8 // table rows of the matched ancestors whose loads go out together, for_rows() (4: 107.9 against 105.4)
#endif
#ifndef PMX_PATH_WINDOWS
#define PMX_PATH_WINDOWS 3 // windows of 64 / G candidates whose loads go out together in path_bound() (1 / 2 / 3 / 4: 114.4 / 106.6 / 105.3 / 109.7 - no register for a fourth)
#endif
#ifndef PMX_PATH_MIN_LEVELS
#define PMX_PATH_MIN_LEVELS 3 // path_bound() is asked where the frame's level and at least this many - 1 more lie below (2 / 4: 106.3 / 107.5 against 105.4)
#endif
#ifndef PMX_SHARE_EVERY
#define PMX_SHARE_EVERY 16 // passes between two exchanges of maxima among the walkers of a split ligand, walk() (64: 102.0 against 99.0-99.5; 8 / 32: noise)
#endif

namespace PMX_NS {
using namespace pmx; // (pmx_device.h)

// ------------------------------------------------------------------------------------------------- walker
// Iterative form of ClusterMatchTree.dfs_run (tree.py:55-104) with wave-uniform control. Frame f is the tree node whose
// children are the candidates of level f (frame 0 = root). State of the current frame in scalars: nm = matches on the
// path, mask = conformers still valid (tree.py:78-84), nb = next candidate to look at, mx = max_num_matches so far
// (tree.py:96-97), flags = {this node is a match, a candidate child existed, skip child done}.
//
// One *pass* evaluates the next 64 / G candidates b of the frame at once (slot s <-> candidate nb + s, lane c <-> conformer):
//   valid(b, c) = mask(c) and P[q -> (f, b)][c] > 0 for every matched ancestor q          (tree.py:78-84)
//   total(b, c) = (total(parent, c) + S[f][b][c]) + sum_q P[q -> (f, b)][c]   in float64   (tree.py:38-41)
// and the walker descends into the first candidate that exists (some conformer valid). After the return the remaining
// candidates are evaluated again from nb on - nothing is cached per frame, which is what keeps the state in registers.
// A frame at the last level is finished inside its pass: every existing candidate is a leaf that feeds the per-conformer
// maximum (graph_match.py:103-109), then the skip leaf (tree.py:98-101).
//
// Exactness of pruning and splitting. `num_matches(A) + max_num_matches(A)` (tree.py:98) is the largest match count of a leaf
// below A's candidate children, so the skip rule only asks whether a node with >= 5 matches exists there. For a child Y
// of a frame with >= 4 matches (Y holds >= 5): every ancestor's skip decision is settled by Y's existence, decisions
// inside Y's subtree depend on candidate existence only (nm + mx < 5 is never true there), and its leaves only feed a
// per-conformer maximum. So Y may be (i) dropped when no leaf below it can exceed the maxima found so far - leaf totals
// are bounded by total(Y) + W[Y] (build_bounds) - and (ii) walked by another wavefront (task queue); both count as
// "returned >= 1" for the parent. A child Y with fewer than 5 matches whose bound fails feeds no maximum either; what its
// parent's decision (nm + mx < 5) needs from it is whether a node with >= 5 matches exists below it - probe() - and nothing
// once mx has reached 5 - nm through a sibling. The order in which children are visited changes neither maxima nor
// existence. Scores and every skip decision stay what the reference computes.

template <int G>
struct Walk {
    // tables of the job
    const unsigned char *Sb, *Pb, *Rb, *Wb, *Vb, *OBb; // (CI follows OB)
    int nl;
    uint32_t ksumtot;
    bool path_on = false; // the job's tables fit the wave's path-sum buffer: path_bound() may be used
    int hk, hks, hrow; // lane l: k[l], ksum[l], rowbase[l]
    // path: lane q holds match q
    int matB = 0, matKA = 0; // entry(match, x) - x = rowbase[j] + a * nd_j - ksum[j + 1] | a << 8 | j << 16
    // stack: lane f holds frame f
    int stA = 0, stB = 0, stC = 0; // mask lo, mask hi, nb | mx << 8 | flags << 16 | nm << 24
    double best = 0.0, flushed = 0.0;
    uint32_t frames = 0, passes = 0, npath = 0, ndrop = 0; // (npath / ndrop: path_bound() calls, children it dropped)
    // current frame (its state is in lane f of the stack like every other frame's; a walk can be interrupted and resumed, see kOverBudget)
    int f = 0, f0 = 0;
};
// entry((f, b) -> x) - x for a match (f, b): what lane q of Walk::matB holds for match q
template <int G>
__device__ __forceinline__ int match_base(const Walk<G> &w, int f, int b) {
    const int k1 = rl(w.hks, f + 1);
    return rl(w.hrow, f) + b * ((int)w.ksumtot - k1) - k1;
}
constexpr int kOverBudget = -1;

// per-level facts in bits 8.. of Walk::hk: the last level | its parent level with the children's leaves fused into its pass |
// a level whose children's totals are cached (slot number in bits 12..14)
constexpr int kLvLeaf = 256, kLvFuse = 512, kLvCache = 1024;
constexpr unsigned kMatched = 1, kAny = 2, kSkipped = 4, kCached = 8, kFused = 16, kFiltered = 32, kPath = 64; // kPath: the path sums of this frame's matches are in the wave's buffer
constexpr int kPathMinLevels = PMX_PATH_MIN_LEVELS;
constexpr int kPathWindows = PMX_PATH_WINDOWS;

// Row loops of the walker: `load(q)` for q = 0 .. n - 1 go out kRowBatch at a time and `use(value)` takes them in order; what is
// left at the end goes out as ONE batch too. (A remainder loop that loads one row, waits, uses it and loads the next costs a
// memory round trip per row: with 7 matched ancestors - the average of a table pass - that was four round trips instead of two.)
constexpr int kRowBatch = PMX_ROW_BATCH;
template <int N, typename Load, typename Use>
__device__ __forceinline__ void rows_batch(int q, Load &&load, Use &&use) {
    decltype(load(0)) v[N];
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = load(q + u);
#pragma unroll
    for (int u = 0; u < N; ++u) use(v[u]);
}
template <typename Load, typename Use>
__device__ __forceinline__ void for_rows(int n, Load &&load, Use &&use) {
    int q = 0;
    for (; q + kRowBatch <= n; q += kRowBatch) rows_batch<kRowBatch>(q, load, use);
    static_assert(kRowBatch == 4 || kRowBatch == 8, "remainder cases");
    if (kRowBatch == 8 && n - q >= 4) {
        switch (n - q) {
        case 7: rows_batch<7>(q, load, use); break;
        case 6: rows_batch<6>(q, load, use); break;
        case 5: rows_batch<5>(q, load, use); break;
        default: rows_batch<4>(q, load, use); break;
        }
        return;
    }
    switch (n - q) {
    case 3: rows_batch<3>(q, load, use); break;
    case 2: rows_batch<2>(q, load, use); break;
    case 1: rows_batch<1>(q, load, use); break;
    default: break;
    }
}

// Can the child (frame f, candidate `cand`, conformer mask `cmask`) of the current frame, which holds nm matches, still
// reach 5 matches - i.e. does the reference's tree hold a node with >= 5 matches below it? The same depth-first search on
// validity alone (no totals), stopped at the first such node; it follows the skip rule of tree.py:98, under which a node
// with >= 5 matches is reached whenever a valid assignment with >= 5 matches exists (see walk()). Uses the stack and path
// lanes above the current frame, which the walker re-writes when it descends itself.
template <int G>
__device__ __forceinline__ bool probe(Walk<G> &w, int f, int nm, int cand, uint64_t cmask, uint32_t &passes) {
    const int lane = lane_id();
    const int nl = w.nl;
    const unsigned char *Vb = w.Vb;
    if (nm + 1 >= 5) return true;
    // DP[x]: no chain of pairwise compatible candidates that starts with x holds more than DP[x] of them (chain_lengths()), so a
    // node with 5 matches lies below a path of nm matches through x only if DP[x] >= 5 - nm. The child itself first, then every
    // candidate the search would try: what they rule out is not there to find.
    const unsigned char *DP = w.OBb + (round16((uint64_t)ob_rows<G>((uint32_t)nl) * w.ksumtot * G * ob_elt_bytes<G>()) + (size_t)round16((uint64_t)w.ksumtot));
    if (uni((int)DP[rl(w.hks, f) + cand]) < 5 - nm) return false;
    // enter the child
    const int fbase = f;
    w.matB = wl(w.matB, nm, match_base(w, f, cand));
    w.matKA = wl(w.matKA, nm, (cand << 8) | (f << 16));
    ++f;
    ++nm;
    uint64_t mask = cmask;
    int nb = 0, mx = 0;
    unsigned flags = kMatched;
    for (;;) {
        int ret;
        if (f == nl) { // below the last level: a leaf
            ret = (flags & kMatched) ? 1 : 0;
        } else {
            const int kf = rl(w.hk, f) & 255, ksf = rl(w.hks, f);
            bool descended = false;
            if (nb < kf) {
                const int ebv = w.matB + ksf;
                // every candidate of the level at once, lane l <-> candidate l: which exist as children - some conformer of
                // the frame has every pair entry > 0 - is one AND of V masks per matched ancestor (no table row is read)
                constexpr uint32_t VB = vmask_bytes<G>();
                bool in = lane >= nb && lane < kf;
                const uint32_t lo_ = (uint32_t)(lane < kf ? lane : 0) * VB;
                const int reach = DP[(uint32_t)ksf + (lane < kf ? (uint32_t)lane : 0u)];
                auto vload = [&](int q) -> unsigned long long {
                    const unsigned char *ve = Vb + (uint32_t)rl(ebv, q) * VB + lo_;
                    if (G <= 8) return *ve;
                    else if (G == 16) return *reinterpret_cast<const uint16_t *>(ve);
                    else if (G == 32) return *reinterpret_cast<const uint32_t *>(ve);
                    else return *reinterpret_cast<const unsigned long long *>(ve);
                };
                unsigned long long m = mask;
                for_rows(nm, vload, [&](unsigned long long v) { m &= v; });
                in = in && reach >= 5 - nm;
                const unsigned long long ex = __ballot(in && m != 0ull);
                ++passes;
                if (!ex) {
                    nb = kf;
                } else {
                    flags |= kAny;
                    if (nm + 1 >= 5) return true; // a node with 5 matches
                    const int bsel = __ffsll(ex) - 1;
                    nb = bsel + 1;
                    w.stA = wl(w.stA, f, (int)(uint32_t)mask);
                    if (G > 32) w.stB = wl(w.stB, f, (int)(uint32_t)(mask >> 32));
                    w.stC = wl(w.stC, f, nb | (mx << 8) | ((int)flags << 16) | (nm << 24));
                    w.matB = wl(w.matB, nm, match_base(w, f, bsel));
                    w.matKA = wl(w.matKA, nm, (bsel << 8) | (f << 16));
                    mask = (uint64_t)(uint32_t)rl((int)(uint32_t)m, bsel);
                    if (G > 32) mask |= (uint64_t)(uint32_t)rl((int)(uint32_t)(m >> 32), bsel) << 32;
                    ++f;
                    ++nm;
                    flags = kMatched;
                    nb = 0;
                    mx = 0;
                    descended = true;
                }
            }
            if (descended) continue;
            if (!(flags & kSkipped) && (!(flags & kAny) || nm + mx < 5)) { // skip child (tree.py:98-101)
                flags |= kSkipped;
                w.stA = wl(w.stA, f, (int)(uint32_t)mask);
                if (G > 32) w.stB = wl(w.stB, f, (int)(uint32_t)(mask >> 32));
                w.stC = wl(w.stC, f, nb | (mx << 8) | ((int)flags << 16) | (nm << 24));
                ++f;
                flags = 0;
                nb = 0;
                mx = 0;
                continue;
            }
            ret = mx + ((flags & kMatched) ? 1 : 0);
        }
        --f;
        if (f <= fbase) return false; // the child's subtree is exhausted: no node with 5 matches
        const int sc = rl(w.stC, f);
        mask = (uint64_t)(uint32_t)rl(w.stA, f);
        if (G > 32) mask |= (uint64_t)(uint32_t)rl(w.stB, f) << 32;
        nb = sc & 255;
        mx = (sc >> 8) & 255;
        flags = (unsigned)(sc >> 16) & 255u;
        nm = (sc >> 24) & 255;
        mx = mx > ret ? mx : ret;
    }
}

// Path-aware bound (round 4). W[(f, b)] bounds what the levels below f can add under a child Y = (f, b) with every level
// above f at its *maximum* pair entry; with seven matches on the path that is far from what they do add. Here the deeper
// candidates are priced with the pair entries of the matches actually on the path: for a candidate x = (l, b') of a level l > f
//     v(x)[c] = OB[f][x][c] + sum_{q on the path, Y included} P[q -> x][c]        (left out unless every such entry is > 0)
// (OB: x's self entry + the maxima of the levels between f and l, build_bounds), a level adds at most max(0, max_x v(x)), and
// the subtree below Y at most the sum of that over the levels l > f: no leaf below Y exceeds total(Y) + that. Nothing else
// changes - a child that fails is dropped exactly as one that fails the W test (see walk(): "exactness"). The pair sums of
// the path are kept per match count in a buffer of the wave (pa[matches][candidate][conformer], float32: an upper bound needs
// no more; the sums are of non-negative terms, so rounding to nearest loses at most 2^-24 per addition, which the final
// factor covers) and extended by Y's entries here - they are the sums of Y's own frame when the walker goes there.
// On the bench library the walker enters 4 times fewer frames with it (tests/bound_study: 272 -> 69 per ligand), 9-13 times
// fewer on the fixture pockets.
template <int G>
__device__ __forceinline__ bool path_bound(const Walk<G> &w, const ScreenParams &p, float *pa, float *ub, const double *tch, const unsigned long long *pool,
                                           int f, int nm, int bsel, uint64_t cmask) {
    constexpr int SLOTS = 64 / G;
    const int lane = lane_id();
    const int s = lane / G, c = lane % G;
    const int nl = w.nl;
    const uint32_t ksumtot = w.ksumtot;
    const uint32_t x0 = (uint32_t)rl(w.hks, f + 1); // first candidate of the levels below f
    const float *Pf = reinterpret_cast<const float *>(w.Pb) + (long)match_base<G>(w, f, bsel) * G; // Y's entries: Pf[x * G + c] (the base may be negative, base + x is not)
    const unsigned char *OB = w.OBb + (size_t)f * ksumtot * G * ob_elt_bytes<G>();
    const unsigned char *LV = w.OBb + round16((uint64_t)nl * ksumtot * G * ob_elt_bytes<G>());
    const float *pin = pa + (size_t)nm * ksumtot * G;
    float *pout = pa + (size_t)(nm + 1) * ksumtot * G;
    for (int i = lane; i < (nl - f - 1) * G; i += 64) ub[(f + 1) * G + i] = 0.f;
    lds_sync();
    // kPathWindows windows of SLOTS candidates per trip, everything of a window in one round of loads (the entries of Y with the deeper
    // candidates are one contiguous run: no lookup in front of the pair rows)
    for (uint32_t x = x0; x < ksumtot; x += kPathWindows * SLOTS) {
        uint32_t xx[kPathWindows], lv[kPathWindows];
        float ob[kPathWindows], have[kPathWindows], pv[kPathWindows];
        bool on[kPathWindows];
#pragma unroll
        for (int u = 0; u < kPathWindows; ++u) {
            on[u] = x + (uint32_t)(u * SLOTS + s) < ksumtot;
            xx[u] = on[u] ? x + (uint32_t)(u * SLOTS + s) : x0;
            lv[u] = LV[xx[u]];
            if (ob_elt_bytes<G>() == 2) ob[u] = bf16_value(reinterpret_cast<const uint16_t *>(OB)[(size_t)xx[u] * G + c]);
            else ob[u] = reinterpret_cast<const float *>(OB)[(size_t)xx[u] * G + c];
            have[u] = nm ? pin[(size_t)xx[u] * G + c] : 0.f;
            pv[u] = Pf[(size_t)xx[u] * G + c];
        }
#pragma unroll
        for (int u = 0; u < kPathWindows; ++u) {
            const float sum = pv[u] > 0.f ? have[u] + pv[u] : -__builtin_inff(); // (-inf stays -inf: a candidate out for this conformer stays out)
            if (on[u]) {
                pout[(size_t)xx[u] * G + c] = sum;
                const float v = fmaxf(sum + ob[u], 0.f); // (a NaN self entry - zero weights - can raise no maximum: 0)
                atomicMax(reinterpret_cast<unsigned int *>(ub) + lv[u] * G + (uint32_t)c, __float_as_uint(v));
            }
        }
    }
    lds_sync();
    float below = 0.f;
    for (int l = f + 1; l < nl; ++l) below = below + ub[l * G + c];
    const double bound = (double)below * (1.0 + 4e-6);
    const double pooled = __longlong_as_double((long long)pool[c]);
    const double bp = pooled > w.best ? pooled : w.best;
    return __ballot(((cmask >> c) & 1ull) && (tch[c] + bound) * kBoundSlack > bp) != 0ull;
}

// The path-aware test where a pass holds one or two candidates (32 / 64 conformer lanes). There the test above would move a row of
// every deeper candidate per evaluation (250-300 candidates x 64 conformers of the stress model: a quarter of a megabyte). But under
// a path of five matches hardly any deeper candidate is still compatible with ALL of them (a pair of candidates is compatible in
// a fifth of the cases on that model), and which ones are is in the V masks: with the lanes spread over the deeper candidates, one
// AND of masks per match on the path - the child Y = (f, bsel) included - lists them, 64 candidates per trip and 8 bytes per
// candidate and match. Every candidate x left is priced at BF[x] = base(x) rounded up - its self entry plus, for EVERY level above
// its own, the largest pair entry any candidate of that level has with it (build_bounds): no leaf adds more for x whatever is matched
// above it - for the conformers its mask still holds; a level adds at most the largest of its candidates, the subtree below Y at
// most the sum over the levels. Candidate numbers ascend with the level, so the level maxima are a running maximum: no LDS. A child
// that fails is dropped like one that fails the level-bound test (it holds >= 5 matches: nothing else is asked of it).
// tests/bound_study (model_stress64, 16 ligands x 64 conformers): the level bound in index order enters 10 036 frames per ligand,
// this test under >= 5 matches 1 187 with 1 344 evaluations (with the pair entries of the path and the OB table as above: 757).
template <int G>
__device__ __forceinline__ bool path_bound_wide(const Walk<G> &w, const double t /* the child's total, in the lanes of its slot: */, const bool sel,
                                                const unsigned long long *pool, int f, int nm, int bsel, uint64_t cmask) {
    static_assert(G >= 32, "lanes over candidates, conformer masks of 32 / 64 bits");
    constexpr uint32_t VB = vmask_bytes<G>();
    const int lane = lane_id();
    const int c = lane % G;
    const uint32_t ksumtot = w.ksumtot;
    const uint32_t x0 = (uint32_t)rl(w.hks, f + 1); // first candidate of the levels below f
    const float *BF = reinterpret_cast<const float *>(w.OBb);
    const unsigned char *LV = w.OBb + round16((uint64_t)ksumtot * G * 4u);
    const unsigned char *Vy = w.Vb + (long)match_base<G>(w, f, bsel) * (long)VB; // Y's masks: Vy + x * VB (the base may be negative, base + x is not)
    float below = 0.f, cur = 0.f;
    int cur_lv = -1;
    for (uint32_t xb = x0; xb < ksumtot; xb += 64u) {
        const uint32_t x = xb + (uint32_t)lane;
        const bool in = x < ksumtot;
        const uint32_t xo = (in ? x : x0) * VB;
        auto vload = [&](int q) -> unsigned long long {
            const unsigned char *ve = w.Vb + (long)rl(w.matB, q) * (long)VB + xo;
            if (G == 32) return *reinterpret_cast<const uint32_t *>(ve);
            else return *reinterpret_cast<const unsigned long long *>(ve);
        };
        unsigned long long m = cmask;
        if (G == 32) m &= *reinterpret_cast<const uint32_t *>(Vy + xo);
        else m &= *reinterpret_cast<const unsigned long long *>(Vy + xo);
        const int lvl = LV[in ? x : x0];
        for_rows(nm, vload, [&](unsigned long long v) { m &= v; });
        unsigned long long ex = __ballot(in && m != 0ull);
        while (ex) { // the candidates still compatible with the whole path, in ascending order
            const int xl = __ffsll(ex) - 1;
            ex &= ex - 1ull;
            uint64_t mm = (uint64_t)(uint32_t)rl((int)(uint32_t)m, xl);
            if (G > 32) mm |= (uint64_t)(uint32_t)rl((int)(uint32_t)(m >> 32), xl) << 32;
            const int lv = rl(lvl, xl);
            const float bf = BF[(size_t)(xb + (uint32_t)xl) * G + c];
            if (lv != cur_lv) {
                below = below + cur;
                cur = 0.f;
                cur_lv = lv;
            }
            const float v = ((mm >> c) & 1ull) ? bf : 0.f;
            cur = fmaxf(cur, v); // (a NaN base - zero weights - raises no maximum)
        }
    }
    below = below + cur;
    const double bound = (double)below * (1.0 + 4e-6);
    const double pooled = __longlong_as_double((long long)pool[c]);
    const double bp = pooled > w.best ? pooled : w.best;
    return __ballot(sel && ((cmask >> c) & 1ull) && (t + bound) * kBoundSlack > bp) != 0ull;
}

// The path sums of the wave's buffer for a job that starts with matches on its path (a queued subtree): the rows of match
// after match, as path_bound() would have left them.
template <int G>
__device__ __forceinline__ void path_sums_of_root(const Walk<G> &w, float *pa, int nm0) {
    constexpr int SLOTS = 64 / G;
    const int lane = lane_id();
    const int s = lane / G, c = lane % G;
    const uint32_t ksumtot = w.ksumtot;
    for (int q = 0; q < nm0; ++q) {
        const uint32_t jq = ((uint32_t)rl(w.matKA, q) >> 16) & 255u;
        const uint32_t x0 = (uint32_t)rl(w.hks, (int)jq + 1);
        const float *Pq = reinterpret_cast<const float *>(w.Pb) + (long)rl(w.matB, q) * G;
        const float *pin = pa + (size_t)q * ksumtot * G;
        float *pout = pa + (size_t)(q + 1) * ksumtot * G;
        for (uint32_t x = x0; x < ksumtot; x += SLOTS) {
            const bool on = x + (uint32_t)s < ksumtot;
            const uint32_t xx = on ? x + (uint32_t)s : x0;
            const float pv = Pq[(size_t)xx * G + c];
            const float have = q ? pin[(size_t)xx * G + c] : 0.f;
            if (on) pout[(size_t)xx * G + c] = pv > 0.f ? have + pv : -__builtin_inff();
        }
        wave_sync(); // (the next match reads what this one wrote)
    }
}

template <int G>
__device__ __forceinline__ int walk(Walk<G> &w, const ScreenParams &p, double *tot, unsigned long long *pool, uint16_t *pathbuf, double *tch, double *tc,
                                    unsigned long long *cbl, float *pa, float *ub, uint32_t rec16 /* arena record of the job (exports refer to it) */, bool export_mode,
                                    unsigned long long budget, uint32_t wave_id, WaveStats *stat) {
    constexpr int SLOTS = 64 / G;
    constexpr int PSH = G == 1 ? 2 : G == 2 ? 3 : G == 4 ? 4 : G == 8 ? 5 : G == 16 ? 6 : G == 32 ? 7 : 8; // log2 bytes of an entry
    constexpr uint64_t GM = group_mask<G>();
    const int lane = lane_id();
    const int s = lane / G, c = lane % G;
    const uint32_t lane_off = (uint32_t)lane * 4u; // (s * G + c) floats: candidate nb + s, conformer c
    const int nl = w.nl;
    const unsigned char *Sb = w.Sb, *Pb = w.Pb, *Wb = w.Wb, *Vb = w.Vb;
    const int bound_from = (PMX_WFLAGS(p) & 4) ? 255 : 4; // matches on the path from which children are bound-tested
    const bool no_filter = (PMX_WFLAGS(p) & 128) != 0;

    const uint32_t budget32 = (export_mode || budget > 0xfffffff0ull) ? 0xffffffffu : (uint32_t)budget; // (a walk of 2^32 passes does not end in this life)
    const int f0 = w.f0;
    // The only scalar carried from one iteration to the next is the frame number: every frame's state - the current one's
    // too - lives in lane f of stA / stB / stC and is read at the top of an iteration and written back at its end. (With the
    // current frame in scalars of its own, a third of the walker's instructions were copies between registers where the many
    // paths of the loop meet.) One iteration = one pass over the frame's next candidates, or the end of the frame.
    int f = w.f;
    int ret = 0;
    // The walkers of a split ligand (its subtrees, and the walk that queued them) trade maxima through the ligand's record
    // while they run, not only when they end: one returning atomic maximum per conformer every kShareEvery passes gives this
    // wave's maxima to the others and theirs to this wave's bound test. (Maxima of leaves of the same tree: exact.)
    constexpr uint32_t kShareEvery = PMX_SHARE_EVERY;
    uint32_t next_share = w.passes + kShareEvery;
#ifdef PMX_COUNTERS
    uint32_t dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // fused passes | fused children | cached passes | leaf passes | other passes from the tables | descents | ancestors over table passes | shares
    auto flush_dbg = [&]() {
        if (lane == 0)
            for (int i = 0; i < 6; ++i) stat->dbg[i] += dbg[i];
    };
#else
    auto flush_dbg = [&]() {};
#endif
    for (;;) {
        inject_valu<PMX_INJECT_VALU_WALK>();
        inject_salu<PMX_INJECT_SALU_WALK>();
        if (w.passes > budget32) { // over budget: the caller moves the job's tables to the arena and resumes in export mode
            w.f = f;
            flush_dbg();
            return kOverBudget;
        }
        if (rec16 != 0u && w.passes >= next_share && !(PMX_WFLAGS(p) & 8192)) {
            next_share = w.passes + kShareEvery;
            PMX_COUNT(7, 1);
            if (s == 0) {
                unsigned long long *gb = reinterpret_cast<unsigned long long *>(p.arena + (size_t)rec16 * 16 + sizeof(RecHeader));
                const unsigned long long mine = pool[c];
                const unsigned long long theirs = mine ? atomicMax(&gb[c], mine) : __hip_atomic_load(&gb[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (theirs > mine) pool[c] = theirs;
            }
            lds_sync();
        }
        const int sc = rl(w.stC, f);
        int nb = sc & 255, mx = (sc >> 8) & 255;
        unsigned flags = (unsigned)(sc >> 16) & 255u;
        const int nm = (sc >> 24) & 255;
        uint64_t mask = (uint64_t)(uint32_t)rl(w.stA, f);
        if (G > 32) mask |= (uint64_t)(uint32_t)rl(w.stB, f) << 32;
        // what is fixed per level was worked out once per job (prepare_walk): bits 8.. of the level's entry
        const int hv = rl(w.hk, f);
        const int kf = hv & 255, ksf = rl(w.hks, f);
        const bool leaf_level = (hv & kLvLeaf) != 0;
        // ordered frames: of the candidates of a pass (a window of the frame's candidates) the walker visits the surviving child
        // with the largest bound first; rem = the slots of the window not visited yet, in lane f of stB
        constexpr bool ORD = G >= 2 && G <= 32;
        const bool ordered0 = ORD && !leaf_level && !(hv & kLvFuse) && !(PMX_WFLAGS(p) & 2048);
        uint32_t rem = 0xffffffffu;
        if (ORD) rem = (uint32_t)rl(w.stB, f);
        if (nb < kf) {
            // ---------------------------------------------------------------- one pass over candidates nb .. nb + SLOTS - 1
            const double tparent = tot[nm * G + c];
            // the bound row and the pooled maxima go out with the table loads (one memory round trip per pass, not two); frames
            // f < nl only, so row f + 1 exists
            const bool bounded = nm >= bound_from && !leaf_level;
            double pooled = 0.0;
            if (bounded || ordered0) pooled = __longlong_as_double((long long)pool[c]);
            // pair-table rows of the matched ancestors against level f: lane q
            const int ebv = w.matB + ksf;
            // A frame with more candidates than slots is *filtered* first: which candidates exist as children - some conformer of
            // the frame has every pair entry > 0 - is read off the V masks with the lanes spread over candidates, and the passes
            // then take the existing candidates only, SLOTS at a time (most candidates do not exist: without this a frame of a
            // large model, or of a 64-conformer library with one slot per pass, spends its passes on them).
            bool filt = false;
            unsigned long long cb = 0, cb_rest = 0;
            int bvec = nb + s; // the candidate of this lane's slot
            if constexpr (SLOTS <= 2) { // (with 8 slots - the 8-conformer shape - the filter's own pass costs more than it saves: measured)
                filt = kf > SLOTS && nm > 0 && !no_filter;
                if (filt) {
                    if (!(flags & kFiltered)) {
                        constexpr uint32_t VB = vmask_bytes<G>();
                        const bool in = lane < kf;
                        const uint32_t lo_ = (uint32_t)(in ? lane : 0) * VB;
                        unsigned long long m = mask;
                        auto vload = [&](int q) -> unsigned long long {
                            const unsigned char *ve = Vb + (uint32_t)rl(ebv, q) * VB + lo_;
                            if (G <= 8) return *ve;
                            else if (G == 16) return *reinterpret_cast<const uint16_t *>(ve);
                            else if (G == 32) return *reinterpret_cast<const uint32_t *>(ve);
                            else return *reinterpret_cast<const unsigned long long *>(ve);
                        };
                        for_rows(nm, vload, [&](unsigned long long v) { m &= v; });
                        cb = __ballot(in && m != 0ull);
                        flags |= kFiltered;
                        ++w.passes;
                        if (cb == 0ull) { // no child exists: the frame's candidates are done
                            w.stC = wl(w.stC, f, 255 | (mx << 8) | ((int)flags << 16) | (nm << 24));
                            continue;
                        }
                    } else {
                        cb = uni64(cbl[f]);
                    }
                    unsigned long long x = cb;
                    bvec = 255;
#pragma unroll
                    for (int ss = 0; ss < SLOTS; ++ss) {
                        const int bb = x ? __ffsll(x) - 1 : 255;
                        x &= x - 1ull;
                        bvec = s == ss ? bb : bvec;
                    }
                    cb_rest = x;
                }
            }
            const bool ordered = ordered0 && !filt;
            const bool on = bvec < kf;
            const int b_first = filt ? (cb ? __ffsll(cb) - 1 : 0) : nb; // a candidate idle slots may read (in bounds)
            // the candidate's bound goes out with the table loads (one memory round trip per pass, not two)
            double rbound = 0.0;
            if (bounded || (ordered && cand_bounds<G>())) { // (the bound also orders the children of frames it cannot drop yet)
                if constexpr (cand_bounds<G>()) rbound = *reinterpret_cast<const double *>(Wb + (((uint32_t)(ksf + (on ? bvec : b_first))) << (PSH + 1)) + 8u * (uint32_t)c);
                else rbound = *reinterpret_cast<const double *>(w.Rb + (((uint32_t)(f + 1) << (PSH + 1)) + 8u * (uint32_t)c));
            }
            double t;
            bool valid;
            // cache slot of this frame: the kTcLevels frames above the fused one, one pass wide
            const int tci = (hv >> 12) & 7;
            const bool cacheable = (hv & kLvCache) != 0;
            if (cacheable && (flags & kCached)) { // back from a child: the remaining candidates as evaluated on the way in
                const unsigned long long vb0 = *reinterpret_cast<const unsigned long long *>(tc + kTcLevels * 64 + tci);
                const int src = lane + nb * G;
                t = tc[tci * 64 + (on ? src : lane)];
                valid = on && ((uni64(vb0) >> src) & 1ull);
                PMX_COUNT(2, 1);
            } else {
                PMX_COUNT(leaf_level ? 3 : 4, 1);
                PMX_COUNT(6, nm);
                const uint32_t bo = ((uint32_t)(on ? bvec : b_first) << PSH) + (uint32_t)c * 4u; // idle slots read an existing candidate
                const float self = *reinterpret_cast<const float *>(Sb + (((uint32_t)ksf << PSH) + bo));
                float lo = 1.f; // smallest pair entry: the candidate is valid for this conformer iff every entry is > 0 (tree.py:81)
                double sum = 0.0;
                for_rows(
                    nm, [&](int q) { return *reinterpret_cast<const float *>(Pb + (((uint32_t)rl(ebv, q) << PSH) + bo)); },
                    [&](float v) {
                        lo = fminf(lo, v);
                        sum += (double)v;
                    });
                // (v_min_f32 skips a NaN entry - a zero-weight pair, match_utils.py:50-52 - but the sum does not: NaN is not > 0)
                valid = on && ((mask >> c) & 1ull) && lo > 0.f && sum == sum;
                t = (tparent + (double)self) + sum; // parent + self + accumulated pair (tree.py:38-41)
            }
            if (ordered) valid = valid && ((rem >> s) & 1u);
            const unsigned long long vb = __ballot(valid);
            if (cacheable && !(flags & kCached)) { // first pass of the frame (a cached frame has one window)
                tc[tci * 64 + lane] = t;
                if (lane == 0) *reinterpret_cast<unsigned long long *>(tc + kTcLevels * 64 + tci) = vb;
                flags |= kCached;
            }
            ++w.passes;
            if (vb) flags |= kAny;
            unsigned long long ab = vb;
#if defined(PMX_COUNTERS) && PMX_COUNTERS == 2
            const unsigned long long dbg_vb = vb;
#endif
            // Children with fewer than 5 matches are bound-tested too where the frame is ordered: nothing below a child that
            // fails can raise a maximum, so all the frame still needs from it is whether it reaches 5 matches (tree.py:98) -
            // nothing at all once another child has (max_num_matches is a maximum), else what probe() answers.
            const bool shallow = ordered && cand_bounds<G>() && nm < 4 && bound_from != 255 && !(PMX_WFLAGS(p) & 4096);
            if ((bounded || shallow) && vb) { // drop the children that cannot raise a maximum
                const double bp = pooled > w.best ? pooled : w.best;
                ab = __ballot(valid && (t + rbound) * kBoundSlack > bp);
            }
#if defined(PMX_COUNTERS) && PMX_COUNTERS == 2
            { // what the bound test does: [0] passes without an existing child [1] passes whose existing children are all dropped [2] existing children [3] survivors [4] passes under >= 5 matches [5] survivors under >= 5 matches [6] existing under >= 5
                auto slots = [&](unsigned long long b) { int n = 0; for (int ss = 0; ss < SLOTS; ++ss) n += ((b >> (ss * G)) & GM) ? 1 : 0; return n; };
                dbg[0] += dbg_vb == 0;
                dbg[1] += dbg_vb != 0 && ab == 0;
                dbg[2] += slots(dbg_vb);
                dbg[3] += slots(ab);
                dbg[4] += nm >= 4;
                dbg[5] += nm >= 4 ? slots(ab) : 0;
                dbg[6] += nm >= 4 ? slots(dbg_vb) : 0;
            }
#endif
            int probe_slot = -1; // a child of this pass whose reach is probed (one call site)
            bool probe_rem_done = false;
            bool handled = false, pending = false;
            if (shallow && ab != vb) {
                const bool slot_vb = ((vb >> (s * G)) & GM) != 0, slot_ab = ((ab >> (s * G)) & GM) != 0;
                const unsigned long long dropped = __ballot(c == 0 && slot_vb && !slot_ab);
                if (dropped) {
                    if (mx >= 5 - nm) { // a sibling reached 5 matches already: the dropped children change nothing
                        rem &= ~(uint32_t)__ballot(lane < SLOTS && ((dropped >> ((lane * G) & 63)) & 1ull));
                    } else if (!ab) { // nothing left to walk: the frame has to know
                        probe_slot = (__ffsll(dropped) - 1) / G;
                        handled = true;
                    } else { // the survivors first: one of them reaching 5 matches saves the probes
                        pending = true;
                    }
                }
            }
            if (handled) {
            } else if (leaf_level) {
                if (valid && t > w.best) w.best = t; // graph_match.py:105-108
                nb += SLOTS;
                cb = cb_rest;
            } else if (hv & kLvFuse) {
                // The children of this frame are frames of the last level, whose children are leaves: finish all of them here.
                // Lane (s', c) takes leaf candidate s' of level f + 1; what a leaf's total and validity owe to the path above
                // this frame is computed once, then every surviving child b of this pass adds its own pair entry:
                //   total(b, b') = (total(b) + S[f + 1][b']) + (sum_q P[q -> (f + 1, b')] + P[(f, b) -> (f + 1, b')])   (tree.py:38-41)
                // in the reference's order (the child is the deepest ancestor, so its entry comes last).
                if (ab) {
                    PMX_COUNT(0, 1);
                    const int f1 = f + 1, k1 = rl(w.hk, f1) & 255, ks1 = rl(w.hks, f1);
                    tch[lane] = t; // the children's totals, read back per child by every slot
                    const int ebv1 = w.matB + ks1;
                    const bool on1 = s < k1;
                    const uint32_t bo1 = on1 ? lane_off : (uint32_t)c * 4u;
                    const float self1 = *reinterpret_cast<const float *>(Sb + (((uint32_t)ks1 << PSH) + bo1));
                    bool base_valid = on1;
                    double base_sum = 0.0;
                    for_rows(
                        nm, [&](int q) { return *reinterpret_cast<const float *>(Pb + (((uint32_t)rl(ebv1, q)) << PSH) + bo1); },
                        [&](float v) { // added in order
                            base_valid = base_valid & (v > 0.f);
                            base_sum += (double)v;
                        });
                    // entry((f, b) -> (f + 1, b')) = rowbase[f] + b * k1 + b'
                    const uint32_t row_f = (uint32_t)rl(w.hrow, f), nd_f = w.ksumtot - (uint32_t)ks1; // entry((f, b) -> (f + 1, b')) = rowbase[f] + b * nd_f + b'
                    lds_sync();
                    unsigned long long left = ab;
                    while (left) {
                        const int sb = (__ffsll(left) - 1) / G;
                        left &= ~(GM << (sb * G));
                        const uint64_t cm = (vb >> (sb * G)) & GM;
                        const double tb = tch[sb * G + c];
                        const float pfb = *reinterpret_cast<const float *>(Pb + ((row_f + (uint32_t)rl(bvec, sb * G) * nd_f) << PSH) + bo1);
                        const bool v1 = base_valid && pfb > 0.f && ((cm >> c) & 1ull);
                        const double t1 = (tb + (double)self1) + (base_sum + (double)pfb);
                        const bool any1 = __ballot(v1) != 0;
                        if (v1 && t1 > w.best) w.best = t1;                                             // leaves (graph_match.py:105-108)
                        if ((!any1 || nm < 3) && ((cm >> c) & 1ull) && tb > w.best) w.best = tb;        // the child's skip leaf (tree.py:98-101)
                        const int r1 = 1 + (any1 ? 1 : 0);
                        mx = mx > r1 ? mx : r1;
                        ++w.frames;
                        PMX_COUNT(1, 1);
                    }
                    w.passes += 1;
                }
                if (vb) mx = mx > 1 ? mx : 1; // (children dropped by the bound test return at least 1)
                nb += SLOTS;
                cb = cb_rest;
                flags |= kFused;
            } else if (ab) {
                bool keep = true; // the walker descends itself
                if (export_mode && nl - (f + 1) >= (int)p.min_levels) {
                    // Over budget: hand the surviving children of this pass to the task queue - one reservation, one record
                    // per slot. Children with >= 5 matches count as "returned >= 1" (see above). Below that the frame needs
                    // to know whether a child reaches 5 matches (tree.py:98), which probe() answers: only the first
                    // surviving child is handed over then, and this frame's max_num_matches is raised to 5 - nm if
                    // the child can get there (what it returns beyond that changes no decision anywhere).
                    const bool deep = nm >= 4;
                    const int first_ss = (__ffsll(ab) - 1) / G;
                    bool slot_alive = ((ab >> (s * G)) & GM) != 0;
                    if (!deep) slot_alive = slot_alive && s == first_ss;
                    const unsigned long long heads = __ballot(slot_alive && c == 0);
                    const uint32_t n = (uint32_t)__popcll(heads);
                    // all subtrees of a ligand go to one shard, and the task wavefronts of one XCD drain one group of
                    // shards (task_kernel): the walkers that share a ligand's tables run side by side under one L2
                    const uint32_t sh = (PMX_WFLAGS(p) & 256) ? ((wave_id + (uint32_t)(w.passes >> 4)) & (kShards - 1)) : ((rec16 * 2654435761u) >> 26);
                    static_assert(kShards == 64, "shard hash");
                    // one atomic add reserves the records (no retry loop: the walkers of one ligand export to one shard at
                    // the same time); a reservation that crosses the end of the shard fills its part below the end
                    // with empty subtrees of this ligand (no conformer: prepare_walk drops them)
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&p.ctl->q_res[sh], n);
                    base = (uint32_t)uni((int)base);
                    if (base + n > p.qcap) {
                        for (uint32_t i = base + (uint32_t)lane; i < p.qcap; i += 64u) {
                            uint32_t *nr = reinterpret_cast<uint32_t *>(p.queue + ((size_t)sh * p.qcap + i) * task_rec_bytes<G>());
                            for (uint32_t wd = 0; wd < task_rec_bytes<G>() / 4; ++wd) nr[wd] = 0u;
                            nr[0] = rec16;
                            nr[1] = (uint32_t)(f + 1) | (5u << 8); // f0, nm
                        }
                        base = 0xffffffffu;
                    }
                    if (base != 0xffffffffu) {
                        if (lane < nm) pathbuf[lane] = (uint16_t)(((w.matKA >> 16) & 255) | (((w.matKA >> 8) & 255) << 8));
                        lds_sync();
                        if (slot_alive) {
                            const uint32_t rank = (uint32_t)__popcll(heads & ((1ull << (s * G)) - 1ull));
                            unsigned char *tr = p.queue + ((size_t)sh * p.qcap + base + rank) * task_rec_bytes<G>();
                            TaskRec *th = reinterpret_cast<TaskRec *>(tr);
                            if (c == 0) {
                                th->rec16 = rec16;
                                th->f0 = (uint8_t)(f + 1);
                                th->nm = (uint8_t)(nm + 1);
                                th->pad = 0;
                                th->mask = (vb >> (s * G)) & GM;
                            }
                            const uint32_t mine = (uint32_t)f | ((uint32_t)bvec << 8); // this slot's own match, entry nm
                            for (int wd = c; wd < PMX_MAX_LEVELS / 2; wd += G) { // two path entries per 32-bit word
                                const int q0 = 2 * wd, q1 = 2 * wd + 1;
                                const uint32_t e0 = q0 < nm ? pathbuf[q0] : (q0 == nm ? mine : 0u);
                                const uint32_t e1 = q1 < nm ? pathbuf[q1] : (q1 == nm ? mine : 0u);
                                reinterpret_cast<uint32_t *>(th->path)[wd] = e0 | (e1 << 16);
                            }
                            reinterpret_cast<double *>(tr + sizeof(TaskRec))[c] = t;
                        }
                        if (lane == 0) stat->overflow += n; // (records written to the queue)
                        if (deep) {
                            mx = mx > 1 ? mx : 1; // children given away (or dropped) return at least 1
                            nb += SLOTS;
                            rem = 0xffffffffu;
                            cb = cb_rest;
                        } else {
                            probe_slot = first_ss;
                        }
                        keep = false;
                    } else if (lane == 0) {
                        p.ctl->qflag = 1; // shard full: walk the subtree here
                    }
                }
                if (keep) {
                    // descend into the first surviving child (tree.py:94-97)
                    int ss;
                    bool go = true;           // (false: the chosen child fails the path-aware bound test and is dropped)
                    unsigned child_path = 0u; // kPath if the child's path sums are in the wave's buffer
                    if (ordered) {
                      // A child that fails the path-aware test is dropped and the next survivor of the same pass is tried at once: nothing the
                      // next trip round the loop would work out again (the pass from the cache or the tables, its bound test) has changed.
                      const bool path_test = cand_bounds<G>() && (flags & kPath) && nl - f >= kPathMinLevels && !(PMX_WFLAGS(p) & 1024);
                      for (;;) {
                        const bool alive = (ab >> lane) & 1ull;
                        const float key = alive ? fmaxf((float)(t + rbound), 0.f) : -1.f; // (a NaN total orders as 0)
                        const float top = wave_max_f32(key);
                        ss = (__ffsll(__ballot(alive && key == top)) - 1) / G;
                        if (path_test) {
                            // the child with the largest W bound, against the bound its actual path gives (path_bound())
                            if (s == ss) tch[c] = t;
                            lds_sync();
#ifdef PMX_WALK_TICKS // instrumented builds: s_memtime ticks inside path_bound() and probe() in WaveStats::dbg[0], [1]
                            const unsigned long long tk0 = __builtin_amdgcn_s_memtime();
#endif
                            go = path_bound<G>(w, p, pa, ub, tch, pool, f, nm, rl(bvec, ss * G), (vb >> (ss * G)) & GM);
#ifdef PMX_WALK_TICKS
                            if (lane == 0) stat->dbg[0] += __builtin_amdgcn_s_memtime() - tk0;
#endif
                            child_path = kPath;
                            ++w.npath;
                            if (!go) ++w.ndrop;
                        }
                        if (vb != ab || !go) mx = mx > 1 ? mx : 1; // (an existing child - visited, dropped or probed - returns at least 1)
                        rem &= ~(1u << ss);
                        if (!(ab & ~(GM << (ss * G))) && !pending) { // no other survivor: the window ends with this child
                            nb += SLOTS;
                            rem = 0xffffffffu;
                        }
                        if (!go && nm < 4 && mx < 5 - nm) { // the frame still has to know whether the dropped child reaches 5 matches
                            probe_slot = ss;
                            probe_rem_done = true;
                        }
                        if (go || probe_slot >= 0 || !(ab & ~(GM << (ss * G)))) break;
                        ab &= ~(GM << (ss * G)); // (the dropped child leaves the survivors; the trip this saves counts as a pass)
                        ++w.passes;
                      }
                    } else {
                        ss = (__ffsll(ab) - 1) / G;
                        const unsigned long long before = ss == 0 ? 0ull : (vb & ((1ull << (ss * G)) - 1ull));
                        if (before) mx = mx > 1 ? mx : 1; // existing children dropped by the bound test return at least 1
                        if constexpr (G >= 32) {
                            const bool shallow_w = nm < 4 && bound_from != 255 && !(PMX_WFLAGS(p) & 4096) && !(PMX_WFLAGS(p) & 262144);
                            if ((bounded || shallow_w) && !(PMX_WFLAGS(p) & 131072)) { // the path-aware test of these shapes: children that passed the level bound, and children with fewer than 5 matches
                                go = path_bound_wide<G>(w, t, s == ss, pool, f, nm, rl(bvec, ss * G), (vb >> (ss * G)) & GM);
                                ++w.npath;
                                if (!go) {
                                    ++w.ndrop;
                                    const int bdrop = rl(bvec, ss * G);
                                    if (nm < 4 && mx < 5 - nm) { // the frame still has to know whether the dropped child reaches 5 matches (tree.py:98)
                                        probe_slot = ss;         // (the probe's own bookkeeping moves nb / cb past the child)
                                    } else {
                                        mx = mx > 1 ? mx : 1;
                                        nb = bdrop + 1;
                                        cb &= ~((2ull << bdrop) - 1ull);
                                    }
                                }
                            }
                        }
                    }
                    if (go) {
                    const int bsel = rl(bvec, ss * G);
                    if (!ordered) nb = bsel + 1;
                    if (filt) { // what is left of the frame's candidates (the slots below ss were dropped)
                        cb &= ~((2ull << bsel) - 1ull);
                        if (lane == 0) cbl[f] = cb;
                        nb = cb ? 0 : 255;
                    }
                    const uint64_t cmask = (vb >> (ss * G)) & GM;
                    if (s == ss) tot[(nm + 1) * G + c] = t;
                    // this frame's state, then the child's: lane f + 1
                    w.stC = wl(wl(w.stC, f, nb | (mx << 8) | ((int)flags << 16) | (nm << 24)), f + 1, ((int)(kMatched | child_path) << 16) | ((nm + 1) << 24));
                    w.stA = wl(w.stA, f + 1, (int)(uint32_t)cmask);
                    if (G > 32) w.stB = wl(w.stB, f + 1, (int)(uint32_t)(cmask >> 32));
                    if (ORD) w.stB = wl(wl(w.stB, f, (int)rem), f + 1, -1);
                    w.matB = wl(w.matB, nm, match_base(w, f, bsel));
                    w.matKA = wl(w.matKA, nm, (bsel << 8) | (f << 16));
                    ++f;
                    ++w.frames;
                    PMX_COUNT(5, 1);
                    if (totals_in_lds<G>()) lds_sync(); // the child's total is read by all slots
                    else wave_sync();
                    continue;
                    }
                }
            } else { // every existing child of this pass was dropped (or none existed)
                if (vb) mx = mx > 1 ? mx : 1;
                nb += SLOTS;
                rem = 0xffffffffu;
                cb = cb_rest;
            }
            if (probe_slot >= 0) { // (handed over, or dropped by the bound test: either way the walker does not go there)
                uint32_t pp = 0;
                const int bp_ = rl(bvec, probe_slot * G);
#ifdef PMX_WALK_TICKS
                const unsigned long long tk1 = __builtin_amdgcn_s_memtime();
#endif
                const bool reach = probe<G>(w, f, nm, bp_, (vb >> (probe_slot * G)) & GM, pp);
#ifdef PMX_WALK_TICKS
                if (lane == 0) stat->dbg[1] += __builtin_amdgcn_s_memtime() - tk1;
#endif
                if (lane == 0) {
                    stat->pad[0] += pp;
                    stat->pad[1] += 1;
                    stat->passes += pp;
                }
                mx = mx > 1 ? mx : 1;
                if (reach) mx = mx > 5 - nm ? mx : 5 - nm;
                if (ordered) {
                    if (!probe_rem_done) rem &= ~(1u << probe_slot);
                } else {
                    nb = bp_ + 1;
                }
                cb &= ~((2ull << bp_) - 1ull);
            }
            if (filt) {
                if (lane == 0) cbl[f] = cb;
                nb = cb ? 0 : 255;
            }
            if (nb < kf) { // more candidates: another pass
                w.stC = wl(w.stC, f, nb | (mx << 8) | ((int)flags << 16) | (nm << 24));
                if (ORD) w.stB = wl(w.stB, f, (int)rem);
                continue;
            }
        }
        // -------------------------------------------------------------------- the candidates of this frame are done
        if (leaf_level) {
            mx = (flags & kAny) ? 1 : 0;
            if (!(flags & kAny) || nm + mx < 5) { // skip leaf (tree.py:98-101, :42-43): this node's totals
                const double tparent = tot[nm * G + c];
                if (((mask >> c) & 1ull) && tparent > w.best) w.best = tparent;
            }
        }
        if (leaf_level || (flags & kFused)) {
            // publish improved maxima to the other slots (the bound test reads them)
            const bool up = w.best > w.flushed;
            if (__ballot(up)) {
                if (up) {
                    atomicMax(&pool[c], (unsigned long long)__double_as_longlong(w.best));
                    w.flushed = w.best;
                }
            }
        }
        if (!leaf_level && !(flags & kSkipped) && (!(flags & kAny) || nm + mx < 5)) { // skip child (tree.py:98-101)
            flags |= kSkipped;
            w.stC = wl(wl(w.stC, f, nb | (mx << 8) | ((int)flags << 16) | (nm << 24)), f + 1, ((int)(flags & kPath) << 16) | (nm << 24)); // (same matches: same path sums)
            w.stA = wl(w.stA, f + 1, (int)(uint32_t)mask);
            if (G > 32) w.stB = wl(w.stB, f + 1, (int)(uint32_t)(mask >> 32));
            if (ORD) w.stB = wl(w.stB, f + 1, -1);
            ++f;
            ++w.frames;
            continue;
        }
        // return max_num_matches + matched (tree.py:102) to the parent frame - and straight through every ancestor that has
        // nothing left to do: its candidates are done and it needs no skip child (it was entered for one of its children, so a
        // child existed: the skip child is due only while num_matches + max_num_matches < 5, tree.py:98). A third of the
        // walker's iterations used to be such returns, each a full trip round the loop.
        ret = mx + ((flags & kMatched) ? 1 : 0);
        bool out = false;
        for (;;) {
            --f;
            if (f < f0) {
                out = true;
                break;
            }
            int pc = rl(w.stC, f);
            int pmx = (pc >> 8) & 255;
            if (ret > pmx) {
                pmx = ret;
                pc = (pc & ~0xff00) | (ret << 8);
                w.stC = wl(w.stC, f, pc);
            }
            if ((pc & 255) < (rl(w.hk, f) & 255)) break;                                        // candidates left
            const int pfl = (pc >> 16) & 255, pnm = (pc >> 24) & 255;
            if (!(pfl & (int)kSkipped) && pnm + pmx < 5) break;                                  // its skip child is due
            ret = pmx + ((pfl & (int)kMatched) ? 1 : 0);
        }
        if (out) break;
    }
    flush_dbg();
    return ret;
}

// Subtree record -> walker state. Returns false when the subtree can no longer raise any maximum (the maxima may have grown
// since it was queued) and is dropped unwalked.
template <int G>
__device__ __forceinline__ bool prepare_walk(const ScreenParams &p, unsigned char *lds, const WaveShape<G> &ws, const unsigned char *tr, unsigned char *rec, Walk<G> &w) {
    const int lane = lane_id();
    const int s = lane / G, c = lane % G;
    double *tot = totals_in_lds<G>() ? reinterpret_cast<double *>(lds + ws.off_tot) : reinterpret_cast<double *>(p.totbuf + (size_t)blockIdx.x * kTotBufBytes);
    unsigned long long *pool = reinterpret_cast<unsigned long long *>(lds + ws.off_pool);
    const TaskRec *th = reinterpret_cast<const TaskRec *>(tr);
    const RecHeader *H = reinterpret_cast<const RecHeader *>(rec);
    const int nl = uni((int)H->nl);
    const uint32_t ksumtot = (uint32_t)uni((int)H->ksumtot), T = (uint32_t)uni((int)H->T);
    w.Sb = rec + rec_s_off<G>();
    w.Pb = rec + rec_p_off<G>(ksumtot);
    w.Rb = rec + rec_r_off<G>(ksumtot, T);
    w.Wb = rec + rec_w_off<G>(ksumtot, T, (uint32_t)nl);
    w.Vb = rec + rec_v_off<G>(ksumtot, T, (uint32_t)nl);
    w.OBb = rec + rec_ob_off<G>(ksumtot, T, (uint32_t)nl);
    w.nl = nl;
    w.ksumtot = ksumtot;
    // path_bound() keeps a row of pair sums per candidate and match count in the wave's buffer: used when they fit
    // (and the table word X holds a pair entry number in 20 bits)
    w.path_on = cand_bounds<G>() && !(PMX_WFLAGS(p) & (4u | 1024u)) && (uint64_t)(nl + 1) * ksumtot * G * 4u <= (uint64_t)p.pa_bytes && T < (1u << 20);
    {
        const int kl = lane < nl ? (int)H->k[lane] : 0, knext = lane + 1 < nl ? (int)H->k[lane + 1] : 0;
        const int tci = nl - 3 - lane;
        int kind = lane == nl - 1 ? kLvLeaf : 0;
        if (lane == nl - 2 && knext <= 64 / G && !(PMX_WFLAGS(p) & 32)) kind |= kLvFuse;
        if (totals_in_lds<G>() && tci >= 0 && tci < kTcLevels && kl <= 64 / G && !(PMX_WFLAGS(p) & 64)) kind |= kLvCache | (tci << 12);
        w.hk = kl | kind;
    }
    w.hks = lane <= nl ? (int)H->ksum[lane] : 0;
    w.hrow = lane < nl ? (int)H->rowbase[lane] : 0;
    const int nm0 = uni((int)th->nm), f0 = uni((int)th->f0);
    if (lane < nm0) {
        const int j = th->path[2 * lane], a = th->path[2 * lane + 1];
        w.matB = (int)H->rowbase[j] + a * ((int)ksumtot - (int)H->ksum[j + 1]) - (int)H->ksum[j + 1];
        w.matKA = (a << 8) | (j << 16);
    }
    const unsigned long long *gbest = reinterpret_cast<const unsigned long long *>(rec + sizeof(RecHeader));
    if (s == 0) {
        tot[nm0 * G + c] = reinterpret_cast<const double *>(tr + sizeof(TaskRec))[c];
        pool[c] = __hip_atomic_load(&gbest[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // maxima of the ligand's finished walkers
    }
    w.f = w.f0 = f0;
    const uint64_t mask0 = uni64(th->mask);
    w.stA = wl(w.stA, f0, (int)(uint32_t)mask0);
    if (G > 32) w.stB = wl(w.stB, f0, (int)(uint32_t)(mask0 >> 32));
    else w.stB = -1;
    w.stC = wl(w.stC, f0, (((nm0 ? (int)kMatched : 0) | (w.path_on ? (int)kPath : 0)) << 16) | (nm0 << 24));
    wave_sync();
    if (!(PMX_WFLAGS(p) & 4) && f0 < nl && nm0 >= 5) {
        const double r = *reinterpret_cast<const double *>(w.Rb + ((size_t)f0 * G + c) * 8);
        const double t = tot[nm0 * G + c];
        if (__ballot(((mask0 >> c) & 1ull) && (t + r) * kBoundSlack > __longlong_as_double((long long)pool[c])) == 0) return false;
    }
    if (cand_bounds<G>() && w.path_on && nm0 > 0) // a queued subtree: the pair sums of the matches it starts with
        path_sums_of_root<G>(w, reinterpret_cast<float *>(p.pabuf + (size_t)blockIdx.x * p.pa_bytes), nm0);
    return true;
}

// The tree search of a prepared job and what follows it: the maxima go to the score (a ligand walked by this wave alone) or to
// the ligand's record in the arena (a split ligand; finalize_kernel takes the mean). The walk is interrupted once, when it
// runs over its budget: a ligand's tables then move to the arena (queued subtrees refer to them) and the walk resumes handing
// subtrees with >= 5 matches to the queue.
template <int G>
__device__ __forceinline__ void run_job(const ScreenParams &p, unsigned char *lds, const WaveShape<G> &ws, Walk<G> &w, unsigned char *rec, uint32_t rec16,
                                        const bool is_task, const uint32_t wave_id, WaveStats *stat) {
    const int lane = lane_id();
    const int s = lane / G, c = lane % G;
    double *tot = totals_in_lds<G>() ? reinterpret_cast<double *>(lds + ws.off_tot) : reinterpret_cast<double *>(p.totbuf + (size_t)blockIdx.x * kTotBufBytes);
    unsigned long long *pool = reinterpret_cast<unsigned long long *>(lds + ws.off_pool);
    uint16_t *pathbuf = reinterpret_cast<uint16_t *>(lds + kOffPath);
    double *tch = reinterpret_cast<double *>(lds + ws.off_tch);
    double *tc = reinterpret_cast<double *>(lds + ws.off_tc);
    unsigned long long *cbl = reinterpret_cast<unsigned long long *>(lds + ws.off_cb);
    float *pa = reinterpret_cast<float *>(p.pabuf + (size_t)blockIdx.x * p.pa_bytes);
    float *ub = reinterpret_cast<float *>(lds + ws.off_ub);
    const unsigned long long t_d = __builtin_amdgcn_s_memtime();
    unsigned long long budget = ((PMX_WFLAGS(p) & 2) || p.last_round) ? ~0ull : (unsigned long long)p.budget;
    bool export_mode = false, split = is_task;
    for (;;) {
        const int rc = walk<G>(w, p, tot, pool, pathbuf, tch, tc, cbl, pa, ub, rec16, export_mode, budget, wave_id, stat);
        if (rc != kOverBudget) break;
        if (lane == 0) ++stat->over;
        budget = ~0ull;
        RecHeader *H = reinterpret_cast<RecHeader *>(rec);
        if (rec16 == 0) { // tables in the wave's slice: move them to the arena
            const uint32_t bytes = (uint32_t)uni((int)H->bytes);
            const unsigned long long off = arena_alloc(p, bytes);
            if (off != ~0ull) {
                const uint4 *src = reinterpret_cast<const uint4 *>(rec);
                uint4 *dst = reinterpret_cast<uint4 *>(p.arena + off);
                const uint32_t n16 = (bytes + 15u) / 16u;
                for (uint32_t i = lane; i < n16; i += 64) dst[i] = src[i];
                rec16 = (uint32_t)(off >> 4);
                rec = p.arena + off;
                // (the walker keeps reading the slice copy through w.Sb / Pb / Rb: same bytes)
            }
        }
        if (rec16 != 0) { // (arena full otherwise: the wave walks the tree alone - exact, only slower)
            export_mode = true;
            H = reinterpret_cast<RecHeader *>(rec);
            if (!is_task && !split) { // first time: finalize_kernel has to score this ligand
                if (lane == 0) {
                    const uint32_t o = atomicAdd(&p.ctl->heavy_count, 1u);
                    if (o < p.list_cap) p.heavy_list[o] = rec16;
                }
            }
            split = true; // (the arena copy is read by later kernels: nothing to fence)
        }
    }
    if (lane == 0) {
        stat->cyc_walk += __builtin_amdgcn_s_memtime() - t_d;
        stat->frames += w.frames;
        stat->passes += w.passes;
        stat->npath += w.npath;
        stat->dbg[7] += w.ndrop; // (the last word of the instrumented builds' counters is the product's: children dropped by path_bound())
        stat->longest = w.passes > stat->longest ? w.passes : stat->longest;
    }
    // ---- per-conformer maxima over the slots -> score
    if (w.best > 0.0) atomicMax(&pool[c], (unsigned long long)__double_as_longlong(w.best));
    wave_sync();
    const unsigned long long bbits = pool[c];
    const RecHeader *H = reinterpret_cast<const RecHeader *>(rec);
    if (split) { // every walker of a split ligand adds its maxima, finalize_kernel takes the mean
        unsigned long long *gbest = reinterpret_cast<unsigned long long *>(rec + sizeof(RecHeader));
        if (s == 0 && bbits != 0ull) atomicMax(gbest + c, bbits);
    } else { // mean over conformers (graph_match.py:109); lanes beyond C hold 0
        const int C = uni((int)H->C);
        double sum = (s == 0 && c < C) ? __longlong_as_double((long long)bbits) : 0.0;
#pragma unroll
        for (int d = 1; d < G; d <<= 1) sum += __shfl_xor(sum, d);
        if (lane == 0) put_score(p, (uint32_t)uni((int)H->lig), sum / (double)C);
    }
    wave_sync();
}

} // namespace PMX_NS
