// pmx_align.hip - where a binding mode sits in the pocket, on gfx950: for listed (ligand, conformer, key) rows the proper rotation R and
// translation t that bring the matched ligand nodes onto the pharmacophore points of the model nodes they are matched to, in the weighted
// least-squares sense, with the residuals of that fit (pmx_align in include/pmx.h). The reference scores distances only and has no
// counterpart; the correspondence is the match list of graph_match.py:139-172, as pmx_attribute.hip reads it.
//
// pmx_screen_tables.h is compiled here once more, as namespace pmx_g, for parse_record and the wavefront helpers; the level and candidate
// rules are scan_ligand's, in the form pmx_attribute.hip has them. Nothing else of the screening path is part of this translation unit: no
// score table, no tabulated pair function, no slice or arena.
//
// One wavefront handles one row:
//   levels    lane q = ligand cluster q: candidates and tree levels; lane l = level l: the key is checked
//   pairs     lane u = ligand node u: the node subset of (matched model cluster, type mask of u) is exactly the model nodes m that pair with
//             u, in ascending order (sidtab / sub_nodes: the cluster's node words and the type's node words, intersected when the model was
//             created - any number of node words, so models above 64 nodes need nothing special). The lane adds up W_u = sum w and sum w y_m.
//   sums      W, the centroids and S = sum_u (x_u - xbar) (sum_m w y_m - W_u ybar)^T by xor butterflies: lanes i and i ^ k add the same two
//             numbers, so every lane ends with the same bits and everything after it is wave-uniform
//   fit       Horn's 4x4 matrix of S, cyclic Jacobi (at most kSweeps sweeps; the exit test reads wave-uniform numbers), R from the unit quaternion
//   residuals lane u walks its model nodes again: sum w |R x_u + t - y_m|^2 and sum w |y_m - ybar|^2 from the points themselves (sum w |y_m|^2
//             minus the centroid's square would lose |y|^2 / E0 of the precision: pocket coordinates are tens of Angstrom from the origin)
// No lane adds to another lane's sum and there is no floating-point atomic: the same call gives the same bits.
//
// Several targets per node: sum_m w |p - y_m|^2 = W_u |p - ybar_u|^2 + sum_m w |y_m - ybar_u|^2 for any point p, so the fit sees node u
// as one point ybar_u of weight W_u and the second sum is a constant of the row (sse - rmsd_nodes^2 W).
#include <hip/hip_runtime.h>
#include <cstring>

#define PMX_NS pmx_g
#include "pmx_screen_tables.h"
#include "pmx_align.h"

namespace pmx_g {

constexpr uint8_t kNoMatch = 0xFF, kNoLevel = 0xFE;
constexpr int kL = PMX_MAX_LEVELS, kN = PMX_MAX_LIGAND_NODES;
constexpr int kSweeps = 32; // a 4x4 symmetric matrix is diagonal to the last bit after 6 to 8 sweeps
static_assert(kN == 64 && PMX_MAX_LIGAND_CLUSTERS <= 64 && kL <= 32, "one wavefront: a lane per node and per cluster");

// LDS of the wavefront (static)
constexpr uint32_t kAtCb = 0;              // u64 [kL][2]: candidate model clusters of each level
constexpr uint32_t kAtTm = kAtCb + kL * 16; // u8 [kN]: type masks
constexpr uint32_t kAtLs = kAtTm + kN;      // u8 [32]: first node of each level's cluster
constexpr uint32_t kAtLe = kAtLs + 32;      // u8 [32]: one past its last node
constexpr uint32_t kAtKey = kAtLe + 32;     // u8 [32]: the key (kNoMatch for None and for what is not a candidate)
constexpr uint32_t kAtLev = kAtKey + 32;    // u8 [32]: ligand cluster of each level (kNoLevel past nl)
constexpr uint32_t kLdsBytes = kAtLev + 32;

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
__device__ void align_row(const ScreenParams &p, const pmx_aln::Args &a, unsigned char *lds, uint32_t li) {
    const int lane = lane_id();
    unsigned long long *cbl = reinterpret_cast<unsigned long long *>(lds + kAtCb);
    uint8_t *tm = lds + kAtTm, *ls = lds + kAtLs, *le = lds + kAtLe, *keyl = lds + kAtKey, *lev = lds + kAtLev;

    const uint64_t lig = uni64(a.ligands[li]);
    const int c = uni((int)a.conformer[li]);

    if (lane < 32) {
        lev[lane] = kNoLevel;
        keyl[lane] = kNoMatch;
    }
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

    // ---- levels: the clusters that have a candidate, in priority order, at most PMX_MAX_LEVELS (scan_ligand's rules, as in pmx_attribute.hip)
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
            supported = false; // (as pmx_score, pmx_explain and pmx_attribute report such a ligand)
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

    // ---- the key: every match has to be a candidate of its level (it need not be a leaf of the tree: nothing is scored)
    const bool compute = supported && c >= 0 && c < C;
    bool invalid = false;
    if (supported) {
        bool bad = false;
        if (lane < kL) {
            const int kk = a.key[(size_t)li * kL + lane];
            if (kk != kNoMatch) {
                bool ok = lane < nl && kk < p.M.K && kk < PMX_MAX_MODEL_CLUSTERS;
                if (ok) ok = ((kk < 64 ? cbl[2 * lane] >> kk : cbl[2 * lane + 1] >> (kk - 64)) & 1ull) != 0ull;
                bad = !ok;
                if (ok) keyl[lane] = (uint8_t)kk;
            }
        }
        invalid = __ballot(bad) != 0ull || !compute;
    }
    wave_sync();
    const bool ok_row = supported && !invalid;

    double R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}}, t[3] = {0.0, 0.0, 0.0};
    double W = 0.0, sse = 0.0, rn = 0.0, e0 = 0.0, gap = 0.0, dev = -1.0;
    int nfit = 0, npairs = 0;
    if (ok_row) {
        // ---- pairs: the lane's node against the model nodes of its level's match that share a type with it, in model-node order
        uint32_t k0 = 0, k1 = 0;
        double x[3] = {0.0, 0.0, 0.0}, wu = 0.0, sy[3] = {0.0, 0.0, 0.0};
        int np = 0;
        if (lane < n) {
            int mylev = -1;
            for (int l = 0; l < nl; ++l) mylev = (lane >= (int)ls[l] && lane < (int)le[l]) ? l : mylev;
            if (mylev >= 0 && keyl[mylev] != kNoMatch) {
                const uint32_t sid = p.sidtab[(uint32_t)keyl[mylev] * 128u + tm[lane]];
                k0 = p.sub_off[sid], k1 = p.sub_off[sid + 1u]; // (subset 0 is empty)
            }
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
    const int status = !supported ? PMX_LIGAND_UNSUPPORTED : (invalid ? PMX_LIGAND_KEY_INVALID : PMX_LIGAND_OK);
    const double nan = __builtin_nan("");
    a.node[(size_t)li * kN + lane] = status == PMX_LIGAND_OK ? dev : nan;
    if (lane < kL) a.levels[(size_t)li * kL + lane] = lev[lane];
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
        a.status[li] = status;
    }
    wave_sync(); // (the next row starts by clearing this LDS)
}

// Persistent wavefronts over the call's rows.
__global__ __launch_bounds__(64) void align_kernel(const ScreenParams p, const pmx_aln::Args a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
    for (;;) {
        const int lane = lane_id();
        uint32_t next = 0;
        if (lane == 0) next = atomicAdd(a.cursor, 1u);
        next = (uint32_t)uni((int)next);
        if (next >= a.n) break;
        align_row(p, a, lds, next);
    }
}

} // namespace pmx_g

namespace pmx_aln {

size_t lds_bytes() { return pmx_g::kLdsBytes; }

bool launch(unsigned blocks, hipStream_t stream, const void *params, size_t bytes, const Args &a) {
    if (bytes != sizeof(pmx_g::ScreenParams)) return false;
    pmx_g::ScreenParams p;
    std::memcpy(&p, params, sizeof p);
    pmx_g::align_kernel<<<dim3(blocks), dim3(64), 0, stream>>>(p, a);
    return true;
}

} // namespace pmx_aln
