// pmx_lm.h - the bounded Levenberg-Marquardt loop over a row's six rigid degrees of freedom that pmx_pose_refine (pmx_refine.hip),
// pmx_shape_overlay (pmx_shape_overlay.hip) and pmx_combo_overlay (pmx_colour.hip) run, one wavefront per row, once: the 6x6 solve,
// Rodrigues, the iteration with its lambda schedule and three stop reasons, the net angle and centroid shift, and how a row's motion and a
// row that is not OK are written (store_not_ok by the widths of the call's energy and count rows). The calls differ in the objective alone. The definitions are the comment of include/pmx.h; tests/lm_ref.py restates the loop.
//
// An objective supplies
//   Eval                       what an evaluation leaves: c[3], H[21], g[6] and whatever its value is made of
//   eval(R, t, Eval &)         the evaluation at a motion, the same bits in every lane afterwards
//   value(const Eval &)        the number that is followed
//   better(trial, cur)         whether a trial's value is accepted
//   gain(before, after)        what an accepted step won, not negative: the ftol rule stops at gain <= ftol * before
// Everything is computed by all lanes alike and every branch is taken through readfirstlane. H, g and the motions are named by constant
// indices only (every loop over them is unrolled): registers, no scratch. The build has contraction off: the expressions below are the bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pmx.h"
#include "pmx_error.h"

namespace pmx {

__device__ __forceinline__ bool uniform(bool b) { return __builtin_amdgcn_readfirstlane((int)b) != 0; }

// index of H(i, j), i <= j, in the 21 values of the upper triangle
__host__ __device__ constexpr int hidx(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// (H + lambda diag(H_ii + 1e-9)) delta = -g by Cholesky; false when a pivot is not positive.
__device__ __forceinline__ bool lm_solve(const double (&H)[21], const double (&g)[6], double lambda, double (&x)[6]) {
    double L[21]; // L(i, j), j <= i, at hidx(j, i)
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = H[hidx(j, j)] + lambda * (H[hidx(j, j)] + 1e-9);
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[hidx(k, j)] * L[hidx(k, j)];
        ok = ok && s > 0.0;
        const double ljj = __builtin_sqrt(s);
        L[hidx(j, j)] = ljj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = H[hidx(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[hidx(k, i)] * L[hidx(k, j)];
            L[hidx(j, i)] = v / ljj;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[hidx(k, i)] * y[k];
        y[i] = v / L[hidx(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= L[hidx(i, k)] * x[k];
        x[i] = v / L[hidx(i, i)];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) ok = ok && std::isfinite(x[i]);
    return ok;
}

// Rodrigues of omega: I + (sin th / th) K + (2 sin^2(th / 2) / th^2) K^2, K = [omega]_x, K^2 = omega omega^T - th^2 I.
__device__ __forceinline__ void rodrigues(double w0, double w1, double w2, double (&Rd)[9]) {
    const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
    const double th = __builtin_sqrt(th2);
    double sa = 1.0, sb = 0.5;
    if (th > 0.0) {
        const double sh = sin(0.5 * th);
        sa = sin(th) / th;
        sb = ((2.0 * sh) * sh) / (th * th);
    }
    const double w[3] = {w0, w1, w2};
    const double K[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rd[3 * i + j] = (i == j ? 1.0 : 0.0) + (sa * K[3 * i + j] + sb * (w[i] * w[j] - (i == j ? th2 : 0.0)));
}

// What the loop leaves next to the motion: the value at the last accepted evaluation, lambda, and count[0 .. 2] of include/pmx.h.
struct LmRun {
    double value, lambda;
    int iterations, accepted, reason;
};

// The iteration. `cur` is the last accepted evaluation, at (R, t): the caller's first one on entry - it needs that one for its own
// outputs, and decides from it whether there is anything to `follow`. A trial is evaluated at (Rt, tt). (R, t) leave with the last
// accepted motion: the input's own bits when nothing was accepted.
template <class Obj>
__device__ __forceinline__ LmRun lm_run(const Obj &obj, typename Obj::Eval &cur, double (&R)[9], double (&t)[3], bool follow, double ftol, int max_iter) {
    double Rt[9], tt[3];
    typename Obj::Eval tr;
    double E = obj.value(cur);
    double lambda = 1e-3;
    int iterations = 0, accepted = 0, reason = 2;
    if (uniform(!follow)) {
        reason = 0;
    } else {
        while (uniform(iterations < max_iter)) {
            double delta[6];
            if (!uniform(lm_solve(cur.H, cur.g, lambda, delta))) { // (a pivot that is not positive: a rejected trial without an evaluation)
                ++iterations;
                lambda *= 8.0;
                if (uniform(lambda > 1e8)) {
                    reason = 3;
                    break;
                }
                continue;
            }
            double Rd[9];
            rodrigues(delta[0], delta[1], delta[2], Rd);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) Rt[3 * i + j] = (Rd[3 * i] * R[j] + Rd[3 * i + 1] * R[3 + j]) + Rd[3 * i + 2] * R[6 + j];
            }
            {
                const double w0 = t[0] - cur.c[0], w1 = t[1] - cur.c[1], w2 = t[2] - cur.c[2];
#pragma unroll
                for (int i = 0; i < 3; ++i) tt[i] = (((Rd[3 * i] * w0 + Rd[3 * i + 1] * w1) + Rd[3 * i + 2] * w2) + cur.c[i]) + delta[3 + i];
            }
            obj.eval(Rt, tt, tr);
            ++iterations;
            const double Et = obj.value(tr);
            if (uniform(obj.better(Et, E))) {
                const double before = E;
                ++accepted;
                cur = tr;
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = Rt[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) t[k] = tt[k];
                E = Et;
                lambda = fmax(lambda / 4.0, 1e-9);
                if (uniform(obj.gain(before, Et) <= ftol * before)) {
                    reason = 1;
                    break;
                }
            } else {
                lambda *= 8.0;
                if (uniform(lambda > 1e8)) {
                    reason = 3;
                    break;
                }
            }
        }
    }
    return LmRun{E, lambda, iterations, accepted, reason};
}

// The net rotation from the start, Q = R R0^T, angle = atan2(|vee(Q - Q^T)| / 2, (tr Q - 1) / 2) - 0 when no step was accepted - and how
// far the centroid went from where the first evaluation had it.
__device__ __forceinline__ void lm_net_motion(const double (&R)[9], const double (&R0)[9], int accepted, const double (&c)[3], const double (&c_start)[3], double &angle,
                                              double &shift) {
    double Q[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Q[3 * i + j] = (R[3 * i] * R0[3 * j] + R[3 * i + 1] * R0[3 * j + 1]) + R[3 * i + 2] * R0[3 * j + 2];
    }
    const double a0 = Q[7] - Q[5], a1 = Q[2] - Q[6], a2 = Q[3] - Q[1];
    const double sn = 0.5 * __builtin_sqrt((a0 * a0 + a1 * a1) + a2 * a2), cs = 0.5 * (((Q[0] + Q[4]) + Q[8]) - 1.0);
    angle = accepted ? atan2(sn, cs) : 0.0;
    const double h0 = c[0] - c_start[0], h1 = c[1] - c_start[1], h2 = c[2] - c_start[2];
    shift = __builtin_sqrt((h0 * h0 + h1 * h1) + h2 * h2);
}

// A row's motion, lane k storing value k (selects, no indexing by a variable: registers).
__device__ __forceinline__ void store_motion(double *rot_out, double *trans_out, uint32_t row, int lane, const double (&R)[9], const double (&t)[3]) {
    double out = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) out = lane == k ? R[k] : out;
    if (lane < 9) rot_out[(size_t)row * 9 + lane] = out;
#pragma unroll
    for (int k = 0; k < 3; ++k) out = lane == k ? t[k] : out;
    if (lane < 3) trans_out[(size_t)row * 3 + lane] = out;
}

// A row that is not OK: no motion, no energy (kEnergy values a row), count = {0, 0, -1, 0, ...} (kCount), and its status.
template <int kEnergy, int kCount>
__device__ __forceinline__ void store_not_ok(double *rot_out, double *trans_out, double *energy, int32_t *count, int32_t *status_out, uint32_t row, int lane, int status) {
    const double nan = __builtin_nan("");
    if (lane < 9) rot_out[(size_t)row * 9 + lane] = nan;
    if (lane < 3) trans_out[(size_t)row * 3 + lane] = nan;
    if (lane < kEnergy) energy[(size_t)row * kEnergy + lane] = nan;
    if (lane < kCount) count[(size_t)row * kCount + lane] = lane == 2 ? -1 : 0;
    if (lane == 0) status_out[row] = status;
}

// Host: the two arguments of the loop. `fn` names the caller in the message; `what` names what it says must be finite and not negative,
// ftol and, where the caller has one, a value `other` of the same kind.
inline int lm_check(const char *fn, const char *what, double ftol, int max_iter, double other = 0.0) {
    if (!std::isfinite(other) || other < 0.0 || !std::isfinite(ftol) || ftol < 0.0) return pmx_fail(PMX_ERR_INVALID, "%s: %s must be finite and not negative", fn, what);
    if (max_iter < 0 || max_iter > PMX_REFINE_MAX_ITER) return pmx_fail(PMX_ERR_INVALID, "%s: max_iter %d, 0 .. %d", fn, max_iter, PMX_REFINE_MAX_ITER);
    return PMX_OK;
}

} // namespace pmx
