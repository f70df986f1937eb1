// Host side of gpcc_laplace_evidence and gpcc_newton_batch: the lock-step damped Newton polish of the mode of l(u) and the Laplace
// approximation of the evidence there.
//
// P independent maximisations of dimension n advance together, so that every round is ONE batch of (value, gradient, Hessian)
// evaluations while each problem keeps its own trajectory.  Per problem, from the last accepted point (u, l, g, H):
//   - fixed coordinates: u_k on a bound with g_k pointing out of the box; the projected gradient is g with those entries set to 0;
//   - converged when |projected g|_inf <= g_tol: the problem finishes (below);
//   - otherwise the step d solves (A + lambda I) d = g over the free coordinates (d_k = 0 on fixed ones), A = -H: lambda = 0 if the
//     Cholesky factorisation succeeds with every pivot > 1e-8 s, else lambda = 1e-3 s, 1e-2 s, ... (s = max |A_kk| over the free
//     coordinates, 1 if that is 0) until it does (Levenberg damping);
//   - the candidate u + t d (t = 1, clipped to the box) is evaluated in the next round: accepted if its value is finite and not
//     below l - 1e-12 max(1, |l|) (no decrease beyond the rounding of an evaluated l: without that allowance a step within
//     rounding of the mode is refused until t collapses), otherwise t is halved and the candidate evaluated again.
// A problem stops with NOT_CONVERGED once it has taken part in max_rounds evaluations (the start included) or t < 1e-12.  At the
// end: a fixed coordinate with |g_k| > g_tol -> ON_BOUND (the mode lies on the box); else A = -H at the accepted point is
// factorised (no damping): not positive definite -> NOT_MAXIMUM; else info 0 and
//     log Z = l + n/2 log(2 pi) - 1/2 log det A = l + n/2 log(2 pi) - sum_k log L_kk,   cov = A^-1 = L^-T L^-1.
// Every non-zero code gives NaN log Z; cov is returned whenever A is positive definite, NaN otherwise.
//
// gpcc.jl_amd/laplace.py restates this in scalar Python with the same operations in the same order (the explicit Cholesky below,
// not LAPACK), and the tests require bitwise the same trajectories: nothing here may be contracted into FMAs (GPCC_LAP_NO_CONTRACT in
// every function; a gcc build for the generic x86-64 target has no FMA instruction to contract into).
#pragma once

#include <cmath>
#include <limits>
#include <vector>

#if defined(__clang__)
#define GPCC_LAP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GPCC_LAP_NO_CONTRACT
#endif

namespace gpcclap {

// per-problem codes (include/gpcc_hip.h: GPCC_LAPLACE_*); negative, so that they cannot clash with a factorisation's pivot index
enum { NOT_CONVERGED = -10, NOT_MAXIMUM = -11, ON_BOUND = -12, BAD_START = -13 };

// val[i], grad[i][n], hess[i][n][n] of problem pidx[i] at row i of U (K x n); a non-finite val = rejected point
typedef int (*HessFn)(void *ctx, long K, const long *pidx, const double *U, double *val, double *grad, double *hess);

const double LOG2PI = 1.8378770664093453;   // log(2 pi)

// A = Lc Lc' (n x n row-major; Lc lower, its strict upper triangle set to 0).  false when a pivot is not > pmin (NaN included).
inline bool chol(int n, const double *A, double *Lc, double pmin = 0.0)
{
    GPCC_LAP_NO_CONTRACT
    for (int j = 0; j < n; ++j) {
        double d = A[j * n + j];
        for (int k = 0; k < j; ++k) d = d - Lc[j * n + k] * Lc[j * n + k];
        if (!(d > pmin)) return false;
        const double ljj = std::sqrt(d);
        Lc[j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double s = A[i * n + j];
            for (int k = 0; k < j; ++k) s = s - Lc[i * n + k] * Lc[j * n + k];
            Lc[i * n + j] = s / ljj;
        }
        for (int i = 0; i < j; ++i) Lc[i * n + j] = 0.0;
    }
    return true;
}

// x = (Lc Lc')^-1 b
inline void chol_solve(int n, const double *Lc, const double *b, double *x)
{
    GPCC_LAP_NO_CONTRACT
    for (int i = 0; i < n; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s = s - Lc[i * n + k] * x[k];
        x[i] = s / Lc[i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = x[i];
        for (int k = i + 1; k < n; ++k) s = s - Lc[k * n + i] * x[k];
        x[i] = s / Lc[i * n + i];
    }
}

// cov = (Lc Lc')^-1 = Li' Li with Li = Lc^-1, for i <= j and mirrored (bitwise symmetric); Li: n x n scratch
inline void chol_inverse(int n, const double *Lc, double *Li, double *cov)
{
    GPCC_LAP_NO_CONTRACT
    for (int j = 0; j < n; ++j) {
        for (int i = 0; i < j; ++i) Li[i * n + j] = 0.0;
        Li[j * n + j] = 1.0 / Lc[j * n + j];
        for (int i = j + 1; i < n; ++i) {
            double s = 0.0;
            for (int k = j; k < i; ++k) s = s + Lc[i * n + k] * Li[k * n + j];
            Li[i * n + j] = -s / Lc[i * n + i];
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            double s = 0.0;
            for (int k = j; k < n; ++k) s = s + Li[k * n + i] * Li[k * n + j];
            cov[i * n + j] = s;
            cov[j * n + i] = s;
        }
}

// The chain rule from theta = exp(u) (alpha_1..alpha_L, rho) to u, for one evaluation: g_u = theta * g_theta and
// H_u = diag(theta) H_theta diag(theta) + diag(theta * g_theta).  gt: the leading n entries of a gradient row, Ht: n x n.
inline void hyper_to_u(int n, const double *theta, const double *gt, const double *Ht, double *gu, double *Hu)
{
    GPCC_LAP_NO_CONTRACT
    for (int i = 0; i < n; ++i) gu[i] = theta[i] * gt[i];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Hu[i * n + j] = (theta[i] * Ht[i * n + j]) * theta[j];
    for (int i = 0; i < n; ++i) Hu[i * n + i] = Hu[i * n + i] + gu[i];
}

struct BatchedNewton {
    long P;
    int n, max_rounds;
    double g_tol;
    std::vector<double> lo, hi;   // the box (n each; -inf / +inf = unbounded)
    long long f_calls = 0, batches = 0;
    static constexpr double ftol = 1e-12;   // "does not decrease", up to the rounding of an evaluated l (relative)
    // results
    std::vector<double> u, f, g, H, logz, cov;
    std::vector<int> info, rounds;

    BatchedNewton(long P_, int n_, int max_rounds_, double g_tol_, const double *lo_, const double *hi_)
        : P(P_), n(n_), max_rounds(max_rounds_), g_tol(g_tol_), lo(n_, -std::numeric_limits<double>::infinity()),
          hi(n_, std::numeric_limits<double>::infinity())
    {
        for (int k = 0; k < n; ++k) {
            if (lo_) lo[k] = lo_[k];
            if (hi_) hi[k] = hi_[k];
        }
    }

    bool fixed(long p, int k) const
    {
        const double uk = u[(size_t)p * n + k], gk = g[(size_t)p * n + k];
        return (uk <= lo[k] && gk < 0.0) || (uk >= hi[k] && gk > 0.0);
    }

    // the damped Newton direction at the accepted point of problem p; false if no damping made the system positive definite
    bool direction(long p, double *d, std::vector<double> &A, std::vector<double> &Lc, std::vector<double> &rhs)
    {
        GPCC_LAP_NO_CONTRACT
        const double *Hp = &H[(size_t)p * n * n], *gp = &g[(size_t)p * n];
        double s = 0.0;
        for (int i = 0; i < n; ++i) {
            const bool fi = fixed(p, i);
            rhs[i] = fi ? 0.0 : gp[i];
            for (int j = 0; j < n; ++j) A[i * n + j] = (fi || fixed(p, j)) ? ((i == j) ? 1.0 : 0.0) : -Hp[i * n + j];
            if (!fi && std::fabs(A[i * n + i]) > s) s = std::fabs(A[i * n + i]);
        }
        if (!(s > 0.0) || !std::isfinite(s)) s = 1.0;
        double lam = 0.0;
        for (int tries = 0; tries < 40; ++tries) {
            std::vector<double> B(A);
            for (int i = 0; i < n; ++i)
                if (!fixed(p, i)) B[i * n + i] = B[i * n + i] + lam;
            if (chol(n, B.data(), Lc.data(), 1e-8 * s)) {   // (a pivot near 0 would make a huge step, not a useful one)
                chol_solve(n, Lc.data(), rhs.data(), d);
                for (int i = 0; i < n; ++i)
                    if (!std::isfinite(d[i])) return false;
                return true;
            }
            lam = (lam == 0.0) ? 1e-3 * s : lam * 10.0;
        }
        return false;
    }

    // the end of problem p at its accepted point
    void finish(long p, int code, std::vector<double> &Lc, std::vector<double> &Li)
    {
        GPCC_LAP_NO_CONTRACT
        const size_t nn = (size_t)n * n;
        std::vector<double> A(nn);
        for (size_t e = 0; e < nn; ++e) A[e] = -H[(size_t)p * nn + e];
        double *cp = &cov[(size_t)p * nn];
        const bool pd = chol(n, A.data(), Lc.data());
        if (pd) chol_inverse(n, Lc.data(), Li.data(), cp);
        else for (size_t e = 0; e < nn; ++e) cp[e] = std::numeric_limits<double>::quiet_NaN();
        if (code == 0)
            for (int k = 0; k < n; ++k)
                if (fixed(p, k) && std::fabs(g[(size_t)p * n + k]) > g_tol) code = ON_BOUND;
        if (code == 0 && !pd) code = NOT_MAXIMUM;
        info[p] = code;
        if (code == 0) {
            double hl = 0.0;
            for (int k = 0; k < n; ++k) hl = hl + std::log(Lc[k * n + k]);
            logz[p] = f[p] + 0.5 * (double)n * LOG2PI - hl;
        } else
            logz[p] = std::numeric_limits<double>::quiet_NaN();
    }

    int run(HessFn eval, void *ctx, const double *u0)
    {
        GPCC_LAP_NO_CONTRACT
        const size_t nn = (size_t)n * n;
        u.assign((size_t)P * n, 0.0); f.assign(P, 0.0); g.assign((size_t)P * n, 0.0); H.assign((size_t)P * nn, 0.0);
        logz.assign(P, std::numeric_limits<double>::quiet_NaN()); cov.assign((size_t)P * nn, std::numeric_limits<double>::quiet_NaN());
        info.assign(P, 0); rounds.assign(P, 0);
        std::vector<double> t(P, 1.0), dir((size_t)P * n), A(nn), Lc(nn), Li(nn), rhs(n);
        std::vector<char> active(P, 0);
        std::vector<long> pid;
        std::vector<double> X, fv, gv, hv;
        auto evaluate = [&]() -> int {
            const long K = (long)pid.size();
            fv.assign(K, 0.0); gv.assign((size_t)K * n, 0.0); hv.assign((size_t)K * nn, 0.0);
            if (K == 0) return 0;
            const int rc = eval(ctx, K, pid.data(), X.data(), fv.data(), gv.data(), hv.data());
            if (rc) return rc;
            f_calls += K;
            batches += 1;
            for (long i = 0; i < K; ++i) rounds[pid[i]] += 1;
            return 0;
        };
        auto accept = [&](long p, long i) {
            for (int k = 0; k < n; ++k) u[(size_t)p * n + k] = X[(size_t)i * n + k];
            f[p] = fv[i];
            for (int k = 0; k < n; ++k) g[(size_t)p * n + k] = gv[(size_t)i * n + k];
            for (size_t e = 0; e < nn; ++e) H[(size_t)p * nn + e] = hv[(size_t)i * nn + e];
        };
        auto decide = [&](long p) {   // at a newly accepted point: finish, or the next direction
            double pg = 0.0;
            for (int k = 0; k < n; ++k)
                if (!fixed(p, k)) {
                    const double a = std::fabs(g[(size_t)p * n + k]);
                    if (!(a <= pg)) pg = std::isnan(a) ? std::numeric_limits<double>::infinity() : a;   // NaN: never converged
                }
            active[p] = 0;
            if (pg <= g_tol) finish(p, 0, Lc, Li);
            else if (rounds[p] >= max_rounds || !direction(p, &dir[(size_t)p * n], A, Lc, rhs)) finish(p, NOT_CONVERGED, Lc, Li);
            else {
                t[p] = 1.0;
                active[p] = 1;
            }
        };
        auto candidate = [&](long p) {
            for (int k = 0; k < n; ++k) {
                double v = u[(size_t)p * n + k] + t[p] * dir[(size_t)p * n + k];
                if (v < lo[k]) v = lo[k];
                if (v > hi[k]) v = hi[k];
                X.push_back(v);
            }
            pid.push_back(p);
        };

        for (long p = 0; p < P; ++p) {   // the start, clipped to the box
            for (int k = 0; k < n; ++k) {
                double v = u0[(size_t)p * n + k];
                if (v < lo[k]) v = lo[k];
                if (v > hi[k]) v = hi[k];
                X.push_back(v);
            }
            pid.push_back(p);
        }
        int rc = evaluate();
        if (rc) return rc;
        for (long p = 0; p < P; ++p) {
            accept(p, p);
            if (!std::isfinite(fv[p])) {
                info[p] = BAD_START;
                continue;
            }
            decide(p);
        }
        for (;;) {
            pid.clear();
            X.clear();
            for (long p = 0; p < P; ++p)
                if (active[p]) candidate(p);
            if (pid.empty()) break;
            rc = evaluate();
            if (rc) return rc;
            for (long i = 0; i < (long)pid.size(); ++i) {
                const long p = pid[i];
                if (std::isfinite(fv[i]) && fv[i] >= f[p] - ftol * std::fmax(1.0, std::fabs(f[p]))) {
                    accept(p, i);
                    decide(p);
                } else {
                    t[p] = 0.5 * t[p];
                    if (rounds[p] >= max_rounds || t[p] < 1e-12) {
                        active[p] = 0;
                        finish(p, NOT_CONVERGED, Lc, Li);
                    }
                }
            }
        }
        return 0;
    }
};

}   // namespace gpcclap
