// Host-only build of the Newton polish of gpcc_laplace_evidence (gpcc.jl_amd/csrc/gpcc_laplace.h) for AddressSanitizer / UBSan on
// the CPU (GPU sanitizers are not available on the pool).  Built and run by tests/test_laplace_cpu.py.
#include "../../gpcc.jl_amd/csrc/gpcc_laplace.h"

#include <cstdio>

// l(u) = -1/2 sum_k (k + 1) (u_k - 0.1 k)^2 + 3
static int quad(void *, long K, const long *, const double *U, double *v, double *g, double *h)
{
    const int n = 4;
    for (long i = 0; i < K; ++i) {
        double s = 3.0;
        for (int k = 0; k < n; ++k) {
            const double d = U[i * n + k] - 0.1 * k;
            s -= 0.5 * (k + 1) * d * d;
            g[i * n + k] = -(k + 1) * d;
            for (int j = 0; j < n; ++j) h[(i * n + k) * n + j] = (j == k) ? -(double)(k + 1) : 0.0;
        }
        v[i] = s;
    }
    return 0;
}

// -(100 (y - x^2)^2 + (1 - x)^2); NaN for some problems in a region (rejected points)
static int ridge(void *, long K, const long *pidx, const double *U, double *v, double *g, double *h)
{
    for (long i = 0; i < K; ++i) {
        const double x = U[2 * i], y = U[2 * i + 1];
        v[i] = (pidx[i] % 5 == 2 && x > 1.5) ? std::numeric_limits<double>::quiet_NaN()
                                              : -(100.0 * (y - x * x) * (y - x * x) + (1.0 - x) * (1.0 - x));
        g[2 * i] = 400.0 * x * (y - x * x) + 2.0 * (1.0 - x);
        g[2 * i + 1] = -200.0 * (y - x * x);
        h[4 * i] = 400.0 * (y - x * x) - 800.0 * x * x - 2.0;
        h[4 * i + 1] = h[4 * i + 2] = 400.0 * x;
        h[4 * i + 3] = -200.0;
    }
    return 0;
}

int main()
{
    {
        const long P = 33;
        std::vector<double> u0(P * 4);
        for (long p = 0; p < P; ++p)
            for (int k = 0; k < 4; ++k) u0[p * 4 + k] = 0.3 * (double)((p * 7 + k * 3) % 11) - 1.5;
        gpcclap::BatchedNewton nt(P, 4, 10, 1e-10, nullptr, nullptr);
        if (nt.run(quad, nullptr, u0.data())) return 1;
        for (long p = 0; p < P; ++p)
            if (nt.info[p] != 0 || nt.rounds[p] != 2 || !(std::fabs(nt.u[p * 4 + 3] - 0.3) < 1e-12)) return 2;
        std::printf("quadratic: ok, %lld evaluations in %lld batches\n", nt.f_calls, nt.batches);
    }
    {
        const long P = 57;
        std::vector<double> u0(P * 2);
        for (long p = 0; p < P; ++p) {
            u0[2 * p] = -2.0 + 4.0 * (double)(p % 13) / 12.0;
            u0[2 * p + 1] = -1.0 + 3.0 * (double)(p % 7) / 6.0;
        }
        gpcclap::BatchedNewton nt(P, 2, 300, 1e-8, nullptr, nullptr);
        if (nt.run(ridge, nullptr, u0.data())) return 3;
        long good = 0;
        for (long p = 0; p < P; ++p) good += nt.info[p] == 0 && std::fabs(nt.u[2 * p] - 1.0) < 1e-6;
        std::printf("ridge: %ld of %ld converged, %lld evaluations in %lld batches\n", good, P, nt.f_calls, nt.batches);
        if (good < P * 9 / 10) return 4;
        std::printf("ridge: ok\n");
    }
    {
        const double lo[4] = {-1.0, -1.0, -1.0, -1.0}, hi[4] = {1.0, 1.0, 1.0, 0.2};   // the mode's u_3 = 0.3 lies beyond 0.2
        std::vector<double> u0(3 * 4, 5.0);
        gpcclap::BatchedNewton nt(3, 4, 20, 1e-10, lo, hi);
        if (nt.run(quad, nullptr, u0.data())) return 5;
        for (long p = 0; p < 3; ++p)
            if (nt.info[p] != gpcclap::ON_BOUND || nt.u[p * 4 + 3] != 0.2 || !std::isnan(nt.logz[p])) return 6;
        std::printf("bound: ok\n");
    }
    {
        gpcclap::BatchedNewton nt(0, 3, 5, 1e-6, nullptr, nullptr);
        if (nt.run(quad, nullptr, nullptr)) return 7;
        std::printf("empty: ok\n");
    }
    return 0;
}
