// gpcc_markov_pred_inst.hip -- the instantiations of gpcc_markov_taps<P, NOFF, MODE> and gpcc_markov_combine<P, NOFF> that ship
// (GpccMkShipsAll of gpcc_markov.hip.h), the small per-row kernels beside them and their launches, as an object of their own
// (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_pred.hip.h"

hipError_t gpcc_mkp_launch_taps(const GpccMkLaunch &g, int mode, int ny, const GpccMarkovPredArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsAll>(g.p, g.noff, [&](auto P, auto NOFF) {
        return mode == GPCC_MKP_TAP ? gpcc_mk_launch_kernel(gpcc_markov_taps<P(), NOFF(), GPCC_MKP_TAP>, g, ny, a)
                                    : gpcc_mk_launch_kernel(gpcc_markov_taps<P(), NOFF(), GPCC_MKP_UPDATE>, g, ny, a);
    });
}

hipError_t gpcc_mkp_launch_combine(int p, int noff, const GpccMarkovCombineArgs &a, hipStream_t s)
{
    return gpcc_mk_dispatch<GpccMkShipsAll>(p, noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_combine<P(), NOFF()>, dim3((a.rows + 63) / 64, a.T), 64, 0, s, false, a);
    });
}

static __global__ void __launch_bounds__(64) gpcc_markov_rowinfo(double *mu, double *var, int *info, int N, int T, int row0, int rows)
{
    const int lrow = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (lrow >= rows) return;
    double *m = mu + (long)lrow * T, *v = var + (long)lrow * T;
    bool bad = info[row0 + lrow] != 0;
    if (!bad)
        for (int j = 0; j < T; ++j)
            if (v[j] != v[j]) {
                info[row0 + lrow] = N + j + 1;
                bad = true;
                break;
            }
    if (bad)
        for (int j = 0; j < T; ++j) m[j] = v[j] = __builtin_nan("");
}

hipError_t gpcc_mkp_launch_rowinfo(double *mu, double *var, int *info, int N, int T, int row0, int rows, hipStream_t s)
{
    gpcc_markov_rowinfo<<<(rows + 63) / 64, 64, 0, s>>>(mu, var, info, N, T, row0, rows);
    return hipGetLastError();
}

// gpcc_pred_mix's arithmetic (gpcc_pred.hip.h): W = sum p, the weighted mean, S = sum p (mu - mean)^2 (West's update), V = sum p var
static __global__ void __launch_bounds__(128) gpcc_markov_mix(const double *mu, const double *var, const double *p, double *mix, int T,
                                                              int row0, int rows, int last)
{
    const int j = (int)blockIdx.x * 128 + (int)threadIdx.x;
    if (j >= T) return;
    double W = mix[j], mean = mix[T + j], S = mix[2L * T + j], V = mix[3L * T + j];
    for (int m = 0; m < rows; ++m) {
        const double pm = p[row0 + m];
        if (pm == 0.0) continue;
        const long o = (long)m * T + j;
        const double x = mu[o], v = var[o];
        W += pm;
        const double d = x - mean;
        mean += (pm / W) * d;
        S += pm * d * (x - mean);
        V += pm * v;
    }
    mix[j] = W; mix[T + j] = mean; mix[2L * T + j] = S; mix[3L * T + j] = V;
    if (last) {
        mix[4L * T + j] = mean;
        mix[5L * T + j] = (V + S) / W;
    }
}

hipError_t gpcc_mkp_launch_mix(const double *mu, const double *var, const double *p, double *mix, int T, int row0, int rows, int last,
                               hipStream_t s)
{
    gpcc_markov_mix<<<(T + 127) / 128, 128, 0, s>>>(mu, var, p, mix, T, row0, rows, last);
    return hipGetLastError();
}

static __global__ void __launch_bounds__(64) gpcc_markov_heldout_rows(const double *loglik, int *info, const double *ll2, const int *info2,
                                                                      const int *at2, const int *tperm, double *heldout, int N, int M)
{
    const int m = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (m >= M) return;
    double x = __builtin_nan("");
    if (info[m] == 0) {
        if (info2[m] == 0) x = ll2[m] - loglik[m];
        else info[m] = N + tperm[at2[m]] + 1;
    }
    heldout[m] = x;
}

// gpcc_heldout_mix's arithmetic (gpcc_heldout.hip.h) over all rows in row order: one lane
static __global__ void __launch_bounds__(64) gpcc_markov_heldout_mix(const double *heldout, const double *p, double *mix, int M)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double mx = -__builtin_inf(), s = 0.0, nan = 0.0;
    for (int m = 0; m < M; ++m) {
        const double pm = p[m];
        if (pm == 0.0) continue;
        const double x = heldout[m];
        if (x != x) {
            nan = 1.0;
            continue;
        }
        const double lx = log(pm) + x;
        if (lx == -__builtin_inf()) continue;   // contributes nothing
        if (s == 0.0) {
            mx = lx;
            s = 1.0;
        } else if (lx <= mx) {
            s += exp(lx - mx);
        } else {
            s = fma(s, exp(mx - lx), 1.0);
            mx = lx;
        }
    }
    mix[0] = mx;
    mix[1] = s;
    mix[2] = nan;
    mix[3] = (nan != 0.0) ? __builtin_nan("") : (s == 0.0 ? -__builtin_inf() : mx + log(s));
}

hipError_t gpcc_mkp_launch_heldout_finish(const double *loglik, int *info, const double *ll2, const int *info2, const int *at2,
                                          const int *tperm, double *heldout, const double *p, double *mix, int N, int M, hipStream_t s)
{
    gpcc_markov_heldout_rows<<<(M + 63) / 64, 64, 0, s>>>(loglik, info, ll2, info2, at2, tperm, heldout, N, M);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && p) {
        gpcc_markov_heldout_mix<<<1, 64, 0, s>>>(heldout, p, mix, M);
        e = hipGetLastError();
    }
    return e;
}
