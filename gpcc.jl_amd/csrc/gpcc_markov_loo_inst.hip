// gpcc_markov_loo_inst.hip -- the instantiations of gpcc_markov_loo_taps<P, NOFF> and gpcc_markov_loo_combine<P, NOFF> that ship
// (GpccMkShipsAll of gpcc_markov.hip.h: none spills or uses scratch memory, profiles/markov/kernel_resources_loo.log), the per-row
// kernel beside them and their launches, as an object of their own (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_loo.hip.h"

hipError_t gpcc_mkl_launch_taps(const GpccMkLaunch &g, const GpccMarkovLooArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsAll>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_loo_taps<P(), NOFF()>, g, 2, a);
    });
}

hipError_t gpcc_mkl_launch_combine(int p, int noff, const GpccMarkovLooCombineArgs &a, hipStream_t s)
{
    return gpcc_mk_dispatch<GpccMkShipsAll>(p, noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_loo_combine<P(), NOFF()>, dim3(a.N, (a.rows + 63) / 64), 64, 0, s, false, a);
    });
}

// one workgroup per row of the chunk (256 threads)
static __global__ void __launch_bounds__(256) gpcc_markov_loo_rows(double *mu, double *var, double *lp, double *loo, int *info, int N,
                                                                   int row0, int rows)
{
    const int lrow = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (lrow >= rows) return;
    double *m = mu + (long)lrow * N, *v = var + (long)lrow * N, *p = lp + (long)lrow * N;
    __shared__ int sbad[256];
    __shared__ double ssum[256];
    const bool failed = info[row0 + lrow] != 0;
    int bad = N;   // the first point whose variance is not positive and finite (the combine wrote NaN there)
    if (!failed)
        for (int i = tid; i < N; i += 256)
            if (v[i] != v[i]) { bad = i; break; }
    sbad[tid] = bad;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) sbad[tid] = min(sbad[tid], sbad[tid + h]);
        __syncthreads();
    }
    bad = sbad[0];
    if (failed || bad < N) {
        for (int i = tid; i < N; i += 256) m[i] = v[i] = p[i] = __builtin_nan("");
        if (tid == 0) {
            loo[row0 + lrow] = __builtin_nan("");
            if (!failed) info[row0 + lrow] = N + bad + 1;
        }
        return;
    }
    double s = 0.0;
    for (int i = tid; i < N; i += 256) s += p[i];   // strided in a fixed order per thread
    ssum[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {   // fixed pairwise tree
        if (tid < h) ssum[tid] += ssum[tid + h];
        __syncthreads();
    }
    if (tid == 0) loo[row0 + lrow] = ssum[0];
}

hipError_t gpcc_mkl_launch_rows(double *mu, double *var, double *lp, double *loo, int *info, int N, int row0, int rows, hipStream_t s)
{
    gpcc_markov_loo_rows<<<rows, 256, 0, s>>>(mu, var, lp, loo, info, N, row0, rows);
    return hipGetLastError();
}
