// gpcc_markov_sample_inst.hip -- the instantiations of gpcc_markov_draw<P, NOFF> and gpcc_markov_combine_w<P, NOFF> (P = 1, 2, 3 states of
// the process, NOFF = 0 .. 4 offset states), the finish kernel and their launches, as an object of their own (gpcc.jl_amd/build.py
// compiles the objects side by side).
#include "gpcc_markov_sample.hip.h"

hipError_t gpcc_mks_launch_combine(int p, int noff, const GpccMarkovCombineWArgs &a, hipStream_t s)
{
#define GPCC_MKS_CASE(PP, NN)                                                                                        \
    if (p == PP && noff == NN) {                                                                                     \
        gpcc_markov_combine_w<PP, NN><<<dim3((a.c.rows + 63) / 64, a.c.T), dim3(64), 0, s>>>(a);                     \
        return hipGetLastError();                                                                                    \
    }
    GPCC_MK_EACH(GPCC_MKS_CASE)
#undef GPCC_MKS_CASE
    return hipErrorInvalidValue;
}

hipError_t gpcc_mks_launch_draw(int p, int noff, const GpccMarkovDrawArgs &a, int blocks, int threads, size_t lds, hipStream_t s)
{
    if ((long)blocks * threads > a.lstride || a.lanes < 1 || a.lanes > a.lstride) return hipErrorInvalidValue;   // the scratch's columns
#define GPCC_MKS_CASE(PP, NN)                                                                                        \
    if (p == PP && noff == NN) {                                                                                     \
        gpcc_markov_draw<PP, NN><<<dim3(blocks), dim3(threads), lds, s>>>(a);                                        \
        return hipGetLastError();                                                                                    \
    }
    GPCC_MK_EACH(GPCC_MKS_CASE)
#undef GPCC_MKS_CASE
    return hipErrorInvalidValue;
}

// more than the default 64 KiB of dynamic LDS for the staged points (per device, idempotent)
hipError_t gpcc_mks_configure()
{
#define GPCC_MKS_ATTR(PP, NN)                                                                                                        \
    {                                                                                                                                \
        const hipError_t e = hipFuncSetAttribute((const void *)gpcc_markov_draw<PP, NN>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                                 GPCC_MARKOV_LDS_MAX);                                                               \
        if (e != hipSuccess) return e;                                                                                               \
    }
    GPCC_MK_EACH(GPCC_MKS_ATTR)
#undef GPCC_MKS_ATTR
    return hipSuccess;
}

// grid (ceil(lanes / 64), ceil(T / 64)), 256 threads: a tile of 64 lanes x 64 test points is read along the lanes (acc is
// [test point][lane]) and written along the test points (draws is [row][test point]); the 65-double pitch keeps both conflict-free
static __global__ void __launch_bounds__(256) gpcc_markov_draw_finish(const GpccMarkovDrawFinishArgs a)
{
    __shared__ double tile[64][65];
    const int tx = (int)threadIdx.x & 63, ty = (int)threadIdx.x >> 6;
    const int l0 = (int)blockIdx.x * 64, j0 = (int)blockIdx.y * 64;
    for (int jj = ty; jj < 64; jj += 4)
        if (l0 + tx < a.lanes && j0 + jj < a.T) tile[jj][tx] = a.acc[(long)(j0 + jj) * a.lstride + l0 + tx];
    __syncthreads();
    if (j0 + tx >= a.T) return;
    for (int ll = ty; ll < 64; ll += 4) {
        if (l0 + ll >= a.lanes) break;
        const long lane = (long)a.lane0 + l0 + ll;
        const long lrow = a.lane_row[lane] - a.row0;
        a.draws[(long)a.lane_out[lane] * a.T + j0 + tx] = a.mu[lrow * a.T + j0 + tx] + tile[tx][ll];
    }
}

hipError_t gpcc_mks_launch_finish(const GpccMarkovDrawFinishArgs &a, hipStream_t s)
{
    gpcc_markov_draw_finish<<<dim3((a.lanes + 63) / 64, (a.T + 63) / 64), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}
