// gpcc_markov_sample_inst.hip -- the instantiations of gpcc_markov_draw<P, NOFF> and gpcc_markov_combine_w<P, NOFF> that ship
// (GpccMkShipsAll of gpcc_markov.hip.h), the finish kernel and their launches, as an object of their own (gpcc.jl_amd/build.py
// compiles the objects side by side).
#include "gpcc_markov_sample.hip.h"

hipError_t gpcc_mks_launch_combine(int p, int noff, const GpccMarkovCombineWArgs &a, hipStream_t s)
{
    return gpcc_mk_dispatch<GpccMkShipsAll>(p, noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_combine_w<P(), NOFF()>, dim3((a.c.rows + 63) / 64, a.c.T), 64, 0, s, false, a);
    });
}

hipError_t gpcc_mks_launch_draw(const GpccMkLaunch &g, const GpccMarkovDrawArgs &a)
{
    if ((long)g.blocks * g.threads > a.lstride || a.lanes < 1 || a.lanes > a.lstride) return hipErrorInvalidValue;   // the scratch's columns
    return gpcc_mk_dispatch<GpccMkShipsAll>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_draw<P(), NOFF()>, g, 1, a);
    });
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
