// gpcc_markov_inst.hip -- the instantiations of gpcc_markov_eval<P, NOFF> (P = 1, 2, 3 states of the process, NOFF = 0 .. 4 offset
// states) and their launch, as an object of their own (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov.hip.h"

hipError_t gpcc_markov_launch(int p, int noff, const GpccMarkovArgs &a, int blocks, int threads, size_t lds, hipStream_t s)
{
#define GPCC_MK_CASE(PP, NN)                                                              \
    if (p == PP && noff == NN) {                                                          \
        gpcc_markov_eval<PP, NN><<<dim3(blocks), dim3(threads), lds, s>>>(a);             \
        return hipGetLastError();                                                         \
    }
    GPCC_MK_EACH(GPCC_MK_CASE)
#undef GPCC_MK_CASE
    return hipErrorInvalidValue;
}

// more than the default 64 KiB of dynamic LDS for the staged light curves (per device, idempotent)
hipError_t gpcc_markov_configure()
{
#define GPCC_MK_ATTR(PP, NN)                                                                                                         \
    {                                                                                                                                \
        const hipError_t e = hipFuncSetAttribute((const void *)gpcc_markov_eval<PP, NN>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                                 GPCC_MARKOV_LDS_MAX);                                                               \
        if (e != hipSuccess) return e;                                                                                               \
    }
    GPCC_MK_EACH(GPCC_MK_ATTR)
#undef GPCC_MK_ATTR
    return hipSuccess;
}
