// gpcc_loo.hip.h -- device code of the exact leave-one-out predictive scores (gpcc_loo_batch).
//
// For K, bbar and Y of objective(alpha, rho), G = K^-1 and w = G (Y - bbar), the predictive distribution of y_i given every other
// observation is Gaussian with
//     var_i = 1 / G_ii,   mu_i = y_i - w_i / G_ii,   lp_i = -(log 2 pi + log var_i + (y_i - mu_i)^2 / var_i) / 2.
// No JITTER: this is p(y_i | y_-i) of the model the likelihood uses.  After the gradient's part 1 (enqueue_grad_inverse: the
// launch-per-step factorisation, X = L^-1 over the slot's lower tiles with inv(L_kk) in linv, w in gw) a group runs:
//   gpcc_loo_diag     G_ii = sum_{k >= i} X_ki^2 of every column: one read of the slot's lower tiles (N^2 / 2 doubles per row);
//   gpcc_loo_finish   mu, var, lp of the row's N points, loo = sum_i lp_i, and info = N + i for the first point (1-based) whose
//                     variance is not positive and finite; NaN where the row failed;
//   gpcc_loo_mix      per point, the weighted harmonic mean of the rows' densities, mix_lp_i = -log sum_m p_m exp(-lp_mi): one running,
//                     max-shifted log-sum-exp over the rows in row order (rows with p = 0 skipped), carried from group to group;
//   gpcc_loo_mix_sum  mix_lp from the state, and mix_loo = sum_i mix_lp_i.
// No atomics: every sum has a fixed order, so a result is bitwise repeatable and does not depend on M, the group or the stream.
#pragma once
#include "gpcc_kernels.hip.h"

#define GPCC_LOO_THREADS 256

// mu, var, lp: M x N (NULL: not wanted); loo: M; mix: the mixture state [max | scaled sum | NaN flag | mix_lp] (4 N) and mix_loo (1)
struct GpccLooBuf {
    double *mu, *var, *lp, *loo, *mix;
};

// G_ii of 16 columns (chunk ch of tile column J) per workgroup (grid: cnt x nt x 8; 256 threads).  A chunk of a tile is 128 rows of
// 16 doubles, contiguous (gpcc_elem_off), the 16-byte pairs of a row permuted by gpcc_sw(row): thread (r0 = tid / 8, sl = tid % 8)
// reads pair sl of the rows r0, r0 + 32, r0 + 64, r0 + 96 -- a wave reads 1 KiB of consecutive addresses -- and because gpcc_sw has
// period 16 in the row, the pair is the same two columns in all four rows and in every tile: each thread sums its two columns over its
// rows of the tiles I = J .. nt - 1 in that order, and thread c < 16 adds the 32 partial sums of column c in the order of r0.
static __global__ __launch_bounds__(GPCC_LOO_THREADS) void gpcc_loo_diag(GpccCtx c, GpccGroup g, double *gd)
{
    const int per = c.nt * GpccP64::NCH;
    const int m = (int)blockIdx.x / per, J = ((int)blockIdx.x % per) / GpccP64::NCH, ch = (int)blockIdx.x % GpccP64::NCH;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m;
    if (c.info[slot] != 0) return;
    const int tid = threadIdx.x, sl = tid & 7, r0 = tid >> 3;
    const int cp = 2 * (sl ^ gpcc_sw(r0)), col = GpccP64::KC * ch + cp;   // the columns col, col + 1 of the tile
    const double *tiles = (const double *)c.tiles + (long)slot * c.slot_stride;
    double s0 = 0.0, s1 = 0.0;
    for (int I = J; I < c.nt; ++I) {
        const double *X = (I > J) ? tiles + gpcc_tile_off(I, J) : (const double *)c.linv + gpcc_linv_off(c, slot, J);
        const d2 *src = (const d2 *)(X + ch * (GPCC_TILE * GpccP64::KC));
        d2 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = src[(r0 + 32 * k) * 8 + sl];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = r0 + 32 * k;
            if (I * GPCC_TILE + r >= c.N) continue;            // padding rows
            if (I > J || r >= col) s0 = fma(v[k][0], v[k][0], s0);   // (X_JJ is lower triangular: column i starts at row i)
            if (I > J || r >= col + 1) s1 = fma(v[k][1], v[k][1], s1);
        }
    }
    __shared__ double sp[32][GpccP64::KC];
    sp[r0][cp] = s0;
    sp[r0][cp + 1] = s1;
    __syncthreads();
    if (tid < GpccP64::KC) {
        double s = 0.0;
        for (int r = 0; r < 32; ++r) s += sp[r][tid];
        gd[(long)slot * c.Np + (long)J * GPCC_TILE + GpccP64::KC * ch + tid] = s;
    }
}

// One workgroup per row of the group (grid cnt, 256 threads).  gd: G_ii, gw: w = K^-1 (Y - bbar), per slot (Np each).  The points are
// in the caller's order (band 1 as handed to gpcc_create, then band 2, ...), as the handle stores them.
static __global__ __launch_bounds__(GPCC_LOO_THREADS) void gpcc_loo_finish(GpccCtx c, GpccGroup g, const double *gd, const double *gw,
                                                                          GpccLooBuf lb)
{
    const int m = (int)blockIdx.x;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m, row = g.first + m, tid = (int)threadIdx.x, N = c.N;
    __shared__ int sbad[GPCC_LOO_THREADS];
    __shared__ double ssum[GPCC_LOO_THREADS];
    const bool ok = c.info[slot] == 0 && g.out_info[row] == 0;
    const double *gdi = gd + (long)slot * c.Np, *wi = gw + (long)slot * c.Np;
    int bad = N;   // the first point whose variance is not positive and finite
    if (ok)
        for (int i = tid; i < N; i += GPCC_LOO_THREADS) {
            const double var = 1.0 / gdi[i];
            if (!(var > 0.0 && var < __builtin_inf())) { bad = i; break; }
        }
    sbad[tid] = bad;
    __syncthreads();
    for (int h = GPCC_LOO_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) sbad[tid] = min(sbad[tid], sbad[tid + h]);
        __syncthreads();
    }
    bad = sbad[0];
    const long o = (long)row * N;
    if (!ok || bad < N) {
        const double nan = __builtin_nan("");
        for (int i = tid; i < N; i += GPCC_LOO_THREADS) {
            if (lb.mu) lb.mu[o + i] = nan;
            if (lb.var) lb.var[o + i] = nan;
            if (lb.lp) lb.lp[o + i] = nan;
        }
        if (tid == 0) {
            lb.loo[row] = nan;
            if (ok) g.out_info[row] = N + bad + 1;
        }
        return;
    }
    const double log2pi = 1.8378770664093454835606594728112;
    double s = 0.0;
    for (int i = tid; i < N; i += GPCC_LOO_THREADS) {   // strided in a fixed order per thread
        const double gii = gdi[i], var = 1.0 / gii, d = wi[i] / gii;   // d = y_i - mu_i
        const double lp = -0.5 * (log2pi + log(var) + d * d / var);
        if (lb.mu) lb.mu[o + i] = c.yv[i] - d;
        if (lb.var) lb.var[o + i] = var;
        if (lb.lp) lb.lp[o + i] = lp;
        s += lp;
    }
    ssum[tid] = s;
    __syncthreads();
    for (int h = GPCC_LOO_THREADS / 2; h > 0; h >>= 1) {   // fixed pairwise tree
        if (tid < h) ssum[tid] += ssum[tid + h];
        __syncthreads();
    }
    if (tid == 0) lb.loo[row] = ssum[0];
}

// The delay mixture over the group's rows, one thread per point (grid ceil(N / 256), 256 threads), gpcc_heldout_mix's recurrence on
// x = -lp_mi: state mx = the largest log p_m - lp_mi so far, s = sum exp(log p_m - lp_mi - mx), nan = a failed row with p > 0 was met.
// lp: M x N (lp0: its first row's index, for callers that hold a chunk of rows); p: the normalised weights of the batch; rows
// first .. first + cnt - 1.  init: the batch's first rows (initialises the state).
static __global__ __launch_bounds__(GPCC_LOO_THREADS) void gpcc_loo_mix(const double *lp, long lp0, const double *p, int first, int cnt,
                                                                       int N, double *mix, int init)
{
    const int i = (int)(blockIdx.x * GPCC_LOO_THREADS + threadIdx.x);
    if (i >= N) return;
    double mx = init ? -__builtin_inf() : mix[i], s = init ? 0.0 : mix[N + i], nan = init ? 0.0 : mix[2 * (long)N + i];
    for (int m = 0; m < cnt; ++m) {
        const double pm = p[first + m];
        if (pm == 0.0) continue;
        const double x = -lp[((long)(first + m) - lp0) * N + i];
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
    mix[i] = mx;
    mix[N + i] = s;
    mix[2 * (long)N + i] = nan;
}

// mix_lp_i = -(mx + log s) from the final state (one row of weight 1: its own lp, bitwise), and mix_loo = sum_i mix_lp_i (grid 1)
static __global__ __launch_bounds__(GPCC_LOO_THREADS) void gpcc_loo_mix_sum(int N, double *mix)
{
    const int tid = (int)threadIdx.x;
    __shared__ double ssum[GPCC_LOO_THREADS];
    double t = 0.0;
    for (int i = tid; i < N; i += GPCC_LOO_THREADS) {
        const double mx = mix[i], s = mix[N + i], nan = mix[2 * (long)N + i];
        const double v = (nan != 0.0) ? __builtin_nan("") : (s == 0.0 ? __builtin_inf() : -(mx + log(s)));
        mix[3 * (long)N + i] = v;
        t += v;
    }
    ssum[tid] = t;
    __syncthreads();
    for (int h = GPCC_LOO_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) ssum[tid] += ssum[tid + h];
        __syncthreads();
    }
    if (tid == 0) mix[4 * (long)N] = ssum[0];
}
