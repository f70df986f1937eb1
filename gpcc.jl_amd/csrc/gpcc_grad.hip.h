// gpcc_grad.hip.h -- device code of the marginal-likelihood gradient (gpcc_loglik_grad_batch).
//
// For K = Kd + Sobs (+ B), r = Y - bbar, w = K^-1 r and G = w w' - K^-1, every parameter theta of Kd has
//     d loglik / d theta = 1/2 sum_ij G_ij dKd_ij / d theta,
// with Kd_ij = alpha_{b_i} alpha_{b_j} k(s_ij; rho), s_ij = (t_i - tau_{b_i}) - (t_j - tau_{b_j}).  The reference has no gradient;
// this is the derivative of objective(alpha, rho) of src/gpccfixdelay_marginaliseb.jl:133-141 in its own (constrained) parameters.
//
// After the launch-per-step factorisation has left L in the slot (lower tiles, diagonal blocks as inv(L_kk) in linv, linv_keep = 1)
// and L^-1 r in c.w, a group runs:
//   gpcc_grad_trtri / gpcc_grad_copy  X = L^-1 over the slot's lower tiles, column block by column block from the last
//                                     (LAPACK dtrtri's order): X_Ij = -(sum_{j<K<=I} X_IK L_Kj) inv(L_jj), into a scratch column, then
//                                     copied over L_Ij (jobs of one column read the L_Kj the others would overwrite);
//   gpcc_grad_w                       w = X' (L^-1 r);
//   gpcc_grad_tiles<KID>              per lower tile (I, J): (K^-1)_IJ = sum_{K >= I} X_KI' X_KJ in the accumulators (never stored),
//                                     G = w_I w_J' - that, and the band-pair sums A = sum G k, R = sum G dk/drho, S = sum G dk/ds of its
//                                     elements -> 3 L^2 partials per (slot, tile);
//   gpcc_grad_finish                  the partials in a fixed order (off-diagonal tiles twice: S with the transposed pair negated) and
//                                     d/dalpha_l = sum_q alpha_q A_lq, d/drho = 1/2 sum_pq alpha_p alpha_q R_pq,
//                                     d/dtau_l = -alpha_l sum_q alpha_q S_lq.
// No atomics: every sum has a fixed order, so a result is bitwise repeatable.  fp64 only (v_mfma_f64_16x16x4_f64); the operands are
// read straight from the swizzled tile layout (gpcc_elem_off), 16 consecutive columns of one row per quarter wave.
#pragma once
#include "gpcc_kernels.hip.h"

typedef GpccPrec<double> GpccP64;

__device__ __forceinline__ double gpcc_gld(const double *tile, int r, int col) { return tile[gpcc_elem_off<double>(r, col)]; }

// X = L^-1, column block j (grid: cnt x (nt - 1 - j) jobs, one per tile row I > j; 512 threads).  Wave w computes the columns
// 16w .. 16w+15 of U = T' (T = sum_K X_IK L_Kj), so that U is the B operand of the second product Y' = inv(L_jj)' U as it sits in
// the accumulators (C/D: row q + 4 reg, column lane & 15 -- register reg of block mb is the k-step of rows 16 mb + 4 reg).
static __global__ __launch_bounds__(512) void gpcc_grad_trtri(GpccCtx c, GpccGroup g, int j, double *scr)
{
    const int n = c.nt - 1 - j;
    const int m = (int)blockIdx.x / n, I = j + 1 + (int)blockIdx.x % n;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m;
    if (c.info[slot] != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, q = lane >> 4;
    const double *tiles = (const double *)c.tiles + (long)slot * c.slot_stride;
    const double *lin = (const double *)c.linv;
    d4 acc[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[b] = d4{0.0, 0.0, 0.0, 0.0};
    for (int K = j + 1; K <= I; ++K) {
        const double *A = tiles + gpcc_tile_off(K, j);                                              // L_Kj (column j is still L)
        const double *B = (K < I) ? tiles + gpcc_tile_off(I, K) : lin + gpcc_linv_off(c, slot, I); // X_IK, final
        const int kend = (K < I) ? GPCC_TILE : 16 * w + 16;   // X_II is lower triangular: row i of it ends at column i
        for (int k0 = 0; k0 < kend; k0 += 4) {
            const double b = gpcc_gld(B, 16 * w + lr, k0 + q);
            double a[8];
#pragma unroll
            for (int mb = 0; mb < 8; ++mb) a[mb] = gpcc_gld(A, k0 + q, 16 * mb + lr);
#pragma unroll
            for (int mb = 0; mb < 8; ++mb) acc[mb] = GpccP64::mfma(a[mb], b, acc[mb]);
        }
    }
    // Y' = inv(L_jj)' U: A operand inv(L_jj)[mm][16 cb + row] (zero for mm < 16 cb), B operand the accumulators of U
    const double *Xj = lin + gpcc_linv_off(c, slot, j);
    d4 out[8];
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
        out[cb] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int mb = cb; mb < 8; ++mb)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[cb] = GpccP64::mfma(gpcc_gld(Xj, 16 * mb + 4 * r + q, 16 * cb + lr), acc[mb][r], out[cb]);
    }
    double *dst = scr + ((long)slot * c.nt + I) * GPCC_TILE_ELEMS;
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[gpcc_elem_off<double>(16 * w + lr, 16 * cb + GpccP64::crow(q, r))] = -out[cb][r];
}

// the scratch column of step j over the tiles (I, j), I > j (grid: cnt x (nt - 1 - j); 256 threads)
static __global__ __launch_bounds__(256) void gpcc_grad_copy(GpccCtx c, GpccGroup g, int j, const double *scr)
{
    const int n = c.nt - 1 - j;
    const int m = (int)blockIdx.x / n, I = j + 1 + (int)blockIdx.x % n;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m;
    if (c.info[slot] != 0) return;
    const d2 *src = (const d2 *)(scr + ((long)slot * c.nt + I) * GPCC_TILE_ELEMS);
    d2 *dst = (d2 *)((double *)c.tiles + (long)slot * c.slot_stride + gpcc_tile_off(I, j));
    for (int e = threadIdx.x; e < GPCC_TILE_ELEMS / 2; e += 256) dst[e] = src[e];
}

// w = X' (L^-1 r): gw[slot][J tile] = sum_{I >= J} X_IJ' w_I  (grid: cnt x nt; 128 threads, one column each)
static __global__ __launch_bounds__(GPCC_TILE) void gpcc_grad_w(GpccCtx c, GpccGroup g, double *gw)
{
    const int m = (int)blockIdx.x / c.nt, J = (int)blockIdx.x % c.nt;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m;
    if (c.info[slot] != 0) return;
    const int col = threadIdx.x;
    const double *tiles = (const double *)c.tiles + (long)slot * c.slot_stride;
    const double *wf = c.w + (long)slot * c.nrhs * c.Np;   // (fp64 handles: nrhs = 1)
    double s = 0.0;
    for (int I = J; I < c.nt; ++I) {
        const double *X = (I > J) ? tiles + gpcc_tile_off(I, J) : (const double *)c.linv + gpcc_linv_off(c, slot, J);
        const double *wi = wf + (long)I * GPCC_TILE;
        for (int r = (I > J) ? 0 : col; r < GPCC_TILE; ++r) s = fma(gpcc_gld(X, r, col), wi[r], s);
    }
    gw[(long)slot * c.Np + (long)J * GPCC_TILE + col] = s;
}

// k(s; rho) and its derivatives by rho and by s (ir = 1 / rho).  OU at s = 0: dk/ds = 0 (the mean of the one-sided derivatives).
template <int KID>
__device__ __forceinline__ void gpcc_grad_elem(double s, double ir, double &k, double &dr, double &ds)
{
    const double r = fabs(s);
    if (KID == 0) {          // exp(-r / rho)
        const double e = gpcc_exp_nonpos(-(r * ir));
        k = e;
        dr = (r * ir) * ir * e;
        ds = (s > 0.0) ? -e * ir : (s < 0.0) ? e * ir : 0.0;
    } else if (KID == 1) {   // exp(-s^2 / (4 rho)), src/util.jl:28
        const double u = 0.25 * (s * s) * ir;
        const double e = gpcc_exp_nonpos(-u);
        k = e;
        dr = e * u * ir;
        ds = -e * s * (0.5 * ir);
    } else if (KID == 2) {   // (1 + a) exp(-a), a = sqrt3 r / rho
        const double a = 1.7320508075688772 * r * ir;
        const double e = gpcc_exp_nonpos(-a);
        k = (1.0 + a) * e;
        dr = a * a * e * ir;
        ds = -3.0 * s * (ir * ir) * e;
    } else {                 // (1 + a + a^2 / 3) exp(-a), a = sqrt5 r / rho
        const double a = 2.23606797749979 * r * ir;
        const double e = gpcc_exp_nonpos(-a);
        k = (1.0 + a + (a * a) * (1.0 / 3.0)) * e;
        dr = (a * a) * (1.0 / 3.0) * (1.0 + a) * e * ir;
        ds = -(5.0 / 3.0) * s * (ir * ir) * (1.0 + a) * e;
    }
}

__device__ __forceinline__ void gpcc_grad_tile_ij(int t, int &I, int &J)
{
    int a = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f);
    while (a * (a + 1) / 2 > t) --a;
    while ((a + 1) * (a + 2) / 2 <= t) ++a;
    I = a;
    J = t - a * (a + 1) / 2;
}

// One lower tile (I, J) of K^-1 per workgroup (grid: cnt x nt(nt+1)/2; 512 threads): wave w holds rows 16w .. 16w+15, all 128 columns
// (C/D: row 16w + q + 4 reg, column 16 f + lane & 15).  Partials: part[slot][tile][x][p][q], x = 0 (A), 1 (R), 2 (S), for the
// elements (i in tile row I, j in tile column J) only; the finish adds the transposed pair of an off-diagonal tile.
template <int KID>
__global__ __launch_bounds__(512) void gpcc_grad_tiles(GpccCtx c, GpccGroup g, const double *gw, double *part)
{
    const int ntri = c.nt * (c.nt + 1) / 2;
    const int m = (int)blockIdx.x / ntri, tt = (int)blockIdx.x % ntri;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m;
    if (c.info[slot] != 0) return;
    int I, J;
    gpcc_grad_tile_ij(tt, I, J);
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, q = lane >> 4;
    const int L = c.L;
    __shared__ double su[2][GPCC_TILE], sw[2][GPCC_TILE], sred[8][3], sP[3 * GPCC_MAXL * GPCC_MAXL];
    __shared__ int sb[2][GPCC_TILE];
    if (tid < 2 * GPCC_TILE) {
        const int side = tid >> 7, rr = tid & 127;
        const long gi = (long)(side ? J : I) * GPCC_TILE + rr;
        const int b = c.band[gi];
        sb[side][rr] = b;
        su[side][rr] = (b >= 0) ? c.t[gi] - g.delays[(long)(g.first + m) * L + b] : 0.0;
        sw[side][rr] = gw[(long)slot * c.Np + gi];
    }
    for (int e = tid; e < 3 * L * L; e += 512) sP[e] = 0.0;

    const double *tiles = (const double *)c.tiles + (long)slot * c.slot_stride;
    const double *lin = (const double *)c.linv;
    d4 acc[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) acc[f] = d4{0.0, 0.0, 0.0, 0.0};
    for (int K = I; K < c.nt; ++K) {
        const double *XA = (K > I) ? tiles + gpcc_tile_off(K, I) : lin + gpcc_linv_off(c, slot, I);
        const double *XB = (K > J) ? tiles + gpcc_tile_off(K, J) : lin + gpcc_linv_off(c, slot, J);
        for (int k0 = (K > I) ? 0 : 16 * w; k0 < GPCC_TILE; k0 += 4) {   // (X_II[k][i] = 0 for k < i)
            const double a = gpcc_gld(XA, k0 + q, 16 * w + lr);
            double b[8];
#pragma unroll
            for (int f = 0; f < 8; ++f) b[f] = gpcc_gld(XB, k0 + q, 16 * f + lr);
#pragma unroll
            for (int f = 0; f < 8; ++f) acc[f] = GpccP64::mfma(a, b[f], acc[f]);
        }
    }
    __syncthreads();
    // G = w w' - K^-1, in place
#pragma unroll
    for (int f = 0; f < 8; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[f][r] = sw[0][16 * w + GpccP64::crow(q, r)] * sw[1][16 * f + lr] - acc[f][r];
    // band pairs of the tile: points are in band order, padding (band -1) last, so a tile row covers bands first .. last real point
    const int p0 = c.band[(long)I * GPCC_TILE], p1 = c.band[min(I * GPCC_TILE + GPCC_TILE - 1, c.N - 1)];
    const int q0 = c.band[(long)J * GPCC_TILE], q1 = c.band[min(J * GPCC_TILE + GPCC_TILE - 1, c.N - 1)];
    const double ir = 1.0 / g.rho[g.first + m];
    for (int p = p0; p <= p1; ++p)
        for (int pq = q0; pq <= q1; ++pq) {
            double ra = 0.0, rr = 0.0, rs = 0.0;
#pragma unroll
            for (int f = 0; f < 8; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * w + GpccP64::crow(q, r), jj = 16 * f + lr;
                    if (sb[0][i] == p && sb[1][jj] == pq) {
                        double kv, dkr, dks;
                        gpcc_grad_elem<KID>(su[0][i] - su[1][jj], ir, kv, dkr, dks);
                        const double gv = acc[f][r];
                        ra = fma(gv, kv, ra);
                        rr = fma(gv, dkr, rr);
                        rs = fma(gv, dks, rs);
                    }
                }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                ra += __shfl_xor(ra, o);
                rr += __shfl_xor(rr, o);
                rs += __shfl_xor(rs, o);
            }
            if (lane == 0) { sred[w][0] = ra; sred[w][1] = rr; sred[w][2] = rs; }
            __syncthreads();
            if (tid < 3) {
                double v = 0.0;
                for (int ww = 0; ww < 8; ++ww) v += sred[ww][tid];
                sP[(tid * L + p) * L + pq] = v;
            }
            __syncthreads();
        }
    __syncthreads();
    double *dst = part + ((long)slot * ntri + tt) * 3 * L * L;
    for (int e = tid; e < 3 * L * L; e += 512) dst[e] = sP[e];
}

// One workgroup per evaluation: the tables A, R, S from the partials (tiles in storage order) and the gradient row
// [d/dalpha_1 .. d/dalpha_L, d/drho, d/dtau_1 .. d/dtau_L]; NaN where the evaluation failed (info != 0).
static __global__ __launch_bounds__(256) void gpcc_grad_finish(GpccCtx c, GpccGroup g, const double *part, double *grad)
{
    const int m = blockIdx.x;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m, L = c.L, L2 = L * L, ntri = c.nt * (c.nt + 1) / 2, tid = threadIdx.x;
    __shared__ double sT[3 * GPCC_MAXL * GPCC_MAXL];
    const bool ok = c.info[slot] == 0;
    if (ok && tid < 3 * L2) {
        const int x = tid / L2, p = (tid % L2) / L, pq = tid % L;
        double v = 0.0;
        int tt = 0;
        for (int I = 0; I < c.nt; ++I)
            for (int J = 0; J <= I; ++J, ++tt) {
                const double *P = part + (((long)slot * ntri + tt) * 3 + x) * L2;
                if (I == J) v += P[p * L + pq];
                else v += (x == 2) ? P[p * L + pq] - P[pq * L + p] : P[p * L + pq] + P[pq * L + p];
            }
        sT[tid] = v;
    }
    __syncthreads();
    const double *alpha = g.alpha + (long)(g.first + m) * L;
    double *row = grad + (long)(g.first + m) * (2 * L + 1);
    if (tid >= 2 * L + 1) return;
    if (!ok) {
        row[tid] = __builtin_nan("");
        return;
    }
    // (A and R are symmetric, S antisymmetric; the diagonal tiles' sums are so only up to rounding: taken as (X +- X') / 2, so that
    // the delays' derivatives sum to zero to rounding -- the likelihood does not change when all delays shift together)
    double v = 0.0;
    if (tid < L) {                 // d/dalpha_l = sum_q alpha_q A_lq
        for (int pq = 0; pq < L; ++pq) v += alpha[pq] * (0.5 * (sT[tid * L + pq] + sT[pq * L + tid]));
    } else if (tid == L) {         // d/drho = 1/2 sum_pq alpha_p alpha_q R_pq
        for (int p = 0; p < L; ++p)
            for (int pq = 0; pq < L; ++pq) v += alpha[p] * alpha[pq] * (0.5 * (sT[L2 + p * L + pq] + sT[L2 + pq * L + p]));
        v *= 0.5;
    } else {                       // d/dtau_l = -alpha_l sum_q alpha_q S_lq
        const int l = tid - L - 1;
        for (int pq = 0; pq < L; ++pq) v += alpha[pq] * (0.5 * (sT[2 * L2 + l * L + pq] - sT[2 * L2 + pq * L + l]));
        v *= -alpha[l];
    }
    row[tid] = v;
}
