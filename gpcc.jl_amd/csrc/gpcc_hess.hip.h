// gpcc_hess.hip.h -- device code of the Hessian and the Fisher information of the marginal log-likelihood
// (gpcc_loglik_hess_batch).
//
// theta = (alpha_1 .. alpha_L, rho, tau_1 .. tau_L), P = 2L + 1.  With C = K^-1, w = K^-1 r, G = w w' - C and D_theta = dKd / d theta:
//     H_theta,phi = 1/2 tr(G d2Kd / dtheta dphi) - (D_theta w)' C (D_phi w) + 1/2 tr(C D_theta C D_phi)       (T1 - T2 + T3)
//     F_theta,phi = 1/2 tr(C D_theta C D_phi) = T3                                                              (expected information)
// where, for i in band p and j in band q, s_ij = (t_i - tau_p) - (t_j - tau_q) and k, k_r, k_s, k_rr, k_rs, k_ss are k(s; rho) and its
// derivatives by rho and s at s_ij:
//     D_alpha_l = (d_pl alpha_q + d_ql alpha_p) k      D_rho = alpha_p alpha_q k_r      D_tau_l = alpha_p alpha_q (d_ql - d_pl) k_s.
//
// After the gradient path of a group (gpcc_grad.hip.h: X = L^-1 in the slot's lower tiles and linv, w in gw, loglik and grad written),
// a Hessian group runs:
//   gpcc_hess_ctab<KID>    per lower tile (I, J): C_IJ = sum_{K >= I} X_KI' X_KJ in the accumulators (gpcc_grad_tiles' loop), stored as
//                          the tiles (I, J) and (J, I) of a dense row-major Np x Np copy of C; and the six band-pair sums of G times
//                          k, k_r, k_s, k_rr, k_rs, k_ss over the tile's elements -> 6 L^2 partials per (slot, tile)
//   gpcc_hess_u<KID>       u_theta = D_theta w for every theta, from the band-resolved sums sum_{j in q} {k, k_r, k_s}_ij w_j (row i)
//   gpcc_hess_z            z_theta = C u_theta  (T2_theta,phi = u_theta' z_phi)
//   gpcc_hess_gemm<KID>    M_theta = C D_theta, one 128 x 128 output tile per workgroup (v_mfma_f64_16x16x4_f64): the tiles of D_theta
//                          are generated from t, band, tau, alpha and rho into LDS, 64 rows at a time; C is read from the dense copy
//   gpcc_hess_trace        per tile pair (I >= J) and theta <= phi: sum of M_theta,ij M_phi,ji over (i in I, j in J) and, for I != J, over
//                          (i in J, j in I) -> P^2 partials per (slot, tile pair)
//   gpcc_hess_finish       every partial in a fixed order, T1 from the six tables, H and F for theta <= phi, mirrored: bitwise symmetric.
// Block mode (gpcc_loglik_hess_hyper_batch): only the leading Pa <= P parameters are active (Pa = L + 1: alpha and rho).
// u, z and M_theta are formed for theta < Pa, the traces for theta <= phi < Pa, and the finish writes Pa x Pa blocks; the buffers keep
// their stride P.  Every active entry is computed by exactly the arithmetic of the full Hessian (Pa = P), so the block is bitwise the
// leading block of gpcc_loglik_hess_batch.
// No atomics: every sum has a fixed order, so a result is bitwise repeatable whatever the batch.  Padding (band -1) has D = 0 and
// G is only summed over real points.
#pragma once
#include "gpcc_grad.hip.h"

#define GPCC_HESS_MAXP (2 * GPCC_MAXL + 1)
#define GPCC_HESS_LDW 144   // LDS row of a generated D tile: 128 doubles + 16 (rows k, k+1 of a ds_read_b64 lane group on disjoint banks)

// The Hessian's buffers, per slot: c = dense C (Np^2), m = M_theta (P Np^2), u, z (P Np each), tab = six band-pair
// tables per lower tile (ntri 6 L^2), tr = trace partials per tile pair (ntri P^2).  off: first point of every band (off[L] = N).
// Pa: the active parameters (the leading Pa of theta; Pa = P for the full Hessian).
struct GpccHessBuf {
    double *c, *m, *u, *z, *tab, *tr;
    int P, Pa;
    int off[GPCC_MAXL + 1];
};

// k(s; rho) and its first and second derivatives by rho and s (ir = 1 / rho).  The first three are gpcc_grad_elem's formulas.
// OU at s = 0: k_s = 0 (as the gradient), k_rs = 0, k_ss = 1 / rho^2 (the one-sided limit, the kink's delta left out).
template <int KID>
__device__ __forceinline__ void gpcc_hess_elem(double s, double ir, double &k, double &dr, double &ds, double &drr, double &drs, double &dss)
{
    const double r = fabs(s);
    if (KID == 0) {          // exp(-r / rho)
        const double x = r * ir;
        const double e = gpcc_exp_nonpos(-x);
        k = e;
        dr = x * ir * e;
        ds = (s > 0.0) ? -e * ir : (s < 0.0) ? e * ir : 0.0;
        drr = e * x * (ir * ir) * (x - 2.0);
        const double sg = (s > 0.0) ? 1.0 : (s < 0.0) ? -1.0 : 0.0;
        drs = sg * (ir * ir) * e * (1.0 - x);
        dss = (ir * ir) * e;
    } else if (KID == 1) {   // exp(-s^2 / (4 rho))
        const double u = 0.25 * (s * s) * ir;
        const double e = gpcc_exp_nonpos(-u);
        k = e;
        dr = e * u * ir;
        ds = -e * s * (0.5 * ir);
        drr = e * (ir * ir) * u * (u - 2.0);
        drs = 0.5 * s * e * (ir * ir) * (1.0 - u);
        dss = -(0.5 * ir) * e * (1.0 - 2.0 * u);
    } else if (KID == 2) {   // (1 + a) exp(-a), a = sqrt3 r / rho
        const double a = 1.7320508075688772 * r * ir;
        const double e = gpcc_exp_nonpos(-a);
        k = (1.0 + a) * e;
        dr = a * a * e * ir;
        ds = -3.0 * s * (ir * ir) * e;
        drr = e * (ir * ir) * (a * a) * (a - 3.0);
        drs = 3.0 * s * (ir * ir * ir) * e * (2.0 - a);
        dss = -3.0 * (ir * ir) * e * (1.0 - a);
    } else {                 // (1 + a + a^2 / 3) exp(-a), a = sqrt5 r / rho
        const double a = 2.23606797749979 * r * ir;
        const double e = gpcc_exp_nonpos(-a);
        k = (1.0 + a + (a * a) * (1.0 / 3.0)) * e;
        dr = (a * a) * (1.0 / 3.0) * (1.0 + a) * e * ir;
        ds = -(5.0 / 3.0) * s * (ir * ir) * (1.0 + a) * e;
        drr = (ir * ir) * e * (a * a) * (1.0 / 3.0) * (a * a - 3.0 * a - 3.0);
        drs = (5.0 / 3.0) * s * (ir * ir * ir) * e * (2.0 + 2.0 * a - a * a);
        dss = -(5.0 / 3.0) * (ir * ir) * e * (1.0 + a - a * a);
    }
}

// element (i, j) of D_theta from the base values at s_ij: kind 0 = alpha_l, 1 = rho, 2 = tau_l; p, q the bands (>= 0)
__device__ __forceinline__ double gpcc_hess_d(int kind, int l, int p, int q, double ap, double aq, double k, double kr, double ks)
{
    if (kind == 0) return ((p == l) ? aq : 0.0) * k + ((q == l) ? ap : 0.0) * k;
    if (kind == 1) return ap * aq * kr;
    return ap * aq * ks * (double)((q == l) - (p == l));
}

// One lower tile (I, J) of C per workgroup (grid: cnt x nt(nt+1)/2; 512 threads), as gpcc_grad_tiles: the tile is stored into the dense
// copy of C (and its transpose, I != J), then G = w w' - C and the partials tab[slot][tile][x][p][q], x = k, k_r, k_s, k_rr, k_rs, k_ss.
template <int KID>
__global__ __launch_bounds__(512) void gpcc_hess_ctab(GpccCtx c, GpccGroup g, const double *gw, GpccHessBuf hb)
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
    __shared__ double su[2][GPCC_TILE], sw[2][GPCC_TILE], sred[8][6], sP[6 * GPCC_MAXL * GPCC_MAXL];
    __shared__ int sb[2][GPCC_TILE];
    if (tid < 2 * GPCC_TILE) {
        const int side = tid >> 7, rr = tid & 127;
        const long gi = (long)(side ? J : I) * GPCC_TILE + rr;
        const int b = c.band[gi];
        sb[side][rr] = b;
        su[side][rr] = (b >= 0) ? c.t[gi] - g.delays[(long)(g.first + m) * L + b] : 0.0;
        sw[side][rr] = gw[(long)slot * c.Np + gi];
    }
    for (int e = tid; e < 6 * L * L; e += 512) sP[e] = 0.0;

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
    // the dense copy of C: row-major, tile (I, J) and, below the diagonal, its transpose as tile (J, I)
    {
        const long Np = c.Np;
        double *Cd = hb.c + (long)slot * Np * Np;
#pragma unroll
        for (int f = 0; f < 8; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long i = (long)I * GPCC_TILE + 16 * w + GpccP64::crow(q, r), j = (long)J * GPCC_TILE + 16 * f + lr;
                Cd[i * Np + j] = acc[f][r];
                if (I != J) Cd[j * Np + i] = acc[f][r];
            }
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < 8; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[f][r] = sw[0][16 * w + GpccP64::crow(q, r)] * sw[1][16 * f + lr] - acc[f][r];
    const int p0 = c.band[(long)I * GPCC_TILE], p1 = c.band[min(I * GPCC_TILE + GPCC_TILE - 1, c.N - 1)];
    const int q0 = c.band[(long)J * GPCC_TILE], q1 = c.band[min(J * GPCC_TILE + GPCC_TILE - 1, c.N - 1)];
    const double ir = 1.0 / g.rho[g.first + m];
    for (int p = p0; p <= p1; ++p)
        for (int pq = q0; pq <= q1; ++pq) {
            double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int f = 0; f < 8; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * w + GpccP64::crow(q, r), jj = 16 * f + lr;
                    if (sb[0][i] == p && sb[1][jj] == pq) {
                        double e[6];
                        gpcc_hess_elem<KID>(su[0][i] - su[1][jj], ir, e[0], e[1], e[2], e[3], e[4], e[5]);
                        const double gv = acc[f][r];
#pragma unroll
                        for (int x = 0; x < 6; ++x) v[x] = fma(gv, e[x], v[x]);
                    }
                }
#pragma unroll
            for (int x = 0; x < 6; ++x) {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) v[x] += __shfl_xor(v[x], o);
            }
            if (lane == 0) {
#pragma unroll
                for (int x = 0; x < 6; ++x) sred[w][x] = v[x];
            }
            __syncthreads();
            if (tid < 6) {
                double s = 0.0;
                for (int ww = 0; ww < 8; ++ww) s += sred[ww][tid];
                sP[(tid * L + p) * L + pq] = s;
            }
            __syncthreads();
        }
    __syncthreads();
    double *dst = hb.tab + ((long)slot * ntri + tt) * 6 * L * L;
    for (int e = tid; e < 6 * L * L; e += 512) dst[e] = sP[e];
}

// u_theta = D_theta w (grid: cnt x nt; 128 threads, one row i each; padding rows get 0).  The band-resolved sums over the real points j
// of one band at a time, in point order: Uk[q] = sum k_ij w_j, Ur[q] = sum k_r w_j, Us[q] = sum k_s w_j.
template <int KID>
__global__ __launch_bounds__(GPCC_TILE) void gpcc_hess_u(GpccCtx c, GpccGroup g, const double *gw, GpccHessBuf hb)
{
    const int m = (int)blockIdx.x / c.nt, T = (int)blockIdx.x % c.nt;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m;
    if (c.info[slot] != 0) return;
    const int L = c.L, P = hb.P;
    const long i = (long)T * GPCC_TILE + threadIdx.x;
    const double *dl = g.delays + (long)(g.first + m) * L, *al = g.alpha + (long)(g.first + m) * L;
    const double *wv = gw + (long)slot * c.Np;
    double *U = hb.u + (long)slot * P * c.Np;
    const int p = c.band[i];
    if (p < 0) {
        for (int th = 0; th < hb.Pa; ++th) U[(long)th * c.Np + i] = 0.0;
        return;
    }
    const double ui = c.t[i] - dl[p], ir = 1.0 / g.rho[g.first + m];
    double Uk[GPCC_MAXL], Ur[GPCC_MAXL], Us[GPCC_MAXL];
#pragma unroll
    for (int qq = 0; qq < GPCC_MAXL; ++qq) Uk[qq] = Ur[qq] = Us[qq] = 0.0;
    for (int qb = 0; qb < L; ++qb) {
        const double tq = dl[qb];
        double sk = 0.0, sr = 0.0, ss = 0.0;
        for (int j = hb.off[qb]; j < hb.off[qb + 1]; ++j) {
            double kv, kr, ks;
            gpcc_grad_elem<KID>(ui - (c.t[j] - tq), ir, kv, kr, ks);
            const double wj = wv[j];
            sk = fma(kv, wj, sk);
            sr = fma(kr, wj, sr);
            ss = fma(ks, wj, ss);
        }
#pragma unroll
        for (int qq = 0; qq < GPCC_MAXL; ++qq)
            if (qq == qb) { Uk[qq] = sk; Ur[qq] = sr; Us[qq] = ss; }
    }
    // sum_q alpha_q U[q]; for k_s over the other bands only: in tau_p's row the own band's term, alpha_p Us[p], cancels exactly, so it
    // is never added (added and subtracted it leaves its rounding behind: a tau row that is not 0 where D_tau is identically 0)
    double ak = 0.0, ar = 0.0, as = 0.0;
#pragma unroll
    for (int qq = 0; qq < GPCC_MAXL; ++qq)
        if (qq < L) {
            ak = fma(al[qq], Uk[qq], ak);
            ar = fma(al[qq], Ur[qq], ar);
            if (qq != p) as = fma(al[qq], Us[qq], as);
        }
    const double ap = al[p];
#pragma unroll
    for (int l = 0; l < GPCC_MAXL; ++l)
        if (l < L) {
            U[(long)l * c.Np + i] = ((p == l) ? ak : 0.0) + ap * Uk[l];                             // alpha_l
            if (L + 1 + l < hb.Pa) U[(long)(L + 1 + l) * c.Np + i] = (p == l) ? -(ap * as) : ap * (al[l] * Us[l]);   // tau_l
        }
    U[(long)L * c.Np + i] = ap * ar;                                                              // rho
}

// z_theta = C u_theta (grid: cnt x nt; 128 threads, one row i each: C[k][i] = C[i][k] read along rows k)
static __global__ __launch_bounds__(GPCC_TILE) void gpcc_hess_z(GpccCtx c, GpccGroup g, GpccHessBuf hb)
{
    const int m = (int)blockIdx.x / c.nt, T = (int)blockIdx.x % c.nt;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m;
    if (c.info[slot] != 0) return;
    const int P = hb.P, Pa = hb.Pa;
    const long Np = c.Np, i = (long)T * GPCC_TILE + threadIdx.x;
    const double *Cd = hb.c + (long)slot * Np * Np, *U = hb.u + (long)slot * P * Np;
    double z[GPCC_HESS_MAXP];
#pragma unroll
    for (int th = 0; th < GPCC_HESS_MAXP; ++th) z[th] = 0.0;
    for (long k = 0; k < Np; ++k) {
        const double cv = Cd[k * Np + i];
#pragma unroll
        for (int th = 0; th < GPCC_HESS_MAXP; ++th)
            if (th < Pa) z[th] = fma(cv, U[th * Np + k], z[th]);
    }
    double *Z = hb.z + (long)slot * P * Np;
#pragma unroll
    for (int th = 0; th < GPCC_HESS_MAXP; ++th)
        if (th < Pa) Z[th * Np + i] = z[th];
}

// M_theta = C D_theta, tile (I, J) (grid: cnt x nt x Pa x nt -- J fastest, then theta, so that the workgroups running together share the
// column strip I of C; 512 threads).  Wave w holds rows 16w .. 16w+15 of the tile, all 128 columns (C/D: row 16w + q + 4 reg,
// column 16 f + lane & 15).  A operand C[i][k] = C[k][i] from the dense copy (16 consecutive doubles per quarter wave), B operand
// D_theta[k][j] from LDS, generated 64 rows at a time.
template <int KID>
__global__ __launch_bounds__(512) void gpcc_hess_gemm(GpccCtx c, GpccGroup g, GpccHessBuf hb)
{
    const int nt = c.nt, P = hb.P, Pa = hb.Pa;
    const long per = (long)nt * Pa * nt;
    const int m = (int)(blockIdx.x / per);
    const int rem = (int)(blockIdx.x % per);
    const int I = rem / (Pa * nt), th = (rem / nt) % Pa, J = rem % nt;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m;
    if (c.info[slot] != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, q = lane >> 4;
    const int L = c.L;
    const int kind = (th < L) ? 0 : (th == L) ? 1 : 2, l = (th < L) ? th : th - L - 1;
    __shared__ double sD[64 * GPCC_HESS_LDW];
    __shared__ double suJ[GPCC_TILE], sal[GPCC_MAXL];
    __shared__ int sbJ[GPCC_TILE];
    const double *dl = g.delays + (long)(g.first + m) * L;
    if (tid < GPCC_TILE) {
        const long gj = (long)J * GPCC_TILE + tid;
        const int b = c.band[gj];
        sbJ[tid] = b;
        suJ[tid] = (b >= 0) ? c.t[gj] - dl[b] : 0.0;
    }
    if (tid < L) sal[tid] = g.alpha[(long)(g.first + m) * L + tid];
    const double ir = 1.0 / g.rho[g.first + m];
    const long Np = c.Np;
    const double *Ccol = hb.c + (long)slot * Np * Np + (long)I * GPCC_TILE + 16 * w + lr;   // + k Np: C[k][i]
    d4 acc[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) acc[f] = d4{0.0, 0.0, 0.0, 0.0};
    const int jc = tid & 127, kr0 = tid >> 7;
    for (int K = 0; K < nt; ++K)
        for (int h = 0; h < 2; ++h) {
            const int kbase = K * GPCC_TILE + 64 * h;
            __syncthreads();   // (the previous rows consumed; the column data ready)
            const int qb = sbJ[jc];
            const double uj = suJ[jc];
#pragma unroll 4
            for (int x = 0; x < 16; ++x) {
                const int kr = kr0 + 4 * x;
                const int p = c.band[kbase + kr];
                double v = 0.0;
                if (p >= 0 && qb >= 0) {
                    double kv, kd, ks;
                    gpcc_grad_elem<KID>((c.t[kbase + kr] - dl[p]) - uj, ir, kv, kd, ks);
                    v = gpcc_hess_d(kind, l, p, qb, sal[p], sal[qb], kv, kd, ks);
                }
                sD[kr * GPCC_HESS_LDW + jc] = v;
            }
            __syncthreads();
#pragma unroll 4
            for (int k0 = 0; k0 < 64; k0 += 4) {
                const double a = Ccol[(long)(kbase + k0 + q) * Np];
                double b[8];
#pragma unroll
                for (int f = 0; f < 8; ++f) b[f] = sD[(k0 + q) * GPCC_HESS_LDW + 16 * f + lr];
#pragma unroll
                for (int f = 0; f < 8; ++f) acc[f] = GpccP64::mfma(a, b[f], acc[f]);
            }
        }
    double *Mt = hb.m + ((long)slot * P + th) * Np * Np;
#pragma unroll
    for (int f = 0; f < 8; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            Mt[((long)I * GPCC_TILE + 16 * w + GpccP64::crow(q, r)) * Np + (long)J * GPCC_TILE + 16 * f + lr] = acc[f][r];
}

// T3 partials (grid: cnt x nt(nt+1)/2 tile pairs; 256 threads): for theta <= phi < Pa, tr[slot][pair][theta][phi] = sum over i in I, j in J
// of M_theta[i][j] M_phi[j][i], plus (I != J) the same over i in J, j in I.  A wave reads 8 x 8 blocks: both M[a][b] and M[b][a] come
// as 8 rows of 64 contiguous bytes.
static __global__ __launch_bounds__(256) void gpcc_hess_trace(GpccCtx c, GpccGroup g, GpccHessBuf hb)
{
    const int ntri = c.nt * (c.nt + 1) / 2;
    const int m = (int)blockIdx.x / ntri, tt = (int)blockIdx.x % ntri;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m;
    if (c.info[slot] != 0) return;
    int I, J;
    gpcc_grad_tile_ij(tt, I, J);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, P = hb.P, Pa = hb.Pa;
    const long Np = c.Np, NN = Np * Np;
    const double *Mb = hb.m + (long)slot * P * NN;
    __shared__ double sred[4][GPCC_HESS_MAXP];
    double *dst = hb.tr + ((long)slot * ntri + tt) * P * P;
    const bool off = I != J;
    for (int th = 0; th < Pa; ++th) {
        const double *Mt = Mb + th * NN;
        double acc[GPCC_HESS_MAXP];
#pragma unroll
        for (int ph = 0; ph < GPCC_HESS_MAXP; ++ph) acc[ph] = 0.0;
        for (int blk = w; blk < 256; blk += 4) {
            const long a = (long)I * GPCC_TILE + (blk >> 4) * 8 + (lane >> 3), b = (long)J * GPCC_TILE + (blk & 15) * 8 + (lane & 7);
            const double xa = Mt[a * Np + b], xb = off ? Mt[b * Np + a] : 0.0;
#pragma unroll
            for (int ph = 0; ph < GPCC_HESS_MAXP; ++ph)
                if (ph >= th && ph < Pa) {
                    const double *Mp = Mb + ph * NN;
                    acc[ph] = fma(xa, Mp[b * Np + a], acc[ph]);
                    if (off) acc[ph] = fma(xb, Mp[a * Np + b], acc[ph]);
                }
        }
#pragma unroll
        for (int ph = 0; ph < GPCC_HESS_MAXP; ++ph)
            if (ph >= th && ph < Pa) {
                double v = acc[ph];
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) sred[w][ph] = v;
            }
        __syncthreads();
        if (tid >= th && tid < Pa) dst[th * P + tid] = ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
        __syncthreads();
    }
}

// One workgroup per evaluation (512 threads): the six tables (tiles in storage order, an off-diagonal tile's transposed pair added,
// negated for the odd k_s and k_rs), the T3 partials, T2 = u' z, then H and F for theta <= phi < Pa, written to both halves of a Pa x Pa
// block.  NaN blocks where the evaluation failed (info != 0).
static __global__ __launch_bounds__(512) void gpcc_hess_finish(GpccCtx c, GpccGroup g, GpccHessBuf hb, double *hess, double *fisher)
{
    const int m = blockIdx.x;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m, L = c.L, L2 = L * L, P = hb.P, P2 = P * P, Pa = hb.Pa, Pa2 = Pa * Pa, ntri = c.nt * (c.nt + 1) / 2;
    const int tid = threadIdx.x;
    __shared__ double sT[6 * GPCC_MAXL * GPCC_MAXL], s2[GPCC_HESS_MAXP * GPCC_HESS_MAXP], s3[GPCC_HESS_MAXP * GPCC_HESS_MAXP];
    const bool ok = c.info[slot] == 0;
    if (ok && tid < 6 * L2) {
        const int x = tid / L2, p = (tid % L2) / L, pq = tid % L;
        const bool odd = (x == 2) || (x == 4);
        double v = 0.0;
        int tt = 0;
        for (int I = 0; I < c.nt; ++I)
            for (int J = 0; J <= I; ++J, ++tt) {
                const double *T = hb.tab + (((long)slot * ntri + tt) * 6 + x) * L2;
                if (I == J) v += T[p * L + pq];
                else v += odd ? T[p * L + pq] - T[pq * L + p] : T[p * L + pq] + T[pq * L + p];
            }
        sT[tid] = v;
    }
    const int th = tid / Pa, ph = tid % Pa;
    if (ok && tid < Pa2 && th <= ph) {
        double t3 = 0.0;
        for (int tt = 0; tt < ntri; ++tt) t3 += hb.tr[((long)slot * ntri + tt) * P2 + th * P + ph];
        const long Np = c.Np;
        const double *U = hb.u + (long)slot * P * Np, *Z = hb.z + (long)slot * P * Np;
        double t2 = 0.0;
        for (long i = 0; i < Np; ++i) t2 += U[th * Np + i] * Z[ph * Np + i] + U[ph * Np + i] * Z[th * Np + i];
        s3[tid] = 0.5 * t3;
        s2[tid] = 0.5 * t2;
    }
    __syncthreads();
    if (tid >= Pa2 || th > ph) return;
    double *H = hess + (long)(g.first + m) * Pa2;
    double *F = fisher + (long)(g.first + m) * Pa2;
    if (!ok) {
        H[th * Pa + ph] = H[ph * Pa + th] = __builtin_nan("");
        F[th * Pa + ph] = F[ph * Pa + th] = __builtin_nan("");
        return;
    }
    const double *alpha = g.alpha + (long)(g.first + m) * L;
    // tables symmetrised (A, R, RR, SS) or antisymmetrised (S, RS): their diagonal tiles are so only up to rounding
    auto tab = [&](int x, int a, int b) {
        const double u = sT[x * L2 + a * L + b], v = sT[x * L2 + b * L + a];
        return 0.5 * ((x == 2 || x == 4) ? u - v : u + v);
    };
    auto asum = [&](int x, int a) {   // sum_q alpha_q T_x(a, q)
        double s = 0.0;
        for (int pq = 0; pq < L; ++pq) s += alpha[pq] * tab(x, a, pq);
        return s;
    };
    const int k1 = (th < L) ? 0 : (th == L) ? 1 : 2, l = (th < L) ? th : th - L - 1;
    const int k2 = (ph < L) ? 0 : (ph == L) ? 1 : 2, n = (ph < L) ? ph : ph - L - 1;   // (k1 <= k2: theta <= phi)
    double t1;
    if (k1 == 0 && k2 == 0) t1 = tab(0, l, n);                                                           // alpha_l, alpha_m
    else if (k1 == 0 && k2 == 1) t1 = asum(1, l);                                                        // alpha_l, rho
    else if (k1 == 0) t1 = alpha[n] * tab(2, l, n) - ((l == n) ? asum(2, l) : 0.0);                      // alpha_l, tau_m
    else if (k2 == 1) {                                                                                  // rho, rho
        double s = 0.0;
        for (int p = 0; p < L; ++p) s += alpha[p] * asum(3, p);
        t1 = 0.5 * s;
    } else if (k1 == 1) t1 = -alpha[n] * asum(4, n);                                                     // rho, tau_l
    else if (l == n) {                                                                                   // tau_l, tau_l: the own band's
        double s = 0.0;                                                                                  // SS_ll cancels exactly and is
        for (int pq = 0; pq < L; ++pq)                                                                   // never added
            if (pq != l) s += alpha[pq] * tab(5, l, pq);
        t1 = alpha[l] * s;
    } else t1 = -(alpha[l] * alpha[n] * tab(5, l, n));                                                   // tau_l, tau_m
    const double hv = t1 - s2[tid] + s3[tid];
    H[th * Pa + ph] = H[ph * Pa + th] = hv;
    F[th * Pa + ph] = F[ph * Pa + th] = s3[tid];
}
