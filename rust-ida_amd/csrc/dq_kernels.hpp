// Difference-quotient Jacobians: C IDA's idaLsDenseDQJac and idaLsBandDQJac (SUNDIALS ida_ls.c), for a ctx switched to
// idahip_set_jacobian_dq. The definition, restated (include/ida_hip.h has the same text for users):
//
//   srur = sqrt(DBL_EPSILON) = 2^-26; hh, cj: the system's step size and cj; yy, yp, ewt: the ctx's fields; rr = savres, the
//   residual at (tn, yy, yp) that sys left. MAX(a, b) = a > b ? a : b (SUNMAX, NaN included).
//   inc_j = MAX(srur * MAX(|yy_j|, |hh*yp_j|), 1/ewt_j);  if (hh*yp_j < 0) inc_j = -inc_j;  inc_j = (yy_j + inc_j) - yy_j
//   perturbed: yy_j + inc_j, yp_j + (cj*inc_j)
//   dense: one residual rtemp per column j (only j perturbed); J(:,j) = N_VLinearSum(1/inc_j, rtemp, -1/inc_j, rr), with the
//          serial N_VLinearSum's case order (dq_linsum below)
//   band:  width = ml + mu + 1, min(width, n) groups; group g perturbs every column j = g (mod width) at once, one residual;
//          J(i,j) = (1/inc_j) * (rtemp_i - rr_i) for max(0, j-mu) <= i <= min(n-1, j+ml); every other band entry +0.0
//
// Each problem kind's perturbed residuals are computed here in the operation order of its residual kernel
// (problem_kernels.hpp), so that a DQ entry is what a full evaluation at the perturbed point would give, bit for bit.
// -ffp-contract=off throughout: no FMA, so no MFMA either.
#pragma once
#include "../host/ida_controller.hpp"
#include "common.hpp"
#include "problem_kernels.hpp"

namespace idahip {

struct DqArgs {
    const double* yy;   // [batch][n] the ctx's fields
    const double* yp;
    const double* ewt;
    const double* rr;   // savres
    const int* idx;     // [nsys] system ids
    const double* cj;   // [nsys]
    const double* hh;   // [nsys]
    const int* skip;    // null, or per list position: nonzero = leave this system alone (the device lock-step stepper's flags)
    double* out;        // Jacobians: by system id ([batch][per]), or by list position when compact ([nsys][per])
    int compact;
    int n;
    int ml, mu, ld;     // band storage (ld = 2 ml + mu + 1); ld = 0 for dense
};

__device__ __forceinline__ long dq_slot(const DqArgs& d, int s, int b) { return d.compact ? (long)s : (long)b; }

// the increment of one column (idaLsDenseDQJac / idaLsBandDQJac)
__device__ __forceinline__ double dq_inc(double yj, double ypj, double ewtj, double hh) {
    constexpr double srur = 0x1p-26;  // sqrt(DBL_EPSILON)
    const double ay = fabs(yj), ah = fabs(hh * ypj);
    const double m = ay > ah ? ay : ah;
    const double t = srur * m, w = 1.0 / ewtj;
    double inc = t > w ? t : w;
    if (hh * ypj < 0.0) inc = -inc;
    return (yj + inc) - yj;
}

// N_VLinearSum(inv, rt, -inv, r) of SUNDIALS' serial vector, case for case: VDiff for inv = +-1, VScaleSum for inv == -inv (+-0),
// VScaleDiff for every other non-NaN inv, the general form for NaN
__device__ __forceinline__ double dq_linsum(double inv, double rt, double r) {
    if (inv == 1.0) return rt - r;
    if (inv == -1.0) return r - rt;
    if (inv == -inv) return inv * (rt + r);
    if (inv == inv) return inv * (rt - r);
    return inv * rt + (-inv) * r;
}

// ------------------------------------------------------------------------------------------------ Roberts, Lorenz63 (n = 3)
// one thread per system: three perturbed residuals through the residual kernel's own functions
template <int KIND>
__device__ __forceinline__ void tiny_dq_jac(const double* y, const double* yp, const double* w, const double* r0, double cj, double hh,
                                            const double* prm, double* J) {
    for (int j = 0; j < 3; ++j) {
        const double inc = dq_inc(y[j], yp[j], w[j], hh);
        double yt[3] = {y[0], y[1], y[2]}, ypt[3] = {yp[0], yp[1], yp[2]}, rt[3];
        yt[j] = y[j] + inc;
        ypt[j] = yp[j] + cj * inc;
        if (KIND == IDAHIP_ROBERTS) roberts_res(yt, ypt, rt);
        else lorenz_res(prm, yt, ypt, rt);
        const double inv = 1.0 / inc;
        for (int i = 0; i < 3; ++i) J[3 * j + i] = dq_linsum(inv, rt[i], r0[i]);
    }
}

template <int KIND>
__global__ void tiny_dq_jac_kernel(DqArgs d, const double* __restrict__ params, int nparam, int nsys) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsys) return;
    if (d.skip && d.skip[s] != 0) return;
    const int b = d.idx[s];
    const long vb = (long)b * 3;
    double y[3], yp[3], w[3], r0[3], J[9];
    for (int i = 0; i < 3; ++i) {
        y[i] = d.yy[vb + i]; yp[i] = d.yp[vb + i]; w[i] = d.ewt[vb + i]; r0[i] = d.rr[vb + i];
    }
    tiny_dq_jac<KIND>(y, yp, w, r0, d.cj[s], d.hh[s], params ? params + (long)b * nparam : nullptr, J);
    double* o = d.out + dq_slot(d, s, b) * 9;
    for (int e = 0; e < 9; ++e) o[e] = J[e];
}

// ------------------------------------------------------------------------------------------------ linear dense
// Column j's perturbed residual is r' = (ra' + rb') - c with ra'_i = sum_k A(i,k) yp'_k and rb'_i = sum_k B(i,k) yy'_k, two
// chains over ascending k (linear_sys_kernel, oracle/problems.hpp); yp' is yp with entry j replaced. So the n residuals of a
// system form a GEMM whose right-hand operand is yp 1^T with the diagonal replaced -- every output one sequential chain over k.
// One workgroup computes a 64 x 64 tile of (row i, column j), A and B staged through LDS 16 k at a time, a 4 x 4 register tile
// per lane. Exact savings, bit for bit: (1) for k < j0 (the tile's first column) every column's chain is the unperturbed one, so
// it is run once per row and copied into the column accumulators at k = j0; (2) A(i,k) * yp_k is the same product for every
// column with k != j, so it is formed once per row and k. The difference and N_VLinearSum are the epilogue that writes J.
constexpr int LDQ_T = 64, LDQ_KT = 16;

__global__ __launch_bounds__(256) void linear_dq_jac_kernel(DqArgs d, const double* __restrict__ A, const double* __restrict__ Bm,
                                                            const double* __restrict__ C, int tiles) {
    __shared__ __align__(16) double sA[LDQ_KT][LDQ_T];
    __shared__ __align__(16) double sB[LDQ_KT][LDQ_T];
    __shared__ double syp[LDQ_KT], syy[LDQ_KT];
    const int s = blockIdx.y;
    if (d.skip && d.skip[s] != 0) return;
    const int n = d.n;
    const int b = d.idx[s];
    const int i0 = (int)(blockIdx.x % tiles) * LDQ_T, j0 = (int)(blockIdx.x / tiles) * LDQ_T;
    const int t = threadIdx.x, tr = t & 15, tc = t >> 4;
    const long nn = (long)n * n, vb = (long)b * n;
    const double* __restrict__ Ab = A + (long)b * nn;
    const double* __restrict__ Bb = Bm + (long)b * nn;
    const double cj = d.cj[s], hh = d.hh[s];
    int jc[4];
    double pyp[4], pyy[4], inv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = j0 + tc + 16 * c;
        jc[c] = j;
        pyp[c] = pyy[c] = inv[c] = 0.0;
        if (j < n) {
            const double yj = d.yy[vb + j], ypj = d.yp[vb + j];
            const double inc = dq_inc(yj, ypj, d.ewt[vb + j], hh);
            pyy[c] = yj + inc;
            pyp[c] = ypj + cj * inc;
            inv[c] = 1.0 / inc;
        }
    }
    double pa[4], pb[4], ra[4][4], rb[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pa[r] = pb[r] = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) ra[r][c] = rb[r][c] = 0.0;
    }
    for (int k0 = 0; k0 < n; k0 += LDQ_KT) {
        const int kn = (n - k0 < LDQ_KT) ? n - k0 : LDQ_KT;
        __syncthreads();
        for (int e = t; e < LDQ_KT * LDQ_T; e += 256) {
            const int kk = e / LDQ_T, ii = e % LDQ_T, row = i0 + ii;
            const bool ok = kk < kn && row < n;
            const long off = (long)(k0 + kk) * n + row;
            sA[kk][ii] = ok ? Ab[off] : 0.0;
            sB[kk][ii] = ok ? Bb[off] : 0.0;
        }
        if (t < LDQ_KT) {
            syp[t] = t < kn ? d.yp[vb + k0 + t] : 0.0;
            syy[t] = t < kn ? d.yy[vb + k0 + t] : 0.0;
        }
        __syncthreads();
        if (k0 < j0) {  // (j0 is a multiple of 64, so this chunk lies wholly before it: kn == LDQ_KT)
#pragma unroll 2
            for (int kk = 0; kk < LDQ_KT; ++kk) {
                const double ypk = syp[kk], yyk = syy[kk];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pa[r] = pa[r] + sA[kk][tr + 16 * r] * ypk;
                    pb[r] = pb[r] + sB[kk][tr + 16 * r] * yyk;
                }
            }
            continue;
        }
        if (k0 == j0) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) { ra[r][c] = pa[r]; rb[r][c] = pb[r]; }
        }
        if (k0 < j0 + LDQ_T) {  // the tile's own columns: column j takes the perturbed entry at k = j
#pragma unroll 1
            for (int kk = 0; kk < kn; ++kk) {
                const int k = k0 + kk;
                const double ypk = syp[kk], yyk = syy[kk];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double a = sA[kk][tr + 16 * r], bv = sB[kk][tr + 16 * r];
                    const double qa = a * ypk, qb = bv * yyk;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const bool diag = k == jc[c];
                        ra[r][c] = ra[r][c] + (diag ? a * pyp[c] : qa);
                        rb[r][c] = rb[r][c] + (diag ? bv * pyy[c] : qb);
                    }
                }
            }
        } else if (kn == LDQ_KT) {
#pragma unroll 2
            for (int kk = 0; kk < LDQ_KT; ++kk) {
                const double ypk = syp[kk], yyk = syy[kk];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double qa = sA[kk][tr + 16 * r] * ypk, qb = sB[kk][tr + 16 * r] * yyk;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        ra[r][c] = ra[r][c] + qa;
                        rb[r][c] = rb[r][c] + qb;
                    }
                }
            }
        } else {
#pragma unroll 1
            for (int kk = 0; kk < kn; ++kk) {
                const double ypk = syp[kk], yyk = syy[kk];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double qa = sA[kk][tr + 16 * r] * ypk, qb = sB[kk][tr + 16 * r] * yyk;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        ra[r][c] = ra[r][c] + qa;
                        rb[r][c] = rb[r][c] + qb;
                    }
                }
            }
        }
    }
    double* __restrict__ J = d.out + dq_slot(d, s, b) * nn;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + tr + 16 * r;
        if (i >= n) continue;
        const double ci = C[vb + i], rri = d.rr[vb + i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (jc[c] >= n) continue;
            const double rt = (ra[r][c] + rb[r][c]) - ci;
            J[(long)jc[c] * n + i] = dq_linsum(inv[c], rt, rri);
        }
    }
}

// ------------------------------------------------------------------------------------------------ banded stencil problems
// Heat1D and Bruss1D (stencil_problems.hpp), with P::row as the row: column j's perturbation reaches rows j-HALF_BW .. j+HALF_BW.
// A row reads no y' but its own, so y' is perturbed only on the row that is itself perturbed.

// dense ctx: rows j-HALF_BW .. j+HALF_BW of column j from the perturbed inputs, every other entry the +0.0 the analytic
// stencil_jac_kernel writes there. Same launch shape and the same contract with the factorisation: with `zeroed` (LuWs::jwzero) set,
// the matrix is all +0.0 already and only those rows are written.
template <class P>
__global__ __launch_bounds__(256) void stencil_dq_jac_kernel(DqArgs d, const double* __restrict__ params, int chunks,
                                                             const int* __restrict__ zeroed) {
    if (d.skip && d.skip[blockIdx.x] != 0) return;
    const int s = blockIdx.x;
    const int n = d.n;
    const int b = d.idx[s];
    const long vb = (long)b * n;
    const double cj = d.cj[s], hh = d.hh[s];
    const double* __restrict__ prm = params + (long)b * P::NPARAM;
    const double* __restrict__ y = d.yy + vb;
    const double* __restrict__ yp = d.yp + vb;
    const double* __restrict__ rr = d.rr + vb;
    double* __restrict__ J = d.out + dq_slot(d, s, b) * n * n;
    const int per = (n + chunks - 1) / chunks;
    const int jbeg = blockIdx.y * per;
    const int jend = (jbeg + per < n) ? jbeg + per : n;
    auto entry = [&](int i, int j) {
        const double inc = dq_inc(y[j], yp[j], d.ewt[vb + j], hh);
        const double yj = y[j] + inc;
        const double ypi = (i == j) ? yp[j] + cj * inc : yp[i];
        const double rt = P::row(n, i, ypi, prm, [&](int k) { return (k == j) ? yj : y[k]; });
        return dq_linsum(1.0 / inc, rt, rr[i]);
    };
    if (zeroed && zeroed[b] != 0) {
        for (int j = jbeg + threadIdx.x; j < jend; j += 256)
            for (int i = (j > P::HALF_BW ? j - P::HALF_BW : 0); i <= j + P::HALF_BW && i < n; ++i) J[(long)j * n + i] = entry(i, j);
        return;
    }
    for (int j = jbeg; j < jend; ++j)
        for (int i = threadIdx.x; i < n; i += 256) J[(long)j * n + i] = stencil_in_band<P>(i, j) ? entry(i, j) : 0.0;
}

// band ctx and the Krylov ctx's band preconditioner, any 0 <= ml, mu < n (stencil_band_jac_kernel's launch shape): entry (i, j) of
// column j's band is row i of group (j mod width)'s residual, in which every column of the group is perturbed -- widths below
// (HALF_BW, HALF_BW) fold columns that share a row into one group, exactly as idaLsBandDQJac does
template <class P>
__global__ __launch_bounds__(256) void stencil_band_dq_jac_kernel(DqArgs d, const double* __restrict__ params, int chunks) {
    if (d.skip && d.skip[blockIdx.x] != 0) return;
    const int s = blockIdx.x;
    const int n = d.n, ml = d.ml, mu = d.mu, ld = d.ld, kv = ml + mu, width = ml + mu + 1;
    const int b = d.idx[s];
    const long vb = (long)b * n;
    const double cj = d.cj[s], hh = d.hh[s];
    const double* __restrict__ prm = params + (long)b * P::NPARAM;
    const double* __restrict__ y = d.yy + vb;
    const double* __restrict__ yp = d.yp + vb;
    const double* __restrict__ w = d.ewt + vb;
    double* __restrict__ J = d.out + dq_slot(d, s, b) * ld * n;
    const long total = (long)ld * n;
    const long per = (total + chunks - 1) / chunks;
    const long ebeg = blockIdx.y * per;
    const long eend = (ebeg + per < total) ? ebeg + per : total;
    for (long e = ebeg + threadIdx.x; e < eend; e += 256) {
        const int j = (int)(e / ld);
        const int i = j + (int)(e - (long)j * ld) - kv;
        double v = 0.0;
        if (i >= 0 && i < n && i >= j - mu && i <= j + ml) {
            const int g = j % width;
            double ypi = yp[i];
            if (i % width == g) ypi = ypi + cj * dq_inc(y[i], yp[i], w[i], hh);
            const double rt = P::row(n, i, ypi, prm, [&](int k) {
                return (k % width == g) ? y[k] + dq_inc(y[k], yp[k], w[k], hh) : y[k];
            });
            const double inc = dq_inc(y[j], yp[j], w[j], hh);
            v = (1.0 / inc) * (rt - d.rr[vb + i]);
        }
        J[e] = v;
    }
}

// ------------------------------------------------------------------------------------------------ host-callback problems
// The user's residual runs on the host; the device perturbs and packs, and differences and scatters. A copy is one perturbed
// (yy, yp) of one listed system, staged as [yy'][yp'][r'] (3n doubles): dense, copy q of list position s perturbs column j0 + q
// (G copies per system); band (ld > 0), one copy per system perturbs group j0.
__global__ __launch_bounds__(256) void dq_pack_kernel(DqArgs d, int j0, int G, double* __restrict__ stage) {
    const int s = blockIdx.x, q = blockIdx.y;
    const int n = d.n, width = d.ml + d.mu + 1;
    const int b = d.idx[s];
    const long vb = (long)b * n;
    const double cj = d.cj[s], hh = d.hh[s];
    double* __restrict__ st = stage + ((long)s * G + q) * 3 * n;
    for (int i = threadIdx.x; i < n; i += 256) {
        double y = d.yy[vb + i], p = d.yp[vb + i];
        if (d.ld ? (i % width == j0) : (i == j0 + q)) {
            const double inc = dq_inc(y, p, d.ewt[vb + i], hh);
            y = y + inc;
            p = p + cj * inc;
        }
        st[i] = y;
        st[n + i] = p;
    }
}

__global__ __launch_bounds__(256) void dq_scatter_kernel(DqArgs d, int j0, int G, const double* __restrict__ stage) {
    const int s = blockIdx.x, q = blockIdx.y;
    const int n = d.n;
    const int b = d.idx[s];
    const long vb = (long)b * n;
    const double hh = d.hh[s];
    const double* __restrict__ rt = stage + ((long)s * G + q) * 3 * n + 2 * n;
    const double* __restrict__ rr = d.rr + vb;
    if (!d.ld) {
        const int j = j0 + q;
        const double inv = 1.0 / dq_inc(d.yy[vb + j], d.yp[vb + j], d.ewt[vb + j], hh);
        double* __restrict__ col = d.out + dq_slot(d, s, b) * n * n + (long)j * n;
        for (int i = threadIdx.x; i < n; i += 256) col[i] = dq_linsum(inv, rt[i], rr[i]);
        return;
    }
    const int ml = d.ml, mu = d.mu, ld = d.ld, kv = ml + mu, width = ml + mu + 1;
    double* __restrict__ J = d.out + dq_slot(d, s, b) * ld * n;
    const long cols = (n - 1 - j0) / width + 1;  // the group's columns j0, j0 + width, ...
    for (long e = threadIdx.x; e < cols * ld; e += 256) {
        const int j = j0 + (int)(e / ld) * width, r = (int)(e % ld);
        const int i = j + r - kv;
        double v = 0.0;
        if (i >= 0 && i < n && i >= j - mu && i <= j + ml)
            v = (1.0 / dq_inc(d.yy[vb + j], d.yp[vb + j], d.ewt[vb + j], hh)) * (rt[i] - rr[i]);
        J[(long)j * ld + r] = v;
    }
}

// ------------------------------------------------------------------------------------------------ device lock-step stepper
// The round's step sizes, from the device-resident controller records, and nre_dq += the residual evaluations of one DQ Jacobian
// for each system that forms one this round (skip[b] == 0)
__global__ void dq_round_prep_kernel(idactl::SysCore* __restrict__ sys, const int* __restrict__ skip, double* __restrict__ hh, int batch,
                                     long evals) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    hh[b] = sys[b].hh;
    if (skip[b] == 0) sys[b].nre_dq += evals;
}

}  // namespace idahip
