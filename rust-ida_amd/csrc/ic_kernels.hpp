// Consistent initial conditions (C IDA's IDACalcIC; the reference has none): the device side of idaens_calc_ic. The algorithm is
// DESIGN.md section 4f; the per-system Newton / line-search state machine runs on the host (ensemble_ida.cpp) and reaches these
// kernels through the idahip_ic_* entry points, one list position per system.
//
// Where the vectors live (everything here runs before the first step, when phi[2..5] are free):
//     iterate (y0, y0')       phi[2], phi[3]
//     delnew = J^-1 F(trial)  phi[4]
//     delta  (the direction)  ctx delta
//     trial point             ctx yy, yp (what the Jacobian kernels and the host callbacks read)
//     savres                  ctx savres
//
// The trial -- the line search's hot call, up to 100 per Newton iteration -- is the residual kernels' own bodies
// (problem_kernels.hpp) behind their IC front end (SysArgsIC: the masked update feeds the residual, no pass over y of its own),
// followed in the SAME launch by the solve with the ctx's factors and the left-to-right WRMS sum (SysArgsIC::lu, ic_solve_body /
// ic_tiny_solve in solve_kernels.hpp) wherever both halves map a system to the same threads: one thread (n <= 8), one workgroup
// (linear dense, heat on a dense ctx). A band ctx solves with one lane per system (band_kernels.hpp) and a host-callback residual
// crosses to the host in between: those take the residual and the solve as separate launches. Solves are wg_getrs / tiny_getrs /
// band_getrs_* unchanged, without newton_iter's negation and 2/(1+cjratio) scaling.
#pragma once
#include "common.hpp"
#include "problem_kernels.hpp"
#include "solve_kernels.hpp"
#include "band_kernels.hpp"
#include "vector_kernels.hpp"

namespace idahip {

// ------------------------------------------------------------------------------------------------ solve + norm
template <int VEC>
__global__ __launch_bounds__(256) void ic_solve_kernel(const double* __restrict__ LU, const int* __restrict__ perm, double* x,
                                                       const double* __restrict__ ewt, int n, const int* __restrict__ idx,
                                                       double* __restrict__ out, const unsigned short* __restrict__ ord /* or null */) {
    ic_solve_body<VEC>(LU, perm, x, ewt, n, idx[blockIdx.x], out, ord);
}

__global__ void ic_tiny_solve_kernel(const double* LU, const long long* piv, double* x, const double* ewt, int n, const int* idx,
                                     int nsys, double* out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsys) return;
    out[s] = ic_tiny_solve(LU, piv, x, ewt, n, idx[s]);
}

// one lane per system, as band_newton_iter_kernel
template <int KL, int KU>
__global__ __launch_bounds__(64) void ic_band_solve_kernel(const double* __restrict__ ab, const long long* __restrict__ piv, int ml, int mu,
                                                           double* xv, const double* __restrict__ ewt, int n, const int* __restrict__ idx,
                                                           int nsys, double* __restrict__ out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsys) return;
    const int b = idx[s];
    const long ldab = 2 * ml + mu + 1;
    const double* A = ab + (long)b * ldab * n;
    const long long* P = piv + (long)b * n;
    const long vb = (long)b * n;
    double* x = xv + vb;
    auto src = [&](int i) { return x[i]; };
    if constexpr (KL >= 0) band_getrs_reg<KL, KU>(A, P, n, x, src);
    else band_getrs_generic(A, P, n, ml, mu, x, src);
    const double* __restrict__ wv = ewt + vb;
    double sum = 0.0;
#pragma unroll 8
    for (int i = 0; i < n; ++i) {
        const double p = x[i] * wv[i];
        sum = sum + p * p;
    }
    out[s] = sum;
}

// ------------------------------------------------------------------------------------------------ residual at the IC point
// The residual kernels of problem_kernels.hpp with the IC front end (SysArgsIC): the iterate, or the trial point -- followed, where
// SysArgsIC::lu is set, by the solve and the norm in the same launch.
template <int KIND>
__global__ void ic_tiny_sys_kernel(SysArgsIC a, const double* __restrict__ params, int nparam, int nsys) {
    tiny_sys_body<KIND>(a, params, nparam, nsys);
}
// (linear dense: linear_sys_kernel<VEC, false, SysArgsIC> itself)
template <class P, int VEC>
__global__ __launch_bounds__(256) void ic_stencil_sys_kernel(SysArgsIC a, const double* __restrict__ params) { stencil_sys_body<P, VEC>(a, params); }
__global__ __launch_bounds__(256) void ic_callback_pre_kernel(SysArgsIC a, double* __restrict__ stage) { callback_pre_body(a, stage); }

// ------------------------------------------------------------------------------------------------ bookkeeping around it
// One workgroup per listed system, as the stepper's vector kernels.
struct IcVecs {
    double *y0, *yp0;  // the iterate
    double* delnew;
    double* savres;
};

// ewt = ewt_set(phi[0]); bad = some component <= 0 (a NaN is not); out = sum (phi[1]*ewt)^2; iterate = (phi[0], phi[1])
__global__ __launch_bounds__(256) void ic_begin_kernel(VecState s, IcVecs v, const int* __restrict__ idx, double* __restrict__ out,
                                                       int* __restrict__ ewtbad) {
    extern __shared__ __align__(16) double sm[];
    __shared__ int s_bad;
    const int n = s.n;
    const long vb = (long)idx[blockIdx.x] * n;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const double y = s.phi[vb + i], yp = s.phi[s.phistride + vb + i];
        const double w = ewt_of(s, y, i);
        s.ewt[vb + i] = w;
        if (w <= 0.0) s_bad = 1;
        v.y0[vb + i] = y;
        v.yp0[vb + i] = yp;
        const double p = yp * w;
        sm[i] = p * p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[blockIdx.x] = seq_sum_lds(sm, n);
        ewtbad[blockIdx.x] = s_bad;
    }
}

// iterate = (phi[0], phi[1]): a step size that failed otherwise than by slow convergence starts over from the guess
__global__ __launch_bounds__(256) void ic_reset_kernel(VecState s, IcVecs v, const int* __restrict__ idx) {
    const int n = s.n;
    const long vb = (long)idx[blockIdx.x] * n;
    for (int i = threadIdx.x; i < n; i += 256) {
        v.y0[vb + i] = s.phi[vb + i];
        v.yp0[vb + i] = s.phi[s.phistride + vb + i];
    }
}

// before a linear setup: yy, yp = the iterate (the Jacobian kernels and callbacks read them; a rejected trial point may sit
// there) and delta = savres (nlsIC's restart after slow convergence; the two are equal already at a first setup)
__global__ __launch_bounds__(256) void ic_point_kernel(VecState s, IcVecs v, const int* __restrict__ idx) {
    const int n = s.n;
    const long vb = (long)idx[blockIdx.x] * n;
    for (int i = threadIdx.x; i < n; i += 256) {
        s.yy[vb + i] = v.y0[vb + i];
        s.yp[vb + i] = v.yp0[vb + i];
        s.delta[vb + i] = v.savres[vb + i];
    }
}

// the line search's trial point becomes the iterate (y' only with IDAENS_YA_YDP_INIT) and delnew the next direction
__global__ __launch_bounds__(256) void ic_accept_kernel(VecState s, IcVecs v, int with_yp, const int* __restrict__ idx) {
    const int n = s.n;
    const long vb = (long)idx[blockIdx.x] * n;
    for (int i = threadIdx.x; i < n; i += 256) {
        v.y0[vb + i] = s.yy[vb + i];
        if (with_yp) v.yp0[vb + i] = s.yp[vb + i];
        s.delta[vb + i] = v.delnew[vb + i];
    }
}

// a converged pass: ewt = ewt_set(y0), bad flag as above; phi[0] = yy = y0, phi[1] = yp = y0'
__global__ __launch_bounds__(256) void ic_commit_kernel(VecState s, IcVecs v, const int* __restrict__ idx, int* __restrict__ ewtbad) {
    __shared__ int s_bad;
    const int n = s.n;
    const long vb = (long)idx[blockIdx.x] * n;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const double y = v.y0[vb + i], yp = v.yp0[vb + i];
        const double w = ewt_of(s, y, i);
        s.ewt[vb + i] = w;
        if (w <= 0.0) s_bad = 1;
        s.phi[vb + i] = y;
        s.phi[s.phistride + vb + i] = yp;
        s.yy[vb + i] = y;
        s.yp[vb + i] = yp;
    }
    __syncthreads();
    if (threadIdx.x == 0) ewtbad[blockIdx.x] = s_bad;
}

}  // namespace idahip
