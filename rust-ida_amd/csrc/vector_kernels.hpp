// Kernels for the vector parts of the stepper that share the device-resident IDA state. One workgroup of 256
// threads per listed system. The arithmetic of an element is vector_elems.hpp's, shared with the device-resident steppers; a
// kernel takes its scalars from the per-list arrays and writes its sums (one lane each, left to right) to out[].
#pragma once
#include "vector_elems.hpp"

namespace idahip {

// ewt = ewt_set(phi[0]); out[2s] = sum (phi[1]*ewt)^2; out[2s+1] = sum (phi[0]*ewt)^2
__global__ __launch_bounds__(256) void init_first_kernel(VecState s, const int* __restrict__ idx, double* __restrict__ out) {
    extern __shared__ __align__(16) double sm[];
    const long vb = (long)idx[blockIdx.x] * s.n;
    for (int i = threadIdx.x; i < s.n; i += 256) el_init_first(s, vb, i, LdsSink{sm + i, s.n});
    __syncthreads();
    if (threadIdx.x < 2) out[2 * blockIdx.x + threadIdx.x] = seq_sum_lds(sm + threadIdx.x * s.n, s.n);
}

__global__ __launch_bounds__(256) void scale_phi1_kernel(VecState s, const int* __restrict__ idx, const double* __restrict__ fac) {
    const int b = idx[blockIdx.x];
    const long vb = (long)b * s.n;
    const double f = fac[blockIdx.x];
    for (int i = threadIdx.x; i < s.n; i += 256) s.phi[s.phistride + vb + i] *= f;
}

// phi[j] *= beta[j] (j = ns..kk) when ns <= kk; yypredict = sum_{j<=kk} phi[j]; yppredict = sum_{1<=j<=kk} gamma[j]*phi[j]
__global__ __launch_bounds__(256) void predict_kernel(VecState s, const int* __restrict__ idx, const int* __restrict__ kkns,
                                                      const double* __restrict__ beta, const double* __restrict__ gamma) {
    const int b = idx[blockIdx.x];
    const long vb = (long)b * s.n;
    const int kk = kkns[2 * blockIdx.x], ns = kkns[2 * blockIdx.x + 1];
    const double *bt = beta + MXORDP1 * blockIdx.x, *gm = gamma + MXORDP1 * blockIdx.x;
    for (int i = threadIdx.x; i < s.n; i += 256) el_predict(s, vb, i, kk, ns, bt, gm);
}

// yy = yypredict + ee; yp = yppredict + cj*ee; four sequential squared-norm sums
__global__ __launch_bounds__(256) void post_newton_kernel(VecState s, const int* __restrict__ idx, const double* __restrict__ cjs,
                                                          const int* __restrict__ kks, double* __restrict__ out) {
    extern __shared__ __align__(16) double sm[];
    const int n = s.n;
    const int b = idx[blockIdx.x];
    const long vb = (long)b * n;
    const double cj = cjs[blockIdx.x];
    const int kk = kks[blockIdx.x];
    for (int i = threadIdx.x; i < n; i += 256) el_post_newton(s, vb, i, kk, cj, true, LdsSink{sm + i, n});
    __syncthreads();
    if (threadIdx.x < 4) out[4 * blockIdx.x + threadIdx.x] = seq_sum_lds(sm + threadIdx.x * n, n);
}

// post_newton_kernel followed by the inequality-constraint check of DESIGN.md section 4g (C IDA's IDASetConstraints; the reference
// has none), in one launch. cvec[n]: 0 none, 1: y >= 0, -1: y <= 0, 2: y > 0, -2: y < 0 (idactl::constr_violated).
//   phase 1: yy, yp; v_i = the correction of a violated component (+0.0 elsewhere); sm[i] = (v_i ewt_i)^2
//   decision (one lane, then uniform): no violation -> 0; sqrt(sum / n) <= eps_newt -> 1 (correct); otherwise 2 (recover)
//   phase 2: 0 / 1: ee_i -= v_i for the violated i (flag 1), then post_newton_kernel's four sums of the ee now in memory;
//            2: rr from the minimum of phi[0]_i / (phi[0]_i - yy_i) over the violated i whose denominator is not zero, sums = 0
// The sums of phase 2 reuse the LDS of phase 1's (4 n doubles in all, as post_newton_kernel). check[s] == 0 (the Newton solve
// failed): no check, the system gets post_newton_kernel's results. out [nsys][4] sums, flag [nsys], rr [nsys] (0 unless flag 2).
__global__ __launch_bounds__(256) void post_newton_constr_kernel(VecState s, const double* __restrict__ cvec, const int* __restrict__ idx,
                                                                 const double* __restrict__ cjs, const int* __restrict__ kks,
                                                                 const double* __restrict__ eps_newt, const int* __restrict__ check,
                                                                 double* __restrict__ out, int* __restrict__ flag, double* __restrict__ rr) {
    extern __shared__ __align__(16) double sm[];
    __shared__ double s_q[256];
    __shared__ int s_any, s_flag;
    const int n = s.n;
    const int b = idx[blockIdx.x];
    const long vb = (long)b * n;
    const double cj = cjs[blockIdx.x];
    const int kk = kks[blockIdx.x];
    const bool chk = check[blockIdx.x] != 0;
    if (threadIdx.x == 0) {
        s_any = 0;
        s_flag = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        if (chk) {
            if (el_constr_check(s, vb, i, cvec[i], cj, LdsSink{sm + i, n})) s_any = 1;
        } else {
            el_final_yy(s, vb, i, s.ee[vb + i], cj);
        }
    }
    __syncthreads();
    if (chk && threadIdx.x == 0 && s_any) {
        const double vnorm = sqrt(seq_sum_lds(sm, n) / (double)n);
        s_flag = (vnorm <= eps_newt[blockIdx.x]) ? 1 : 2;
    }
    __syncthreads();
    const int fl = s_flag;
    if (fl == 2) {
        double q = idactl::CONSTR_QMAX;
        for (int i = threadIdx.x; i < n; i += 256) q = el_constr_quot(s, vb, i, cvec[i], q);
        s_q[threadIdx.x] = q;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (threadIdx.x < w && s_q[threadIdx.x + w] < s_q[threadIdx.x]) s_q[threadIdx.x] = s_q[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            flag[blockIdx.x] = 2;
            rr[blockIdx.x] = idactl::constr_rr(s_q[0]);
        }
        if (threadIdx.x < 4) out[4 * blockIdx.x + threadIdx.x] = 0.0;
        return;
    }
    for (int i = threadIdx.x; i < n; i += 256) {
        if (fl == 1) el_constr_correct(s, vb, i, cvec[i]);
        el_post_newton(s, vb, i, kk, cj, false, LdsSink{sm + i, n});
    }
    __syncthreads();
    if (threadIdx.x < 4) out[4 * blockIdx.x + threadIdx.x] = seq_sum_lds(sm + threadIdx.x * n, n);
    if (threadIdx.x == 0) {
        flag[blockIdx.x] = fl;
        rr[blockIdx.x] = 0.0;
    }
}

// the masked weighted norm on its own (idahip_wrms_masked): out[s] = sum_i ((x_i w_i) m_i)^2, m = 1.0 where mask_i != 0, left to right
__global__ __launch_bounds__(256) void wrms_masked_kernel(const double* __restrict__ X, const double* __restrict__ W,
                                                          const double* __restrict__ mask, double* __restrict__ out, int n,
                                                          const int* __restrict__ idx) {
    extern __shared__ __align__(16) double sm[];
    const long vb = (long)idx[blockIdx.x] * n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double p = (X[vb + i] * W[vb + i]) * (mask[i] != 0.0 ? 1.0 : 0.0);
        sm[i] = p * p;
    }
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = seq_sum_lds(sm, n);
}

// the constraint mask of one field (x: [batch][n]): violated[s] = 1 when a component of listed system s violates cvec
__global__ __launch_bounds__(256) void constr_check_kernel(const double* __restrict__ x, const double* __restrict__ cvec, int n,
                                                           const int* __restrict__ idx, int* __restrict__ violated) {
    __shared__ int s_any;
    const long vb = (long)idx[blockIdx.x] * n;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256)
        if (idactl::constr_violated(cvec[i], x[vb + i])) s_any = 1;
    __syncthreads();
    if (threadIdx.x == 0) violated[blockIdx.x] = s_any;
}

// phi[j] *= cvals[j-ns], j = ns..kk
__global__ __launch_bounds__(256) void restore_kernel(VecState s, const int* __restrict__ idx, const int* __restrict__ kkns,
                                                      const double* __restrict__ cvals) {
    const int b = idx[blockIdx.x];
    const long vb = (long)b * s.n;
    const int kk = kkns[2 * blockIdx.x], ns = kkns[2 * blockIdx.x + 1];
    if (ns > kk) return;
    for (int i = threadIdx.x; i < s.n; i += 256) el_restore(s, vb, i, kk, ns, cvals + MXORDP1 * blockIdx.x);
}

// phi[kused+1] = ee (kused < maxord); tmp = ee; for j = kused..0: tmp += phi[j]; phi[j] = tmp; ee *= ck;
// then ewt = ewt_set(phi[0]) and out = sum (phi[0]*ewt)^2
__global__ __launch_bounds__(256) void complete_step_kernel(VecState s, const int* __restrict__ idx, const int* __restrict__ kused_a,
                                                            const double* __restrict__ cks, int maxord, double* __restrict__ out,
                                                            int* __restrict__ ewtbad) {
    extern __shared__ __align__(16) double sm[];
    __shared__ int s_bad;
    const int n = s.n;
    const int b = idx[blockIdx.x];
    const long vb = (long)b * n;
    const int kused = kused_a[blockIdx.x];
    const double ck = cks[blockIdx.x];
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        if (el_complete_step(s, vb, i, kused, ck, maxord, LdsSink{sm + i, n})) s_bad = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = seq_sum_lds(sm, n);
    if (threadIdx.x == 0) ewtbad[blockIdx.x] = s_bad;
}

// yy = sum_{j<=kord} cvals[j]*phi[j]; yp = sum_{1<=j<=kord} dvals[j-1]*phi[j]  (from zero, scaled_add)
__global__ __launch_bounds__(256) void get_solution_kernel(VecState s, const int* __restrict__ idx, const int* __restrict__ kords,
                                                           const double* __restrict__ cvals, const double* __restrict__ dvals) {
    const int b = idx[blockIdx.x];
    const long vb = (long)b * s.n;
    const int kord = kords[blockIdx.x];
    for (int i = threadIdx.x; i < s.n; i += 256) el_get_solution(s, vb, i, kord, cvals + MXORDP1 * blockIdx.x, dvals + 5 * blockIdx.x);
}

// IDAGetDky (lib.rs:517-526): dky = sum_{j = k .. kused} cjk[j] * phi[j], from zero in ascending j, product then sum
__global__ __launch_bounds__(256) void get_dky_kernel(VecState s, const int* __restrict__ idx, const int* __restrict__ kfirst,
                                                      const int* __restrict__ klast, const double* __restrict__ cjk,
                                                      double* __restrict__ out) {
    const int b = idx[blockIdx.x];
    const long vb = (long)b * s.n;
    const int k0 = kfirst[blockIdx.x], k1 = klast[blockIdx.x];
    for (int i = threadIdx.x; i < s.n; i += 256) {
        double d = 0.0;
        for (int j = k0; j <= k1; ++j) d = d + s.phi[j * s.phistride + vb + i] * cjk[MXORDP1 * blockIdx.x + j];
        out[(long)blockIdx.x * s.n + i] = d;
    }
}

// Ida::new for the listed systems (lib.rs:291-293, ida_nls.rs:83-84): phi[0] = yy = y0, phi[1] = yp = y0'
__global__ __launch_bounds__(256) void restore_initial_kernel(VecState s, const double* __restrict__ icy, const double* __restrict__ icyp,
                                                              const int* __restrict__ idx) {
    const int b = idx[blockIdx.x];
    const long vb = (long)b * s.n;
    for (int i = threadIdx.x; i < s.n; i += 256) el_restore_initial(s, vb, i, icy[vb + i], icyp[vb + i]);
}

// Ida::new with new values for the listed systems (idahip_reinit): y0 / yp0 are packed [nsys][n] by list position. add == 0: the
// values themselves; add != 0: the system's current yy / yp plus the packed row, one addition per component, and a null side is
// taken as it is (no + 0.0: a -0.0 stays). icy / icyp: the snapshot's rows follow when it has been taken, else null.
__global__ __launch_bounds__(256) void reinit_kernel(VecState s, const int* __restrict__ idx, const double* __restrict__ y0,
                                                     const double* __restrict__ yp0, int add, double* __restrict__ icy,
                                                     double* __restrict__ icyp) {
    const int b = idx[blockIdx.x];
    const long vb = (long)b * s.n;
    const long src = (long)blockIdx.x * s.n;
    for (int i = threadIdx.x; i < s.n; i += 256) {
        double y, yp;
        if (add) {
            y = s.yy[vb + i];
            yp = s.yp[vb + i];
            if (y0) y = y + y0[src + i];
            if (yp0) yp = yp + yp0[src + i];
        } else {
            y = y0[src + i];
            yp = yp0[src + i];
        }
        el_reinit(s, vb, i, y, yp);
        if (icy) {
            icy[vb + i] = y;
            icyp[vb + i] = yp;
        }
    }
}

}  // namespace idahip
