// The stepper's per-element vector arithmetic, written once. Every function here does the work of ONE element of ONE system --
// no loop over the elements, no barrier, no sum -- and reaches the system's vectors through the VecState, the system's offset vb
// and the element's index i. A summand of a norm leaves through the caller's sink. The callers loop: the workgroup-per-system
// kernels of vector_kernels.hpp (256 threads) and WgVec of round_ida.hpp (64 threads) stride over i and send the summands to LDS
// (LdsSink), where after a barrier one lane adds up each row; the thread-per-system TinyVec / TinyVecConstr of tiny_ida.hpp run
// i = 0..n and accumulate in registers (AccSink). Every expression keeps the reference's association and order (the library is
// built with -ffp-contract=off), so the three steppers carry the same bits.
//   ewt_set        <- /root/reference/src/tol_control.rs:36-44, 71-82
//   predict        <- /root/reference/src/lib.rs:894-959
//   final yy/yp    <- /root/reference/src/lib.rs:845-849
//   test_error     <- /root/reference/src/lib.rs:983-1004 (vector part)
//   restore        <- /root/reference/src/lib.rs:1057-1082
//   complete_step  <- /root/reference/src/impl_complete_step.rs:74-77, 152-176; /root/reference/src/lib.rs:708
//   get_solution   <- /root/reference/src/lib.rs:1319-1340
//   Ida::new       <- /root/reference/src/lib.rs:291-293, /root/reference/src/ida_nls.rs:83-84
//   constraints    <- DESIGN.md section 4g (C IDA's IDASetConstraints; the reference has none)
#pragma once
#include "common.hpp"
#include "solve_kernels.hpp"
#include "../host/ida_controller.hpp"

namespace idahip {

struct VecState {
    double* phi;  // [6][batch][n]
    long phistride;  // batch*n
    double *yy, *yp, *yypredict, *yppredict, *ewt, *ee, *delta;
    int n;
    double rtol, atol_s;
    const double* atol_v;
    const double* mask;  // the ctx's id vector [n] when idahip_set_suppress_alg is on, else null: the local error norms leave out id_i == 0
};

// one summand of a local error norm: p = x_i w_i, times the mask's 1.0 / 0.0 when there is one (norm_rms.rs:49-57 -- the product is
// formed either way, so a non-finite masked element still makes the norm NaN). Without a mask this is p itself.
__device__ __forceinline__ double mask_term(const double* mask, int i, double p) {
    return mask ? p * (mask[i] != 0.0 ? 1.0 : 0.0) : p;
}

__device__ __forceinline__ double ewt_of(const VecState& s, double y, int i) {
    const double at = s.atol_v ? s.atol_v[i] : s.atol_s;
    return 1.0 / (s.rtol * fabs(y) + at);
}

__device__ __forceinline__ double& el_phi(const VecState& s, int j, long vb, int i) { return s.phi[j * s.phistride + vb + i]; }

// the square of one masked summand
__device__ __forceinline__ double el_sq(const VecState& s, int i, double x) {
    const double p = mask_term(s.mask, i, x);
    return p * p;
}

// where an element's k-th summand goes: into the workgroup's LDS, row k of n (after a barrier one lane per row adds it up,
// seq_sum_lds), or straight onto the owning thread's k-th accumulator. Either way a sum is accumulated left to right. An error
// term the order does not have arrives as +0.0: added to a sum of squares it changes no bit.
struct LdsSink {
    double* p;  // &sm[i]
    int n;
    __device__ __forceinline__ void put(int k, double v) const { p[k * n] = v; }
};
struct AccSink {
    double* acc;
    __device__ __forceinline__ void put(int k, double v) const { acc[k] = acc[k] + v; }
};

// first call: ewt = ewt_set(phi[0]); summand 0 = (phi[1] ewt)^2, summand 1 = (phi[0] ewt)^2
template <class Sink>
__device__ __forceinline__ void el_init_first(const VecState& s, long vb, int i, Sink t) {
    const double y = el_phi(s, 0, vb, i);
    const double e = ewt_of(s, y, i);
    s.ewt[vb + i] = e;
    t.put(0, el_sq(s, i, el_phi(s, 1, vb, i) * e));
    t.put(1, el_sq(s, i, y * e));
}

// phi[j] *= beta[j] (j = ns..kk); yypredict = sum_{j<=kk} phi[j]; yppredict = sum_{1<=j<=kk} gamma[j]*phi[j], left to right
__device__ __forceinline__ void el_predict(const VecState& s, long vb, int i, int kk, int ns, const double* beta, const double* gamma) {
    double yyp = 0.0, ypp = 0.0;
    for (int j = 0; j <= kk; ++j) {
        double p = el_phi(s, j, vb, i);
        if (j >= ns) {
            p *= beta[j];
            el_phi(s, j, vb, i) = p;
        }
        yyp = yyp + p;
        if (j >= 1) ypp = ypp + gamma[j] * p;
    }
    s.yypredict[vb + i] = yyp;
    s.yppredict[vb + i] = ypp;
}

// yy = yypredict + ee; yp = yppredict + cj*ee; returns yy
__device__ __forceinline__ double el_final_yy(const VecState& s, long vb, int i, double e, double cj) {
    const double y = s.yypredict[vb + i] + e;
    s.yy[vb + i] = y;
    s.yp[vb + i] = s.yppredict[vb + i] + cj * e;
    return y;
}

// the four error-test summands of e = ee_i, w = ewt_i; a term the order kk does not have is +0.0
template <class Sink>
__device__ __forceinline__ void el_error_terms(const VecState& s, long vb, int i, int kk, double e, double w, Sink t) {
    t.put(0, el_sq(s, i, e * w));
    double d = 0.0;
    if (kk > 1) d = el_phi(s, kk, vb, i) + e;  // delta = phi[kk] + ee   (lib.rs:992)
    t.put(1, kk > 1 ? el_sq(s, i, d * w) : 0.0);
    if (kk > 2) d = d + el_phi(s, kk - 1, vb, i);  // delta += phi[kk-1]  (lib.rs:1002)
    t.put(2, kk > 2 ? el_sq(s, i, d * w) : 0.0);
    const bool up = kk + 1 < MXORDP1;
    t.put(3, up ? el_sq(s, i, (e - el_phi(s, kk + 1, vb, i)) * w) : 0.0);  // ee - phi[kk+1]  (impl_complete_step.rs:75)
}

// the end of a Newton solve: the final yy / yp (when write_yy) and the four error-test summands of the ee in memory
template <class Sink>
__device__ __forceinline__ void el_post_newton(const VecState& s, long vb, int i, int kk, double cj, bool write_yy, Sink t) {
    const double e = s.ee[vb + i];
    const double w = s.ewt[vb + i];
    if (write_yy) el_final_yy(s, vb, i, e, cj);
    el_error_terms(s, vb, i, kk, e, w, t);
}

// phi[j] *= cvals[j-ns], j = ns..kk
__device__ __forceinline__ void el_restore(const VecState& s, long vb, int i, int kk, int ns, const double* cvals) {
    for (int j = ns; j <= kk; ++j) el_phi(s, j, vb, i) *= cvals[j - ns];
}

// phi[kused+1] = ee (kused < maxord); tmp = ee; for j = kused..0: tmp += phi[j]; phi[j] = tmp; ee *= ck; then
// ewt = ewt_set(phi[0]) and the summand (phi[0] ewt)^2. Returns whether the new ewt is bad.
template <class Sink>
__device__ __forceinline__ bool el_complete_step(const VecState& s, long vb, int i, int kused, double ck, int maxord, Sink t) {
    const double e = s.ee[vb + i];
    if (kused < maxord) el_phi(s, kused + 1, vb, i) = e;
    double tmp = e;
    for (int j = kused; j >= 0; --j) {
        tmp = tmp + el_phi(s, j, vb, i);
        el_phi(s, j, vb, i) = tmp;
    }
    s.ee[vb + i] = e * ck;
    const double w = ewt_of(s, tmp, i);  // tmp == new phi[0]
    s.ewt[vb + i] = w;
    t.put(0, el_sq(s, i, tmp * w));
    return w <= 0.0;  // `x <= 0` (impl_solve.rs:272): a NaN component is not bad
}

// yy = sum_{j<=kord} cvals[j]*phi[j]; yp = sum_{1<=j<=kord} dvals[j-1]*phi[j]  (from zero, scaled_add)
__device__ __forceinline__ void el_get_solution(const VecState& s, long vb, int i, int kord, const double* cvals, const double* dvals) {
    double y = 0.0, yp = 0.0;
    for (int j = 0; j <= kord; ++j) {
        const double p = el_phi(s, j, vb, i);
        y = y + cvals[j] * p;
        if (j >= 1) yp = yp + dvals[j - 1] * p;
    }
    s.yy[vb + i] = y;
    s.yp[vb + i] = yp;
}

// Ida::new again: phi[0] = yy = y0, phi[1] = yp = y0'
__device__ __forceinline__ void el_restore_initial(const VecState& s, long vb, int i, double y, double yp) {
    el_phi(s, 0, vb, i) = y;
    el_phi(s, 1, vb, i) = yp;
    s.yy[vb + i] = y;
    s.yp[vb + i] = yp;
}

// Ida::new with values of the caller's (idahip_reinit): as above, and the higher columns +0.0 as a created system has them
__device__ __forceinline__ void el_reinit(const VecState& s, long vb, int i, double y, double yp) {
    el_restore_initial(s, vb, i, y, yp);
    for (int j = 2; j < MXORDP1; ++j) el_phi(s, j, vb, i) = 0.0;
}

// the root finding's yy (ida_flow.hpp)
__device__ __forceinline__ void el_yy_from_phi01(const VecState& s, long vb, int i, double f) {
    s.yy[vb + i] = el_phi(s, 0, vb, i) + f * el_phi(s, 1, vb, i);
}
__device__ __forceinline__ void el_yy_add_phi1(const VecState& s, long vb, int i, double f) {
    s.yy[vb + i] = s.yy[vb + i] + f * el_phi(s, 1, vb, i);
}

// constraint check, first pass: the final yy / yp, then the summand (v ewt)^2 with v the correction of a violated component (+0.0
// elsewhere). c = the component's constraint (0 none, 1: y >= 0, -1: y <= 0, 2: y > 0, -2: y < 0). Returns violated or not.
template <class Sink>
__device__ __forceinline__ bool el_constr_check(const VecState& s, long vb, int i, double c, double cj, Sink t) {
    const double y = el_final_yy(s, vb, i, s.ee[vb + i], cj);
    const double w = s.ewt[vb + i];
    double v = 0.0;
    const bool bad = idactl::constr_violated(c, y);
    if (bad) v = idactl::constr_correction(c, y, w);
    const double p = v * w;
    t.put(0, p * p);
    return bad;
}

// constraint check, the correction accepted: ee -= v for a violated component (yy and yp keep their uncorrected values)
__device__ __forceinline__ void el_constr_correct(const VecState& s, long vb, int i, double c) {
    const double y = s.yy[vb + i];
    if (idactl::constr_violated(c, y)) s.ee[vb + i] = s.ee[vb + i] - idactl::constr_correction(c, y, s.ewt[vb + i]);
}

// constraint check, the step rejected: the smaller of q and phi[0] / (phi[0] - yy) for a violated component whose denominator is not zero
__device__ __forceinline__ double el_constr_quot(const VecState& s, long vb, int i, double c, double q) {
    const double y = s.yy[vb + i];
    if (!idactl::constr_violated(c, y)) return q;
    const double p0 = el_phi(s, 0, vb, i);
    const double t = p0 - y;
    if (t != 0.0) {
        const double quot = p0 / t;
        if (quot < q) q = quot;
    }
    return q;
}

}  // namespace idahip
