// The one-thread stepper of tiny_ida.hpp over a reaction network's tables (IDAHIP_MASS_ACTION, 2 <= n <= TINY_N, opted in with
// idahip_set_mass_action_tiny): the same launch, flow, vector backend and Newton::solve text, with a Newton backend that interprets
// the tables through mass_action.hpp's ma_term / ma_sum / ma_row -- the one source of the residual, the Jacobian and the difference
// quotient, so every entry has the operations, in the order, of ma_sys_wave_kernel, ma_jac_kernel and ma_dq_jac_kernel, and the
// factorisation is tiny_getrf as the host stepper launches it for n <= TINY_N.
//
// n is a run-time value here. A private array indexed by it would live in scratch memory, so the backend keeps none: y and y' are
// read where the vector code keeps them (the system's block of LDS, or the global arrays in the no-LDS fallback), the Jacobian is
// formed in the system's matrix and factored in place, and the linear solve runs in delta itself.
#pragma once
#include "mass_action.hpp"
#include "tiny_ida.hpp"

namespace idahip {

// LDS a workgroup of the network kernels may take when the batch fills the device: a quarter of the CU's 160 KB, so that one
// wavefront per SIMD stays resident (idahip_tiny_solve bounds the systems per wavefront by it; DESIGN.md section 4m+)
constexpr size_t TINY_NET_LDS_PER_WG = 160 * 1024 / 4;

template <bool LAWS>
struct TinyNetNewton {
    const TinyIdaArgs& a;
    idactl::SysCore& s;
    const MaNetOf<LAWS>& m;
    const double* k;  // the system's parameters
    const int n;
    const long vb;    // as in TinyVec
    const long lub;   // offset of the system's matrix in a.lu

    // idaNlsResidual
    __device__ void nls_sys(bool reset_ee) const {
        for (int i = 0; i < n; ++i) {
            double yc = a.v.ee[vb + i];
            if (reset_ee) {
                yc = 0.0;
                a.v.ee[vb + i] = 0.0;
            }
            a.v.yy[vb + i] = a.v.yypredict[vb + i] + yc;
            a.v.yp[vb + i] = a.v.yppredict[vb + i] + s.cj * yc;
        }
        for (int i = 0; i < n; ++i) {
            const double r = ma_row<LAWS>(m, i, a.v.yp[vb + i], k, [&](int q) { return a.v.yy[vb + q]; });
            a.v.delta[vb + i] = r;
            a.savres[vb + i] = r;
        }
        s.nre += 1;
    }
    // idaNlsLSetup: the Jacobian at the current yy into the system's matrix + dense_get_rf in place; returns info
    __device__ int lsetup() const {
        double* M = a.lu + lub;
        const double cj = s.cj;
        if (a.jac_dq) {  // ma_dq_jac_kernel's entry, column by column: n residual evaluations
            for (int j = 0; j < n; ++j) {
                const double inc = dq_inc(a.v.yy[vb + j], a.v.yp[vb + j], a.v.ewt[vb + j], s.hh);
                const double yj = a.v.yy[vb + j] + inc;
                for (int i = 0; i < n; ++i) {
                    const double ypi = (i == j) ? a.v.yp[vb + j] + cj * inc : a.v.yp[vb + i];
                    const double rt = ma_row<LAWS>(m, i, ypi, k, [&](int q) { return (q == j) ? yj : a.v.yy[vb + q]; });
                    M[j * n + i] = dq_linsum(1.0 / inc, rt, a.savres[vb + i]);
                }
            }
            s.nre_dq += n;
        } else {  // ma_jac_kernel's: J <- +0.0, then base - acc at every position of the pattern, in its column-major order
            for (int e = 0; e < n * n; ++e) M[e] = 0.0;
            for (int j = 0; j < n; ++j)
                for (int p = m.col_ptr[j]; p < m.col_ptr[j + 1]; ++p) {
                    const int i = m.pos_row[p];
                    const double acc = ma_sum<LAWS, true>(m, m.jterms, m.pos_ptr[p], m.pos_ptr[p + 1], k, [&](int q) { return a.v.yy[vb + q]; });
                    const double base = (i == j) ? cj * m.d[i] : 0.0;
                    M[j * n + i] = base - acc;
                }
        }
        int lperm[TINY_N];  // (the composed permutation: written by tiny_getrf, read by nobody here)
        return tiny_getrf(M, n, a.piv + vb, lperm);
    }
    // one Newton iteration body, delta solved in place; returns delnrm
    __device__ double newton_iter() const {
        double* vv = a.v.delta + vb;
        for (int i = 0; i < n; ++i) vv[i] = -vv[i];
        tiny_getrs(a.lu + lub, n, a.piv + vb, vv);
        const double sc = idactl::after_lsolve(s, IDAHIP_LS_DIRECT, 0, false) ? 2.0 / (1.0 + s.cjratio) : 1.0;  // ida_ls.rs:387-418
        double acc = 0.0;
        for (int i = 0; i < n; ++i) {
            const double d = vv[i] * sc;
            vv[i] = d;
            a.v.ee[vb + i] = a.v.ee[vb + i] + d;
            const double p = d * a.v.ewt[vb + i];
            acc = acc + p * p;
        }
        return sqrt(acc / (double)n);
    }
    __device__ void solve() const { tiny_newton_solve(*this); }
};

// tiny_ida_kernel's staging with a run-time n (that kernel keeps its own text, with n a constant: moving it into these functions
// changes the registers of one of its instantiations, DESIGN.md section 4m+): the system's vectors, matrix and pivots from the
// global arrays into its block of LDS (tiny_lds_doubles(n) doubles); `a` (this thread's copy of the arguments)
// then points every field at the block, indexed from 0
__device__ __forceinline__ void tiny_stage_in(const TinyIdaArgs& ga, TinyIdaArgs& a, double* blk, int b, int n) {
    const long gvb = (long)b * n;
    for (int j = 0; j < MXORDP1; ++j)
        for (int i = 0; i < n; ++i) blk[j * n + i] = ga.v.phi[j * ga.v.phistride + gvb + i];
    double* const src[8] = {ga.v.yy, ga.v.yp, ga.v.yypredict, ga.v.yppredict, ga.v.ewt, ga.v.ee, ga.v.delta, ga.savres};
    for (int f = 0; f < 8; ++f)
        for (int i = 0; i < n; ++i) blk[(6 + f) * n + i] = src[f][gvb + i];
    for (int e = 0; e < n * n; ++e) blk[14 * n + e] = ga.lu[(long)b * n * n + e];
    long long* pv = reinterpret_cast<long long*>(blk + 14 * n + n * n);
    for (int i = 0; i < n; ++i) pv[i] = ga.piv[gvb + i];
    a.v.phi = blk;
    a.v.phistride = n;
    a.v.yy = blk + 6 * n;
    a.v.yp = blk + 7 * n;
    a.v.yypredict = blk + 8 * n;
    a.v.yppredict = blk + 9 * n;
    a.v.ewt = blk + 10 * n;
    a.v.ee = blk + 11 * n;
    a.v.delta = blk + 12 * n;
    a.savres = blk + 13 * n;
    a.lu = blk + 14 * n;
    a.piv = pv;
}
// and back
__device__ __forceinline__ void tiny_stage_out(const TinyIdaArgs& ga, const double* blk, int b, int n) {
    const long gvb = (long)b * n;
    for (int j = 0; j < MXORDP1; ++j)
        for (int i = 0; i < n; ++i) ga.v.phi[j * ga.v.phistride + gvb + i] = blk[j * n + i];
    double* const dst[8] = {ga.v.yy, ga.v.yp, ga.v.yypredict, ga.v.yppredict, ga.v.ewt, ga.v.ee, ga.v.delta, ga.savres};
    for (int f = 0; f < 8; ++f)
        for (int i = 0; i < n; ++i) dst[f][gvb + i] = blk[(6 + f) * n + i];
    for (int e = 0; e < n * n; ++e) ga.lu[(long)b * n * n + e] = blk[14 * n + e];
    const long long* pv = reinterpret_cast<const long long*>(blk + 14 * n + n * n);
    for (int i = 0; i < n; ++i) ga.piv[gvb + i] = pv[i];
}

// tiny_ida_kernel's body with n, the network and the parameters as kernel arguments of their own: TinyIdaArgs, TinyVec and FlowArgs
// are what they are for the built-in kinds (the comment above TinyVecConstr says why). LAWS x ROOTS x CONSTR: eight instantiations.
template <bool LAWS, bool ROOTS, bool CONSTR>
__global__ __launch_bounds__(64) void tiny_net_ida_kernel(TinyIdaArgs ga, int lds_vec, const double* constr, MaNetOf<LAWS> m,
                                                          const double* params, int n) {
    extern __shared__ __align__(16) unsigned char tiny_sm[];
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= ga.f.batch) return;
    idactl::SysCore& s = *reinterpret_cast<idactl::SysCore*>(tiny_sm + threadIdx.x * sizeof(idactl::SysCore));
    s = ga.sys[b];
    TinyIdaArgs a = ga;
    const long gvb = (long)b * n;
    double* blk = reinterpret_cast<double*>(tiny_sm + blockDim.x * sizeof(idactl::SysCore)) + (long)threadIdx.x * tiny_lds_doubles(n);
    if (lds_vec) tiny_stage_in(ga, a, blk, b, n);
    const long vb = lds_vec ? 0 : gvb, lub = lds_vec ? 0 : (long)b * n * n;
    using Vec = std::conditional_t<CONSTR, TinyVecConstr, TinyVec>;
    Vec v = [&] {
        if constexpr (CONSTR) return TinyVecConstr{{a, b, n, vb, gvb}, constr};
        else return TinyVec{a, b, n, vb, gvb};
    }();
    idahip_root_state rs;
    if (ROOTS) rs = ga.roots[b];
    const IdaFlow<Vec, ROOTS, CONSTR> F{a.f, s, v, ROOTS ? &rs : nullptr};
    const TinyNetNewton<LAWS> N{a, s, m, params + (long)b * m.nparam, n, vb, lub};
    long long ground = a.round_base;
    long long done = 0;
    bool stepping = F.enter(ground, b);
    for (;;) {
        if (a.max_rounds > 0 && done >= a.max_rounds) break;
        if (!stepping && !a.f.recycle) break;
        if (stepping) {
            if (s.ph == idactl::PH_LOOP_TOP && !F.loop_top()) {
                stepping = false;
                if (!a.f.recycle) break;
            } else {
                F.attempt_begin();
                N.solve();
                stepping = F.attempt_end();
            }
        }
        done += 1;
        ground += 1;
        if (a.f.recycle) {
            stepping = F.after_round_stream(stepping, ground, b, true);
            if (!stepping && s.status < 0) break;
        }
    }
    if (lds_vec) tiny_stage_out(ga, blk, b, n);
    ga.sys[b] = s;
    if (ROOTS) ga.roots[b] = rs;
    ga.rounds_done[b] = done;
}

}  // namespace idahip
