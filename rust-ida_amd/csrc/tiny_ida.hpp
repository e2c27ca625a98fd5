// Device-resident BDF stepper for small systems (n <= TINY_N): the WHOLE of Ida::solve -- step-size and order controller
// included -- runs on the device, one thread per IVP, for as many step attempts as the caller allows. No host round trip per
// Newton iteration, per step attempt or per output time: one launch per idaens_solve / _schedule / _stream call.
// (before this, a lock-step round of config 2 was ~12 launches and ~5 host synchronisations of pure latency.)
//
// The scalar decisions are the SAME source as the host stepper's (host/ida_controller.hpp: set_coeffs, begin_attempt,
// conv_test, test_error, handle_n_flag, complete_step_scalars, get_solution_coeffs), compiled for the device with
// pow = glibc_pow::pow (glibc_pow.hpp: glibc's __pow_fma restated instruction for instruction), so h, order and every counter
// carry the reference's bits. The arithmetic of a vector element is vector_elems.hpp's, shared with the batched kernels
// (vector_kernels.hpp); the residuals, the Jacobians and the LU repeat problem_kernels.hpp, solve_kernels.hpp and lu_kernels.hpp's
// tiny_getrf element for element. With one thread per system every sum is sequential by construction. The control flow of
// Ida::solve is ida_flow.hpp's (shared with the workgroup-per-system stepper of round_ida.hpp); this file supplies the
// one-thread vector backend and the in-thread Newton solve:
//   Ida::solve            /root/reference/src/impl_solve.rs:69-376     (first-call block, loop-top checks, stop tests)
//   Ida::step             /root/reference/src/lib.rs:613-711
//   nonlinear_solve       /root/reference/src/lib.rs:787-890
//   Newton::solve         /root/reference/crates/nonlinear/src/newton.rs:51-167 (Q3: break on ConvergenceRecover with a current J)
//   IdaNLProblem          /root/reference/src/ida_nls.rs:118-266
//   complete_step         /root/reference/src/impl_complete_step.rs:22-177
// Root finding for the family g_i = y[c_i] - thr_i runs here too (ida_flow.hpp), and so does the inequality-constraint check of
// DESIGN.md section 4g (TinyVecConstr, the CONSTR instantiations). Not handled here (the host stepper keeps those
// cases): user root functions, IDA_ONE_STEP, host-callback problems, per-step traces.
#pragma once
#include "ida_flow.hpp"
#include "dq_kernels.hpp"
#include "lu_kernels.hpp"
#include "problem_kernels.hpp"
#include "solve_kernels.hpp"
#include "vector_kernels.hpp"

namespace idahip {

struct TinyIdaArgs {
    FlowArgs f;
    idactl::SysCore* sys;  // [batch] the controller state, uploaded before and downloaded after the launch
    VecState v;            // phi, yy, yp, yypredict, yppredict, ewt, ee, delta
    double* savres;
    double* lu;            // [batch][n*n] Jacobian, factored in place
    long long* piv;        // [batch][n]
    const double* params;
    int nparam;
    int jac_dq;                  // idahip_set_jacobian_dq: difference-quotient Jacobians (dq_kernels.hpp)
    const double *ic_y, *ic_yp;  // initial conditions (idaens_stream's restarts)
    long max_rounds;             // step attempts per system in this launch (0: until done)
    long long round_base;        // rounds executed before this launch
    double *yout, *ypout;        // [ntout][batch][n] or null: y, y' at every tout reached
    long long* rounds_done;      // [batch] rounds this system took part in during this launch
    idahip_root_state* roots;    // [batch] or null (f.nrt == 0)
};

// vector backend of IdaFlow: one thread owns system b and loops over its elements (vector_elems.hpp's arithmetic; the sums
// accumulate in registers)
struct TinyVec {
    const TinyIdaArgs& a;
    const int b, n;
    const long vb;   // offset of the system's vectors in a.v's arrays (0 when they are this thread's block of LDS)
    const long gvb;  // offset of the system in the global arrays (initial conditions)

    __device__ double& phi(int j, int i) const { return el_phi(a.v, j, vb, i); }

    // initial_setup's ewt_set(phi[0]) and the two norms of the first call
    __device__ void init_first(double* ypnorm, double* p0nrm) const {
        double acc[2] = {0.0, 0.0};
        for (int i = 0; i < n; ++i) el_init_first(a.v, vb, i, AccSink{acc});
        *ypnorm = sqrt(acc[0] / (double)n);
        *p0nrm = sqrt(acc[1] / (double)n);
    }
    __device__ void scale_phi1(double f) const {
        for (int i = 0; i < n; ++i) phi(1, i) *= f;
    }
    __device__ void predict(const idactl::SysCore& s) const {
        for (int i = 0; i < n; ++i) el_predict(a.v, vb, i, s.kk, s.ns, s.beta, s.gamma);
    }
    // the four error-test norms of the ee in memory, after the final yy / yp when write_yy
    __device__ void post_newton(const idactl::SysCore& s, double* norms, bool write_yy = true) const {
        const int kk = s.kk;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < n; ++i) el_post_newton(a.v, vb, i, kk, s.cj, write_yy, AccSink{acc});
        for (int k = 0; k < 4; ++k) norms[k] = sqrt(acc[k] / (double)n);
    }
    // the kk / ns of the failed attempt (cvals from restore_scalars)
    __device__ void restore_vec(const idactl::SysCore& s, int kk_att, int ns_att) const {
        for (int i = 0; i < n; ++i) el_restore(a.v, vb, i, kk_att, ns_att, s.cvals);
    }
    // the phi recurrence, ee *= ck, the new ewt and ||phi[0]||
    __device__ void complete_step_vec(idactl::SysCore& s, int kused, double ck, int maxord) const {
        bool bad = false;
        double acc = 0.0;
        for (int i = 0; i < n; ++i)
            if (el_complete_step(a.v, vb, i, kused, ck, maxord, AccSink{&acc})) bad = true;
        s.phi0nrm = sqrt(acc / (double)n);
        s.ewt_bad = bad;
    }
    __device__ void get_solution_vec(const idactl::SysCore& s, int kord) const {
        for (int i = 0; i < n; ++i) el_get_solution(a.v, vb, i, kord, s.cvals, s.dvals);
    }
    // root functions (ida_flow.hpp's backend of the shared root finding): one thread owns the system, nothing to synchronise
    __device__ void sync() const {}
    __device__ double yy_at(int i) const { return a.v.yy[vb + i]; }
    __device__ double phi_at(int j, int i) const { return phi(j, i); }
    __device__ void yy_from_phi01(double f) const {
        for (int i = 0; i < n; ++i) el_yy_from_phi01(a.v, vb, i, f);
    }
    __device__ void yy_add_phi1(double f) const {
        for (int i = 0; i < n; ++i) el_yy_add_phi1(a.v, vb, i, f);
    }
    __device__ void emit_output(int slot) const {  // the output of the tout just reached (idaens_solve_schedule's hYout / hYPout)
        if (a.yout)
            for (int i = 0; i < n; ++i) a.yout[((long)slot * a.f.batch + b) * n + i] = a.v.yy[vb + i];
        if (a.ypout)
            for (int i = 0; i < n; ++i) a.ypout[((long)slot * a.f.batch + b) * n + i] = a.v.yp[vb + i];
    }
    __device__ void restore_initial() const {  // Ida::new again
        for (int i = 0; i < n; ++i) el_restore_initial(a.v, vb, i, a.ic_y[gvb + i], a.ic_yp[gvb + i]);
    }
};

// TinyVec with the constraint check (the CONSTR instantiations). The constraint vector travels in this backend and not in
// TinyIdaArgs or TinyVec: the root-finding kernels keep both of those in scratch, and eight more bytes there change the resources of
// kernels that never read them.
struct TinyVecConstr : TinyVec {
    const double* constr;  // [n] idahip_set_constraints

    // post_newton_constr_kernel: post_newton with the constraint check between the final yy / yp and the
    // norms. checked = the Newton solve succeeded. Returns 0 passed, 1 ee corrected, 2 recover with *rr (norms are 0 then).
    __device__ int post_newton_constr(const idactl::SysCore& s, bool checked, double* norms, double* rr) const {
        *rr = 0.0;
        if (checked) {
            bool any = false;
            double sv = 0.0;
            for (int i = 0; i < n; ++i)
                if (el_constr_check(a.v, vb, i, constr[i], s.cj, AccSink{&sv})) any = true;
            if (any) {
                if (sqrt(sv / (double)n) <= s.eps_newt) {
                    for (int i = 0; i < n; ++i) el_constr_correct(a.v, vb, i, constr[i]);
                } else {
                    double q = idactl::CONSTR_QMAX;
                    for (int i = 0; i < n; ++i) q = el_constr_quot(a.v, vb, i, constr[i], q);
                    *rr = idactl::constr_rr(q);
                    norms[0] = norms[1] = norms[2] = norms[3] = 0.0;
                    return 2;
                }
                post_newton(s, norms, false);  // of the corrected ee; yy and yp keep their uncorrected values
                return 1;
            }
        }
        post_newton(s, norms);
        return 0;
    }
    // the start check: a component of phi[0] violates its constraint
    __device__ bool constr_phi0_violated() const {
        for (int i = 0; i < n; ++i)
            if (idactl::constr_violated(constr[i], phi(0, i))) return true;
        return false;
    }
};

// Newton::solve over a backend N that supplies s, nls_sys, lsetup and newton_iter (TinyNewton below, TinyNetNewton of
// tiny_net_ida.hpp). The flow is ida_controller.hpp's (newton_begin / newton_after_ctest); here: restart = the loop's first block
// again, iterate = sys(y) and the loop's body again, done = return
template <class N>
__device__ __forceinline__ void tiny_newton_solve(const N& nb) {
    idactl::SysCore& s = nb.s;
    bool restart = true;
    for (;;) {
        if (restart) {
            nb.nls_sys(true);  // sys(y0), y <- y0 = 0 (newton.rs:73)
            if (s.call_lsetup) idactl::after_lsetup(s, nb.lsetup());
            if (!idactl::newton_begin(s, s.call_lsetup)) return;
            restart = false;
        }
        const double delnrm = nb.newton_iter();
        s.niters += 1;
        bool converged = false;
        const int ret = idactl::conv_test(s, delnrm, &converged);
        const idactl::NewtonNext next = idactl::newton_after_ctest(s, ret, converged);
        if (next == idactl::NEWTON_DONE) return;
        if (next == idactl::NEWTON_ITERATE) nb.nls_sys(false);  // sys(y)
        else restart = true;
    }
}

// Newton::solve for one attempt of one small system, in the owning thread (newton.rs:51-167 as ensemble_ida.cpp's
// newton_solve_batched runs it for one system; tiny_sys_kernel / tiny_jac_kernel / tiny_getrf / tiny_newton_iter_kernel)
template <int KIND>
struct TinyNewton {
    const TinyIdaArgs& a;
    idactl::SysCore& s;
    const int b, n;
    const long vb;   // as in TinyVec
    const long lub;  // offset of the system's matrix in a.lu

    // idaNlsResidual
    __device__ void nls_sys(bool reset_ee) const {
        double yy[TINY_N], yp[TINY_N], r[TINY_N];
        for (int i = 0; i < n; ++i) {
            double yc = a.v.ee[vb + i];
            if (reset_ee) {
                yc = 0.0;
                a.v.ee[vb + i] = 0.0;
            }
            yy[i] = a.v.yypredict[vb + i] + yc;
            yp[i] = a.v.yppredict[vb + i] + s.cj * yc;
            a.v.yy[vb + i] = yy[i];
            a.v.yp[vb + i] = yp[i];
        }
        if (KIND == IDAHIP_ROBERTS) roberts_res(yy, yp, r);
        else lorenz_res(a.params + (long)b * a.nparam, yy, yp, r);
        for (int i = 0; i < n; ++i) {
            a.v.delta[vb + i] = r[i];
            a.savres[vb + i] = r[i];
        }
        s.nre += 1;
    }
    // idaNlsLSetup: jac at the current yy + dense_get_rf in place; returns info
    __device__ int lsetup() const {
        double y[TINY_N], J[TINY_N * TINY_N];
        for (int i = 0; i < n; ++i) y[i] = a.v.yy[vb + i];
        const double* prm = KIND == IDAHIP_ROBERTS ? nullptr : a.params + (long)b * a.nparam;
        if (a.jac_dq) {  // idaLsDenseDQJac at (yy, yp, savres) with the attempt's hh: n residual evaluations
            double yp[3], w[3], r0[3];
            for (int i = 0; i < 3; ++i) { yp[i] = a.v.yp[vb + i]; w[i] = a.v.ewt[vb + i]; r0[i] = a.savres[vb + i]; }
            tiny_dq_jac<KIND>(y, yp, w, r0, s.cj, s.hh, prm, J);
            s.nre_dq += 3;
        } else if (KIND == IDAHIP_ROBERTS) {
            roberts_jac(s.cj, y, J);
        } else {
            lorenz_jac(prm, s.cj, y, J);
        }
        double* M = a.lu + lub;
        for (int e = 0; e < n * n; ++e) M[e] = J[e];
        int lperm[TINY_N];
        return tiny_getrf(M, n, a.piv + vb, lperm);
    }
    // one Newton iteration body; returns delnrm
    __device__ double newton_iter() const {
        double vv[TINY_N];
        for (int i = 0; i < n; ++i) vv[i] = -a.v.delta[vb + i];
        tiny_getrs(a.lu + lub, n, a.piv + vb, vv);
        const double sc = idactl::after_lsolve(s, IDAHIP_LS_DIRECT /* = idahip_ls_type(): the only LSolver of this library */, 0, false) ? 2.0 / (1.0 + s.cjratio) : 1.0;  // ida_ls.rs:387-418
        double acc = 0.0;
        for (int i = 0; i < n; ++i) {
            const double d = vv[i] * sc;
            a.v.delta[vb + i] = d;
            a.v.ee[vb + i] = a.v.ee[vb + i] + d;
            const double p = d * a.v.ewt[vb + i];
            acc = acc + p * p;
        }
        return sqrt(acc / (double)n);
    }
    __device__ void solve() const { tiny_newton_solve(*this); }
};

// doubles of LDS one system's vectors take: phi[6], yy, yp, yypredict, yppredict, ewt, ee, delta, savres (14 n), the Jacobian /
// its factors (n^2) and the pivots (n)
__host__ __device__ constexpr int tiny_lds_doubles(int n) { return 14 * n + n * n + n; }

// Everything a system owns sits in LDS for the length of the launch -- the controller record (752 B) and, when the launch was
// given room for them (lds_vec), its vectors and its Jacobian: one lane walks dependent fp64 chains, and what it waits for is
// the latency of its own state (scratch and global memory: ~500 cycles a touch; LDS: ~60). The vector code is the same either way: the
// per-thread copy of the arguments points each field at this thread's block and the offsets vb / lub are zero. Config 2 (Lorenz63, 1024 systems): 26.0 -> 31.0 M iterations/s with the controller
// record alone.
template <int KIND, bool ROOTS, bool CONSTR>
__global__ __launch_bounds__(64) void tiny_ida_kernel(TinyIdaArgs ga, int lds_vec, const double* constr) {
    extern __shared__ __align__(16) unsigned char tiny_sm[];
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= ga.f.batch) return;
    // (blockDim.x = systems per wavefront, 64 or fewer: idahip_tiny_solve picks it by the batch size)
    idactl::SysCore& s = *reinterpret_cast<idactl::SysCore*>(tiny_sm + threadIdx.x * sizeof(idactl::SysCore));
    s = ga.sys[b];
    TinyIdaArgs a = ga;
    constexpr int n = 3;  // Roberts and Lorenz63 (idahip_create insists): a constant lets every vector loop unroll into registers
    const long gvb = (long)b * n;
    double* blk = reinterpret_cast<double*>(tiny_sm + blockDim.x * sizeof(idactl::SysCore)) + (long)threadIdx.x * tiny_lds_doubles(n);
    if (lds_vec) {
        for (int j = 0; j < MXORDP1; ++j)
            for (int i = 0; i < n; ++i) blk[j * n + i] = ga.v.phi[j * ga.v.phistride + gvb + i];
        double* const src[8] = {ga.v.yy, ga.v.yp, ga.v.yypredict, ga.v.yppredict, ga.v.ewt, ga.v.ee, ga.v.delta, ga.savres};
        for (int f = 0; f < 8; ++f)
            for (int i = 0; i < n; ++i) blk[(6 + f) * n + i] = src[f][gvb + i];
        for (int e = 0; e < n * n; ++e) blk[14 * n + e] = ga.lu[(long)b * n * n + e];
        long long* pv = reinterpret_cast<long long*>(blk + 14 * n + n * n);
        for (int i = 0; i < n; ++i) pv[i] = ga.piv[gvb + i];
        a.v.phi = blk;  // every field is indexed from 0 (vb = 0 below)
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
    const long vb = lds_vec ? 0 : gvb, lub = lds_vec ? 0 : (long)b * n * n;
    using Vec = std::conditional_t<CONSTR, TinyVecConstr, TinyVec>;
    Vec v = [&] {
        if constexpr (CONSTR) return TinyVecConstr{{a, b, n, vb, gvb}, constr};
        else return TinyVec{a, b, n, vb, gvb};
    }();
    idahip_root_state rs;
    if (ROOTS) rs = ga.roots[b];
    const IdaFlow<Vec, ROOTS, CONSTR> F{a.f, s, v, ROOTS ? &rs : nullptr};
    const TinyNewton<KIND> N{a, s, b, n, vb, lub};
    long long ground = a.round_base;  // global round counter (idaens_stream: every system takes part in every round)
    long long done = 0;
    bool stepping = F.enter(ground, b);
    for (;;) {
        if (a.max_rounds > 0 && done >= a.max_rounds) break;
        if (!stepping && !a.f.recycle) break;
        if (stepping) {
            if (s.ph == idactl::PH_LOOP_TOP && !F.loop_top()) {
                stepping = false;
                if (!a.f.recycle) break;  // (the call returned at the top of a round the system takes no part in)
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
            if (!stepping && s.status < 0) break;  // failed while streaming: the host reports it
        }
    }
    if (lds_vec) {
        for (int j = 0; j < MXORDP1; ++j)
            for (int i = 0; i < n; ++i) ga.v.phi[j * ga.v.phistride + gvb + i] = blk[j * n + i];
        double* const dst[8] = {ga.v.yy, ga.v.yp, ga.v.yypredict, ga.v.yppredict, ga.v.ewt, ga.v.ee, ga.v.delta, ga.savres};
        for (int f = 0; f < 8; ++f)
            for (int i = 0; i < n; ++i) dst[f][gvb + i] = blk[(6 + f) * n + i];
        for (int e = 0; e < n * n; ++e) ga.lu[(long)b * n * n + e] = blk[14 * n + e];
        const long long* pv = reinterpret_cast<const long long*>(blk + 14 * n + n * n);
        for (int i = 0; i < n; ++i) ga.piv[gvb + i] = pv[i];
    }
    ga.sys[b] = s;
    if (ROOTS) ga.roots[b] = rs;
    ga.rounds_done[b] = done;
}

}  // namespace idahip
