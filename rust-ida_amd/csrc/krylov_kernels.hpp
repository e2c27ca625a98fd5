// Matrix-free SPGMR for a Krylov ctx (idahip_create_krylov): C IDA's default iterative linear solver -- no preconditioner, scaling by
// ewt on both sides, modified Gram-Schmidt, no restarts, J v by a difference quotient of the residual (idaLsDQJtimes) -- batched over
// the ensemble. The definition, restated (DESIGN.md section 4h and include/ida_hip.h carry the same text):
//
//   kdot(x, y): p_i = x_i*y_i; partial q (0..63) = p_q + p_{q+64} + ... left to right from +0.0; result = the 64 partials summed
//               left to right from +0.0.
//   1. V0 = w*b; beta = sqrt(kdot(V0, V0)); beta <= tol: nli = 0, SUCCESS, res_norm = beta, x = b.
//   2. V0 *= 1/beta; rot = 1.
//   3. l = 0..maxl-1 (nli += 1): z = V_l/w; sig = sqrt(n); y' = sig*z + yy; yp' = (cj*sig)*z + yp; F' = F(tn, y', yp');
//      Jv = (1/sig)*(F' - rr); V_{l+1} = w*Jv; modified Gram-Schmidt against V_0..V_l with kdot; hn = sqrt(kdot(V_{l+1}, V_{l+1}));
//      Givens update of column l (host/krylov_scalar.hpp); rho = |rot*beta| <= tol: converged; else V_{l+1} *= 1/hn.
//   4. not converged: !(rho < beta): CONV_FAIL, no solution; else RES_REDUCED.
//   5. g = Q [beta, 0, ..]; back-substitution (a zero diagonal: QRSOL_FAIL); xc = g_0 V_0 + g_1 V_1 + ...; x = xc/w.
//
// One workgroup of 256 threads owns a listed system in every kernel here, and thread t owns the elements t, t + 256, ... of every
// vector of that system from the first launch to the last: the element-wise steps need no barrier among themselves, and the
// device functions below compute the same bits from the fused kernel (the whole solve in one launch) and from the split kernels
// (one launch per step, the host loops over l: host-callback residuals, and the cross-check of the fused kernel).
// The perturbed residual is computed in the operation order of the problem's residual kernel (problem_kernels.hpp), as
// dq_kernels.hpp does. -ffp-contract=off: no FMA. All per-system scalars are written with ordinary vector stores from plain C++.
//
// Band preconditioner (idahip_set_krylov_band_prec; DESIGN.md section 4i and include/ida_hip.h carry the same text): C IDA's IDABBDPRE
// with one block, applied on the left. Per system P is held in LAPACK band storage with half-bandwidths (ml, mu), ldab = 2 ml + mu + 1,
// [batch][ldab * n] doubles and [batch][n] int64 pivots, exactly as a band ctx holds its Jacobian (band_kernels.hpp).
//   psetup:     P = the band DQ Jacobian of dq_kernels.hpp (same increments, groups g < min(ml + mu + 1, n)) at the ctx's yy, yp, ewt,
//               rr = savres and the caller's tn, cj, hh, factored by band_kernels.hpp's getrf; info = 0 | 1-based zero-pivot column.
//   psolve(r):  band_kernels.hpp's getrs on those factors (interleaved forward solve, back substitution with true division).
//   the solve:  the definition above with two changes --
//     1. r = psolve(b); V0 = w*r; the zero-iteration return gives x = r (r is parked in the V_1 slot, unused until iteration 0).
//     3. after Jv = (1/sig)*(F' - rr): u = psolve(Jv); V_{l+1} = w*u.
//   Everything else is unchanged; rho is the norm of the preconditioned scaled residual; a solve performs 1 + nli psolves.
// kry_psolve below is the one device function behind all of it: the vector lives in LDS and is solved in place. (1, 1): one lane runs
// band_getrs_reg<1, 1> (its factor loads are prefetched off the dependent chain). (0, 0): element-wise division. Every other width:
// the workgroup shares each step's independent row updates, one row per lane, with a workgroup barrier between a step's reads and
// its writes and between its writes and the next step's reads; every entry receives band_getrs_generic's subtractions in its order.
#pragma once
#include "../host/krylov_scalar.hpp"
#include "common.hpp"
#include "solve_kernels.hpp"
#include "band_kernels.hpp"
#include "problem_kernels.hpp"

namespace idahip {

struct KryArgs {
    const double* yy;   // [batch][n] the ctx's fields
    const double* yp;
    const double* ewt;
    const double* rr;   // savres
    double* V;          // [batch][maxl + 1][n] Krylov basis
    idakry::Sys* st;    // [batch] per-system solver state (split path)
    double* stage;      // [nsys][3][n] by list position: y', yp', F' (split path)
    const int* idx;     // [nsys] system ids
    const double* cj;   // [nsys]
    const double* tol;  // [nsys]
    const int* skip;    // split path, per list position: nonzero = this system's loop has ended (null: none)
    // right-hand side and solution: [nsys][n] by list position (idahip_krylov_solve), or -- newton != 0 -- the ctx's delta, negated first
    const double* b;
    double* x;
    int newton;
    double* delta;      // [batch][n]
    double* ee;
    int* nli;           // [nsys] results
    int* flag;
    double* resnorm;
    double* nrm;        // [nsys] newton: sum_i (delta_i ewt_i)^2 left to right, 0 for a flag other than SUCCESS
    int* done;          // [nsys] split path: the loop of this system has ended
    int n, maxl;
    const double* params;  // a stencil problem's [batch][NPARAM]
    const double *A, *Bm, *C;  // linear dense
    // band preconditioner (the kernels instantiated with PREC only): factors [batch][(2 pml + pmu + 1) * n], pivots [batch][n]
    const double* pab;
    const long long* ppiv;
    int pml, pmu;
};

constexpr int KRY_T = 256;
// fixed LDS in front of the vectors: the solver state, 64 partials + the broadcast slots (all from the dynamic region, whose base
// stays 16-byte aligned)
constexpr int KRY_PART = 80;
constexpr size_t KRY_LDS_FIXED = sizeof(idakry::Sys) + sizeof(double) * KRY_PART;
static_assert(sizeof(idakry::Sys) % 16 == 0, "the vectors behind the state stay 16-byte aligned");

__host__ __device__ inline size_t kry_lds_bytes(int n, int vectors) { return KRY_LDS_FIXED + sizeof(double) * (size_t)n * vectors; }

// ---------------------------------------------------------------------------------------------- shared device functions
// kdot of the definition; sp: n doubles of LDS, part: KRY_PART doubles of LDS. Every thread returns the result.
__device__ __forceinline__ double kry_kdot(const double* __restrict__ x, const double* __restrict__ y, int n, double* sp, double* part) {
    const int t = threadIdx.x;
    for (int i = t; i < n; i += KRY_T) sp[i] = x[i] * y[i];
    __syncthreads();
    if (t < 64) {  // one wavefront forms the partials
        double a = 0.0;
        for (int i = t; i < n; i += 64) a = a + sp[i];
        part[t] = a;
    }
    __syncthreads();
    if (t == 0) {
        double r = 0.0;
        for (int q = 0; q < 64; ++q) r = r + part[q];
        part[64] = r;
    }
    __syncthreads();
    const double r = part[64];
    __syncthreads();  // sp and part are free again
    return r;
}

// x <- P^-1 x for one system, x: n doubles of LDS (band_kernels.hpp's getrs on the factors A / pivots P). Called by every thread of
// the workgroup; barriers on entry (x is complete) and on exit (x is the solution).
__device__ __forceinline__ void kry_psolve(const double* __restrict__ A, const long long* __restrict__ P, int n, int ml, int mu, double* x) {
    const int t = threadIdx.x;
    __syncthreads();
    if (ml == 1 && mu == 1) {
        if (t == 0) band_getrs_reg<1, 1>(A, P, n, x, [&](int i) { return x[i]; });
        __syncthreads();
        return;
    }
    const int kv = ml + mu, ld = 2 * ml + mu + 1;
    if (kv == 0) {  // a diagonal P: no elimination, pivots j
        for (int i = t; i < n; i += KRY_T) x[i] = x[i] / A[band_at(ld, kv, i, i)];
        __syncthreads();
        return;
    }
    // forward: step j swaps x_j / x_l (l = piv[j], j <= l <= j + lm) and eliminates with column j of L. Every lane reads x_j and x_l,
    // then the rows j + 1 .. j + lm are updated one per lane (row l from the swapped-in x_j) and lane 0 stores the swapped-in x_l
    for (int j = 0; j < n && ml > 0; ++j) {
        const int lm = (n - 1 - j) < ml ? (n - 1 - j) : ml;
        if (lm == 0) break;  // the last column: nothing below it, no swap
        const int l = (int)P[j];
        const double xj = x[j], bj = x[l];
        __syncthreads();  // x_j and x_l are read
        for (int r = 1 + t; r <= lm; r += KRY_T) {
            const int i = j + r;
            const double v = (i == l) ? xj : x[i];
            x[i] = v - A[band_at(ld, kv, i, j)] * bj;
        }
        if (t == 0) x[j] = bj;
        __syncthreads();  // the step's writes are visible
    }
    // backward: x_k = x_k / U(k, k), then the rows k - kv .. k - 1 one per lane
    for (int k = n - 1; k >= 0; --k) {
        const double xk = x[k] / A[band_at(ld, kv, k, k)];
        const int lo = k - kv > 0 ? k - kv : 0;
        __syncthreads();  // x_k is read
        for (int i = lo + t; i < k; i += KRY_T) x[i] = x[i] - A[band_at(ld, kv, i, k)] * xk;
        if (t == 0) x[k] = xk;
        __syncthreads();
    }
}

__device__ __forceinline__ void kry_psolve(const KryArgs& a, int b, double* x) {
    const long ldab = 2 * a.pml + a.pmu + 1;
    kry_psolve(a.pab + (long)b * ldab * a.n, a.ppiv + (long)b * a.n, a.n, a.pml, a.pmu, x);
}

// step 1: (newton: delta = -delta, b = delta;) V0 = w*b; returns beta. PREC: r = psolve(b) in sp, V0 = w*r, r parked in the V_1 slot
template <bool PREC>
__device__ __forceinline__ double kry_start(const KryArgs& a, int s, int b, double* sp, double* part) {
    const int n = a.n;
    const long vb = (long)b * n;
    double* V0 = a.V + (long)b * (a.maxl + 1) * n;
    for (int i = threadIdx.x; i < n; i += KRY_T) {
        double bi;
        if (a.newton) {
            bi = -a.delta[vb + i];
            a.delta[vb + i] = bi;
        } else {
            bi = a.b[(long)s * n + i];
        }
        if constexpr (PREC) sp[i] = bi;
        else V0[i] = a.ewt[vb + i] * bi;
    }
    if constexpr (PREC) {
        kry_psolve(a, b, sp);
        double* V1 = V0 + n;
        for (int i = threadIdx.x; i < n; i += KRY_T) {
            const double r = sp[i];
            V1[i] = r;
            V0[i] = a.ewt[vb + i] * r;
        }
    }
    __syncthreads();
    return sqrt(kry_kdot(V0, V0, n, sp, part));
}

// v *= 1/d
__device__ __forceinline__ void kry_normalise(double* __restrict__ v, int n, double d) {
    const double inv = 1.0 / d;
    for (int i = threadIdx.x; i < n; i += KRY_T) v[i] = v[i] * inv;
}

// the perturbed point of column l: y' = sig*z + yy, yp' = (cj*sig)*z + yp with z = V_l/w, into oy / oyp (LDS or the stage buffer)
__device__ __forceinline__ void kry_point(const KryArgs& a, int b, const double* __restrict__ Vl, double cj, double* oy, double* oyp) {
    const int n = a.n;
    const long vb = (long)b * n;
    const double sig = idakry::dq_sigma(n);
    const double cjsig = cj * sig;
    for (int i = threadIdx.x; i < n; i += KRY_T) {
        const double z = Vl[i] / a.ewt[vb + i];
        oy[i] = sig * z + a.yy[vb + i];
        oyp[i] = cjsig * z + a.yp[vb + i];
    }
}

// row i of the linear dense residual at (y', yp'): linear_sys_kernel's two chains over ascending columns (a stencil problem's row
// is its description's P::row itself, stencil_problems.hpp)
__device__ __forceinline__ double kry_res_linear(const double* __restrict__ Ab, const double* __restrict__ Bb, double ci, const double* y,
                                                 const double* ypv, int n, int i) {
    double ra = 0.0, rb = 0.0;
    int j = 0;
    for (; j + 8 <= n; j += 8) {
        double av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            av[u] = Ab[(long)(j + u) * n + i];
            bv[u] = Bb[(long)(j + u) * n + i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            ra = ra + av[u] * ypv[j + u];
            rb = rb + bv[u] * y[j + u];
        }
    }
    for (; j < n; ++j) {
        ra = ra + Ab[(long)j * n + i] * ypv[j];
        rb = rb + Bb[(long)j * n + i] * y[j];
    }
    return (ra + rb) - ci;
}

// F' of a built-in problem at the point in y / ypv (both complete: call after a barrier), row by row through `put`
template <int KIND, class Put>
__device__ __forceinline__ void kry_residual(const KryArgs& a, int b, const double* y, const double* ypv, Put put) {
    const int n = a.n;
    using P = typename stencil_of<KIND>::type;
    if constexpr (!std::is_void_v<P>) {
        const double* __restrict__ prm = a.params + (long)b * P::NPARAM;
        for (int i = threadIdx.x; i < n; i += KRY_T) put(i, P::row(n, i, ypv[i], prm, [&](int k) { return y[k]; }));
    } else {
        const double* __restrict__ Ab = a.A + (long)b * n * n;
        const double* __restrict__ Bb = a.Bm + (long)b * n * n;
        for (int i = threadIdx.x; i < n; i += KRY_T) put(i, kry_res_linear(Ab, Bb, a.C[(long)b * n + i], y, ypv, n, i));
    }
}

// Jv = (1/sig)*(F' - rr); V_{l+1} = w*Jv
__device__ __forceinline__ double kry_jv(const KryArgs& a, long e, double f) {
    const double inv_sig = 1.0 / idakry::dq_sigma(a.n);
    const double jv = inv_sig * (f - a.rr[e]);
    return a.ewt[e] * jv;
}
// PREC: Jv alone (into sp); then u = psolve(Jv) and V_{l+1} = w*u
__device__ __forceinline__ double kry_jv_raw(const KryArgs& a, long e, double f) {
    const double inv_sig = 1.0 / idakry::dq_sigma(a.n);
    return inv_sig * (f - a.rr[e]);
}
__device__ __forceinline__ void kry_prec_column(const KryArgs& a, int b, double* sp, double* __restrict__ Vn) {
    kry_psolve(a, b, sp);
    const long vb = (long)b * a.n;
    for (int i = threadIdx.x; i < a.n; i += KRY_T) Vn[i] = a.ewt[vb + i] * sp[i];
}

// Modified Gram-Schmidt of V_{l+1} against V_0..V_l, hn, the Givens update of column l by one lane, the convergence decision and
// (not converged) the normalisation of V_{l+1}; the last column without convergence ends the loop. k: the system's state (LDS or
// device memory); every thread returns k->done.
__device__ __forceinline__ int kry_orthogonalise(const KryArgs& a, int b, int l, idakry::Sys* k, double* sp, double* part) {
    const int n = a.n;
    double* Vb = a.V + (long)b * (a.maxl + 1) * n;
    double* Vn = Vb + (long)(l + 1) * n;
    __syncthreads();  // V_{l+1} is complete
    for (int i = 0; i <= l; ++i) {
        const double* Vi = Vb + (long)i * n;
        const double h = kry_kdot(Vi, Vn, n, sp, part);
        if (threadIdx.x == 0) k->H[i][l] = h;
        for (int e = threadIdx.x; e < n; e += KRY_T) Vn[e] = Vn[e] - h * Vi[e];
        __syncthreads();
    }
    const double hn = sqrt(kry_kdot(Vn, Vn, n, sp, part));
    if (threadIdx.x == 0) {
        k->H[l + 1][l] = hn;
        k->nli += 1;
        k->l = l;
        if (!idakry::givens_column(*k, l) && l + 1 == a.maxl) idakry::end_unconverged(*k, a.maxl);
        part[65] = (double)k->done;
    }
    __syncthreads();
    const int done = part[65] != 0.0;
    if (!done) kry_normalise(Vn, n, hn);
    __syncthreads();
    return done;
}

// steps 4 and 5 and the results of list position s; newton: the Newton body's tail (ee += delta, the sum of the WRMS norm)
template <bool PREC>
__device__ __forceinline__ void kry_finish(const KryArgs& a, int s, int b, idakry::Sys* k, double* sp, double* part) {
    const int n = a.n;
    const long vb = (long)b * n;
    const double* Vb = a.V + (long)b * (a.maxl + 1) * n;
    if (threadIdx.x == 0) {
        part[66] = (double)idakry::qr_solve(*k);
        part[67] = (double)k->krydim;
    }
    __syncthreads();
    const int flag = (int)part[66], m = (int)part[67];
    const bool formed = (flag == idakry::SUCCESS || flag == idakry::RES_REDUCED) && m > 0;
    double* xo = a.newton ? a.delta + vb : a.x + (long)s * n;
    for (int i = threadIdx.x; i < n; i += KRY_T) {
        double xi;
        if (formed) {
            double xc = k->g[0] * Vb[i];
            for (int j = 1; j < m; ++j) xc = xc + k->g[j] * Vb[(long)j * n + i];
            xi = xc / a.ewt[vb + i];
        } else {
            xi = a.newton ? a.delta[vb + i] : a.b[(long)s * n + i];  // x = b (the zero-iteration return; a failure forms nothing)
            if constexpr (PREC)
                if (flag == idakry::SUCCESS) xi = Vb[n + i];  // the zero-iteration return: x = P^-1 b, parked in the V_1 slot
        }
        if (!a.newton) {
            xo[i] = xi;
        } else if (flag == idakry::SUCCESS) {
            xo[i] = xi;
            a.ee[vb + i] = a.ee[vb + i] + xi;
            const double p = xi * a.ewt[vb + i];
            sp[i] = p * p;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.nli[s] = k->nli;
        a.flag[s] = flag;
        a.resnorm[s] = k->rho;
        if (a.newton) a.nrm[s] = flag == idakry::SUCCESS ? seq_sum_lds(sp, n) : 0.0;
    }
}

__device__ __forceinline__ void kry_lds(double* sm, idakry::Sys** k, double** part, double** v0) {
    *k = reinterpret_cast<idakry::Sys*>(sm);
    *part = sm + sizeof(idakry::Sys) / sizeof(double);
    *v0 = *part + KRY_PART;
}

// ---------------------------------------------------------------------------------------------- fused path
// The whole solve of one listed system in one launch (IDAHIP_HEAT1D, IDAHIP_BRUSS1D, IDAHIP_LINEAR_DENSE). Dynamic LDS: the state and the partials,
// then 3 n doubles (products, y', yp'); the basis lives in a.V and stays in L2.
// ROUND: the instantiation of the device lock-step rounds (round_ida.hpp), launched over the whole batch with a.skip per system; a
// skipped system's workgroup leaves at once. The host stepper's launches are the ROUND = false instantiations, which have no such test.
template <int KIND, bool PREC, bool ROUND = false>
__global__ __launch_bounds__(KRY_T) void krylov_fused_kernel(KryArgs a) {
    extern __shared__ __align__(16) double sm[];
    idakry::Sys* k;
    double *part, *sp;
    kry_lds(sm, &k, &part, &sp);
    const int n = a.n;
    double* sy = sp + n;
    double* syp = sy + n;
    const int s = blockIdx.x;
    if constexpr (ROUND) {
        if (a.skip[s] != 0) return;  // (uniform over the workgroup, before the first barrier)
    }
    const int b = a.idx[s];
    const long vb = (long)b * n;
    double* Vb = a.V + (long)b * (a.maxl + 1) * n;
    const double cj = a.cj[s];
    const double beta = kry_start<PREC>(a, s, b, sp, part);
    if (threadIdx.x == 0) part[65] = idakry::begin(*k, beta, a.tol[s]) ? 1.0 : 0.0;
    __syncthreads();
    int done = part[65] != 0.0;
    __syncthreads();
    if (!done) kry_normalise(Vb, n, beta);
    for (int l = 0; l < a.maxl && !done; ++l) {  // (done is uniform over the workgroup)
        kry_point(a, b, Vb + (long)l * n, cj, sy, syp);
        __syncthreads();
        double* Vn = Vb + (long)(l + 1) * n;
        if constexpr (PREC) {  // the products buffer is free here: Jv into it, solved in place
            kry_residual<KIND>(a, b, sy, syp, [&](int i, double f) { sp[i] = kry_jv_raw(a, vb + i, f); });
            kry_prec_column(a, b, sp, Vn);
        } else {
            kry_residual<KIND>(a, b, sy, syp, [&](int i, double f) { Vn[i] = kry_jv(a, vb + i, f); });
        }
        done = kry_orthogonalise(a, b, l, k, sp, part);
    }
    kry_finish<PREC>(a, s, b, k, sp, part);
}

// ---------------------------------------------------------------------------------------------- split path
// begin: steps 1 and 2; done[s] = 1 when the solve has ended there
template <bool PREC>
__global__ __launch_bounds__(KRY_T) void krylov_begin_kernel(KryArgs a) {
    extern __shared__ __align__(16) double sm[];
    idakry::Sys* kl;
    double *part, *sp;
    kry_lds(sm, &kl, &part, &sp);
    const int s = blockIdx.x;
    const int b = a.idx[s];
    idakry::Sys* k = a.st + b;
    const double beta = kry_start<PREC>(a, s, b, sp, part);
    if (threadIdx.x == 0) {
        const bool ended = idakry::begin(*k, beta, a.tol[s]);
        part[65] = ended ? 1.0 : 0.0;
        a.done[s] = ended ? 1 : 0;
    }
    __syncthreads();
    if (part[65] == 0.0) kry_normalise(a.V + (long)b * (a.maxl + 1) * a.n, a.n, beta);
}

// point: the perturbed point of column l, packed as the residual round trip of a host callback packs its point
__global__ __launch_bounds__(KRY_T) void krylov_point_kernel(KryArgs a, int l) {
    const int s = blockIdx.x;
    if (a.skip && a.skip[s] != 0) return;
    const int b = a.idx[s];
    const int n = a.n;
    double* st = a.stage + (long)s * 3 * n;
    kry_point(a, b, a.V + ((long)b * (a.maxl + 1) + l) * n, a.cj[s], st, st + n);
}

// the residual of a built-in problem at the packed point, into the stage buffer's third vector (dynamic LDS: 2 n doubles)
template <int KIND>
__global__ __launch_bounds__(KRY_T) void krylov_res_kernel(KryArgs a) {
    extern __shared__ __align__(16) double sm[];
    const int s = blockIdx.x;
    if (a.skip && a.skip[s] != 0) return;
    const int b = a.idx[s];
    const int n = a.n;
    double* st = a.stage + (long)s * 3 * n;
    double* sy = sm;
    double* syp = sm + n;
    for (int i = threadIdx.x; i < n; i += KRY_T) {
        sy[i] = st[i];
        syp[i] = st[n + i];
    }
    __syncthreads();
    kry_residual<KIND>(a, b, sy, syp, [&](int i, double f) { st[2 * n + i] = f; });
}

// step: Jv and its scaling from the staged residual, then the rest of iteration l; done[s] = 1 when the loop has ended
template <bool PREC>
__global__ __launch_bounds__(KRY_T) void krylov_step_kernel(KryArgs a, int l) {
    extern __shared__ __align__(16) double sm[];
    idakry::Sys* kl;
    double *part, *sp;
    kry_lds(sm, &kl, &part, &sp);
    const int s = blockIdx.x;
    if (a.skip && a.skip[s] != 0) return;
    const int b = a.idx[s];
    const int n = a.n;
    const long vb = (long)b * n;
    const double* f = a.stage + (long)s * 3 * n + 2 * n;
    double* Vn = a.V + ((long)b * (a.maxl + 1) + l + 1) * n;
    if constexpr (PREC) {
        for (int i = threadIdx.x; i < n; i += KRY_T) sp[i] = kry_jv_raw(a, vb + i, f[i]);
        kry_prec_column(a, b, sp, Vn);
    } else {
        for (int i = threadIdx.x; i < n; i += KRY_T) Vn[i] = kry_jv(a, vb + i, f[i]);
    }
    const int done = kry_orthogonalise(a, b, l, a.st + b, sp, part);
    if (threadIdx.x == 0) a.done[s] = done;
}

template <bool PREC>
__global__ __launch_bounds__(KRY_T) void krylov_finish_kernel(KryArgs a) {
    extern __shared__ __align__(16) double sm[];
    idakry::Sys* kl;
    double *part, *sp;
    kry_lds(sm, &kl, &part, &sp);
    const int s = blockIdx.x;
    const int b = a.idx[s];
    kry_finish<PREC>(a, s, b, a.st + b, sp, part);
}

// psolve alone (idahip_krylov_psolve): z = P^-1 r for the listed systems, r and z [nsys][n] by list position (dynamic LDS: n doubles)
__global__ __launch_bounds__(KRY_T) void krylov_psolve_kernel(const double* __restrict__ pab, const long long* __restrict__ ppiv, int n, int ml,
                                                              int mu, const double* __restrict__ r, double* __restrict__ z,
                                                              const int* __restrict__ idx) {
    extern __shared__ __align__(16) double sm[];
    const int s = blockIdx.x;
    const int b = idx[s];
    const long ldab = 2 * ml + mu + 1;
    for (int i = threadIdx.x; i < n; i += KRY_T) sm[i] = r[(long)s * n + i];
    kry_psolve(pab + (long)b * ldab * n, ppiv + (long)b * n, n, ml, mu, sm);
    for (int i = threadIdx.x; i < n; i += KRY_T) z[(long)s * n + i] = sm[i];
}

}  // namespace idahip
