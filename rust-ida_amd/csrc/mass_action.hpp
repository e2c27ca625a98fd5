// IDAHIP_MASS_ACTION: a mass-action reaction network as a device problem. The network is data (include/ida_hip.h has the definition:
// reactant slots, stoichiometry entries, d, one rate constant per reaction and system); these kernels interpret two tables that
// idahip_set_mass_action builds on the host and uploads once:
//
//   residual   row_ptr[n+1] into rterms: the entries of row i in the caller's order, each (nu, r, the reaction's three slots)
//   Jacobian   the PATTERN: every diagonal position and every (i, j) that some entry of row i reaches through a slot holding j, in
//              column-major order; col_ptr[n+1] into the positions, pos_ptr[nnz+1] into jterms: the position's terms in the header's
//              order, each (nu, r, the reaction's two OTHER slots in slot order)
//
// A term is evaluated by one function, ma_term, for both tables: g = k_r, then g = g*y[slot] for the slots present, then (a network
// with rate laws, idahip_set_rate_network) g = g*f for the reaction's factors in order -- f a saturation or inhibition term, or its
// derivative for the one factor a Jacobian term differentiates --, then nu*g: every line one IEEE operation (-ffp-contract=off).
// The kernels are instantiated on LAWS: a polynomial network runs the <false> instantiations, which hold no factor code at all. The first term starts a sum (acc = t, not 0.0 + t: a first term of -0.0
// stays -0.0). Nothing is accumulated by two lanes: a residual row, a Jacobian position and a difference-quotient entry each
// belong to one lane, which walks its own term list. No atomics.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "dq_kernels.hpp"
#include "problem_kernels.hpp"
#include "solve_kernels.hpp"

namespace idahip {

struct MaTerm {
    double nu;
    int r;        // reaction: k[r]
    int a, b, c;  // species whose y multiply k[r], in this order; -1: none (trailing)
};

struct MaFac {
    int op;  // IDAHIP_RATE_SAT: y^h / (K^h + y^h), IDAHIP_RATE_INH: K^h / (K^h + y^h)
    int s;   // species
    int c;   // constant: params[nreac + c]
    int h;   // exponent, 1..4
};

struct MaNet {
    const int* row_ptr = nullptr;     // [n+1]
    const MaTerm* rterms = nullptr;   // [E]
    const double* d = nullptr;        // [n]
    const int* col_ptr = nullptr;     // [n+1] positions of column j: col_ptr[j] .. col_ptr[j+1]
    const int* pos_row = nullptr;     // [nnz]
    const int* pos_ptr = nullptr;     // [nnz+1]
    const MaTerm* jterms = nullptr;   // [T]
    int nparam = 0;                   // parameters per system: k[nreac], then (idahip_set_rate_network) K[nconst]
};

// A network with rate laws: the polynomial network's tables and the factors. The LAWS = true instantiations take this struct, the
// LAWS = false ones the MaNet above -- the argument, and with it the code, of a polynomial network's kernels is what it was before
// there were rate laws. The factors of reaction r are facs[fac_ptr[r] .. fac_ptr[r+1]), in the caller's order; jdfac[e]: which of
// its reaction's factors Jacobian term e differentiates (0..3), -1 for none (a slot's term).
struct MaLawNet : MaNet {
    int nreac = 0;                    // the constants follow the rate constants: K_c = params[nreac + c]
    const int* fac_ptr = nullptr;     // [nreac+1]
    const MaFac* facs = nullptr;      // [nfac]
    const int* jdfac = nullptr;       // [T]
};
template <bool LAWS>
using MaNetOf = std::conditional_t<LAWS, MaLawNet, MaNet>;

constexpr int MA_WAVE_MAX_N = 64;  // up to here: one wavefront per system, four systems per workgroup
constexpr int MA_SPW = 4;          // systems per 256-thread workgroup in that layout

// pw(x, h) of the header: x multiplied up, h - 1 products (1 <= h <= 4: no loop, nothing indexed)
__device__ __forceinline__ double ma_pw(double x, int h) {
    double p = x;
    if (h > 1) p = p * x;
    if (h > 2) p = p * x;
    if (h > 3) p = p * x;
    return p;
}

// f(factor), or df(factor) with deriv: one division either way (numerator and denominator are chosen first)
template <class Y>
__device__ __forceinline__ double ma_factor(const MaFac f, const double* __restrict__ K, Y y, bool deriv) {
    const double ys = y(f.s);
    const double yh = ma_pw(ys, f.h), Kh = ma_pw(K[f.c], f.h);
    const double den = Kh + yh;
    const bool sat = f.op == IDAHIP_RATE_SAT;
    double num = sat ? yh : Kh, dn = den;
    if (deriv) {
        num = Kh;
        if (f.h > 1) num = ((double)f.h * Kh) * ma_pw(ys, f.h - 1);
        dn = den * den;
    }
    const double q = num / dn;
    return (deriv && !sat) ? -q : q;
}

// dfac: the factor (its number within the reaction) that the term differentiates, -1 for none
template <bool LAWS, class Y>
__device__ __forceinline__ double ma_term(const MaNetOf<LAWS>& m, const MaTerm& t, int dfac, const double* __restrict__ k, Y y) {
    double g = k[t.r];
    if (t.a >= 0) g = g * y(t.a);
    if (t.b >= 0) g = g * y(t.b);
    if (t.c >= 0) g = g * y(t.c);
    if constexpr (LAWS) {
        const int f0 = m.fac_ptr[t.r], f1 = m.fac_ptr[t.r + 1];
        for (int f = f0; f < f1; ++f) g = g * ma_factor(m.facs[f], k + m.nreac, y, f - f0 == dfac);
    }
    return t.nu * g;
}

// the sum of terms [e0, e1) in order, the first term starting it; +0.0 for none. JAC: the terms are the Jacobian's (with rate laws
// each names the factor it differentiates, m.jdfac), else the residual's (none does)
template <bool LAWS, bool JAC, class Y>
__device__ __forceinline__ double ma_sum(const MaNetOf<LAWS>& m, const MaTerm* __restrict__ terms, int e0, int e1, const double* __restrict__ k, Y y) {
    double acc = 0.0;
    for (int e = e0; e < e1; ++e) {
        int dfac = -1;
        if constexpr (LAWS && JAC) dfac = m.jdfac[e];
        const double t = ma_term<LAWS>(m, terms[e], dfac, k, y);
        acc = (e == e0) ? t : acc + t;
    }
    return acc;
}

// F_i = d_i * y'_i - acc. With rate laws a zero denominator makes acc a NaN (0/0 comes out of the division with the sign bit set, as
// on the host), and the subtraction here is an addition of the NEGATED operand, which would hand that NaN on with its sign flipped:
// a NaN acc is F_i as it is, so that the residual has the bits the host's a - b gives. (A polynomial network has no division, and
// its row is the one line it always was.)
template <bool LAWS, class Y>
__device__ __forceinline__ double ma_row(const MaNetOf<LAWS>& m, int i, double ypi, const double* __restrict__ k, Y y) {
    const double acc = ma_sum<LAWS, false>(m, m.rterms, m.row_ptr[i], m.row_ptr[i + 1], k, y);
    const double r = m.d[i] * ypi - acc;
    if constexpr (LAWS) return (acc != acc) ? acc : r;
    return r;
}

// ------------------------------------------------------------------------------------------------ residual
// n <= 64: one wavefront per listed system, MA_SPW systems per workgroup, each wavefront with its own LDS slice; lane i stages
// (y_i, y'_i) and then evaluates row i. A wavefront whose system is skipped or past the list idles through the barrier: no lane
// returns ahead of it.
template <bool LAWS, class ARGS>
__device__ __forceinline__ void ma_sys_wave_body(ARGS a, MaNetOf<LAWS> m, const double* __restrict__ params, int nsys) {
    __shared__ double sy[MA_SPW][MA_WAVE_MAX_N];
    const int n = a.n;
    const int w = threadIdx.x >> 6, i = threadIdx.x & 63;
    const int s = blockIdx.x * MA_SPW + w;
    bool active = s < nsys;
    if (active && a.skip && a.skip[s] != 0) active = false;
    int b = 0;
    double ypi = 0.0;
    if (active && i < n) {
        b = a.idx[s];
        double y;
        sys_point(a, s, (long)b * n + i, i, a.cj[s], y, ypi);
        sy[w][i] = y;
    }
    __syncthreads();
    if (active && i < n) {
        const double* __restrict__ ys = sy[w];
        const double r = ma_row<LAWS>(m, i, ypi, params + (long)b * m.nparam, [&](int q) { return ys[q]; });
        a.delta[(long)b * n + i] = r;
        a.savres[(long)b * n + i] = r;
    }
}
template <bool LAWS, class ARGS>
__global__ __launch_bounds__(256) void ma_sys_wave_kernel(ARGS a, MaNetOf<LAWS> m, const double* __restrict__ params, int nsys) {
    ma_sys_wave_body<LAWS>(a, m, params, nsys);
}

// n > 64: one workgroup per listed system, y staged in LDS (dynamic: n doubles; 2 n with the IC front end's in-launch solve). A
// skipped system's workgroup leaves as a whole, ahead of the first barrier. VEC: the rows a lane takes in that solve.
template <bool LAWS, int VEC, class ARGS>
__device__ __forceinline__ void ma_sys_wg_body(ARGS a, MaNetOf<LAWS> m, const double* __restrict__ params) {
    extern __shared__ __align__(16) double sm[];
    const int n = a.n;
    double* syy = sm;
    if (a.skip && a.skip[blockIdx.x] != 0) return;
    const int b = a.idx[blockIdx.x];
    const long vb = (long)b * n;
    const double cj = a.cj[blockIdx.x];
    const double* __restrict__ k = params + (long)b * m.nparam;
    for (int i = threadIdx.x; i < n; i += 256) {
        double y, yp;
        sys_point(a, (int)blockIdx.x, vb + i, i, cj, y, yp);
        syy[i] = y;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const double r = ma_row<LAWS>(m, i, a.yp[vb + i], k, [&](int q) { return syy[q]; });
        a.delta[vb + i] = r;
        a.savres[vb + i] = r;
    }
    if constexpr (ARGS::IC) {
        if (a.lu) {
            __syncthreads();
            ic_solve_body<VEC>(a.lu, a.perm, a.delta, a.ewt, n, b, a.out, a.ord);
        }
    }
}
template <bool LAWS, int VEC, class ARGS>
__global__ __launch_bounds__(256) void ma_sys_kernel(ARGS a, MaNetOf<LAWS> m, const double* __restrict__ params) {
    ma_sys_wg_body<LAWS, VEC>(a, m, params);
}

// ------------------------------------------------------------------------------------------------ analytic Jacobian
// J = dF/dy + cj dF/dy' into the work matrix (column-major, n x n per system): (system, column chunk). The chunk's columns are
// written +0.0 first (J <- 0, ida_ls.rs:254), always: the stencil kernels' shortcut for a matrix the last factorisation left zeroed
// (LuWs::jwzero) is not taken here. After the workgroup's barrier one lane per pattern position writes base - acc. compact: the matrices go by list position, not by
// system id (idahip_mass_action_jac's buffer).
template <bool LAWS>
__global__ __launch_bounds__(256) void ma_jac_kernel(double* __restrict__ mats, int n, const double* __restrict__ yy, MaNetOf<LAWS> m,
                                                     const double* __restrict__ params, const int* __restrict__ idx,
                                                     const double* __restrict__ cjs, int chunks, const int* __restrict__ skip,
                                                     int compact) {
    if (skip && skip[blockIdx.x] != 0) return;
    const int b = idx[blockIdx.x];
    const double cj = cjs[blockIdx.x];
    const double* __restrict__ k = params + (long)b * m.nparam;
    const double* __restrict__ y = yy + (long)b * n;
    double* __restrict__ J = mats + (compact ? (long)blockIdx.x : (long)b) * n * n;
    const int per = (n + chunks - 1) / chunks;  // columns per block
    const int jbeg = blockIdx.y * per;
    const int jend = (jbeg + per < n) ? jbeg + per : n;
    if (jbeg >= jend) return;
    for (long e = (long)jbeg * n + threadIdx.x; e < (long)jend * n; e += 256) J[e] = 0.0;
    __syncthreads();
    const int pend = m.col_ptr[jend];
    int j = jbeg;
    for (int p = m.col_ptr[jbeg] + threadIdx.x; p < pend; p += 256) {
        while (m.col_ptr[j + 1] <= p) ++j;  // (p < col_ptr[jend]: j stays below jend)
        const int i = m.pos_row[p];
        const double acc = ma_sum<LAWS, true>(m, m.jterms, m.pos_ptr[p], m.pos_ptr[p + 1], k, [&](int q) { return y[q]; });
        const double base = (i == j) ? cj * m.d[i] : 0.0;
        J[(long)j * n + i] = base - acc;
    }
}

// ------------------------------------------------------------------------------------------------ difference-quotient Jacobian
// idaLsDenseDQJac as dq_kernels.hpp states it, every entry of the n x n matrix by the definition: entry (i, j) is row i of the
// residual with y_j and y'_j perturbed (ma_row, the residual kernel's row), differenced by dq_linsum. (system, column chunk); the
// system's y and y' are staged in LDS (dynamic: 2 n doubles).
template <bool LAWS>
__global__ __launch_bounds__(256) void ma_dq_jac_kernel(DqArgs d, MaNetOf<LAWS> m, const double* __restrict__ params, int chunks) {
    extern __shared__ __align__(16) double sm[];
    if (d.skip && d.skip[blockIdx.x] != 0) return;
    const int s = blockIdx.x;
    const int n = d.n;
    const int b = d.idx[s];
    const long vb = (long)b * n;
    const double cj = d.cj[s], hh = d.hh[s];
    const double* __restrict__ k = params + (long)b * m.nparam;
    double* sy = sm;
    double* syp = sm + n;
    for (int i = threadIdx.x; i < n; i += 256) {
        sy[i] = d.yy[vb + i];
        syp[i] = d.yp[vb + i];
    }
    __syncthreads();
    double* __restrict__ J = d.out + dq_slot(d, s, b) * n * n;
    const int per = (n + chunks - 1) / chunks;
    const int jbeg = blockIdx.y * per;
    const int jend = (jbeg + per < n) ? jbeg + per : n;
    for (long e = (long)jbeg * n + threadIdx.x; e < (long)jend * n; e += 256) {
        const int j = (int)(e / n), i = (int)(e - (long)j * n);
        const double inc = dq_inc(sy[j], syp[j], d.ewt[vb + j], hh);
        const double yj = sy[j] + inc;
        const double ypi = (i == j) ? syp[j] + cj * inc : syp[i];
        const double rt = ma_row<LAWS>(m, i, ypi, k, [&](int q) { return (q == j) ? yj : sy[q]; });
        J[e] = dq_linsum(1.0 / inc, rt, d.rr[vb + i]);
    }
}

}  // namespace idahip
