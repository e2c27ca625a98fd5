// The scalar part of the matrix-free SPGMR solver of a Krylov ctx (include/ida_hip.h has the same text): the
// tolerance, the Givens update of one Hessenberg column, the convergence decision, the rotation of g with the back-substitution, and
// the flags. One source for the device (csrc/krylov_kernels.hpp: one lane per system runs it) and the host (tests/native/
// krylov_scalar_check.cpp), like ida_controller.hpp. Every line is one IEEE operation: no FMA (-ffp-contract=off on both sides), 1/x
// is a true division.
//
// The solver is C IDA's default iterative setup: SPGMR, no preconditioner, scaling by ewt on both sides, modified Gram-Schmidt, no
// restarts. SUNDIALS' rare re-orthogonalisation pass is left out.
#pragma once
#include "ida_controller.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define IDAKRY_SQRT(x) ::sqrt(x)  // correctly rounded, as every sqrt of the device code
#else
#define IDAKRY_SQRT(x) std::sqrt(x)
#endif

namespace idakry {

constexpr int MAXL_MAX = 16;     // 1 <= maxl <= 16
constexpr int MAXL_DEFAULT = 5;  // C IDA's SUNSPGMR_MAXL_DEFAULT

enum Flag { SUCCESS = 0, RES_REDUCED = 1, CONV_FAIL = 2, QRSOL_FAIL = 3 };

// one linear solve of one system
struct Sys {
    double H[MAXL_MAX + 1][MAXL_MAX];  // Hessenberg matrix, H[i][l] = row i of column l
    double q[2 * MAXL_MAX];            // Givens rotations (c, s) of columns 0, 1, ...
    double g[MAXL_MAX + 1];            // the rotated right-hand side, then the coefficients of the solution
    double rot, beta, rho, tol;
    int l;       // the column being built
    int nli;     // linear iterations so far
    int flag;    // Flag, valid once `done`
    int krydim;  // columns the solution is formed from
    int done;    // 0 iterating, 1 the loop has ended (flag and krydim are set)
    int pad_;
};

// tol = (sqrt(n) * 0.05) * eps_newt: C IDA's eplin. idactl::lsolve_tol gives sqrt(n) * eplifac as the reference does (it has the
// eps_newt factor commented out, src/ida_ls.rs:325-326); the factor is applied here.
IDA_HD inline double tolerance(int n, double eps_newt) {
    return idactl::lsolve_tol(1, IDAKRY_SQRT((double)n), idactl::EPLIFAC) * eps_newt;
}
// sig = sqrt(n) * 1.0: the increment of idaLsDQJtimes (dqincfac = 1)
IDA_HD inline double dq_sigma(int n) { return IDAKRY_SQRT((double)n) * 1.0; }

// step 1 and 2 of the definition, after beta = sqrt(kdot(V0, V0)): returns true when the solve ends there (beta <= tol)
IDA_HD inline bool begin(Sys& k, double beta, double tol) {
    for (int i = 0; i <= MAXL_MAX; ++i)
        for (int j = 0; j < MAXL_MAX; ++j) k.H[i][j] = 0.0;
    for (int i = 0; i < 2 * MAXL_MAX; ++i) k.q[i] = 0.0;
    for (int i = 0; i <= MAXL_MAX; ++i) k.g[i] = 0.0;
    k.rot = 1.0;
    k.beta = beta;
    k.rho = beta;
    k.tol = tol;
    k.l = 0;
    k.nli = 0;
    k.flag = SUCCESS;
    k.krydim = 0;
    k.done = 0;
    k.pad_ = 0;
    if (beta <= tol) {
        k.done = 1;
        return true;
    }
    return false;
}

// Column l of H holds the Gram-Schmidt coefficients H[0..l][l] and hn = H[l+1][l]: apply the earlier rotations, form the new one,
// update rot and rho. Returns true when rho <= tol (converged: krydim = l + 1, flag SUCCESS).
IDA_HD inline bool givens_column(Sys& k, int l) {
    for (int j = 0; j < l; ++j) {
        const double c = k.q[2 * j], s = k.q[2 * j + 1];
        const double t1 = k.H[j][l], t2 = k.H[j + 1][l];
        k.H[j][l] = c * t1 - s * t2;
        k.H[j + 1][l] = s * t1 + c * t2;
    }
    const double t1 = k.H[l][l], t2 = k.H[l + 1][l];
    double c, s;
    if (t2 == 0.0) {
        c = 1.0;
        s = 0.0;
    } else if (IDA_FABS(t2) >= IDA_FABS(t1)) {
        const double t3 = t1 / t2;
        s = -1.0 / IDAKRY_SQRT(1.0 + t3 * t3);
        c = -s * t3;
    } else {
        const double t3 = t2 / t1;
        c = 1.0 / IDAKRY_SQRT(1.0 + t3 * t3);
        s = -c * t3;
    }
    k.q[2 * l] = c;
    k.q[2 * l + 1] = s;
    k.H[l][l] = c * t1 - s * t2;
    k.rot = k.rot * s;
    k.rho = IDA_FABS(k.rot * k.beta);
    if (k.rho <= k.tol) {
        k.krydim = l + 1;
        k.flag = SUCCESS;
        k.done = 1;
        return true;
    }
    return false;
}

// the loop has run its maxl columns without convergence
IDA_HD inline void end_unconverged(Sys& k, int maxl) {
    k.krydim = maxl;
    k.flag = !(k.rho < k.beta) ? CONV_FAIL : RES_REDUCED;
    k.done = 1;
}

// g = Q [beta, 0, ...], then the back-substitution with the triangular H; QRSOL_FAIL on a zero diagonal entry. A solve that ended
// in begin() or in CONV_FAIL forms no solution and is left alone. Returns the flag.
IDA_HD inline int qr_solve(Sys& k) {
    if (k.flag == CONV_FAIL || k.krydim == 0) return k.flag;
    const int m = k.krydim;
    k.g[0] = k.beta;
    for (int i = 1; i <= m; ++i) k.g[i] = 0.0;
    for (int j = 0; j < m; ++j) {
        const double c = k.q[2 * j], s = k.q[2 * j + 1];
        const double t1 = k.g[j], t2 = k.g[j + 1];
        k.g[j] = c * t1 - s * t2;
        k.g[j + 1] = s * t1 + c * t2;
    }
    for (int j = m - 1; j >= 0; --j) {
        if (k.H[j][j] == 0.0) {
            k.flag = QRSOL_FAIL;
            return k.flag;
        }
        k.g[j] = k.g[j] / k.H[j][j];
        for (int i = 0; i < j; ++i) k.g[i] = k.g[i] - k.g[j] * k.H[i][j];
    }
    return k.flag;
}

}  // namespace idakry
