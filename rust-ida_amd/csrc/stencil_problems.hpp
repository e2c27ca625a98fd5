// The banded method-of-lines device problems, one description each: everything the stencil kernels (problem_kernels.hpp,
// dq_kernels.hpp, krylov_kernels.hpp) and the host side's dispatch need to know about a problem. Plain C++17, no HIP types: the
// same text compiles for the device and, under g++, for the host-side check of tests/native/stencil_check.cpp.
//
// A description P has
//   KIND, NPARAM, HALF_BW   its idahip_problem value, parameters per system, and the half-bandwidth of dF/dy
//   row(n, r, ypr, prm, py) row r of F at the point whose component k is py(k) -- the state itself or a perturbed one -- and whose
//                           own y' is ypr. The residual kernel, the DQ Jacobians and the Krylov residual all evaluate this one
//                           expression.
//   jac_entry(y, n, r, c, cj, prm)
//                           J(r, c) = dF_r/dy_c + cj dF_r/dy'_c at y, for |r - c| <= HALF_BW (every other entry is +0.0, and so are
//                           the in-band ones no term reaches)
// Every line is one IEEE operation in the order include/ida_hip.h defines (-ffp-contract=off); nothing may be re-associated.
#pragma once
#include "../../include/ida_hip.h"

#if defined(__HIPCC__)
#define IDAHIP_STENCIL_FN __host__ __device__ __forceinline__
#else
#define IDAHIP_STENCIL_FN inline
#endif

namespace idahip {

// 1-D heat equation: prm = [kappa/dx^2]; Dirichlet end rows F_r = y_r
struct Heat1D {
    static constexpr int KIND = IDAHIP_HEAT1D, NPARAM = 1, HALF_BW = 1;

    template <class PY>
    static IDAHIP_STENCIL_FN double row(int n, int r, double ypr, const double* prm, PY py) {
        if (r == 0 || r == n - 1) return py(r);
        const double coef = prm[0];
        return ypr - coef * ((py(r - 1) - 2.0 * py(r)) + py(r + 1));
    }

    static IDAHIP_STENCIL_FN double jac_entry(const double*, int n, int r, int c, double cj, const double* prm) {
        if (r == 0 || r == n - 1) return r == c ? 1.0 : 0.0;
        const double coef = prm[0];
        if (r == c) return cj + 2.0 * coef;
        return -coef;
    }
};

// 1-D Brusselator: n = 2m, y[2i] = u_i, y[2i+1] = v_i; prm = [a, b, d, ub, vb] (include/ida_hip.h has the definition)
struct Bruss1D {
    static constexpr int KIND = IDAHIP_BRUSS1D, NPARAM = 5, HALF_BW = 2;

    template <class PY>
    static IDAHIP_STENCIL_FN double row(int n, int r, double ypr, const double* prm, PY py) {
        const int i = r >> 1, m = n >> 1;
        if (i == 0 || i == m - 1) return py(r) - prm[3 + (r & 1)];
        const double a = prm[0], b = prm[1], d = prm[2];
        const double u = py(2 * i), v = py(2 * i + 1);
        const double w = (u * u) * v;
        if ((r & 1) == 0) {
            const double lu = (py(r - 2) - 2.0 * u) + py(r + 2);
            return ypr - (((a - (b + 1.0) * u) + w) + d * lu);
        }
        const double lv = (py(r - 2) - 2.0 * v) + py(r + 2);
        return ypr - ((b * u - w) + d * lv);
    }

    static IDAHIP_STENCIL_FN double jac_entry(const double* y, int n, int r, int c, double cj, const double* prm) {
        const int i = r >> 1, m = n >> 1;
        if (i == 0 || i == m - 1) return r == c ? 1.0 : 0.0;
        const double b = prm[1], d = prm[2];
        const int off = c - r;
        if (off == -2 || off == 2) return -d;
        const double u = y[2 * i], v = y[2 * i + 1];
        if ((r & 1) == 0) {
            if (off == 0) {
                const double t2 = (2.0 * u) * v;
                return cj - ((t2 - (b + 1.0)) - 2.0 * d);
            }
            if (off == 1) return -(u * u);
            return 0.0;
        }
        if (off == -1) {
            const double t2 = (2.0 * u) * v;
            return -(b - t2);
        }
        if (off == 0) return cj + (u * u + 2.0 * d);
        return 0.0;
    }
};

// the kernels' band predicate: is entry (r, c) inside P's band (and so jac_entry's to give), or one of the +0.0 outside it
template <class P>
IDAHIP_STENCIL_FN bool stencil_in_band(int r, int c) {
    return r >= c - P::HALF_BW && r <= c + P::HALF_BW;
}

// the description of a problem kind; void for the kinds that are no stencil
template <int KIND> struct stencil_of { using type = void; };
template <> struct stencil_of<Heat1D::KIND> { using type = Heat1D; };
template <> struct stencil_of<Bruss1D::KIND> { using type = Bruss1D; };

}  // namespace idahip
