// Batched band LU (getrf / getrs), and the band form of the fused Newton-iteration body, for gfx950.
//
// Storage: LAPACK dgbtrf's, 0-based. A system with lower bandwidth ml and upper bandwidth mu has ldab = 2 ml + mu + 1 and
// kv = ml + mu; element (i, j), j - mu <= i <= j + ml, is ab[j * ldab + kv + i - j]. The top ml rows of every column are fill
// space: the factorisation writes U's fill (up to kv above the diagonal) there and needs nothing in them on entry. One system is
// ldab * n doubles, systems are [batch][ldab * n]; pivots are int64, 0-based rows, one per column -- the values dense_get_rf
// returns. The L multipliers stay where they were computed: as in LAPACK, a later row swap does not re-permute them (the dense
// factorisation's L is that L with the later swaps applied to its rows; idahip.band_expand_factors does exactly that).
//
// Arithmetic: that of dense_get_rf / dense_get_rs (crates/linear/src/dense.rs:86-206) on the band: strict `>` pivot search
// (lowest row on ties), reciprocal then multiply for the multipliers, unfused a_ij -= a_kj * a_ik, a column skipped when
// a_kj == 0, true division in the back substitution. The forward solve is LAPACK's interleaved one (swap b_k / b_piv[k], then
// eliminate with column k), which gives every entry the same subtractions in the same order as dense_get_rs' permute-then-
// substitute.
//
// Exactness contract. For finite inputs whose pivots have finite reciprocals, pivots and info are identical to dense_get_rf on
// the same matrix in dense storage, and factors and solutions are equal BY VALUE (-0.0 == +0.0): outside the band the dense code
// only forms x -= (+-0) * y, which can flip the sign of a zero and nothing else. Non-finite inputs may differ where the dense code
// forms 0 * inf outside the band. No stepper decision reads the sign of a zero (the weighted RMS norm squares it), so an
// integration on band factors takes the same steps, orders and step sizes as the dense one.
//
// Kernel shape. A band factorisation is a dependent chain of n steps per system: latency-bound, not bandwidth-bound. One lane
// walks one system's chain. For the narrow bands the library is built for (template <KL, KU>, instantiated for (1, 1)) the active
// (KL + 1) x (KL + KU + 1) window lives in registers, and the row (factorisation) or column (solves) that enters the window is
// loaded DIST steps ahead: its address never depends on a computed value, so no global load sits on the chain. Every other band
// takes the generic kernels, which run LAPACK's dgbtf2 / dgbtrs loops on global memory: correct for every 0 <= ml, mu <= n - 1,
// not made to be fast. All offsets are 64-bit.
#pragma once
#include "common.hpp"

namespace idahip {

constexpr int BAND_DIST = 8;  // steps between a load and the step that uses it (the register kernels' prefetch ring)

struct BandArgs {
    double* ab;           // [..][sstride] band storage
    long sstride;         // doubles per system (ldab * n for the ctx buffers)
    long long* piv;       // [..][pstride]
    long pstride;
    int n, ml, mu;
    const int* idx;       // list of systems
    int nsys;             // list length (upper bound when cnt != nullptr)
    const int* cnt;       // optional: the list's length on the device
    int* info;            // [batch] 0 | 1-based zero-pivot column
};

__device__ __forceinline__ long band_at(int ld, int kv, int i, int j) { return (long)j * ld + kv + i - j; }

__device__ __forceinline__ int band_list_len(const int* cnt, int nsys) { return cnt ? *cnt : nsys; }

// ------------------------------------------------------------------------------------------------ getrf, registers (narrow bands)
template <int KL, int KU>
__global__ __launch_bounds__(64) void band_getrf_reg_kernel(BandArgs g) {
    constexpr int KV = KL + KU, LD = 2 * KL + KU + 1, R = KL + 1, C = KV + 1, D = BAND_DIST;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= band_list_len(g.cnt, g.nsys)) return;
    const int b = g.idx[s];
    const int n = g.n;
    double* __restrict__ A = g.ab + (long)b * g.sstride;
    long long* __restrict__ P = g.piv + (long)b * g.pstride;
    // row q of the original matrix from column q - KL to q + KU (the part of it that enters the window), zeros past the matrix
    auto load_row = [&](int q, double (&v)[C]) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int col = q - KL + c;
            v[c] = (q < n && col < n) ? A[band_at(LD, KV, q, col)] : 0.0;
        }
    };
    double W[R][C];  // W[r][c] = entry (j + r, j + c)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c) W[r][c] = (r < n && c < n && c - KU <= r) ? A[band_at(LD, KV, r, c)] : 0.0;  // (above the band: fill)
    double pre[D][C];
#pragma unroll
    for (int u = 0; u < D; ++u) load_row(KL + 1 + u, pre[u]);
    int info = 0;
#pragma unroll 1
    for (int j0 = 0; j0 < n && info == 0; j0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int j = j0 + u;
            if (j >= n || info != 0) break;
            const int km = (n - 1 - j) < KL ? (n - 1 - j) : KL;
            int jp = 0;
            double amax = fabs(W[0][0]);
#pragma unroll
            for (int r = 1; r < R; ++r)
                if (r <= km && fabs(W[r][0]) > amax) { jp = r; amax = fabs(W[r][0]); }
            P[j] = j + jp;
            if (amax == 0.0) {  // zero pivot (|x| == 0 iff x == 0): the window goes back to memory as it stands, the system stops
                info = j + 1;
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        if (j + r < n && j + c < n) A[band_at(LD, KV, j + r, j + c)] = W[r][c];
                break;
            }
            // row swap over the window (past the last column any earlier row reached both rows hold +0.0: a no-op there)
#pragma unroll
            for (int r = 1; r < R; ++r)
                if (jp == r) {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const double t = W[0][c];
                        W[0][c] = W[r][c];
                        W[r][c] = t;
                    }
                }
            const double mult = 1.0 / W[0][0];
#pragma unroll
            for (int r = 1; r < R; ++r) W[r][0] *= mult;
#pragma unroll
            for (int c = 1; c < C; ++c) {
                const double akj = W[0][c];
                if (akj != 0.0) {
#pragma unroll
                    for (int r = 1; r < R; ++r) W[r][c] -= akj * W[r][0];
                }
            }
            // row j of U (fill included) and column j of L are final
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (j + c < n) A[band_at(LD, KV, j, j + c)] = W[0][c];
#pragma unroll
            for (int r = 1; r < R; ++r)
                if (j + r < n) A[band_at(LD, KV, j + r, j)] = W[r][0];
            // slide: rows up, columns left; column j + 1 + KV enters as fill zeros (no earlier step reached it), row j + 1 + KL from the ring
#pragma unroll
            for (int r = 0; r + 1 < R; ++r) {
#pragma unroll
                for (int c = 0; c + 1 < C; ++c) W[r][c] = W[r + 1][c + 1];
                W[r][C - 1] = 0.0;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) W[R - 1][c] = pre[u][c];
            load_row(j + 1 + KL + D, pre[u]);
        }
    }
    g.info[b] = info;
}

// ------------------------------------------------------------------------------------------------ getrf, generic (any band)
// LAPACK dgbtf2 on global memory, one lane per system; stops at the first zero pivot as dense_get_rf does.
__global__ __launch_bounds__(64) void band_getrf_kernel(BandArgs g) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= band_list_len(g.cnt, g.nsys)) return;
    const int b = g.idx[s];
    const int n = g.n, kl = g.ml, ku = g.mu, kv = kl + ku, ld = 2 * kl + ku + 1;
    double* __restrict__ A = g.ab + (long)b * g.sstride;
    long long* __restrict__ P = g.piv + (long)b * g.pstride;
    for (int j = 0; j < n; ++j)  // the fill rows start as zeros
        for (int i = j - kv; i < j - ku; ++i)
            if (i >= 0) A[band_at(ld, kv, i, j)] = 0.0;
    int info = 0, ju = 0;
    for (int j = 0; j < n; ++j) {
        const int km = (n - 1 - j) < kl ? (n - 1 - j) : kl;
        int jp = 0;
        for (int r = 1; r <= km; ++r)
            if (fabs(A[band_at(ld, kv, j + r, j)]) > fabs(A[band_at(ld, kv, j + jp, j)])) jp = r;
        P[j] = j + jp;
        if (A[band_at(ld, kv, j + jp, j)] == 0.0) { info = j + 1; break; }
        const int jr = (j + ku + jp) < (n - 1) ? (j + ku + jp) : (n - 1);
        ju = ju > jr ? ju : jr;
        if (jp != 0)
            for (int c = j; c <= ju; ++c) {
                const double t = A[band_at(ld, kv, j, c)];
                A[band_at(ld, kv, j, c)] = A[band_at(ld, kv, j + jp, c)];
                A[band_at(ld, kv, j + jp, c)] = t;
            }
        const double mult = 1.0 / A[band_at(ld, kv, j, j)];
        for (int r = 1; r <= km; ++r) A[band_at(ld, kv, j + r, j)] *= mult;
        for (int c = j + 1; c <= ju; ++c) {
            const double akj = A[band_at(ld, kv, j, c)];
            if (akj != 0.0)
                for (int r = 1; r <= km; ++r) A[band_at(ld, kv, j + r, c)] -= akj * A[band_at(ld, kv, j + r, j)];
        }
    }
    g.info[b] = info;
}

// ------------------------------------------------------------------------------------------------ solves
// x <- A^-1 x for one system, in place in `x` (global memory, this lane's own vector). `src(i)` gives the right-hand side's entry
// i, read once, in ascending i, before x[i] is first written (x may be the right-hand side itself).
template <int KL, int KU, class Src>
__device__ __forceinline__ void band_getrs_reg(const double* __restrict__ A, const long long* __restrict__ P, int n, double* x, Src src) {
    constexpr int KV = KL + KU, LD = 2 * KL + KU + 1, D = BAND_DIST;
    // ---- forward (L y = P b, interleaved): w[r] = b_{j + r}
    double w[KL + 1];
#pragma unroll
    for (int r = 0; r <= KL; ++r) w[r] = r < n ? src(r) : 0.0;
    double pl[D][KL + 1];  // ring: [0] = pivot offset of column j (as a double: exact), [1..KL] = L column j; b_{j + 1 + KL}: pb
    double pb[D];
    auto load_f = [&](int j, double (&l)[KL + 1], double& bb) {
        l[0] = j < n ? (double)(P[j] - j) : 0.0;
#pragma unroll
        for (int r = 1; r <= KL; ++r) l[r] = (j + r < n) ? A[band_at(LD, KV, j + r, j)] : 0.0;
        bb = (j + 1 + KL < n) ? src(j + 1 + KL) : 0.0;
    };
#pragma unroll
    for (int u = 0; u < D; ++u) load_f(u, pl[u], pb[u]);
#pragma unroll 1
    for (int j0 = 0; j0 < n; j0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int j = j0 + u;
            if (j >= n) break;
            const int l = (int)pl[u][0];
#pragma unroll
            for (int r = 1; r <= KL; ++r)
                if (l == r) {
                    const double t = w[0];
                    w[0] = w[r];
                    w[r] = t;
                }
            const double bj = w[0];
#pragma unroll
            for (int r = 1; r <= KL; ++r) w[r] -= pl[u][r] * bj;
            x[j] = bj;
#pragma unroll
            for (int r = 0; r < KL; ++r) w[r] = w[r + 1];
            w[KL] = pb[u];
            load_f(j + D, pl[u], pb[u]);
        }
    }
    // ---- backward (U x = y): v[c] = y_{k - KV + c}; column k of U = rows k - KV .. k
    double v[KV + 1];
#pragma unroll
    for (int c = 0; c <= KV; ++c) {
        const int i = n - 1 - KV + c;
        v[c] = i >= 0 ? x[i] : 0.0;
    }
    double pu[D][KV + 1], px[D];
    auto load_b = [&](int k, double (&uc)[KV + 1], double& xx) {
#pragma unroll
        for (int c = 0; c <= KV; ++c) {
            const int i = k - KV + c;
            uc[c] = (k >= 0 && i >= 0) ? A[band_at(LD, KV, i, k)] : 1.0;
        }
        const int ie = k - 1 - KV;
        xx = ie >= 0 ? x[ie] : 0.0;
    };
#pragma unroll
    for (int u = 0; u < D; ++u) load_b(n - 1 - u, pu[u], px[u]);
#pragma unroll 1
    for (int k0 = n - 1; k0 >= 0; k0 -= D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int k = k0 - u;
            if (k < 0) break;
            v[KV] = v[KV] / pu[u][KV];
            const double xk = v[KV];
#pragma unroll
            for (int c = 0; c < KV; ++c) v[c] -= pu[u][c] * xk;
            x[k] = xk;
#pragma unroll
            for (int c = KV; c > 0; --c) v[c] = v[c - 1];
            v[0] = px[u];
            load_b(k - D, pu[u], px[u]);
        }
    }
}

// LAPACK dgbtrs on global memory (any band)
template <class Src>
__device__ __forceinline__ void band_getrs_generic(const double* __restrict__ A, const long long* __restrict__ P, int n, int kl, int ku,
                                                   double* x, Src src) {
    const int kv = kl + ku, ld = 2 * kl + ku + 1;
    for (int i = 0; i < n; ++i) x[i] = src(i);
    for (int j = 0; j < n; ++j) {
        const int l = (int)P[j];
        if (l != j) {
            const double t = x[l];
            x[l] = x[j];
            x[j] = t;
        }
        const double bj = x[j];
        const int lm = (n - 1 - j) < kl ? (n - 1 - j) : kl;
        for (int r = 1; r <= lm; ++r) x[j + r] -= A[band_at(ld, kv, j + r, j)] * bj;
    }
    for (int k = n - 1; k >= 0; --k) {
        x[k] = x[k] / A[band_at(ld, kv, k, k)];
        const double xk = x[k];
        for (int i = (k - kv > 0 ? k - kv : 0); i < k; ++i) x[i] -= A[band_at(ld, kv, i, k)] * xk;
    }
}

// stand-alone solve: X[b] <- A_b^-1 B[b] (X may equal B)
template <int KL, int KU>
__global__ __launch_bounds__(64) void band_getrs_kernel(const double* __restrict__ ab, long sstride, const long long* __restrict__ piv,
                                                        long pstride, double* X, const double* Bv, int n, int ml, int mu,
                                                        const int* __restrict__ idx, int nsys) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsys) return;
    const int b = idx[s];
    const double* A = ab + (long)b * sstride;
    const long long* P = piv + (long)b * pstride;
    double* x = X + (long)b * n;
    const double* bv = Bv + (long)b * n;
    auto src = [&](int i) { return bv[i]; };
    if constexpr (KL >= 0) band_getrs_reg<KL, KU>(A, P, n, x, src);
    else band_getrs_generic(A, P, n, ml, mu, x, src);
}

// ------------------------------------------------------------------------------------------------ fused Newton body (band)
// newton_iter_kernel's epilogue op for op: delta = -delta; delta = A^-1 delta; d = delta * scale; delta = d; ee += d;
// out = sum_i (d_i ewt_i)^2, left to right from 0.0 by this lane. KL < 0: the generic solve.
template <int KL, int KU>
__global__ __launch_bounds__(64) void band_newton_iter_kernel(const double* __restrict__ ab, const long long* __restrict__ piv, int ml, int mu,
                                                              double* delta, double* __restrict__ ee, const double* __restrict__ ewt, int n,
                                                              const int* __restrict__ idx, int nsys, const double* __restrict__ scale,
                                                              double* __restrict__ out, const int* __restrict__ skip) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsys) return;
    if (skip && skip[s] != 0) return;
    const int b = idx[s];
    const long ldab = 2 * ml + mu + 1;
    const double* A = ab + (long)b * ldab * n;
    const long long* P = piv + (long)b * n;
    const long vb = (long)b * n;
    double* x = delta + vb;
    auto src = [&](int i) { return -x[i]; };  // neg_mut (newton.rs:100)
    if constexpr (KL >= 0) band_getrs_reg<KL, KU>(A, P, n, x, src);
    else band_getrs_generic(A, P, n, ml, mu, x, src);
    const double sc = scale[s];
    const double* __restrict__ wv = ewt + vb;
    double* __restrict__ ev = ee + vb;
    double sum = 0.0;
#pragma unroll 8
    for (int i = 0; i < n; ++i) {
        const double d = x[i] * sc;  // ida_ls.rs:406-410
        x[i] = d;
        ev[i] = ev[i] + d;           // newton.rs:106
        const double p = d * wv[i];
        sum = sum + p * p;
    }
    out[s] = sum;
}

}  // namespace idahip
