// Batched triangular solves, the fused Newton-iteration body and the WRMS norm for gfx950.
//   dense_get_rs           <- /root/reference/crates/linear/src/dense.rs:165-206
//   Newton loop body       <- /root/reference/crates/nonlinear/src/newton.rs:98-110
//   idaNlsLSolve/idaLsSolve<- /root/reference/src/ida_nls.rs:190-215, /root/reference/src/ida_ls.rs:298-455
//   norm_wrms              <- /root/reference/src/norm_rms.rs:31-38
//
// Bit-exactness: each b_i receives b_i -= a_ik * b_k in ascending (forward) / descending (backward) k exactly as
// the reference's column-oriented loops do; unfused mul/sub; true division by u_kk. The WRMS sum is accumulated
// left to right by one lane (512 dependent adds ~ 2 us, hidden behind the other resident workgroups' streaming);
// the final sqrt(sum/N) is done by the host libm so the norm equals the reference's to the last bit.
//
// Performance model: the solve reads every LU entry once (8 N^2 B) in coalesced column segments, 16 B per lane;
// it is HBM-bound, so the kernel keeps registers low (8 workgroups of 256 threads per CU) and lets workgroups of
// different systems overlap the short serial diagonal phases with each other's streaming.
#pragma once
#include "common.hpp"
#include "../host/ida_controller.hpp"

namespace idahip {

// Sequential sum of sq[0..n) by the calling lane (LDS source), left to right from 0.0.
__device__ __forceinline__ double seq_sum_lds(const double* sq, int n) {
    double s = 0.0;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        const double a0 = sq[i], a1 = sq[i + 1], a2 = sq[i + 2], a3 = sq[i + 3], a4 = sq[i + 4], a5 = sq[i + 5], a6 = sq[i + 6],
                     a7 = sq[i + 7];
        s = s + a0; s = s + a1; s = s + a2; s = s + a3; s = s + a4; s = s + a5; s = s + a6; s = s + a7;
    }
    for (; i < n; ++i) s = s + sq[i];
    return s;
}

// Workgroup-cooperative getrs on the right-hand side held in LDS (bs[0..n)). blockDim.x == T.
// VEC = 2 requires n even (16-byte aligned column segments).
// zmap (T > 256 only, may be null): the factorisation's map of 64 x 64 blocks, zmap[K * 64 + I] = 0 when block (rows I, columns
// K) of LU holds only zeros. A sweep then leaves out the rows of such a block -- b_i -= 0 * b_k changes nothing -- unless that
// is not exactly true: a b_k of the column block is not finite (0 * inf is NaN), or the row's b_i is -0.0 (which -0.0 - (-0.0)
// would turn into +0.0). The factors of a banded matrix (the heat equation's Jacobian) are zero almost everywhere, and the
// reference's solve multiplies through all of it; so did this kernel, 134 MB per system and iteration at n = 4096.
// A solve reads every entry of the factors once: tb::NT_SOLVE (exp_switches.hpp) marks the loads of the sweeps and, with 256
// threads, of the diagonal blocks non-temporal. The staging loads of the diagonal blocks (T > 256, n >= 2048: 1/64 of a block
// column) keep the default policy: no run has compared the two there.
// dg (T > 256 only): 64 x 64 doubles of LDS for the diagonal block. With few, large systems per call a workgroup's life is
// its 2 n / 64 diagonal solves, and each of those was eight dependent round trips to memory (eight columns loaded, eight
// steps, ...): 17 us per block at n = 4096. The block a solve needs is instead fetched by all threads while the sweep before
// it streams (the factors are read-only), and the solve reads LDS.
// SL (T == 256, n <= 512; staged L, idahip_set_lu_staged): the factors hold L21 of block column q in the order of the live list behind
// super-panel q (LuWs::ord, lu_kernels.hpp) and bs arrives in PHYSICAL row order. In front of forward block q the entries bs[kb .. n)
// -- in the order of the live list in front of the super-panel -- move where its map sends them: the 64 pivots to kb .. kb + 63 in pivot
// order, the others behind them in the order of the next live list (registers, barrier, LDS, barrier). The diagonal solve and the
// sweep then read rows kb .. n of the block column exactly as they do in the reference layout, every b_i receives its updates in
// the same ascending k, and bs ends the forward pass in pivot order: the backward pass is the same code. ord = the system's maps,
// [ceil(n / 64)][n]. A thread needs two entries per block, at most sixteen per solve. They are NOT all fetched at kernel start: held in
// registers across the `unroll 1` block loop they would be an array indexed at run time (scratch, or eight more live VGPRs in a
// kernel that is asked for four workgroups per CU), and every __syncthreads() waits for all loads in flight anyway, so an early
// request buys nothing past the next barrier. Instead block q + 1's two entries are requested right behind block q's second barrier:
// the load travels with the diagonal block's first column group and has a whole diagonal solve and sweep to arrive -- never a
// dependent load in front of a permutation. (Block 0's entries are requested before the loop, beside nothing: the one exposed trip.)
template <int VEC, int T = 256, bool SL = false>
__device__ __forceinline__ void wg_getrs(const double* __restrict__ LU, int n, double* bs, double* dg = nullptr,
                                         const unsigned char* __restrict__ zmap = nullptr, const unsigned short* __restrict__ ord = nullptr) {
    static_assert(!SL || T == 256, "staged L is the 256-thread solve's (n <= 512: two entries of a block's map per thread)");
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    constexpr bool STAGE = T > 256;
    constexpr int UNR = 8;  // columns in flight per thread (16 changes nothing: a workgroup's stream is bound by its CU, ~30 GB/s)
    constexpr int SPT = STAGE ? (64 * 64) / T : 1;  // staged entries per thread
    double stg[SPT];
    auto stage_load = [&](int kb) {  // diagonal block at (kb, kb): entry e = t + j T is row e & 63 of column e >> 6
        const int kw = (n - kb) < 64 ? (n - kb) : 64;
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const int e = t + j * T, c = e >> 6, r = e & 63;
            stg[j] = (c < kw && r < kw) ? LU[(long)(kb + c) * n + kb + r] : 0.0;
        }
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int j = 0; j < SPT; ++j) dg[t + j * T] = stg[j];
    };
    if (STAGE) {
        stage_load(0);
        stage_store();
        __syncthreads();
    }
    // Diagonal blocks from global memory (T = 256): buffer loads whose per-lane offset is out of range for the lanes that take no
    // part -- they read +0.0 -- instead of a guarded load per column. Eight guarded loads are eight branches; the compiler's
    // wait-count bookkeeping then gives up and every step of the solve waits for ALL outstanding loads, the next group's
    // prefetch included: one trip to memory per eight steps, 5 us per diagonal block, 32 blocks per solve at n = 512.
    // (32-bit byte counts and scalar offsets: exact up to the largest matrix this library factors, LU_BIG_MAX_N = 4096 -> 128 MiB)
    static_assert((long long)LU_BIG_MAX_N * LU_BIG_MAX_N * 8 < (1ll << 31), "the buffer descriptor's 32-bit sizes and offsets assume n * n * 8 < 2^31");
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(LU), 0, STAGE ? 0 : n * n * 8, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;
    __shared__ int s_kfin;  // the entries of b the running column block multiplies with are all finite
    auto neg_zero = [](double x) { return __double_as_longlong(x) == (long long)0x8000000000000000ull; };

    int so[2] = {0, 0};  // SL: where entries t and t + 256 of bs[kb .. n) go (the running block's map)
    auto ld_ord = [&](const int kb) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int j = t + 256 * r;
            so[r] = (kb < n && j < n - kb) ? (int)ord[(kb >> 6) * n + j] : 0;
        }
    };
    if constexpr (SL) ld_ord(0);

    // ---- forward: L y = b, unit diagonal (dense.rs:188-194)
#pragma unroll 1
    for (int kb = 0; kb < n; kb += 64) {
        const int kw = (n - kb) < 64 ? (n - kb) : 64;
        if constexpr (SL) {  // (the sweep of the block before ended with a barrier)
            const int m = n - kb;
            double pv[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) pv[r] = (t + 256 * r < m) ? bs[kb + t + 256 * r] : 0.0;
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 2; ++r)
                if (t + 256 * r < m && so[r] < m) bs[kb + so[r]] = pv[r];  // (a map is a permutation of 0 .. m - 1; the test keeps one that was never written inside bs)
            __syncthreads();
            ld_ord(kb + 64);  // (behind the barrier, which waits for every load in flight: the request travels with the diagonal block's)
        }
        if (!tb::NODIAG && wave == 0) {  // (tb::NODIAG / tb::NOSWEEP: timing builds of exp_switches.hpp, false in the product)
            const int i = kb + lane;
            double bi = (lane < kw) ? bs[i] : 0.0;
            // The columns of the diagonal block come in groups of UNR; the NEXT group is requested before the steps of the current
            // one run (two register sets). Requested after them, every group was a round trip to memory in the middle of a
            // 64-step dependent chain: ~10 us per diagonal block, 16 blocks per solve at n = 512 -- the lifetime of a workgroup, and
            // of every launch that serves few systems (the later Newton iterations of a round).
            auto ldl = [&](const int k0, double (&l)[UNR]) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int k = k0 + u;
                    if (STAGE) l[u] = (k + 1 < kw && lane > k && lane < kw) ? dg[k * 64 + lane] : 0.0;
                    else l[u] = buf_load_f64<tb::NT_SOLVE>(rsrc, (k + 1 < kw && lane > k && lane < kw) ? (unsigned)i * 8u : OOB, __builtin_amdgcn_readfirstlane((kb + (k < kw ? k : kw - 1)) * n * 8));  // (groups past the block's end: every lane out of range anyway; the scalar offset stays inside the matrix)
                }
            };
            auto fwd = [&](const int k0, const double (&l)[UNR]) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int k = k0 + u;
                    if (k + 1 < kw) {
                        const double bk = readlane_f64(bi, k);
                        if (lane > k && lane < kw) bi -= l[u] * bk;
                    }
                }
            };
            double la[UNR], lb[UNR];
            ldl(0, la);
#pragma unroll 1
            for (int k0 = 0; k0 + 1 < kw; k0 += 2 * UNR) {
                ldl(k0 + UNR, lb);  // (past the block's end: every entry is 0.0, no load)
                fwd(k0, la);
                ldl(k0 + 2 * UNR, la);
                fwd(k0 + UNR, lb);
            }
            if (lane < kw) bs[i] = bi;
            if (STAGE) {
                const unsigned long long bad = __ballot(lane < kw && !(fabs(bi) <= 1.7976931348623157e308));
                if (lane == 0) s_kfin = bad == 0ull;
            }
        }
        __syncthreads();
        const unsigned char* zk = (STAGE && zmap) ? zmap + (kb >> 6) * 64 : nullptr;
        const bool kfin = zk != nullptr && s_kfin != 0;
        const int ibeg = kb + 64;
        if (STAGE && ibeg < n) stage_load(ibeg);  // the next diagonal block, in flight behind the sweep
        if (!tb::NOSWEEP && ibeg < n) {  // rows below a full 64-column block
#pragma unroll 1
            for (int i = ibeg + VEC * t; i < n; i += VEC * T) {
                double acc[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = (i + v < n) ? bs[i + v] : 0.0;
                if (kfin && zk[i >> 6] == 0) {  // a zero block of L: nothing to subtract from these rows
                    bool nz = false;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) nz = nz || neg_zero(acc[v]);
                    if (!nz) continue;
                }
#pragma unroll 1
                for (int k = 0; k < 64; k += UNR) {
                    double lv[UNR][VEC];
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const double* p = LU + (long)(kb + k + u) * n + i;
                        if constexpr (VEC == 2) {
                            const double2 q = ld_f64x2<tb::NT_SOLVE>(p);
                            lv[u][0] = q.x;
                            lv[u][1] = q.y;
                        } else {
                            lv[u][0] = ld_f64<tb::NT_SOLVE>(p);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const double bk = bs[kb + k + u];
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[v] -= lv[u][v] * bk;
                    }
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (i + v < n) bs[i + v] = acc[v];
            }
        }
        if (STAGE && ibeg < n) stage_store();  // (the solve that read dg ended before the barrier above)
        __syncthreads();
    }

    // ---- backward: U x = y (dense.rs:197-205): b_k /= u_kk, then b_i -= u_ik b_k for i < k, k descending
    const int nblk = (n + 63) / 64;
#pragma unroll 1
    for (int blk = nblk - 1; blk >= 0; --blk) {
        const int kb = blk * 64;
        const int kw = (n - kb) < 64 ? (n - kb) : 64;
        if (!tb::NODIAG && wave == 0) {
            const int i = kb + lane;
            double bi = (lane < kw) ? bs[i] : 0.0;
            auto ldu = [&](const int k0, double (&uu)[UNR]) {  // (the next group in flight behind the current one's steps, as above)
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int k = k0 - u;
                    if (STAGE) uu[u] = (k >= 0 && lane <= k) ? dg[k * 64 + lane] : 1.0;
                    else uu[u] = buf_load_f64<tb::NT_SOLVE>(rsrc, (k >= 0 && lane <= k) ? (unsigned)i * 8u : OOB, __builtin_amdgcn_readfirstlane((kb + (k >= 0 ? k : 0)) * n * 8));  // (0.0 where 1.0 stood: never used)
                }
            };
            auto bwd = [&](const int k0, const double (&uu)[UNR]) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int k = k0 - u;
                    if (k >= 0) {
                        if (lane == k) bi = bi / uu[u];
                        const double bk = readlane_f64(bi, k);
                        if (lane < k) bi -= uu[u] * bk;
                    }
                }
            };
            double ua[UNR], ub[UNR];
            ldu(kw - 1, ua);
#pragma unroll 1
            for (int k0 = kw - 1; k0 >= 0; k0 -= 2 * UNR) {
                ldu(k0 - UNR, ub);  // (below column 0: every entry is 1.0, no load)
                bwd(k0, ua);
                ldu(k0 - 2 * UNR, ua);
                bwd(k0 - UNR, ub);
            }
            if (lane < kw) bs[i] = bi;
            if (STAGE) {
                const unsigned long long bad = __ballot(lane < kw && !(fabs(bi) <= 1.7976931348623157e308));
                if (lane == 0) s_kfin = bad == 0ull;
            }
        }
        __syncthreads();
        const unsigned char* zk = (STAGE && zmap) ? zmap + (kb >> 6) * 64 : nullptr;
        const bool kfin = zk != nullptr && s_kfin != 0;
        if (STAGE && kb > 0) stage_load(kb - 64);
        if (!tb::NOSWEEP && kb > 0) {
#pragma unroll 1
            for (int i = VEC * t; i < kb; i += VEC * T) {  // kb is a multiple of 64 (hence even): i + v < kb
                double acc[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = bs[i + v];
                if (kfin && zk[i >> 6] == 0) {  // a zero block of U
                    bool nz = false;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) nz = nz || neg_zero(acc[v]);
                    if (!nz) continue;
                }
#pragma unroll 1
                for (int k0 = kw - 1; k0 >= 0; k0 -= UNR) {
                    double uv[UNR][VEC];
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const int k = (k0 - u) >= 0 ? (k0 - u) : 0;
                        const double* p = LU + (long)(kb + k) * n + i;
                        if constexpr (VEC == 2) {
                            const double2 q = ld_f64x2<tb::NT_SOLVE>(p);
                            uv[u][0] = q.x;
                            uv[u][1] = q.y;
                        } else {
                            uv[u][0] = ld_f64<tb::NT_SOLVE>(p);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const int k = k0 - u;
                        if (k >= 0) {
                            const double bk = bs[kb + k];
#pragma unroll
                            for (int v = 0; v < VEC; ++v) acc[v] -= uv[u][v] * bk;
                        }
                    }
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) bs[i + v] = acc[v];
            }
        }
        if (STAGE && kb > 0) stage_store();
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ stand-alone solve
// x <- b (dense.rs:59), permute by pivots, forward/backward substitution. One workgroup per system.
template <int VEC>
__global__ __launch_bounds__(256, 4) void ls_solve_kernel(const double* __restrict__ LU, long mstride, const long long* __restrict__ piv,
                                                       long pstride, const int* __restrict__ perm /* or null */,
                                                       double* __restrict__ X, const double* __restrict__ Bv, int n,
                                                       const int* __restrict__ idx) {
    extern __shared__ __align__(16) double sm[];
    double* bs = sm;
    int* sperm = reinterpret_cast<int*>(sm + n);
    const int b = idx[blockIdx.x];
    const int t = threadIdx.x;
    if (perm) {
        for (int i = t; i < n; i += 256) bs[i] = Bv[(long)b * n + perm[(long)b * n + i]];
    } else {
        // compose the reference's sequential swaps (dense.rs:181-185) into a permutation, one lane, in LDS
        for (int i = t; i < n; i += 256) sperm[i] = i;
        __syncthreads();
        if (t == 0) {
            const long long* pv = piv + (long)b * pstride;
            for (int k = 0; k < n; ++k) {
                const int pk = (int)pv[k];
                if (pk != k) {
                    const int tmp = sperm[k];
                    sperm[k] = sperm[pk];
                    sperm[pk] = tmp;
                }
            }
        }
        __syncthreads();
        for (int i = t; i < n; i += 256) bs[i] = Bv[(long)b * n + sperm[i]];
    }
    __syncthreads();
    wg_getrs<VEC>(LU + (long)b * mstride, n, bs);
    for (int i = t; i < n; i += 256) X[(long)b * n + i] = bs[i];
}

// ------------------------------------------------------------------------------------------------ WRMS
__global__ __launch_bounds__(256) void wrms_kernel(const double* __restrict__ X, const double* __restrict__ W, double* __restrict__ out,
                                                   int n, const int* __restrict__ idx) {
    extern __shared__ __align__(16) double sm[];
    const int b = idx[blockIdx.x];
    for (int i = threadIdx.x; i < n; i += 256) {
        const double p = X[(long)b * n + i] * W[(long)b * n + i];
        sm[i] = p * p;
    }
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = seq_sum_lds(sm, n);
}

// ------------------------------------------------------------------------------------------------ fused Newton body
// delta = -delta; delta = LU^-1 delta; delta *= scale; ee += delta; out = sum_i (delta_i ewt_i)^2 (sequential).
// T = 1024 for n >= 2048: one workgroup per system streams 8 n^2 bytes, and with few large systems in a call (config 4: ~128
// of 134 MB each) 256 threads per system do not keep enough loads in flight to fill the memory system.
// SL: the ctx's factors are staged (wg_getrs): the right-hand side is taken in physical order, no gather through perm; ord = LuWs::ord.
template <int VEC, int T = 256, bool SL = false>
__global__ __launch_bounds__(T, T == 256 ? 4 : 1) void newton_iter_kernel(const double* __restrict__ LU, const int* __restrict__ perm, double* __restrict__ delta,
                                                          double* __restrict__ ee, const double* __restrict__ ewt, int n,
                                                          const int* __restrict__ idx, const double* __restrict__ scale,
                                                          double* __restrict__ out, const int* __restrict__ skip,
                                                          const unsigned char* __restrict__ zmap /* or null: lu_kernels.hpp, LuWs::zmap */,
                                                          const unsigned short* __restrict__ ord = nullptr) {
    extern __shared__ __align__(16) double sm[];
    double* bs = sm;
    double* sq = sm + n;
    if (skip && skip[blockIdx.x] != 0) return;  // (idahip_newton_iter2: this system's Newton solve has ended)
    const int b = idx[blockIdx.x];
    const int t = threadIdx.x;
    const long vb = (long)b * n;
    for (int i = t; i < n; i += T) bs[i] = -delta[vb + (SL ? i : perm[vb + i])];  // neg_mut, then the row permutation (SL: inside the solve)
    __syncthreads();
    wg_getrs<VEC, T, SL>(LU + (long)b * n * n, n, bs, T > 256 ? sq : nullptr, zmap ? zmap + (long)b * 4096 : nullptr,  // sq (>= 4096 doubles for T > 256) is free until the solve is done
                         SL ? ord + (long)b * ((n + 63) >> 6) * n : nullptr);
    const double sc = scale[blockIdx.x];
    for (int i = t; i < n; i += T) {
        const double d = bs[i] * sc;  // ida_ls.rs:406-410 (sc == 1.0 exactly when cjratio == 1)
        delta[vb + i] = d;
        ee[vb + i] = ee[vb + i] + d;  // newton.rs:106
        const double p = d * ewt[vb + i];
        sq[i] = p * p;
    }
    __syncthreads();
    if (t == 0) out[blockIdx.x] = seq_sum_lds(sq, n);
}

// ------------------------------------------------------------------------------------------------ tiny (n <= 8)
__device__ inline void tiny_getrs(const double* __restrict__ a, int n, const long long* __restrict__ pivot, double* b) {
    for (int k = 0; k < n; ++k) {
        const int pk = (int)pivot[k];
        if (pk != k) {
            const double tmp = b[k];
            b[k] = b[pk];
            b[pk] = tmp;
        }
    }
    for (int k = 0; k + 1 < n; ++k) {
        const double bk = b[k];
        for (int i = k + 1; i < n; ++i) b[i] -= a[k * n + i] * bk;
    }
    for (int k = n - 1; k >= 1; --k) {
        b[k] /= a[k * n + k];
        const double bk = b[k];
        for (int i = 0; i < k; ++i) b[i] -= a[k * n + i] * bk;
    }
    b[0] /= a[0];
}

__global__ void tiny_solve_kernel(const double* LU, long mstride, const long long* piv, long pstride, double* X, const double* Bv,
                                  int n, const int* idx, int nsys) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsys) return;
    const int b = idx[s];
    double v[TINY_N];
    for (int i = 0; i < n; ++i) v[i] = Bv[(long)b * n + i];
    tiny_getrs(LU + (long)b * mstride, n, piv + (long)b * pstride, v);
    for (int i = 0; i < n; ++i) X[(long)b * n + i] = v[i];
}

__global__ void tiny_wrms_kernel(const double* X, const double* W, double* out, int n, const int* idx, int nsys) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsys) return;
    const int b = idx[s];
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
        const double p = X[(long)b * n + i] * W[(long)b * n + i];
        acc = acc + p * p;
    }
    out[s] = acc;
}

__global__ void tiny_newton_iter_kernel(const double* LU, const long long* piv, double* delta, double* ee, const double* ewt, int n,
                                        const int* idx, int nsys, const double* scale, double* out, const int* skip) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsys) return;
    if (skip && skip[s] != 0) return;
    const int b = idx[s];
    const long vb = (long)b * n;
    double v[TINY_N];
    for (int i = 0; i < n; ++i) v[i] = -delta[vb + i];
    tiny_getrs(LU + (long)b * n * n, n, piv + vb, v);
    const double sc = scale[s];
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
        const double d = v[i] * sc;
        delta[vb + i] = d;
        ee[vb + i] = ee[vb + i] + d;
        const double p = d * ewt[vb + i];
        acc = acc + p * p;
    }
    out[s] = acc;
}

// ------------------------------------------------------------------------------------------------ solve + norm (IDACalcIC)
// What idaens_calc_ic solves with (ic_kernels.hpp): getrs with the ctx's factors and the WRMS sum, without the Newton body's
// negation, scaling and accumulation into ee.
// x <- LU^-1 x in place (rows gathered by the composed permutation), out = sum_i (x_i ewt_i)^2 left to right. One workgroup of 256
// per system; dynamic LDS: 2 n doubles.
template <int VEC>
__device__ __forceinline__ void ic_solve_body(const double* __restrict__ LU, const int* __restrict__ perm, double* x,
                                              const double* __restrict__ ewt, int n, int b, double* __restrict__ out,
                                              const unsigned short* __restrict__ ord = nullptr /* staged L: LuWs::ord, else null */) {
    extern __shared__ __align__(16) double sm[];
    double* bs = sm;
    double* sq = sm + n;
    const int t = threadIdx.x;
    const long vb = (long)b * n;
    if (ord) {  // (uniform over the launch; this solve is not the hot one: both forms in one kernel)
        for (int i = t; i < n; i += 256) bs[i] = x[vb + i];
        __syncthreads();
        wg_getrs<VEC, 256, true>(LU + (long)b * n * n, n, bs, nullptr, nullptr, ord + (long)b * ((n + 63) >> 6) * n);
    } else {
        for (int i = t; i < n; i += 256) bs[i] = x[vb + perm[vb + i]];
        __syncthreads();
        wg_getrs<VEC>(LU + (long)b * n * n, n, bs);
    }
    for (int i = t; i < n; i += 256) {
        const double d = bs[i];
        x[vb + i] = d;
        const double p = d * ewt[vb + i];
        sq[i] = p * p;
    }
    __syncthreads();
    if (t == 0) out[blockIdx.x] = seq_sum_lds(sq, n);
}

__device__ __forceinline__ double ic_tiny_solve(const double* __restrict__ LU, const long long* __restrict__ piv, double* x,
                                                const double* __restrict__ ewt, int n, int b) {
    const long vb = (long)b * n;
    double v[TINY_N];
    for (int i = 0; i < n; ++i) v[i] = x[vb + i];
    tiny_getrs(LU + (long)b * n * n, n, piv + vb, v);
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
        x[vb + i] = v[i];
        const double p = v[i] * ewt[vb + i];
        acc = acc + p * p;
    }
    return acc;
}


// ------------------------------------------------------------------------------------------------ idaNlsConvTest on the device
// The first two convergence tests of a Newton solve are the controller's conv_test_core<M> (host/ida_controller.hpp) with the
// iteration M = 0 or 1 fixed at compile time, so no pow is compiled in: m = 0 is two comparisons, m = 1 has
// rate = (delnrm / oldnrm)^(1/1) = delnrm / oldnrm exactly. sum[q] is the kernel's sequential sum of (delta_i ewt_i)^2;
// delnrm = sqrt(sum / n) -- a correctly rounded division and square root, as on the host (norm_rms.rs:36-37).
// conv[q]: 0 = keep iterating, 1 = converged at m = 0, 2 = converged at m = 1, 3 = ConvergenceRecover at m = 1 (rate > 0.9).
// ss[q] is the ss of the previous solve / setup; the host replays both tests over delnrm to bring its records up to date.
template <int M>
__global__ void ctest_kernel(const double* __restrict__ sum, int n, const double* __restrict__ toldel, const double* __restrict__ ss,
                             const double* __restrict__ eps_newt, double* __restrict__ delnrm /*[nsys][2]*/, int* __restrict__ conv,
                             int nsys) {
    static_assert(M == 0 || M == 1, "the two tests that need no pow");
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nsys) return;
    if (M == 1 && conv[q] != 0) return;
    const double d = sqrt(sum[q] / (double)n);
    double oldnrm = 0.0;
    if (M == 0) delnrm[2 * q + 1] = 0.0;
    else oldnrm = delnrm[2 * q];
    delnrm[2 * q + M] = d;
    double ssq = ss[q];
    bool converged = false;
    const int ret = idactl::conv_test_core<M>(M, d, toldel[q], eps_newt[q], oldnrm, ssq, &converged);
    conv[q] = ret != idactl::NLS_SUCCESS ? 3 : converged ? M + 1 : 0;
}

}  // namespace idahip
