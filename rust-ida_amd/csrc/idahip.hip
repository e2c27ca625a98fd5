// libidahip.so -- implementation of include/ida_hip.h (single translation unit; gfx950; -ffp-contract=off).
#include <algorithm>
#include <cmath>
#include <map>
#include <thread>

#include "common.hpp"
#include "list_call.hpp"
#include "lu_kernels.hpp"
#include "lu_driver.hpp"
#include "problem_kernels.hpp"
#include "solve_kernels.hpp"
#include "band_kernels.hpp"
#include "dq_kernels.hpp"
#include "mass_action.hpp"
#include "vector_kernels.hpp"
#include "ic_kernels.hpp"
#include "krylov_kernels.hpp"
#include "tiny_ida.hpp"
#include "tiny_net_ida.hpp"
#include "round_ida.hpp"

using namespace idahip;

namespace {

template <class T>
int dalloc(idahip_ctx* c, T** p, size_t count) {
    *p = nullptr;
    if (count == 0) return 0;
    IDAHIP_HIP(c, hipMalloc((void**)p, count * sizeof(T)));
    return 0;
}

// What the host side knows about a problem kind, by idahip_problem value. band_min: the least ml and mu of the kind's device band
// form (0: it has none); banded: the Jacobian's content is banded by construction (the super-panel LU's default).
// IDAHIP_HOST_CALLBACK runs the user's functions instead: its band form takes every width and is asked for by name where it matters.
struct KindFacts {
    int nparam, band_min;
    bool krylov, rounds, banded;
};
const KindFacts KIND_FACTS[] = {
    {0, 0, false, false, false},                               // IDAHIP_ROBERTS
    {3, 0, false, false, false},                               // IDAHIP_LORENZ63
    {0, 0, true, true, false},                                 // IDAHIP_LINEAR_DENSE
    {Heat1D::NPARAM, Heat1D::HALF_BW, true, true, true},       // IDAHIP_HEAT1D
    {0, 0, true, false, false},                                // IDAHIP_HOST_CALLBACK
    {Bruss1D::NPARAM, Bruss1D::HALF_BW, true, true, true},     // IDAHIP_BRUSS1D
    {0, 0, false, true, false},                                // IDAHIP_MASS_ACTION (nparam = R: known when the network is set)
};
constexpr int KIND_COUNT = (int)(sizeof(KIND_FACTS) / sizeof(KIND_FACTS[0]));
const KindFacts& kind_facts(idahip_problem kind) { return KIND_FACTS[(int)kind]; }

// f(P{}) with the stencil description (stencil_problems.hpp) of the ctx's kind; false, and nothing called, for every other kind
template <class F>
bool with_stencil(const idahip_ctx* c, F f) {
    switch (c->kind) {
        case IDAHIP_HEAT1D: f(Heat1D{}); return true;
        case IDAHIP_BRUSS1D: f(Bruss1D{}); return true;
        default: return false;
    }
}

// what a launch site returns where with_stencil found no description: a kind that has no kernel there
int no_kernel(idahip_ctx* c, const char* what) { return fail(c, -2, "no %s kernel for problem kind %d", what, (int)c->kind); }

// IDAHIP_MASS_ACTION before idahip_set_mass_action: every call that would evaluate the problem ends here, nothing launched
int ma_unset(idahip_ctx* c, const char* who) {
    if (c && c->kind == IDAHIP_MASS_ACTION && !c->ma) return fail(c, -2, "%s: the reaction network is not set (idahip_set_mass_action)", who);
    return 0;
}

// does the network carry rate-law factors (idahip_set_rate_network with nfac > 0)? Every launch of a mass_action.hpp kernel picks
// its instantiation by this: a polynomial network runs <false>, the code without factors
bool ma_laws(const idahip_ctx* c) { return c->ma_law != nullptr; }
// the kernel argument of an instantiation: the polynomial network's struct, or the one with the factors
template <bool LAWS>
const MaNetOf<LAWS>& ma_net(const idahip_ctx* c) {
    if constexpr (LAWS) return *c->ma_law;
    else return *c->ma;
}

// the residual of a mass-action ctx (mass_action.hpp): n <= 64 one wavefront per system, above one workgroup per system
template <bool LAWS, class ARGS>
void launch_ma_sys_as(idahip_ctx* c, const ARGS& a, int nsys) {
    const int n = c->n;
    if (n <= MA_WAVE_MAX_N && !c->ma_force_wg) {
        hipLaunchKernelGGL((ma_sys_wave_kernel<LAWS, ARGS>), dim3((nsys + MA_SPW - 1) / MA_SPW), dim3(256), 0, c->stream, a, ma_net<LAWS>(c), (const double*)c->params, nsys);
        return;
    }
    bool solve = false;
    if constexpr (ARGS::IC) solve = a.lu != nullptr;
    const size_t shm = (solve ? 2 : 1) * sizeof(double) * n;
    if (n % 2 == 0) hipLaunchKernelGGL((ma_sys_kernel<LAWS, 2, ARGS>), dim3(nsys), dim3(256), shm, c->stream, a, ma_net<LAWS>(c), (const double*)c->params);
    else hipLaunchKernelGGL((ma_sys_kernel<LAWS, 1, ARGS>), dim3(nsys), dim3(256), shm, c->stream, a, ma_net<LAWS>(c), (const double*)c->params);
}
template <class ARGS>
void launch_ma_sys(idahip_ctx* c, const ARGS& a, int nsys) {
    if (ma_laws(c)) launch_ma_sys_as<true>(c, a, nsys);
    else launch_ma_sys_as<false>(c, a, nsys);
}

// grid.y of the kernels that split one system's work into chunks: the launch reaches 2048 workgroups, or `cap` chunks per system
int launch_chunks(int nsys, int cap) {
    int chunks = 1;
    while ((long)nsys * chunks < 2048 && chunks < cap) chunks *= 2;
    return chunks;
}

// the one-launch Krylov solve of nsys listed systems (ROUND: inside a device lock-step round); false: the ctx's kind has no such kernel
template <bool ROUND>
bool launch_krylov_fused(idahip_ctx* c, const KryArgs& a, int nsys) {
    const dim3 grid(nsys), blk(KRY_T);
    const size_t shm = kry_lds_bytes(c->n, 3);
    const bool prec = c->kry_prec != 0;
    if (with_stencil(c, [&](auto p) {
            constexpr int K = decltype(p)::KIND;
            if (prec) hipLaunchKernelGGL((krylov_fused_kernel<K, true, ROUND>), grid, blk, shm, c->stream, a);
            else hipLaunchKernelGGL((krylov_fused_kernel<K, false, ROUND>), grid, blk, shm, c->stream, a);
        }))
        return true;
    if (c->kind != IDAHIP_LINEAR_DENSE) return false;
    hipLaunchKernelGGL((krylov_fused_kernel<IDAHIP_LINEAR_DENSE, false, ROUND>), grid, blk, shm, c->stream, a);
    return true;
}

double* field_ptr(idahip_ctx* c, idahip_field f) {
    switch (f) {
        case IDAHIP_F_YY: return c->yy;
        case IDAHIP_F_YP: return c->yp;
        case IDAHIP_F_YYPREDICT: return c->yypredict;
        case IDAHIP_F_YPPREDICT: return c->yppredict;
        case IDAHIP_F_EWT: return c->ewt;
        case IDAHIP_F_EE: return c->ee;
        case IDAHIP_F_DELTA: return c->delta;
        case IDAHIP_F_SAVRES: return c->savres;
        default: break;
    }
    if (f >= IDAHIP_F_PHI0 && f <= IDAHIP_F_PHI5) return c->phi + (size_t)(f - IDAHIP_F_PHI0) * c->batch * c->n;
    return nullptr;
}

VecState vec_state(idahip_ctx* c) {
    VecState s;
    s.phi = c->phi;
    s.phistride = (long)c->batch * c->n;
    s.yy = c->yy; s.yp = c->yp; s.yypredict = c->yypredict; s.yppredict = c->yppredict;
    s.ewt = c->ewt; s.ee = c->ee; s.delta = c->delta;
    s.n = c->n;
    s.rtol = c->rtol; s.atol_s = c->atol_s; s.atol_v = c->d_atol_v;
    s.mask = (c->suppress_alg && !c->h_id.empty()) ? c->d_id : nullptr;
    return s;
}

// C IDA's IDA_MISSING_ID: the masked norms (idahip_set_suppress_alg) need the id vector; nothing is launched without it
int missing_id(idahip_ctx* c, const char* who) {
    if (c->suppress_alg && c->h_id.empty()) return fail(c, -2, "%s: suppress_alg is on and no id vector is set (idahip_set_id)", who);
    return 0;
}

// Band LU launches (band_kernels.hpp): one lane per system; systems per wavefront as idahip_tiny_solve chooses them -- the fewest
// (64, 32, ... 1) that keep the wavefront count at or below the device's SIMD count (a chain's steps cost the same for one lane as
// for 64). IDAHIP_BAND_SPW overrides (measurements; the results do not depend on it).
int band_spw(const idahip_ctx* c, int nsys) {
    int spw = 64;
    const int simds = c->simds > 0 ? c->simds : 1024;
    while (spw > 1 && (long)(nsys + spw / 2 - 1) / (spw / 2) <= simds) spw >>= 1;
    if (const char* e = std::getenv("IDAHIP_BAND_SPW")) {
        const int v = (int)std::strtol(e, nullptr, 10);
        if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64) spw = v;
    }
    return spw;
}

// batched band getrf of dAB [.][sstride] in place for the listed systems (d_cnt: the list's length on the device, nsys its bound);
// per-system info into ctx->lu_info
int band_factor(idahip_ctx* c, double* dAB, long sstride, int64_t* dPiv, long pstride, int ml, int mu, const int* d_idx, int nsys,
                const int* d_cnt = nullptr) {
    if (nsys == 0) return 0;
    BandArgs g;
    g.ab = dAB; g.sstride = sstride; g.piv = (long long*)dPiv; g.pstride = pstride; g.n = c->n; g.ml = ml; g.mu = mu;
    g.idx = d_idx; g.nsys = nsys; g.cnt = d_cnt; g.info = c->lu_info;
    const int spw = band_spw(c, nsys);
    const dim3 grid((nsys + spw - 1) / spw), blk(spw);
    if (ml == 1 && mu == 1) hipLaunchKernelGGL((band_getrf_reg_kernel<1, 1>), grid, blk, 0, c->stream, g);
    else hipLaunchKernelGGL(band_getrf_kernel, grid, blk, 0, c->stream, g);
    return post_launch(c, "band_getrf");
}

int create_ctx(idahip_ctx** out, int device, int n, int batch, idahip_problem kind, void* hip_stream, bool band, int ml, int mu, int krylov_maxl = 0) {
    if (!out) return -1;
    *out = nullptr;
    if (n < 1 || batch < 1) return -2;
    if ((int)kind < 0 || (int)kind >= KIND_COUNT) return -2;
    const KindFacts& facts = kind_facts(kind);
    if ((kind == IDAHIP_ROBERTS || kind == IDAHIP_LORENZ63) && n != 3) return -2;
    if (kind == IDAHIP_BRUSS1D && (n % 2 != 0 || n < 10)) {
        std::fprintf(stderr, "IDAHIP_BRUSS1D: n = %d is not 2 m with m >= 5 grid points (two interleaved species)\n", n);
        return -2;
    }
    if (kind == IDAHIP_MASS_ACTION && (n < 2 || n > LU_BIG_MAX_N)) {
        std::fprintf(stderr, "IDAHIP_MASS_ACTION: n = %d outside 2 <= n <= %d\n", n, LU_BIG_MAX_N);
        return -2;
    }
    idahip_ctx* c = new idahip_ctx();
    c->device = device; c->n = n; c->batch = batch; c->kind = kind;
    if (const char* e = std::getenv("IDAHIP_MA_WG")) c->ma_force_wg = std::strtol(e, nullptr, 10) != 0 ? 1 : 0;
    if (band) {
        c->band = 1; c->ml = ml; c->mu = mu; c->ldab = 2 * ml + mu + 1;
    }
    if (krylov_maxl > 0) {
        c->krylov = 1; c->kry_maxl = krylov_maxl;
        c->kry_fused = kind == IDAHIP_HOST_CALLBACK ? 0 : 1;
    }
    const bool nomat = band || krylov_maxl > 0;  // no n x n storage
    c->npad16 = (n + 15) & ~15;
    c->list_seen.assign(((size_t)batch + 63) / 64, 0);
    c->lu_superpanel = facts.banded ? 1 : 0;
    if (const char* sp = std::getenv("IDAHIP_LU_SUPERPANEL")) c->lu_superpanel = std::strtol(sp, nullptr, 10) != 0 ? 1 : 0;
    if (const char* sp = std::getenv("IDAHIP_LU_PERIOD")) {
        const int v = (int)std::strtol(sp, nullptr, 10);
        if (v >= 1 && v <= 64) c->lu_period = v;
    }
    if (const char* sp = std::getenv("IDAHIP_LU_COUNT_ON_HOST")) {  // (A/B runs of one library: -1, 0 or 1 as idahip_set_lu_count_on_host)
        const int v = (int)std::strtol(sp, nullptr, 10);
        if (v >= -1 && v <= 1) c->lu_count_on_host = v;
    }
    int ndev = 0;
    if (device < 0 || hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { delete c; return -100; }
    DevGuard dev_guard__(device);  // allocations, stream and events below belong to `device`; the caller's device is restored
    if (hipSetDevice(device) != hipSuccess) { delete c; return -100; }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->simds = 4 * cus;
    }
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return -100; }
        c->own_stream = true;
    }
    const size_t bn = (size_t)batch * n, bnn = bn * n;
    int rc = 0;
    rc |= dalloc(c, &c->yy, bn); rc |= dalloc(c, &c->yp, bn); rc |= dalloc(c, &c->yypredict, bn); rc |= dalloc(c, &c->yppredict, bn);
    rc |= dalloc(c, &c->ewt, bn); rc |= dalloc(c, &c->ee, bn); rc |= dalloc(c, &c->delta, bn); rc |= dalloc(c, &c->savres, bn);
    rc |= dalloc(c, &c->phi, (size_t)MXORDP1 * bn);
    if (!krylov_maxl) { rc |= dalloc(c, &c->piv, bn); rc |= dalloc(c, &c->perm, bn); }  // a Krylov ctx has no pivots
    rc |= dalloc(c, &c->lu_info, (size_t)batch);  // (also the band calls on caller-owned buffers report through it, on any ctx)
    if (!krylov_maxl) { rc |= dalloc(c, &c->lu_redo, (size_t)LU_REDO_SLOTS + 2 * (size_t)batch); rc |= dalloc(c, &c->lu_nzb, (size_t)batch); }  // (lu_redo: counters, then flag and list entry interleaved: LuWs::redo)
    if (band) rc |= dalloc(c, &c->bab, bn * c->ldab);  // instead of every n x n buffer below
    if (!nomat) rc |= dalloc(c, &c->lu, bnn);
    if (!nomat && n > LU_MAX_N) rc |= dalloc(c, &c->lu_bz, (size_t)batch * 64);
    if (!nomat && n >= LU_ZMAP_MIN_N) rc |= dalloc(c, &c->lu_zmap, (size_t)batch * 4096);
    if (!nomat && n >= LU_ZMAP_MIN_N) rc |= dalloc(c, &c->lu_dirty, (size_t)batch * 4096);
    if (!nomat && n >= LU_ZMAP_MIN_N) rc |= dalloc(c, &c->lu_jwzero, (size_t)batch);
    if (!nomat && n > TINY_N) {
        rc |= dalloc(c, &c->jw, bnn);
        rc |= dalloc(c, &c->lu_pos, bn); rc |= dalloc(c, &c->lu_live, bn); rc |= dalloc(c, &c->lu_prow, bn);
        rc |= dalloc(c, &c->lu_l11, (size_t)batch * L11_STRIDE);
        if (n <= WP_MAX_ROWS) rc |= dalloc(c, &c->lu_ord, (size_t)batch * ((n + 63) / 64) * n);  // staged L: LuWs::ord
    }
    if (krylov_maxl > 0) {
        idakry::Sys* st = nullptr;
        rc |= dalloc(c, &c->kry_V, bn * (size_t)(krylov_maxl + 1));
        rc |= dalloc(c, &st, (size_t)batch);
        c->kry_st = st;
        rc |= dalloc(c, &c->kry_stage, 3 * bn);
        rc |= dalloc(c, &c->kry_b, bn); rc |= dalloc(c, &c->kry_x, bn);
    }
    if (kind == IDAHIP_LINEAR_DENSE) {
        rc |= dalloc(c, &c->A, bnn); rc |= dalloc(c, &c->B, bnn); rc |= dalloc(c, &c->C, bn);
    }
    c->nparam = facts.nparam;
    rc |= dalloc(c, &c->params, (size_t)batch * facts.nparam);
    if (kind == IDAHIP_HOST_CALLBACK) rc |= dalloc(c, &c->cb_stage, 3 * bn);
    c->slot_cap = (size_t)batch * 256 + 4096;  // per call: <= ~110 B of scalars per system (predict) + list ids + results
    for (int i = 0; i < NSLOT && !rc; ++i) {
        if (hipHostMalloc((void**)&c->slots[i].h, c->slot_cap) != hipSuccess) rc = -100;
        else if (hipMalloc((void**)&c->slots[i].d, c->slot_cap) != hipSuccess) rc = -100;
        else if (hipEventCreateWithFlags(&c->slots[i].done, hipEventDisableTiming) != hipSuccess) rc = -100;
    }
    if (!rc && (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess || hipEventCreate(&c->ev2) != hipSuccess ||
                hipEventCreate(&c->ev3) != hipSuccess || hipEventCreateWithFlags(&c->ev_cnt, hipEventDisableTiming) != hipSuccess))
        rc = -100;

    if (rc) {
        idahip_destroy(c);
        return -100;
    }
    // deterministic initial contents
    (void)hipMemsetAsync(c->ee, 0, bn * sizeof(double), c->stream);
    (void)hipMemsetAsync(c->delta, 0, bn * sizeof(double), c->stream);
    (void)hipMemsetAsync(c->phi, 0, (size_t)MXORDP1 * bn * sizeof(double), c->stream);
    (void)hipMemsetAsync(c->lu_info, 0, (size_t)batch * sizeof(int), c->stream);
    // pivots and row permutation in range before the first setup: a Newton iteration or solve ahead of it gathers rows by them
    if (c->piv) (void)hipMemsetAsync(c->piv, 0, bn * sizeof(int64_t), c->stream);
    if (c->perm) (void)hipMemsetAsync(c->perm, 0, bn * sizeof(int32_t), c->stream);
    if (c->lu_ord) (void)hipMemsetAsync(c->lu_ord, 0, (size_t)batch * ((n + 63) / 64) * n * sizeof(uint16_t), c->stream);  // (and the staged solve's maps)
    if (c->lu_redo) (void)hipMemsetAsync(c->lu_redo, 0, ((size_t)LU_REDO_SLOTS + 2 * (size_t)batch) * sizeof(int), c->stream);
    if (c->bab) (void)hipMemsetAsync(c->bab, 0, bn * c->ldab * sizeof(double), c->stream);
    if (c->lu_dirty) {  // the factors start as zeros, and so does the map of their blocks that have ever held anything else
        (void)hipMemsetAsync(c->lu, 0, bnn * sizeof(double), c->stream);
        (void)hipMemsetAsync(c->lu_dirty, 0, (size_t)batch * 4096, c->stream);
        (void)hipMemsetAsync(c->lu_jwzero, 0, (size_t)batch * sizeof(int), c->stream);
    }
    (void)hipStreamSynchronize(c->stream);
    *out = c;
    return 0;
}

}  // namespace

extern "C" {

int idahip_create(idahip_ctx** out, int device, int n, int batch, idahip_problem kind, void* hip_stream) {
    return create_ctx(out, device, n, batch, kind, hip_stream, false, 0, 0);
}

int idahip_create_band(idahip_ctx** out, int device, int n, int batch, idahip_problem kind, void* hip_stream, int ml, int mu) {
    if (!out) return -1;
    *out = nullptr;
    const int band_min = ((int)kind >= 0 && (int)kind < KIND_COUNT) ? kind_facts(kind).band_min : 0;
    if (!band_min && kind != IDAHIP_HOST_CALLBACK) {
        std::fprintf(stderr, "idahip_create_band: problem kind %d has no band form (IDAHIP_HEAT1D, IDAHIP_BRUSS1D or IDAHIP_HOST_CALLBACK)\n", (int)kind);
        return -2;
    }
    if (n <= TINY_N || n > LU_BIG_MAX_N) {
        std::fprintf(stderr, "idahip_create_band: n = %d outside %d < n <= %d\n", n, TINY_N, LU_BIG_MAX_N);
        return -2;
    }
    if (ml < 0 || mu < 0 || ml >= n || mu >= n || ml < band_min || mu < band_min) {
        std::fprintf(stderr, "idahip_create_band: bandwidths ml = %d, mu = %d outside 0 <= ml, mu < n (>= 1 for IDAHIP_HEAT1D, >= 2 for IDAHIP_BRUSS1D)\n", ml, mu);
        return -2;
    }
    return create_ctx(out, device, n, batch, kind, hip_stream, true, ml, mu);
}

int idahip_band(const idahip_ctx* c, int* ml, int* mu) {
    if (!c) return -1;
    if (c->band) {
        if (ml) *ml = c->ml;
        if (mu) *mu = c->mu;
    }
    return c->band;
}

int idahip_destroy(idahip_ctx* c) {
    DevGuard dev_guard__(c);
    if (!c) return 0;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    void* ptrs[] = {c->kry_rcnt, c->kry_rint, c->kry_rres, c->kry_pab, c->kry_ppiv, c->kry_V, c->kry_st, c->kry_stage, c->kry_b, c->kry_x, c->dq_stage, c->dq_out, c->dq_hh, c->yy, c->yp, c->yypredict, c->yppredict, c->ewt, c->ee, c->delta, c->savres, c->phi, c->lu, c->jw, c->piv, c->perm,
                    c->lu_pos, c->lu_live, c->lu_prow, c->lu_info, c->lu_redo, c->lu_nzb, c->lu_bz, c->lu_zmap, c->lu_dirty, c->lu_jwzero, c->lu_l11, c->lu_ord, c->params, c->A, c->B, c->C, c->d_atol_v, c->d_id, c->d_constr, c->ic_y,
                    c->ic_yp, c->reinit_stage, c->bab, c->dky, c->cb_stage, c->tiny_sys, c->tiny_touts, c->tiny_yout, c->tiny_ypout, c->tiny_start, c->tiny_rounds,
                    c->tiny_acc, c->tiny_roots, c->rnd_i, c->rnd_d, c->ma_blob};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete c->ma;
    delete c->ma_law;
    if (c->rnd_host) (void)hipHostFree(c->rnd_host);
    if (c->rnd_mail) (void)hipHostFree(c->rnd_mail);
    if (c->cb_jpin) (void)hipHostFree(c->cb_jpin);
    if (c->cb_jdev) (void)hipFree(c->cb_jdev);
    for (int i = 0; i < NSLOT; ++i) {
        if (c->slots[i].h) (void)hipHostFree(c->slots[i].h);
        if (c->slots[i].d) (void)hipFree(c->slots[i].d);
        if (c->slots[i].done) (void)hipEventDestroy(c->slots[i].done);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev2) (void)hipEventDestroy(c->ev2);
    if (c->ev3) (void)hipEventDestroy(c->ev3);
    if (c->ev_cnt) (void)hipEventDestroy(c->ev_cnt);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

const char* idahip_last_error(const idahip_ctx* c) { return c ? c->err.c_str() : "null ctx"; }
int idahip_n(const idahip_ctx* c) { return c ? c->n : -1; }
int idahip_batch(const idahip_ctx* c) { return c ? c->batch : -1; }

int idahip_sync(idahip_ctx* c) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------ streams that really run side by side
// A HIP stream is not a hardware queue: the runtime multiplexes its streams onto a few of them (four by default) and which
// stream lands on which is its business -- the kernel trace of two builds of the same program showed three of four streams on
// ONE queue, their launches strictly one after the other (tools/group_trace.sh). Ensembles that are meant
// to fill each other's idle stretches (idaens_stream_group) need streams the device runs CONCURRENTLY, so this entry point
// finds them by experiment: it creates candidate streams and lets a probe kernel (one wavefront that waits 300 us on the
// constant 100 MHz clock and notes when it started and ended) run on the candidate and on every stream chosen so far at once;
// the candidate is kept if its interval overlaps all of theirs. Rejected candidates stay alive until the end (a destroyed
// stream gives its queue back and the next one would take the same) and are destroyed then.
__global__ void stream_probe_kernel(unsigned long long* out, long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while ((long long)(wall_clock64() - t0) < ticks) __builtin_amdgcn_s_sleep(16);  // (ends by itself: the clock runs on)
    if (threadIdx.x == 0) {
        out[0] = t0;
        out[1] = wall_clock64();
    }
}

int idahip_concurrent_streams(int device, int count, void** streams_out, int* nconcurrent) {
    if (!streams_out || count < 1 || count > 64) return -2;
    int ndev = 0;
    if (device < 0 || hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return -100;
    DevGuard dev_guard__(device);
    if (hipSetDevice(device) != hipSuccess) return -100;
    unsigned long long* stamps = nullptr;
    if (hipHostMalloc((void**)&stamps, sizeof(unsigned long long) * 2 * (size_t)(count + 1)) != hipSuccess) return -100;
    std::vector<hipStream_t> sel, rejected;
    int rc = 0;
    const long long ticks = 30000;  // 300 us at 100 MHz
    for (int attempt = 0; attempt < 6 * count + 8 && (int)sel.size() < count && !rc; ++attempt) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { rc = -100; break; }
        if (sel.empty()) {
            sel.push_back(s);
            continue;
        }
        const int k = (int)sel.size();
        for (int i = 0; i <= k; ++i) stamps[2 * i] = stamps[2 * i + 1] = 0ull;
        for (int i = 0; i < k; ++i) hipLaunchKernelGGL(stream_probe_kernel, dim3(1), dim3(64), 0, sel[i], stamps + 2 * i, ticks);
        hipLaunchKernelGGL(stream_probe_kernel, dim3(1), dim3(64), 0, s, stamps + 2 * k, ticks);
        bool ok = hipGetLastError() == hipSuccess;
        for (int i = 0; i < k; ++i) ok = (hipStreamSynchronize(sel[i]) == hipSuccess) && ok;
        ok = (hipStreamSynchronize(s) == hipSuccess) && ok;
        if (!ok) { rc = -100; (void)hipStreamDestroy(s); break; }
        bool overlaps_all = stamps[2 * k + 1] > stamps[2 * k];
        for (int i = 0; i < k; ++i)
            overlaps_all = overlaps_all && stamps[2 * k] < stamps[2 * i + 1] && stamps[2 * i] < stamps[2 * k + 1];
        (overlaps_all ? sel : rejected).push_back(s);
    }
    const int found = (int)sel.size();
    // fewer hardware queues than asked for: the remaining streams are ordinary ones (they share a queue with somebody)
    while (!rc && (int)sel.size() < count) {
        if (!rejected.empty()) {
            sel.push_back(rejected.back());
            rejected.pop_back();
        } else {
            hipStream_t s = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) rc = -100;
            else sel.push_back(s);
        }
    }
    for (hipStream_t s : rejected) (void)hipStreamDestroy(s);
    (void)hipHostFree(stamps);
    if (rc) {
        for (hipStream_t s : sel) (void)hipStreamDestroy(s);
        return rc;
    }
    for (int i = 0; i < count; ++i) streams_out[i] = (void*)sel[i];
    if (nconcurrent) *nconcurrent = found;
    return 0;
}

// Diagnostic (tools/half_streams.py): how evenly the device shares itself between two streams whose kernels each want all of it.
// A grid of 2048 workgroups that hold 64 KB of LDS each (two fit a CU: 512 resident) and wait 20 us is launched on A and, right
// behind it, on B; every workgroup notes its start and end. *frac = the part of the two kernels' joint span in which both had
// workgroups running: ~1 when the dispatcher interleaves the two grids, ~0.5 when B's workgroups only start once A's are all out.
__global__ void stream_share_kernel(unsigned long long* out, long long ticks) {
    extern __shared__ unsigned char pad_lds[];
    const unsigned long long t0 = wall_clock64();
    if (threadIdx.x == 0) pad_lds[0] = 1;  // (keeps the allocation)
    while ((long long)(wall_clock64() - t0) < ticks) __builtin_amdgcn_s_sleep(16);
    if (threadIdx.x == 0) {
        atomicMin(out, t0);
        atomicMax(out + 1, wall_clock64());
    }
}

int idahip_stream_pair_share(int device, void* streamA, void* streamB, double* frac) {
    if (!streamA || !streamB || !frac) return -2;
    DevGuard dev_guard__(device);
    unsigned long long* st = nullptr;
    if (hipHostMalloc((void**)&st, 4 * sizeof(unsigned long long)) != hipSuccess) return -100;
    st[0] = st[2] = ~0ull;
    st[1] = st[3] = 0ull;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)stream_share_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        attr_set = true;
    }
    hipLaunchKernelGGL(stream_share_kernel, dim3(2048), dim3(64), 65536, (hipStream_t)streamA, st, 2000ll);
    hipLaunchKernelGGL(stream_share_kernel, dim3(2048), dim3(64), 65536, (hipStream_t)streamB, st + 2, 2000ll);
    int rc = hipGetLastError() == hipSuccess ? 0 : -100;
    if (hipStreamSynchronize((hipStream_t)streamA) != hipSuccess) rc = -100;
    if (hipStreamSynchronize((hipStream_t)streamB) != hipSuccess) rc = -100;
    if (!rc) {
        const double lo = (double)(st[0] < st[2] ? st[0] : st[2]), hi = (double)(st[1] > st[3] ? st[1] : st[3]);
        const double olo = (double)(st[0] > st[2] ? st[0] : st[2]), ohi = (double)(st[1] < st[3] ? st[1] : st[3]);
        *frac = hi > lo ? (ohi > olo ? (ohi - olo) / (hi - lo) : 0.0) : 0.0;
    }
    (void)hipHostFree(st);
    return rc;
}

int idahip_release_streams(int device, int count, void** streams) {
    if (!streams || count < 0) return -2;
    DevGuard dev_guard__(device);
    int rc = 0;
    for (int i = 0; i < count; ++i)
        if (streams[i] && hipStreamDestroy((hipStream_t)streams[i]) != hipSuccess) rc = -100;
    return rc;
}

int idahip_set_tolerances(idahip_ctx* c, double rtol, const double* hAtol, int natol) {
    DevGuard dev_guard__(c);
    if (!c || !hAtol) return -1;
    if (natol != 1 && natol != c->n) return fail(c, -2, "natol must be 1 or n");
    c->rtol = rtol;
    if (natol == 1 && c->n != 1) {
        c->atol_s = hAtol[0];
        if (c->d_atol_v) { (void)hipFree(c->d_atol_v); c->d_atol_v = nullptr; }
    } else {
        c->atol_s = hAtol[0];
        if (!c->d_atol_v) { int rc = dalloc(c, &c->d_atol_v, (size_t)c->n); if (rc) return rc; }
        IDAHIP_HIP(c, hipMemcpy(c->d_atol_v, hAtol, sizeof(double) * c->n, hipMemcpyHostToDevice));
    }
    return 0;
}

int idahip_set_id(idahip_ctx* c, const double* hId) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    if (!hId) {
        c->h_id.clear();
        return 0;
    }
    for (int i = 0; i < c->n; ++i)
        if (!(hId[i] == 0.0 || hId[i] == 1.0)) return fail(c, -2, "id[%d] = %g: 1.0 (differential) or 0.0 (algebraic)", i, hId[i]);
    if (!c->d_id) { int rc = dalloc(c, &c->d_id, (size_t)c->n); if (rc) return rc; }
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    IDAHIP_HIP(c, hipMemcpy(c->d_id, hId, sizeof(double) * c->n, hipMemcpyHostToDevice));
    c->h_id.assign(hId, hId + c->n);
    return 0;
}

int idahip_id(const idahip_ctx* c, double* hId) {
    if (!c) return -1;
    if (c->h_id.empty()) return 0;
    if (hId) std::memcpy(hId, c->h_id.data(), sizeof(double) * c->n);
    return 1;
}

int idahip_set_suppress_alg(idahip_ctx* c, int on) {
    if (!c) return -1;
    c->suppress_alg = on != 0;
    return 0;
}

int idahip_suppress_alg(const idahip_ctx* c) { return c ? (c->suppress_alg ? 1 : 0) : -1; }

int idahip_set_constraints(idahip_ctx* c, const double* hC) {
    if (int rc = refuse_krylov(c, "idahip_set_constraints")) return rc;
    DevGuard dev_guard__(c);
    if (!c) return -1;
    if (!hC) {
        c->h_constr.clear();
        return 0;
    }
    for (int i = 0; i < c->n; ++i)
        if (!idactl::constr_value_ok(hC[i])) return fail(c, -2, "constraint[%d] = %g: 0 (none), 1 (>= 0), -1 (<= 0), 2 (> 0) or -2 (< 0)", i, hC[i]);
    if (!c->d_constr) { int rc = dalloc(c, &c->d_constr, (size_t)c->n); if (rc) return rc; }
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    IDAHIP_HIP(c, hipMemcpy(c->d_constr, hC, sizeof(double) * c->n, hipMemcpyHostToDevice));
    c->h_constr.assign(hC, hC + c->n);
    return 0;
}

int idahip_constraints(const idahip_ctx* c, double* hC) {
    if (!c) return -1;
    if (c->h_constr.empty()) return 0;
    if (hC) std::memcpy(hC, c->h_constr.data(), sizeof(double) * c->n);
    return 1;
}

int idahip_set_problem_params(idahip_ctx* c, int first, int count, const double* hParams, int nparam) {
    DevGuard dev_guard__(c);
    if (!c || !hParams) return -1;
    if (int rc = ma_unset(c, "idahip_set_problem_params")) return rc;
    if (!c->params || nparam != c->nparam) return fail(c, -2, "problem kind takes %d parameters per system", c->nparam);
    if (first < 0 || count < 0 || first + count > c->batch) return fail(c, -2, "system range out of bounds");
    IDAHIP_HIP(c, hipMemcpy(c->params + (size_t)first * nparam, hParams, sizeof(double) * count * nparam, hipMemcpyHostToDevice));
    return 0;
}

int idahip_set_linear_dense(idahip_ctx* c, int first, int count, const double* hA, const double* hB, const double* hC) {
    DevGuard dev_guard__(c);
    if (!c || !hA || !hB || !hC) return -1;
    if (c->kind != IDAHIP_LINEAR_DENSE) return fail(c, -2, "not a LINEAR_DENSE ctx");
    if (c->band) return fail(c, -2, "idahip_set_linear_dense on a band ctx");
    if (first < 0 || count < 0 || first + count > c->batch) return fail(c, -2, "system range out of bounds");
    const size_t nn = (size_t)c->n * c->n;
    IDAHIP_HIP(c, hipMemcpy(c->A + first * nn, hA, sizeof(double) * count * nn, hipMemcpyHostToDevice));
    IDAHIP_HIP(c, hipMemcpy(c->B + first * nn, hB, sizeof(double) * count * nn, hipMemcpyHostToDevice));
    IDAHIP_HIP(c, hipMemcpy(c->C + (size_t)first * c->n, hC, sizeof(double) * count * c->n, hipMemcpyHostToDevice));
    return 0;
}

// IDAHIP_MASS_ACTION: validate the network, build the residual's row-CSR and the Jacobian pattern's CSR (mass_action.hpp) on the host,
// upload both in one allocation, and allocate the parameters [batch][nreac + nconst]. Both setters end here (who: the one called);
// without factors the tables are the polynomial network's, and nothing of the rate laws is uploaded.
static int set_network(idahip_ctx* c, const char* who, int nreac, const int32_t* reactants, int nfac, const int32_t* factors, int nconst,
                       int nentries, const int32_t* rows, const int32_t* reacs, const double* nu, const double* d) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    if (c->kind != IDAHIP_MASS_ACTION) return fail(c, -2, "%s: not an IDAHIP_MASS_ACTION ctx (kind %d)", who, (int)c->kind);
    if (c->ma) return fail(c, -2, "%s: the reaction network is already set (once per ctx)", who);
    if (nreac < 1) return fail(c, -2, "%s: nreac = %d, at least one reaction", who, nreac);
    if (nentries < 0) return fail(c, -2, "%s: nentries = %d is negative", who, nentries);
    if (nfac < 0) return fail(c, -2, "%s: nfac = %d is negative", who, nfac);
    if (nconst < 0) return fail(c, -2, "%s: nconst = %d is negative", who, nconst);
    if (!reactants || !d || (nentries > 0 && (!rows || !reacs || !nu)) || (nfac > 0 && !factors)) return null_argument(c);
    const int n = c->n;
    for (int r = 0; r < nreac; ++r) {
        bool ended = false;
        for (int p = 0; p < 3; ++p) {
            const int sp = reactants[3 * r + p];
            if (sp < -1 || sp >= n) return fail(c, -2, "%s: reaction %d, slot %d: species %d outside [0, %d)", who, r, p, sp, n);
            if (sp == -1) ended = true;
            else if (ended) return fail(c, -2, "%s: reaction %d, slot %d: a species after an unused slot (-1 only in trailing slots)", who, r, p);
        }
    }
    // the factors, reaction by reaction: a stable counting sort keeps the caller's order within a reaction
    std::vector<int> fac_ptr(nreac + 1, 0);
    for (int f = 0; f < nfac; ++f) {
        const int32_t* q = factors + 5 * f;
        if (q[0] < 0 || q[0] >= nreac) return fail(c, -2, "%s: factor %d: reaction %d outside [0, %d)", who, f, q[0], nreac);
        if (q[1] != IDAHIP_RATE_SAT && q[1] != IDAHIP_RATE_INH)
            return fail(c, -2, "%s: factor %d: op %d is neither IDAHIP_RATE_SAT (1) nor IDAHIP_RATE_INH (2)", who, f, q[1]);
        if (q[2] < 0 || q[2] >= n) return fail(c, -2, "%s: factor %d: species %d outside [0, %d)", who, f, q[2], n);
        if (q[3] < 0 || q[3] >= nconst) return fail(c, -2, "%s: factor %d: constant %d outside [0, %d)", who, f, q[3], nconst);
        if (q[4] < 1 || q[4] > 4) return fail(c, -2, "%s: factor %d: exponent %d outside [1, 4]", who, f, q[4]);
        if (++fac_ptr[q[0] + 1] > IDAHIP_RATE_MAX_FACTORS)
            return fail(c, -2, "%s: factor %d: reaction %d has more than %d factors", who, f, q[0], IDAHIP_RATE_MAX_FACTORS);
    }
    for (int r = 0; r < nreac; ++r) fac_ptr[r + 1] += fac_ptr[r];
    std::vector<MaFac> facs((size_t)nfac);
    {
        std::vector<int> fill(fac_ptr.begin(), fac_ptr.end() - 1);
        for (int f = 0; f < nfac; ++f) {
            const int32_t* q = factors + 5 * f;
            facs[(size_t)fill[q[0]]++] = MaFac{q[1], q[2], q[3], q[4]};
        }
    }
    for (int e = 0; e < nentries; ++e) {
        if (rows[e] < 0 || rows[e] >= n) return fail(c, -2, "%s: entry %d: row %d outside [0, %d)", who, e, rows[e], n);
        if (reacs[e] < 0 || reacs[e] >= nreac) return fail(c, -2, "%s: entry %d: reaction %d outside [0, %d)", who, e, reacs[e], nreac);
        if (!std::isfinite(nu[e])) return fail(c, -2, "%s: entry %d: nu = %g is not finite", who, e, nu[e]);
    }
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(d[i])) return fail(c, -2, "%s: d[%d] = %g is not finite", who, i, d[i]);
    // the residual's rows: a stable counting sort of the entries by row keeps the caller's order within a row
    std::vector<int> row_ptr(n + 1, 0);
    for (int e = 0; e < nentries; ++e) row_ptr[rows[e] + 1] += 1;
    for (int i = 0; i < n; ++i) row_ptr[i + 1] += row_ptr[i];
    std::vector<MaTerm> rterms((size_t)nentries);
    {
        std::vector<int> fill(row_ptr.begin(), row_ptr.end() - 1);
        for (int e = 0; e < nentries; ++e) {
            const int32_t* s = reactants + 3 * reacs[e];
            rterms[(size_t)fill[rows[e]]++] = MaTerm{nu[e], reacs[e], s[0], s[1], s[2]};
        }
    }
    // the Jacobian's pattern, column-major: every diagonal position, and (i, j) for every slot of an entry of row i that holds j;
    // a position's terms in the header's order (the row's entries in order, within an entry the slots in order, then the reaction's
    // factors in order: those terms keep all three slots and name the factor they differentiate)
    struct JTerm { MaTerm t; int dfac; };
    std::map<long, std::vector<JTerm>> pat;
    for (int i = 0; i < n; ++i) {
        pat[(long)i * n + i];
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const MaTerm& t = rterms[(size_t)e];
            const int s[3] = {t.a, t.b, t.c};
            for (int p = 0; p < 3 && s[p] >= 0; ++p) {
                int o[2] = {-1, -1}, k = 0;
                for (int q = 0; q < 3; ++q)
                    if (q != p && s[q] >= 0) o[k++] = s[q];
                pat[(long)s[p] * n + i].push_back(JTerm{MaTerm{t.nu, t.r, o[0], o[1], -1}, -1});
            }
            for (int f = fac_ptr[t.r]; f < fac_ptr[t.r + 1]; ++f)
                pat[(long)facs[(size_t)f].s * n + i].push_back(JTerm{t, f - fac_ptr[t.r]});
        }
    }
    const int nnz = (int)pat.size();
    std::vector<int> col_ptr(n + 1, 0), pos_row, pos_ptr;
    std::vector<MaTerm> jterms;
    std::vector<int> jdfac;
    pos_row.reserve(nnz);
    pos_ptr.reserve(nnz + 1);
    int ml = 0, mu = 0;
    for (const auto& kv : pat) {
        const int j = (int)(kv.first / n), i = (int)(kv.first % n);
        col_ptr[j + 1] += 1;
        pos_row.push_back(i);
        pos_ptr.push_back((int)jterms.size());
        for (const JTerm& jt : kv.second) {
            jterms.push_back(jt.t);
            jdfac.push_back(jt.dfac);
        }
        ml = std::max(ml, i - j);
        mu = std::max(mu, j - i);
    }
    pos_ptr.push_back((int)jterms.size());
    for (int j = 0; j < n; ++j) col_ptr[j + 1] += col_ptr[j];
    // one allocation: the int tables, then (8-byte aligned) d and the two term tables
    const size_t ints = 2 * (size_t)(n + 1) + (size_t)nnz + (size_t)(nnz + 1);
    const size_t off_d = (ints * sizeof(int) + 7) & ~(size_t)7;
    const size_t off_rt = off_d + sizeof(double) * n;
    const size_t off_jt = off_rt + sizeof(MaTerm) * rterms.size();
    // (rate laws only, after the polynomial network's tables: the factors, 16 bytes each, then fac_ptr and jdfac)
    const size_t off_fc = off_jt + sizeof(MaTerm) * jterms.size();
    const size_t off_fp = off_fc + (nfac > 0 ? sizeof(MaFac) * facs.size() : 0);
    const size_t off_jd = off_fp + (nfac > 0 ? sizeof(int) * fac_ptr.size() : 0);
    const size_t total = off_jd + (nfac > 0 ? sizeof(int) * jdfac.size() : 0);
    const int nparam = nreac + nconst;
    std::vector<char> blob(total, 0);
    int* hi = reinterpret_cast<int*>(blob.data());
    std::memcpy(hi, row_ptr.data(), sizeof(int) * (n + 1));
    std::memcpy(hi + (n + 1), col_ptr.data(), sizeof(int) * (n + 1));
    std::memcpy(hi + 2 * (n + 1), pos_row.data(), sizeof(int) * nnz);
    std::memcpy(hi + 2 * (n + 1) + nnz, pos_ptr.data(), sizeof(int) * (nnz + 1));
    std::memcpy(blob.data() + off_d, d, sizeof(double) * n);
    if (!rterms.empty()) std::memcpy(blob.data() + off_rt, rterms.data(), sizeof(MaTerm) * rterms.size());
    if (!jterms.empty()) std::memcpy(blob.data() + off_jt, jterms.data(), sizeof(MaTerm) * jterms.size());
    if (nfac > 0) {
        std::memcpy(blob.data() + off_fc, facs.data(), sizeof(MaFac) * facs.size());
        std::memcpy(blob.data() + off_fp, fac_ptr.data(), sizeof(int) * fac_ptr.size());
        if (!jdfac.empty()) std::memcpy(blob.data() + off_jd, jdfac.data(), sizeof(int) * jdfac.size());
    }
    char* dev = nullptr;
    double* params = nullptr;
    if (hipMalloc((void**)&dev, total) != hipSuccess) return fail(c, -100, "%s: %zu bytes of network tables", who, total);
    if (hipMalloc((void**)&params, sizeof(double) * (size_t)c->batch * nparam) != hipSuccess) {
        (void)hipFree(dev);
        return fail(c, -100, "%s: parameters of %d systems x %d", who, c->batch, nparam);
    }
    hipError_t e = hipMemcpy(dev, blob.data(), total, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(params, 0, sizeof(double) * (size_t)c->batch * nparam);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        (void)hipFree(params);
        return fail(c, -100, "%s: upload failed: %s", who, hipGetErrorString(e));
    }
    MaNet* m = new MaNet();
    const int* di = reinterpret_cast<const int*>(dev);
    m->row_ptr = di; m->col_ptr = di + (n + 1); m->pos_row = di + 2 * (n + 1); m->pos_ptr = di + 2 * (n + 1) + nnz;
    m->d = reinterpret_cast<const double*>(dev + off_d);
    m->rterms = reinterpret_cast<const MaTerm*>(dev + off_rt);
    m->jterms = reinterpret_cast<const MaTerm*>(dev + off_jt);
    m->nparam = nparam;
    if (nfac > 0) {
        MaLawNet* l = new MaLawNet();
        static_cast<MaNet&>(*l) = *m;
        l->nreac = nreac;
        l->facs = reinterpret_cast<const MaFac*>(dev + off_fc);
        l->fac_ptr = reinterpret_cast<const int*>(dev + off_fp);
        l->jdfac = reinterpret_cast<const int*>(dev + off_jd);
        c->ma_law = l;
    }
    c->ma_blob = dev; c->ma = m; c->ma_nnz = nnz; c->ma_ml = ml; c->ma_mu = mu;
    c->params = params; c->nparam = nparam;
    return 0;
}

int idahip_set_mass_action(idahip_ctx* c, int nreac, const int32_t* reactants, int nentries, const int32_t* rows, const int32_t* reacs,
                           const double* nu, const double* d) {
    return set_network(c, "idahip_set_mass_action", nreac, reactants, 0, nullptr, 0, nentries, rows, reacs, nu, d);
}

int idahip_set_rate_network(idahip_ctx* c, int nreac, const int32_t* reactants, int nfac, const int32_t* factors, int nconst, int nentries,
                            const int32_t* rows, const int32_t* reacs, const double* nu, const double* d) {
    return set_network(c, "idahip_set_rate_network", nreac, reactants, nfac, factors, nconst, nentries, rows, reacs, nu, d);
}

int idahip_mass_action_pattern(idahip_ctx* c, int* nnz, int* ml, int* mu) {
    if (!c) return -1;
    if (c->kind != IDAHIP_MASS_ACTION) return fail(c, -2, "idahip_mass_action_pattern: not an IDAHIP_MASS_ACTION ctx (kind %d)", (int)c->kind);
    if (int rc = ma_unset(c, "idahip_mass_action_pattern")) return rc;
    if (nnz) *nnz = c->ma_nnz;
    if (ml) *ml = c->ma_ml;
    if (mu) *mu = c->ma_mu;
    return 0;
}

int idahip_set_mass_action_tiny(idahip_ctx* c, int on) {
    if (!c) return -1;
    if (c->kind != IDAHIP_MASS_ACTION) return fail(c, -2, "idahip_set_mass_action_tiny: not an IDAHIP_MASS_ACTION ctx (kind %d)", (int)c->kind);
    if (c->n > TINY_N) return fail(c, -2, "idahip_set_mass_action_tiny: n = %d, the one-thread stepper takes n <= %d", c->n, TINY_N);
    if (c->band || c->krylov) return fail(c, -2, "idahip_set_mass_action_tiny: not on a band or Krylov ctx");
    c->ma_tiny = on ? 1 : 0;
    return 0;
}

int idahip_mass_action_tiny(const idahip_ctx* c) { return c ? c->ma_tiny : -1; }

int idahip_set_host_problem(idahip_ctx* c, idahip_res_fn res, idahip_jac_fn jac, void* user) {
    if (int rc = refuse_krylov(c, "idahip_set_host_problem")) return rc;
    if (!c || !res || !jac) return -1;
    if (c->kind != IDAHIP_HOST_CALLBACK) return fail(c, -2, "not an IDAHIP_HOST_CALLBACK ctx");
    if (c->band) return fail(c, -2, "a band ctx takes a band Jacobian: idahip_set_host_band_problem");
    c->cb_res = res;
    c->cb_jac = jac;
    c->cb_bjac = nullptr;
    c->cb_user = user;
    c->dq_locked = 0;  // a Jacobian exists again: the mode may be switched off (it is left as it is)
    return 0;
}

int idahip_set_host_residual(idahip_ctx* c, idahip_res_fn res, void* user) {
    if (!c || !res) return -1;
    if (c->kind != IDAHIP_HOST_CALLBACK) return fail(c, -2, "not an IDAHIP_HOST_CALLBACK ctx");
    c->cb_res = res;
    c->cb_jac = nullptr;
    c->cb_bjac = nullptr;
    c->cb_user = user;
    if (c->krylov) return 0;  // no Jacobian to ask for: the residual is all a Krylov ctx takes
    c->jac_dq = 1;
    c->dq_locked = 1;
    return 0;
}

int idahip_set_host_band_problem(idahip_ctx* c, idahip_res_fn res, idahip_band_jac_fn bjac, void* user) {
    if (int rc = refuse_krylov(c, "idahip_set_host_band_problem")) return rc;
    if (!c || !res || !bjac) return -1;
    if (c->kind != IDAHIP_HOST_CALLBACK) return fail(c, -2, "not an IDAHIP_HOST_CALLBACK ctx");
    if (!c->band) return fail(c, -2, "a dense ctx takes a dense Jacobian: idahip_set_host_problem");
    c->cb_res = res;
    c->cb_jac = nullptr;
    c->cb_bjac = bjac;
    c->cb_user = user;
    c->dq_locked = 0;
    return 0;
}

int idahip_upload(idahip_ctx* c, idahip_field f, int first, int count, const double* h) {
    DevGuard dev_guard__(c);
    if (!c || !h) return -1;
    double* d = field_ptr(c, f);
    if (!d) return fail(c, -2, "unknown field %d", (int)f);
    if (first < 0 || count < 0 || first + count > c->batch) return fail(c, -2, "system range out of bounds");
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    IDAHIP_HIP(c, hipMemcpy(d + (size_t)first * c->n, h, sizeof(double) * count * c->n, hipMemcpyHostToDevice));
    return 0;
}

int idahip_download(idahip_ctx* c, idahip_field f, int first, int count, double* h) {
    DevGuard dev_guard__(c);
    if (!c || !h) return -1;
    double* d = field_ptr(c, f);
    if (!d) return fail(c, -2, "unknown field %d", (int)f);
    if (first < 0 || count < 0 || first + count > c->batch) return fail(c, -2, "system range out of bounds");
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    IDAHIP_HIP(c, hipMemcpy(h, d + (size_t)first * c->n, sizeof(double) * count * c->n, hipMemcpyDeviceToHost));
    return 0;
}

int idahip_download_lu(idahip_ctx* c, int sys, double* hLU, int64_t* hPiv) {
    if (int rc = refuse_krylov(c, "idahip_download_lu")) return rc;
    DevGuard dev_guard__(c);
    if (!c) return -1;
    if (sys < 0 || sys >= c->batch) return fail(c, -2, "system out of range");
    if (c->band) return fail(c, -2, "idahip_download_lu on a band ctx: idahip_download_lu_band");
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    const size_t nn = (size_t)c->n * c->n;
    if (hLU) IDAHIP_HIP(c, hipMemcpy(hLU, c->lu + sys * nn, sizeof(double) * nn, hipMemcpyDeviceToHost));
    if (hPiv) IDAHIP_HIP(c, hipMemcpy(hPiv, c->piv + (size_t)sys * c->n, sizeof(int64_t) * c->n, hipMemcpyDeviceToHost));
    if (hLU && lu_staged_on(c)) {
        // staged L: rows >= k0 + 64 of block column q stand in the order of the live list behind super-panel q. Composing the maps of
        // the super-panels after it gives every such row its pivot position; the caller receives the reference layout as ever.
        const int n = c->n, nq = (n + 63) / 64;
        std::vector<uint16_t> ord((size_t)nq * n);
        IDAHIP_HIP(c, hipMemcpy(ord.data(), c->lu_ord + (size_t)sys * nq * n, sizeof(uint16_t) * ord.size(), hipMemcpyDeviceToHost));
        std::vector<int> fin(n), nxt(n);  // fin[i]: pivot position of entry i of the live list behind super-panel q
        std::vector<double> col(n);
        for (int q = nq - 2; q >= 0; --q) {
            const int k1 = (q + 1) * 64, m1 = n - k1;  // the next super-panel's first column and live rows
            for (int i = 0; i < m1; ++i) {
                const int o = ord[(size_t)(q + 1) * n + i];
                nxt[i] = o < 64 ? k1 + o : (o - 64 < m1 - 64 ? fin[o - 64] : k1);  // (a map never written -- no factorisation yet -- stays inside the matrix)
            }
            std::swap(fin, nxt);
            for (int j = q * 64; j < k1; ++j) {
                double* cj = hLU + (size_t)j * n;
                for (int i = 0; i < m1; ++i) col[i] = cj[k1 + i];
                for (int i = 0; i < m1; ++i)
                    if (fin[i] < n) cj[fin[i]] = col[i];
            }
        }
    }
    return 0;
}

int idahip_download_lu_band(idahip_ctx* c, int sys, double* hAB, int64_t* hPiv) {
    if (int rc = refuse_krylov(c, "idahip_download_lu_band")) return rc;
    DevGuard dev_guard__(c);
    if (!c) return -1;
    if (sys < 0 || sys >= c->batch) return fail(c, -2, "system out of range");
    if (!c->band) return fail(c, -2, "idahip_download_lu_band on a dense ctx");
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    const size_t ne = (size_t)c->ldab * c->n;
    if (hAB) IDAHIP_HIP(c, hipMemcpy(hAB, c->bab + sys * ne, sizeof(double) * ne, hipMemcpyDeviceToHost));
    if (hPiv) IDAHIP_HIP(c, hipMemcpy(hPiv, c->piv + (size_t)sys * c->n, sizeof(int64_t) * c->n, hipMemcpyDeviceToHost));
    return 0;
}

void* idahip_dev_alloc(idahip_ctx* c, size_t bytes) {
    DevGuard dev_guard__(c);
    void* p = nullptr;
    if (!c || hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    return p;
}
int idahip_dev_free(idahip_ctx* c, void* d) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    IDAHIP_HIP(c, hipFree(d));
    return 0;
}
int idahip_memcpy_h2d(idahip_ctx* c, void* d, const void* h, size_t bytes) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    IDAHIP_HIP(c, hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return 0;
}
int idahip_memcpy_d2h(idahip_ctx* c, void* h, const void* d, size_t bytes) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    IDAHIP_HIP(c, hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------------ LSolver
int idahip_ls_setup(idahip_ctx* c, double* dA, int64_t* dPiv, int32_t* hInfo, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({dA, dPiv, hInfo})) return f.rc;
    if (c->band) return fail(c, -2, "idahip_ls_setup on a band ctx (no dense work matrices): idahip_ls_setup_band");
    if (c->krylov) return fail(c, -2, "idahip_ls_setup on a Krylov ctx (idahip_create_krylov): it holds no dense work matrices");
    if (!f.stage()) return f.rc;
    const int n = c->n;
    const long nn = (long)n * n;
    f.launch(IDAHIP_K_LU, nsys, "lu", [&] {
        if (n <= TINY_N) return lu_factor_batched(c, dA, nn, dA, nn, (long long*)dPiv, n, nullptr, f.idx, nsys);
        // factor in place in dA (physical row order), scatter rows into the ctx work matrix, copy back
        const int rc = lu_factor_batched(c, dA, nn, c->jw, nn, (long long*)dPiv, n, nullptr, f.idx, nsys);
        for (int s = 0; s < nsys && !rc; ++s)  // listed systems only; info != 0 systems keep their partial factors
            (void)hipMemcpyAsync(dA + hIdx[s] * nn, c->jw + hIdx[s] * nn, sizeof(double) * nn, hipMemcpyDeviceToDevice, c->stream);
        return rc;
    });
    return f.rc ? f.rc : report_info(c, hIdx, nsys, hInfo);
}

int idahip_ls_solve(idahip_ctx* c, const double* dLU, const int64_t* dPiv, double* dX, const double* dB, double /*tol*/,
                    const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({dLU, dPiv, dX, dB})) return f.rc;
    if (!f.stage()) return f.rc;
    const int n = c->n;
    f.launch(IDAHIP_K_SOLVE, nsys, "ls_solve", [&] {
        if (n <= TINY_N) {
            hipLaunchKernelGGL(tiny_solve_kernel, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, dLU, (long)n * n, (const long long*)dPiv,
                               (long)n, dX, dB, n, f.idx, nsys);
        } else {
            const size_t shm = sizeof(double) * n + sizeof(int) * n;
            if (n % 2 == 0)
                hipLaunchKernelGGL(ls_solve_kernel<2>, dim3(nsys), dim3(256), shm, c->stream, dLU, (long)n * n, (const long long*)dPiv,
                                   (long)n, (const int*)nullptr, dX, dB, n, f.idx);
            else
                hipLaunchKernelGGL(ls_solve_kernel<1>, dim3(nsys), dim3(256), shm, c->stream, dLU, (long)n * n, (const long long*)dPiv,
                                   (long)n, (const int*)nullptr, dX, dB, n, f.idx);
        }
    });
    return f.done();
}

int idahip_ls_setup_band(idahip_ctx* c, int ml, int mu, double* dAB, int64_t* dPiv, int32_t* hInfo, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({dAB, dPiv, hInfo})) return f.rc;
    if (ml < 0 || mu < 0 || ml >= c->n || mu >= c->n) return fail(c, -2, "bandwidths ml = %d, mu = %d outside [0, n)", ml, mu);
    if (!f.stage()) return f.rc;
    const int n = c->n;
    f.launch(IDAHIP_K_LU, nsys, nullptr, [&] { return band_factor(c, dAB, (long)(2 * ml + mu + 1) * n, dPiv, n, ml, mu, f.idx, nsys); });
    return f.rc ? f.rc : report_info(c, hIdx, nsys, hInfo);
}

int idahip_ls_solve_band(idahip_ctx* c, int ml, int mu, const double* dAB, const int64_t* dPiv, double* dX, const double* dB, double /*tol*/,
                         const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({dAB, dPiv, dX, dB})) return f.rc;
    if (ml < 0 || mu < 0 || ml >= c->n || mu >= c->n) return fail(c, -2, "bandwidths ml = %d, mu = %d outside [0, n)", ml, mu);
    if (!f.stage()) return f.rc;
    const int n = c->n;
    f.launch(IDAHIP_K_SOLVE, nsys, "ls_solve_band", [&] {
        const int spw = band_spw(c, nsys);
        const dim3 grid((nsys + spw - 1) / spw), blk(spw);
        const long ss = (long)(2 * ml + mu + 1) * n;
        if (ml == 1 && mu == 1)
            hipLaunchKernelGGL((band_getrs_kernel<1, 1>), grid, blk, 0, c->stream, dAB, ss, (const long long*)dPiv, (long)n, dX, dB, n, ml, mu, f.idx, nsys);
        else
            hipLaunchKernelGGL((band_getrs_kernel<-1, -1>), grid, blk, 0, c->stream, dAB, ss, (const long long*)dPiv, (long)n, dX, dB, n, ml, mu, f.idx, nsys);
    });
    return f.done();
}

int idahip_wrms(idahip_ctx* c, const double* dX, const double* dW, double* hOut, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({dX, dW, hOut})) return f.rc;
    if (!f.stage()) return f.rc;
    const int n = c->n;
    double* d_out = f.out<double>(nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "wrms", [&] {
        if (n <= TINY_N)
            hipLaunchKernelGGL(tiny_wrms_kernel, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, dX, dW, d_out, n, f.idx, nsys);
        else
            hipLaunchKernelGGL(wrms_kernel, dim3(nsys), dim3(256), sizeof(double) * n, c->stream, dX, dW, d_out, n, f.idx);
    });
    if (!f.fetch()) return f.rc;
    f.rms(hOut, d_out, nsys);
    return 0;
}

int idahip_wrms_masked(idahip_ctx* c, const double* dX, const double* dW, double* hOut, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({dX, dW, hOut})) return f.rc;
    if (c->h_id.empty()) return fail(c, -2, "idahip_wrms_masked: no id vector is set (idahip_set_id)");
    if (!f.stage()) return f.rc;
    const int n = c->n;
    double* d_out = f.out<double>(nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "wrms_masked", [&] {
        hipLaunchKernelGGL(wrms_masked_kernel, dim3(nsys), dim3(256), sizeof(double) * n, c->stream, dX, dW, (const double*)c->d_id, d_out, n, f.idx);
    });
    if (!f.fetch()) return f.rc;
    f.rms(hOut, d_out, nsys);  // by the full n (norm_rms.rs:56)
    return 0;
}


// ------------------------------------------------------------------------------------------------ NLProblem
namespace {

// residual kernels of IdaNLProblem::sys; jac_out != nullptr (linear dense, column-major work matrix only) also forms J
// residual of a host-callback problem: device forms and packs yy, yp; host calls the user's res per listed system; device
// scatters the residuals (launch_sys with c->kind == IDAHIP_HOST_CALLBACK)
// (ic: the same round trip with the IC front end, idahip_ic_res / idahip_ic_trial)
int callback_sys(idahip_ctx* c, const SysArgs& a, const double* hTn, const int32_t* hIdx, int nsys, const SysArgsIC* ic = nullptr) {
    const int n = c->n;
    if (!c->cb_res || !(c->cb_jac || c->cb_bjac || c->dq_locked || c->krylov))
        return fail(c, -2, "IDAHIP_HOST_CALLBACK: idahip_set_host_problem has not been called");
    const size_t cnt = (size_t)nsys * 3 * n;
    if (ic) hipLaunchKernelGGL(ic_callback_pre_kernel, dim3(nsys), dim3(256), 0, c->stream, *ic, c->cb_stage);
    else hipLaunchKernelGGL(callback_pre_kernel, dim3(nsys), dim3(256), 0, c->stream, a, c->cb_stage);
    if (c->cb_host.size() < cnt) c->cb_host.resize(cnt);
    double* h = c->cb_host.data();
    IDAHIP_HIP(c, hipMemcpyAsync(h, c->cb_stage, sizeof(double) * cnt, hipMemcpyDeviceToHost, c->stream));
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < nsys; ++s) {
        double* hs = h + (size_t)s * 3 * n;
        if (c->cb_res(hIdx[s], hTn[s], hs, hs + n, hs + 2 * n, c->cb_user) != 0)
            return fail(c, -7, "the user's residual function failed for system %d", hIdx[s]);
    }
    IDAHIP_HIP(c, hipMemcpyAsync(c->cb_stage, h, sizeof(double) * cnt, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(callback_post_kernel, dim3(nsys), dim3(256), 0, c->stream, a, (const double*)c->cb_stage);
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));  // cb_host is reused by the next call
    return post_launch(c, "nls_sys (host callback)");
}

// Jacobian of a host-callback problem into the LU work matrices (column-major per system), or on a band ctx into the band
// storage (ldab * n doubles per system)
int callback_jac(idahip_ctx* c, double* work, const int* d_idx, const double* hTn, const double* hCj, const int32_t* hIdx, int nsys) {
    const int n = c->n;
    const size_t nn = c->band ? (size_t)c->ldab * n : (size_t)n * n;
    if (!c->cb_res || !(c->band ? (bool)c->cb_bjac : (bool)c->cb_jac))
        return fail(c, -2, "IDAHIP_HOST_CALLBACK: %s has not been called", c->band ? "idahip_set_host_band_problem" : "idahip_set_host_problem");
    const size_t cnt = (size_t)nsys * 3 * n;
    hipLaunchKernelGGL(callback_pack_kernel, dim3(nsys), dim3(256), 0, c->stream, (const double*)c->yy, (const double*)c->yp,
                       (const double*)c->savres, d_idx, n, c->cb_stage);
    if (c->cb_host.size() < cnt) c->cb_host.resize(cnt);
    double* h = c->cb_host.data();
    // The Jacobians go up a chunk at a time: the user's function fills a pinned buffer system by system, ONE asynchronous copy
    // takes the chunk to a device staging buffer and one kernel scatters it into the listed systems' work matrices (a pageable
    // hipMemcpy per system on the null stream before: O(nsys) blocking copies per setup). A chunk is <= 64 MB.
    const size_t chunk = std::max<size_t>(1, std::min<size_t>((size_t)nsys, ((size_t)64 << 20) / (nn * sizeof(double))));
    if (c->cb_jcap < chunk) {
        if (c->cb_jpin) (void)hipHostFree(c->cb_jpin);
        if (c->cb_jdev) (void)hipFree(c->cb_jdev);
        c->cb_jpin = nullptr; c->cb_jdev = nullptr; c->cb_jcap = 0;
        if (hipHostMalloc((void**)&c->cb_jpin, chunk * nn * sizeof(double)) != hipSuccess) { c->cb_jpin = nullptr; return fail(c, -100, "pinned staging for %zu Jacobians", chunk); }
        if (hipMalloc((void**)&c->cb_jdev, chunk * nn * sizeof(double)) != hipSuccess) {
            (void)hipHostFree(c->cb_jpin);
            c->cb_jpin = nullptr; c->cb_jdev = nullptr;
            return fail(c, -100, "device staging for %zu Jacobians", chunk);
        }
        c->cb_jcap = chunk;
    }
    IDAHIP_HIP(c, hipMemcpyAsync(h, c->cb_stage, sizeof(double) * cnt, hipMemcpyDeviceToHost, c->stream));
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t s0 = 0; s0 < (size_t)nsys; s0 += chunk) {
        const size_t m = std::min(chunk, (size_t)nsys - s0);
        for (size_t q = 0; q < m; ++q) {
            const size_t s = s0 + q;
            const double* hs = h + s * 3 * n;
            double* J = c->cb_jpin + q * nn;
            for (size_t e = 0; e < nn; ++e) J[e] = 0.0;  // J <- 0 (ida_ls.rs:255)
            if ((c->band ? c->cb_bjac(hIdx[s], hTn[s], hCj[s], hs, hs + n, hs + 2 * n, J, c->ldab, c->cb_user)
                         : c->cb_jac(hIdx[s], hTn[s], hCj[s], hs, hs + n, hs + 2 * n, J, c->cb_user)) != 0)
                return fail(c, -7, "the user's Jacobian function failed for system %d", hIdx[s]);
        }
        IDAHIP_HIP(c, hipMemcpyAsync(c->cb_jdev, c->cb_jpin, sizeof(double) * m * nn, hipMemcpyHostToDevice, c->stream));
        const int gy = (int)std::min<size_t>(64, (nn + 255) / 256);
        hipLaunchKernelGGL(callback_scatter_jac_kernel, dim3((unsigned)m, gy), dim3(256), 0, c->stream, (const double*)c->cb_jdev, work, d_idx + s0, (long)nn);
        if (s0 + chunk < (size_t)nsys) IDAHIP_HIP(c, hipStreamSynchronize(c->stream));  // the pinned buffer is filled again
    }
    return 0;
}

int launch_sys(idahip_ctx* c, const SysArgs& a, int nsys, double* jac_out, const double* hTn = nullptr, const int32_t* hIdx = nullptr) {
    const int n = c->n;
    switch (c->kind) {
        case IDAHIP_HOST_CALLBACK:
            return callback_sys(c, a, hTn, hIdx, nsys);
        case IDAHIP_ROBERTS:
            hipLaunchKernelGGL(tiny_sys_kernel<IDAHIP_ROBERTS>, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, a, (const double*)nullptr, 0, nsys);
            break;
        case IDAHIP_LORENZ63:
            hipLaunchKernelGGL(tiny_sys_kernel<IDAHIP_LORENZ63>, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, a, (const double*)c->params, 3, nsys);
            break;
        case IDAHIP_LINEAR_DENSE: {
            const size_t shm = 2 * sizeof(double) * n;
            const double *A = c->A, *B = c->B, *C = c->C;
            if (jac_out) {
                if (n % 2 == 0) hipLaunchKernelGGL((linear_sys_kernel<2, true>), dim3(nsys), dim3(256), shm, c->stream, a, A, B, C, jac_out);
                else hipLaunchKernelGGL((linear_sys_kernel<1, true>), dim3(nsys), dim3(256), shm, c->stream, a, A, B, C, jac_out);
            } else {
                if (n % 2 == 0) hipLaunchKernelGGL((linear_sys_kernel<2, false>), dim3(nsys), dim3(256), shm, c->stream, a, A, B, C, (double*)nullptr);
                else hipLaunchKernelGGL((linear_sys_kernel<1, false>), dim3(nsys), dim3(256), shm, c->stream, a, A, B, C, (double*)nullptr);
            }
            break;
        }
        case IDAHIP_MASS_ACTION:
            if (int rc = ma_unset(c, "nls_sys")) return rc;
            launch_ma_sys(c, a, nsys);
            break;
        default:
            if (!with_stencil(c, [&](auto p) {
                    hipLaunchKernelGGL(stencil_sys_kernel<decltype(p)>, dim3(nsys), dim3(256), sizeof(double) * n, c->stream, a, (const double*)c->params);
                }))
                return no_kernel(c, "residual");
            break;
    }
    return post_launch(c, "nls_sys");
}


// ------------------------------------------------------------------------------------------------ difference-quotient Jacobians
// (dq_kernels.hpp; idahip_set_jacobian_dq)

// residual evaluations of one DQ Jacobian of this ctx (what C IDA adds to nreDQ)
long dq_evals(const idahip_ctx* c) { return c->band ? std::min(c->ml + c->mu + 1, c->n) : c->n; }

int dq_grow(idahip_ctx* c, double** p, size_t* cap, size_t want) {
    if (*cap >= want) return 0;
    if (*p) IDAHIP_HIP(c, hipFree(*p));
    *p = nullptr;
    *cap = 0;
    if (hipMalloc((void**)p, want * sizeof(double)) != hipSuccess) {
        *p = nullptr;
        return fail(c, -100, "DQ staging of %zu doubles", want);
    }
    *cap = want;
    return 0;
}

// Host-callback problems: dq_pack_kernel writes perturbed copies of (yy, yp), the host calls the user's residual on each copy,
// dq_scatter_kernel differences the residuals into the Jacobian. Dense: up to G columns of m systems per pass, as many as the
// bounded staging holds; band: one group of every system per pass. The host does no arithmetic on the entries.
int callback_dq_jac(idahip_ctx* c, const DqArgs& d0, const double* hTn, const int32_t* hIdx, int nsys) {
    const int n = c->n;
    if (!c->cb_res) return fail(c, -2, "IDAHIP_HOST_CALLBACK: no residual registered (idahip_set_host_residual)");
    if (!hTn || !hIdx) return fail(c, -2, "a host-callback DQ Jacobian needs the systems' tn and ids on the host");
    const size_t per = 3 * (size_t)n;
    const size_t copies = std::max<size_t>(1, ((size_t)32 << 20) / (per * sizeof(double)));  // staging <= 32 MB (or one copy)
    const bool band = d0.ld > 0;  // (a band ctx, or the band preconditioner of a Krylov ctx)
    const int ngroups = band ? std::min(d0.ml + d0.mu + 1, n) : n;
    const int msys = (int)std::min<size_t>((size_t)nsys, copies);
    const int G = band ? 1 : (int)std::max<size_t>(1, std::min<size_t>((size_t)n, copies / msys));
    int rc = dq_grow(c, &c->dq_stage, &c->dq_stage_cap, (size_t)msys * G * per);
    if (rc) return rc;
    if (c->cb_host.size() < (size_t)msys * G * per) c->cb_host.resize((size_t)msys * G * per);
    double* h = c->cb_host.data();
    const size_t mat = band ? (size_t)d0.ld * n : (size_t)n * n;
    for (int s0 = 0; s0 < nsys; s0 += msys) {
        const int m = std::min(msys, nsys - s0);
        DqArgs d = d0;
        d.idx += s0; d.cj += s0; d.hh += s0;
        if (d.compact) d.out += (size_t)s0 * mat;
        for (int j0 = 0; j0 < ngroups; j0 += G) {
            const int g = std::min(G, ngroups - j0);
            const size_t cnt = (size_t)m * g * per;
            hipLaunchKernelGGL(dq_pack_kernel, dim3(m, g), dim3(256), 0, c->stream, d, j0, g, c->dq_stage);
            IDAHIP_HIP(c, hipMemcpyAsync(h, c->dq_stage, sizeof(double) * cnt, hipMemcpyDeviceToHost, c->stream));
            IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
            for (int q = 0; q < m * g; ++q) {
                double* hs = h + (size_t)q * per;
                const int sp = s0 + q / g;
                if (c->cb_res(hIdx[sp], hTn[sp], hs, hs + n, hs + 2 * n, c->cb_user) != 0)
                    return fail(c, -7, "the user's residual function failed for system %d (DQ Jacobian)", hIdx[sp]);
            }
            IDAHIP_HIP(c, hipMemcpyAsync(c->dq_stage, h, sizeof(double) * cnt, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(dq_scatter_kernel, dim3(m, g), dim3(256), 0, c->stream, d, j0, g, (const double*)c->dq_stage);
            IDAHIP_HIP(c, hipStreamSynchronize(c->stream));  // the host staging is filled again
        }
    }
    return post_launch(c, "DQ jac (host callback)");
}

// the band DQ kernel of the ctx's device kind (a band ctx, or the band preconditioner of a Krylov ctx)
int launch_band_dq(idahip_ctx* c, const DqArgs& d, int nsys, const char* what) {
    const int chunks = launch_chunks(nsys, 64);
    if (!with_stencil(c, [&](auto p) {
            hipLaunchKernelGGL(stencil_band_dq_jac_kernel<decltype(p)>, dim3(nsys, chunks), dim3(256), 0, c->stream, d, (const double*)c->params, chunks);
        }))
        return no_kernel(c, what);
    return post_launch(c, what);
}

// the ctx's fields a DQ Jacobian reads, and the storage it is formed in (ld = 0: dense); the caller adds the list and the output
void fill_dq_args(const idahip_ctx* c, DqArgs& d, int ml, int mu, int ld) {
    d.yy = c->yy; d.yp = c->yp; d.ewt = c->ewt; d.rr = c->savres;
    d.n = c->n; d.ml = ml; d.mu = mu; d.ld = ld;
}

// DQ Jacobians of the listed systems at the ctx's yy, yp, ewt and savres: into `out` by system id (the work matrices or the band
// storage) or, with `compact`, by list position. d_hh: the systems' step sizes, per list position.
int launch_dq_jac(idahip_ctx* c, double* out, bool compact, const int* d_idx, const double* d_cj, const double* d_hh, int nsys,
                  const double* hTn, const int32_t* hIdx, const int* d_skip) {
    const int n = c->n;
    if (nsys == 0) return 0;
    DqArgs d;
    fill_dq_args(c, d, c->band ? c->ml : 0, c->band ? c->mu : 0, c->band ? c->ldab : 0);
    d.idx = d_idx; d.cj = d_cj; d.hh = d_hh; d.skip = d_skip;
    d.out = out; d.compact = compact ? 1 : 0;
    if (c->kind == IDAHIP_HOST_CALLBACK) return callback_dq_jac(c, d, hTn, hIdx, nsys);
    if (c->band) {  // (idahip_create_band: the stencil problems are the band ctx's device kinds)
        return launch_band_dq(c, d, nsys, "band DQ jac");
    }
    switch (c->kind) {
        case IDAHIP_ROBERTS:
            hipLaunchKernelGGL(tiny_dq_jac_kernel<IDAHIP_ROBERTS>, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, d, (const double*)nullptr, 0, nsys);
            break;
        case IDAHIP_LORENZ63:
            hipLaunchKernelGGL(tiny_dq_jac_kernel<IDAHIP_LORENZ63>, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, d, (const double*)c->params, 3, nsys);
            break;
        case IDAHIP_LINEAR_DENSE: {
            const int tiles = (n + LDQ_T - 1) / LDQ_T;
            const size_t mat = (size_t)n * n;
            for (int s0 = 0; s0 < nsys; s0 += 65535) {  // (the list runs along the grid's y dimension)
                const int m = std::min(65535, nsys - s0);
                DqArgs e = d;
                e.idx += s0; e.cj += s0; e.hh += s0;
                if (e.skip) e.skip += s0;
                if (e.compact) e.out += (size_t)s0 * mat;
                hipLaunchKernelGGL(linear_dq_jac_kernel, dim3(tiles * tiles, m), dim3(256), 0, c->stream, e, (const double*)c->A,
                                   (const double*)c->B, (const double*)c->C, tiles);
            }
            break;
        }
        case IDAHIP_MASS_ACTION: {
            if (int rc = ma_unset(c, "DQ jac")) return rc;
            const int chunks = launch_chunks(nsys, n);
            if (ma_laws(c)) hipLaunchKernelGGL(ma_dq_jac_kernel<true>, dim3(nsys, chunks), dim3(256), 2 * sizeof(double) * n, c->stream, d, *c->ma_law, (const double*)c->params, chunks);
            else hipLaunchKernelGGL(ma_dq_jac_kernel<false>, dim3(nsys, chunks), dim3(256), 2 * sizeof(double) * n, c->stream, d, *c->ma, (const double*)c->params, chunks);
            break;
        }
        default: {
            const int chunks = launch_chunks(nsys, n);
            const bool stencil = with_stencil(c, [&](auto p) {
                hipLaunchKernelGGL(stencil_dq_jac_kernel<decltype(p)>, dim3(nsys, chunks), dim3(256), 0, c->stream, d, (const double*)c->params, chunks,
                                   (!compact && out == c->jw) ? (const int*)c->lu_jwzero : nullptr);
            });
            if (!stencil) return fail(c, -2, "no DQ Jacobian for problem kind %d", (int)c->kind);
            break;
        }
    }
    return post_launch(c, "DQ jac");
}

// Jacobian kernels of IdaNLProblem::setup (jac at the current yy, yp, cj) into the LU work matrix
int launch_jac(idahip_ctx* c, double* work, const int* d_idx, const double* d_cj, int nsys, const double* hTn = nullptr,
               const double* hCj = nullptr, const int32_t* hIdx = nullptr, const int* d_skip = nullptr, const double* d_hh = nullptr) {
    const int n = c->n;
    const long nn = (long)n * n;
    if (c->jac_dq) {  // every Jacobian of a DQ ctx is a DQ one: dense into the work matrix, band into the band storage
        if (!d_hh) return fail(c, -2, "a DQ Jacobian needs the systems' step sizes");
        return launch_dq_jac(c, c->band ? c->bab : work, false, d_idx, d_cj, d_hh, nsys, hTn, hIdx, d_skip);
    }
    if (c->band) {  // the band storage is the work matrix: the factorisation runs in place
        if (c->kind == IDAHIP_HOST_CALLBACK) return callback_jac(c, c->bab, d_idx, hTn, hCj, hIdx, nsys);
        const int chunks = launch_chunks(nsys, 64);
        if (!with_stencil(c, [&](auto p) {
                hipLaunchKernelGGL(stencil_band_jac_kernel<decltype(p)>, dim3(nsys, chunks), dim3(256), 0, c->stream, c->bab, n, c->ml, c->mu,
                                   (const double*)c->yy, (const double*)c->params, d_idx, d_cj, chunks, d_skip);
            }))
            return no_kernel(c, "band jac");
        return post_launch(c, "band jac");
    }
    switch (c->kind) {
        case IDAHIP_HOST_CALLBACK:
            return callback_jac(c, work, d_idx, hTn, hCj, hIdx, nsys);
        case IDAHIP_ROBERTS:
            hipLaunchKernelGGL(tiny_jac_kernel<IDAHIP_ROBERTS>, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, work, (const double*)c->yy,
                               (const double*)nullptr, 0, d_idx, d_cj, nsys);
            break;
        case IDAHIP_LORENZ63:
            hipLaunchKernelGGL(tiny_jac_kernel<IDAHIP_LORENZ63>, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, work, (const double*)c->yy,
                               (const double*)c->params, 3, d_idx, d_cj, nsys);
            break;
        case IDAHIP_LINEAR_DENSE: {
            const int chunks = launch_chunks(nsys, 64);
            hipLaunchKernelGGL(linear_jac_kernel, dim3(nsys, chunks), dim3(256), 0, c->stream, work, (const double*)c->A,
                               (const double*)c->B, nn, d_idx, d_cj, chunks);
            break;
        }
        case IDAHIP_MASS_ACTION: {
            if (int rc = ma_unset(c, "jac")) return rc;
            const int chunks = launch_chunks(nsys, n);
            if (ma_laws(c)) hipLaunchKernelGGL(ma_jac_kernel<true>, dim3(nsys, chunks), dim3(256), 0, c->stream, work, n, (const double*)c->yy, *c->ma_law, (const double*)c->params,
                                               d_idx, d_cj, chunks, d_skip, 0);
            else hipLaunchKernelGGL(ma_jac_kernel<false>, dim3(nsys, chunks), dim3(256), 0, c->stream, work, n, (const double*)c->yy, *c->ma, (const double*)c->params,
                                    d_idx, d_cj, chunks, d_skip, 0);
            break;
        }
        default: {
            const int chunks = launch_chunks(nsys, n);
            if (!with_stencil(c, [&](auto p) {
                    hipLaunchKernelGGL(stencil_jac_kernel<decltype(p)>, dim3(nsys, chunks), dim3(256), 0, c->stream, work, n, (const double*)c->yy,
                                       (const double*)c->params, d_idx, d_cj, chunks, d_skip, (work == c->jw) ? (const int*)c->lu_jwzero : nullptr);
                }))
                return no_kernel(c, "jac");
            break;
        }
    }
    return post_launch(c, "jac");
}

// idahip_set_jac_in_lu: can this ctx form J = B + cj*A inside the factorisation at all, and does it now (LuJac, lu_driver.hpp)
bool jac_in_lu_can(const idahip_ctx* c) {
    return c->kind == IDAHIP_LINEAR_DENSE && !c->band && !c->krylov && c->n > TINY_N && c->n <= WP_MAX_ROWS;
}
// list_entry: asked by idahip_nls_lsetup / idahip_nls_sys_setup, which take the path only once it has been switched on by name --
// left alone they launch the kernel classes they always launched. idahip_round_solve takes it unasked only where the first panel is
// the eight-slot instantiation (n > 448: the size it was measured at, profiles/r08_jac_in_lu_ab.txt); smaller matrices go through an
// instantiation that reads its slot count at run time and have not been measured: on request only.
bool jac_in_lu_on(const idahip_ctx* c, bool list_entry) {
    const bool asked = c->jac_in_lu == 1;
    const bool unasked = c->jac_in_lu < 0 && !list_entry && c->n > WP_MAX_ROWS - 64;
    if (!asked && !unasked) return false;
    return jac_in_lu_can(c) && !c->jac_dq && lu_jac_eligible(c);
}

// batched getrf of the work matrices into ctx->lu / piv / perm, then the per-system info of the listed systems
// (jq: the work matrices do not hold J, the factorisation forms it: jac_in_lu_on)
int factor_and_report(ListCall& f, double* work, int32_t* hInfo, const LuJac* jq = nullptr) {
    idahip_ctx* c = f.c;
    const int n = c->n, nsys = f.nsys;
    const long nn = (long)n * n;
    f.launch(IDAHIP_K_LU, nsys, "lu", [&] {
        if (c->band) return band_factor(c, c->bab, (long)c->ldab * n, c->piv, n, c->ml, c->mu, f.idx, nsys);
        return lu_factor_batched(c, work, nn, c->lu, nn, (long long*)c->piv, n, c->perm, f.idx, nsys, nullptr, jq);
    });
    return f.rc ? f.rc : report_info(c, f.hIdx, nsys, hInfo);
}

void fill_sys_args(idahip_ctx* c, SysArgs& a, int reset_ee) {
    a.yypredict = c->yypredict; a.yppredict = c->yppredict; a.yy = c->yy; a.yp = c->yp; a.ee = c->ee; a.delta = c->delta;
    a.savres = c->savres; a.n = c->n; a.reset_ee = reset_ee;
}

}  // namespace

int idahip_nls_sys(idahip_ctx* c, const double* hTn, const double* hCj, int reset_ee, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hTn, hCj})) return f.rc;
    if (int rcu = ma_unset(c, "idahip_nls_sys")) return rcu;
    if (!f.stage()) return f.rc;
    SysArgs a;
    a.idx = f.idx;
    a.tn = f.in(hTn, nsys);
    a.cj = f.in(hCj, nsys);
    fill_sys_args(c, a, reset_ee);
    f.launch(IDAHIP_K_SYS, nsys, nullptr, [&] { return launch_sys(c, a, nsys, nullptr, hTn, hIdx); });
    return f.done();
}

int idahip_nls_lsetup(idahip_ctx* c, const double* hTn, const double* hCj, int32_t* hInfo, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_nls_lsetup");
    if (!f.args({hTn, hCj, hInfo})) return f.rc;
    if (int rcu = ma_unset(c, "idahip_nls_lsetup")) return rcu;
    if (c->jac_dq) return fail(c, -2, "a DQ ctx forms its Jacobians with the step sizes: idahip_nls_lsetup_dq");
    if (!f.stage()) return f.rc;
    const double* d_cj = f.in(hCj, nsys);
    double* work = (c->n <= TINY_N) ? c->lu : c->jw;
    const bool jin = jac_in_lu_on(c, true);  // J = B + cj*A is formed by the factorisation itself: no Jacobian kernel
    const LuJac jq{c->A, c->B, d_cj, 0};
    if (!jin) f.launch(IDAHIP_K_JAC, nsys, nullptr, [&] { return launch_jac(c, work, f.idx, d_cj, nsys, hTn, hCj, hIdx); });
    return factor_and_report(f, work, hInfo, jin ? &jq : nullptr);
}

int idahip_nls_sys_setup(idahip_ctx* c, const double* hTn, const double* hCj, int reset_ee, int32_t* hInfo, const int32_t* hIdx,
                         int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_nls_sys_setup");
    if (!f.args({hTn, hCj, hInfo})) return f.rc;
    if (int rcu = ma_unset(c, "idahip_nls_sys_setup")) return rcu;
    if (c->jac_dq) return fail(c, -2, "a DQ ctx forms its Jacobians with the step sizes: idahip_nls_sys, then idahip_nls_lsetup_dq");
    if (!f.stage()) return f.rc;
    SysArgs a;
    a.idx = f.idx;
    a.tn = f.in(hTn, nsys);
    a.cj = f.in(hCj, nsys);
    fill_sys_args(c, a, reset_ee);
    double* work = (c->n <= TINY_N) ? c->lu : c->jw;
    // the linear dense residual sweeps A and B anyway: J = B + cj*A falls out of the same pass -- unless the factorisation forms it
    // as it loads (jac_in_lu_on): the plain sweep then, and no J in memory at all
    const bool jin = jac_in_lu_on(c, true);
    const LuJac jq{c->A, c->B, a.cj, 0};
    const bool fused = c->kind == IDAHIP_LINEAR_DENSE && c->n > TINY_N && !jin;
    f.launch(fused ? IDAHIP_K_SYS_JAC : IDAHIP_K_SYS, nsys, nullptr, [&] { return launch_sys(c, a, nsys, fused ? work : nullptr, hTn, hIdx); });
    if (!fused && !jin) f.launch(IDAHIP_K_JAC, nsys, nullptr, [&] { return launch_jac(c, work, a.idx, a.cj, nsys, hTn, hCj, hIdx); });
    return factor_and_report(f, work, hInfo, jin ? &jq : nullptr);
}

int idahip_nls_lsetup_dq(idahip_ctx* c, const double* hTn, const double* hCj, const double* hHh, int32_t* hInfo, const int32_t* hIdx,
                         int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_nls_lsetup_dq");
    if (!f.args({hTn, hCj, hHh, hInfo})) return f.rc;
    if (int rcu = ma_unset(c, "idahip_nls_lsetup_dq")) return rcu;
    if (!c->jac_dq) return fail(c, -2, "idahip_nls_lsetup_dq on a ctx with analytic Jacobians (idahip_set_jacobian_dq)");
    if (!f.stage()) return f.rc;
    const double* d_cj = f.in(hCj, nsys);
    const double* d_hh = f.in(hHh, nsys);
    double* work = (c->n <= TINY_N) ? c->lu : c->jw;
    f.launch(IDAHIP_K_JAC, nsys, nullptr, [&] { return launch_jac(c, work, f.idx, d_cj, nsys, hTn, hCj, hIdx, nullptr, d_hh); });
    return factor_and_report(f, work, hInfo);
}

int idahip_jac_dq(idahip_ctx* c, const double* hTn, const double* hCj, const double* hHh, double* hJ, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hTn, hCj, hHh, hJ})) return f.rc;
    if (int rcu = ma_unset(c, "idahip_jac_dq")) return rcu;
    if (!f.stage()) return f.rc;
    const size_t mat = c->band ? (size_t)c->ldab * c->n : (size_t)c->n * c->n;
    const double* d_cj = f.in(hCj, nsys);
    const double* d_hh = f.in(hHh, nsys);
    if (!f.send()) return f.rc;
    // a chunk of systems at a time through a buffer of its own: the ctx's work matrices and factors are left as they are
    const int m = (int)std::max<size_t>(1, std::min<size_t>((size_t)nsys, ((size_t)256 << 20) / (mat * sizeof(double))));
    if (int rc = dq_grow(c, &c->dq_out, &c->dq_out_cap, (size_t)m * mat)) return rc;
    for (int s0 = 0; s0 < nsys; s0 += m) {
        const int k = std::min(m, nsys - s0);
        if (!f.launch(IDAHIP_K_JAC, k, nullptr, [&] { return launch_dq_jac(c, c->dq_out, true, f.idx + s0, d_cj + s0, d_hh + s0, k, hTn + s0, hIdx + s0, nullptr); }))
            return f.rc;
        IDAHIP_HIP(c, hipMemcpyAsync(hJ + (size_t)s0 * mat, c->dq_out, sizeof(double) * k * mat, hipMemcpyDeviceToHost, c->stream));
        IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    }
    return f.done();
}


int idahip_mass_action_jac(idahip_ctx* c, int sys, double cj, double* hJ) {
    const int32_t one = sys;
    ListCall f(c, &one, 1);  // (a list of one system: the staging slot carries its id and cj to the kernel)
    if (!f.args({hJ})) return f.rc;
    if (c->kind != IDAHIP_MASS_ACTION) return fail(c, -2, "idahip_mass_action_jac: not an IDAHIP_MASS_ACTION ctx (kind %d)", (int)c->kind);
    if (int rcu = ma_unset(c, "idahip_mass_action_jac")) return rcu;
    if (!f.stage()) return f.rc;
    const int n = c->n;
    const size_t mat = (size_t)n * n;
    const double* d_cj = f.in(&cj, 1);
    if (!f.send()) return f.rc;
    // through idahip_jac_dq's buffer: the ctx's work matrices and factors are left as they are
    if (int rc = dq_grow(c, &c->dq_out, &c->dq_out_cap, mat)) return rc;
    const int chunks = launch_chunks(1, n);
    if (!f.launch(IDAHIP_K_JAC, 1, "ma_jac", [&] {
            if (ma_laws(c)) hipLaunchKernelGGL(ma_jac_kernel<true>, dim3(1, chunks), dim3(256), 0, c->stream, c->dq_out, n, (const double*)c->yy, *c->ma_law,
                                               (const double*)c->params, f.idx, d_cj, chunks, (const int*)nullptr, 1);
            else hipLaunchKernelGGL(ma_jac_kernel<false>, dim3(1, chunks), dim3(256), 0, c->stream, c->dq_out, n, (const double*)c->yy, *c->ma,
                                    (const double*)c->params, f.idx, d_cj, chunks, (const int*)nullptr, 1);
        }))
        return f.rc;
    IDAHIP_HIP(c, hipMemcpyAsync(hJ, c->dq_out, sizeof(double) * mat, hipMemcpyDeviceToHost, c->stream));
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    return f.done();
}

int idahip_set_jacobian_dq(idahip_ctx* c, int on) {
    if (!c) return -1;
    if (!on && c->dq_locked) return fail(c, -2, "the ctx has a residual and no Jacobian (idahip_set_host_residual): DQ stays on");
    if (on && c->krylov) return fail(c, -2, "idahip_set_jacobian_dq on a Krylov ctx (idahip_create_krylov): it forms no Jacobian");
    c->jac_dq = on ? 1 : 0;
    return 0;
}

int idahip_jacobian_dq(const idahip_ctx* c) { return c ? c->jac_dq : -1; }

// One Newton iteration body for the listed systems (shared by idahip_newton_iter and idahip_newton_iter2)
static int launch_newton_iter(idahip_ctx* c, const int* d_idx, const double* d_scale, double* d_out, const int* d_skip, int nsys) {
    const int n = c->n;
    if (c->band) {
        const int spw = band_spw(c, nsys);
        const dim3 grid((nsys + spw - 1) / spw), blk(spw);
        if (c->ml == 1 && c->mu == 1)
            hipLaunchKernelGGL((band_newton_iter_kernel<1, 1>), grid, blk, 0, c->stream, (const double*)c->bab, (const long long*)c->piv, c->ml, c->mu,
                               c->delta, c->ee, (const double*)c->ewt, n, d_idx, nsys, d_scale, d_out, d_skip);
        else
            hipLaunchKernelGGL((band_newton_iter_kernel<-1, -1>), grid, blk, 0, c->stream, (const double*)c->bab, (const long long*)c->piv, c->ml,
                               c->mu, c->delta, c->ee, (const double*)c->ewt, n, d_idx, nsys, d_scale, d_out, d_skip);
    } else if (n <= TINY_N) {
        hipLaunchKernelGGL(tiny_newton_iter_kernel, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, (const double*)c->lu,
                           (const long long*)c->piv, c->delta, c->ee, (const double*)c->ewt, n, d_idx, nsys, d_scale, d_out, d_skip);
    } else if (n % 2 == 0 && n >= 2048) {
        hipLaunchKernelGGL((newton_iter_kernel<2, 1024>), dim3(nsys), dim3(1024), sizeof(double) * (n + (n > 4096 ? n : 4096)), c->stream, (const double*)c->lu,
                           (const int*)c->perm, c->delta, c->ee, (const double*)c->ewt, n, d_idx, d_scale, d_out, d_skip, (const unsigned char*)c->lu_zmap, (const unsigned short*)nullptr);
    } else if (lu_staged_on(c)) {  // the ctx's factors are staged (lu_driver.hpp): no gather through perm, the maps instead
        if (n % 2 == 0)
            hipLaunchKernelGGL((newton_iter_kernel<2, 256, true>), dim3(nsys), dim3(256), 2 * sizeof(double) * n, c->stream, (const double*)c->lu,
                               (const int*)c->perm, c->delta, c->ee, (const double*)c->ewt, n, d_idx, d_scale, d_out, d_skip, (const unsigned char*)nullptr, (const unsigned short*)c->lu_ord);
        else
            hipLaunchKernelGGL((newton_iter_kernel<1, 256, true>), dim3(nsys), dim3(256), 2 * sizeof(double) * n, c->stream, (const double*)c->lu,
                               (const int*)c->perm, c->delta, c->ee, (const double*)c->ewt, n, d_idx, d_scale, d_out, d_skip, (const unsigned char*)nullptr, (const unsigned short*)c->lu_ord);
    } else if (n % 2 == 0) {
        hipLaunchKernelGGL(newton_iter_kernel<2>, dim3(nsys), dim3(256), 2 * sizeof(double) * n, c->stream, (const double*)c->lu,
                           (const int*)c->perm, c->delta, c->ee, (const double*)c->ewt, n, d_idx, d_scale, d_out, d_skip, (const unsigned char*)nullptr, (const unsigned short*)nullptr);
    } else {
        hipLaunchKernelGGL(newton_iter_kernel<1>, dim3(nsys), dim3(256), 2 * sizeof(double) * n, c->stream, (const double*)c->lu,
                           (const int*)c->perm, c->delta, c->ee, (const double*)c->ewt, n, d_idx, d_scale, d_out, d_skip, (const unsigned char*)nullptr, (const unsigned short*)nullptr);
    }
    return post_launch(c, "newton_iter");
}

int idahip_newton_iter(idahip_ctx* c, const double* hScale, double* hDelnrm, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_newton_iter");
    if (!f.args({hScale, hDelnrm})) return f.rc;
    if (!f.stage()) return f.rc;
    const double* d_scale = f.in(hScale, nsys);
    double* d_out = f.out<double>(nsys);
    f.launch(IDAHIP_K_NEWTON_ITER, nsys, nullptr, [&] { return launch_newton_iter(c, f.idx, d_scale, d_out, nullptr, nsys); });
    if (!f.fetch()) return f.rc;
    f.rms(hDelnrm, d_out, nsys);
    return 0;
}

int idahip_newton_iter2(idahip_ctx* c, const double* hScale, const double* hTn, const double* hCj, const double* hToldel, const double* hSs,
                        const double* hEpsNewt, double* hDelnrm, int32_t* hConv, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_newton_iter2");
    if (!f.args({hScale, hTn, hCj, hToldel, hSs, hEpsNewt, hDelnrm, hConv})) return f.rc;
    if (int rcu = ma_unset(c, "idahip_newton_iter2")) return rcu;
    if (c->kind == IDAHIP_HOST_CALLBACK) return fail(c, -2, "idahip_newton_iter2 needs a device residual (not for IDAHIP_HOST_CALLBACK)");
    if (!f.stage()) return f.rc;
    const int n = c->n;
    SysArgs a;
    a.idx = f.idx;
    a.tn = f.in(hTn, nsys);
    a.cj = f.in(hCj, nsys);
    const double* d_scale = f.in(hScale, nsys);
    const double* d_toldel = f.in(hToldel, nsys);
    const double* d_ss = f.in(hSs, nsys);
    const double* d_eps = f.in(hEpsNewt, nsys);
    double* d_dn = f.out<double>(2 * (size_t)nsys);
    int* d_conv = f.out<int>(nsys);
    double* d_sum = f.out<double>(nsys);
    fill_sys_args(c, a, 0);
    const dim3 tg((nsys + 255) / 256), tb(256);
    // iteration m = 0 and its convergence test
    f.launch(IDAHIP_K_NEWTON_ITER, nsys, nullptr, [&] {
        const int rc = launch_newton_iter(c, a.idx, d_scale, d_sum, nullptr, nsys);
        if (!rc) hipLaunchKernelGGL(ctest_kernel<0>, tg, tb, 0, c->stream, (const double*)d_sum, n, d_toldel, d_ss, d_eps, d_dn, d_conv, nsys);
        return rc;
    });
    a.skip = d_conv;
    // NLProblem::sys at the corrected y for the systems that go on (conv == 0)
    f.launch(IDAHIP_K_SYS, 0, nullptr, [&] { return launch_sys(c, a, nsys, nullptr, hTn, hIdx); });
    // iteration m = 1 and its convergence test
    f.launch(IDAHIP_K_NEWTON_ITER, 0, "ctest", [&] {
        const int rc = launch_newton_iter(c, a.idx, d_scale, d_sum, d_conv, nsys);
        if (!rc) hipLaunchKernelGGL(ctest_kernel<1>, tg, tb, 0, c->stream, (const double*)d_sum, n, d_toldel, d_ss, d_eps, d_dn, d_conv, nsys);
        return rc;
    });
    if (!f.fetch()) return f.rc;
    f.copy(hDelnrm, d_dn, 2 * (size_t)nsys);
    f.copy(hConv, d_conv, nsys);
    return 0;
}


int idahip_kind(const idahip_ctx* c) { return c ? (int)c->kind : -1; }

// ------------------------------------------------------------------------------------------------ Krylov ctx (krylov_kernels.hpp)
int idahip_create_krylov(idahip_ctx** out, int device, int n, int batch, idahip_problem kind, void* hip_stream, int maxl) {
    if (!out) return -1;
    *out = nullptr;
    if ((int)kind < 0 || (int)kind >= KIND_COUNT || !kind_facts(kind).krylov) {
        std::fprintf(stderr, "idahip_create_krylov: problem kind %d (IDAHIP_HEAT1D, IDAHIP_BRUSS1D, IDAHIP_LINEAR_DENSE or IDAHIP_HOST_CALLBACK)\n", (int)kind);
        return -2;
    }
    if (n <= TINY_N || n > LU_BIG_MAX_N) {
        std::fprintf(stderr, "idahip_create_krylov: n = %d outside %d < n <= %d\n", n, TINY_N, LU_BIG_MAX_N);
        return -2;
    }
    if (maxl == 0) maxl = idakry::MAXL_DEFAULT;
    if (maxl < 1 || maxl > idakry::MAXL_MAX || maxl > n) {
        std::fprintf(stderr, "idahip_create_krylov: maxl = %d outside 1 <= maxl <= min(%d, n)\n", maxl, idakry::MAXL_MAX);
        return -2;
    }
    return create_ctx(out, device, n, batch, kind, hip_stream, false, 0, 0, maxl);
}

int idahip_krylov(const idahip_ctx* c, int* maxl) {
    if (!c) return -1;
    if (c->krylov && maxl) *maxl = c->kry_maxl;
    return c->krylov;
}

int idahip_set_krylov_fused(idahip_ctx* c, int on) {
    if (!c) return -1;
    if (!c->krylov) return fail(c, -2, "idahip_set_krylov_fused: not a Krylov ctx (idahip_create_krylov)");
    if (on && c->kind == IDAHIP_HOST_CALLBACK) return fail(c, -2, "a host-callback residual runs on the host: the split path only");
    c->kry_fused = on ? 1 : 0;
    return 0;
}

int idahip_krylov_fused(const idahip_ctx* c) { return c ? (c->krylov ? c->kry_fused : 0) : -1; }

int idahip_set_krylov_rounds(idahip_ctx* c, int on) {
    if (!c) return -1;
    if (!c->krylov) return fail(c, -2, "idahip_set_krylov_rounds: not a Krylov ctx (idahip_create_krylov)");
    if (c->kind == IDAHIP_HOST_CALLBACK) return fail(c, -2, "idahip_set_krylov_rounds: a host-callback residual cannot run inside a device round");
    if (on && c->n <= TINY_N) return fail(c, -2, "idahip_set_krylov_rounds: n = %d outside %d < n <= %d", c->n, TINY_N, LU_BIG_MAX_N);
    c->kry_rounds = on ? 1 : 0;
    return 0;
}

int idahip_krylov_rounds(const idahip_ctx* c) { return c ? (c->krylov ? c->kry_rounds : 0) : -1; }

int idahip_krylov_rounds_put_counters(idahip_ctx* c, const int64_t* hNpe, const int64_t* hNps) {
    if (!c) return -1;
    if (!c->krylov) return fail(c, -2, "idahip_krylov_rounds_put_counters: not a Krylov ctx (idahip_create_krylov)");
    if (!hNpe || !hNps) return null_argument(c);
    c->kry_h_npe.assign(hNpe, hNpe + c->batch);
    c->kry_h_nps.assign(hNps, hNps + c->batch);
    return 0;
}

int idahip_krylov_rounds_get_counters(const idahip_ctx* c, int64_t* hNpe, int64_t* hNps) {
    if (!c || !hNpe || !hNps) return -1;
    for (int b = 0; b < c->batch; ++b) {
        hNpe[b] = (size_t)b < c->kry_h_npe.size() ? c->kry_h_npe[b] : 0;
        hNps[b] = (size_t)b < c->kry_h_nps.size() ? c->kry_h_nps[b] : 0;
    }
    return 0;
}

namespace {

// the ctx's part of a solve's arguments; the caller adds the list, the tolerances and where the results go
void fill_kry_args(const idahip_ctx* c, KryArgs& a) {
    a.yy = c->yy; a.yp = c->yp; a.ewt = c->ewt; a.rr = c->savres;
    a.V = c->kry_V; a.st = (idakry::Sys*)c->kry_st; a.stage = c->kry_stage;
    a.delta = c->delta; a.ee = c->ee;
    a.n = c->n; a.maxl = c->kry_maxl;
    a.params = c->params; a.A = c->A; a.Bm = c->B; a.C = c->C;
    a.pab = c->kry_pab; a.ppiv = (const long long*)c->kry_ppiv; a.pml = c->kry_pml; a.pmu = c->kry_pmu;
}

// the solve of the listed systems, fused or split; a.idx / cj / tol / results point into `ap`'s slot, already uploaded
int krylov_launch(idahip_ctx* c, KryArgs& a, const double* hTn, const int32_t* hIdx, int nsys) {
    const int n = c->n;
    fill_kry_args(c, a);
    a.skip = nullptr;
    const bool prec = c->kry_prec != 0;
    const dim3 grid(nsys), blk(KRY_T);
    if (c->kry_fused) {
        if (!launch_krylov_fused<false>(c, a, nsys)) return fail(c, -2, "no fused Krylov kernel for problem kind %d", (int)c->kind);
        return post_launch(c, "krylov_fused");
    }
    if (c->kind == IDAHIP_HOST_CALLBACK && !c->cb_res) return fail(c, -2, "IDAHIP_HOST_CALLBACK: idahip_set_host_residual has not been called");
    const size_t shm1 = kry_lds_bytes(n, 1);
    std::vector<int> done((size_t)nsys, 0);
    auto fetch_done = [&]() -> int {
        IDAHIP_HIP(c, hipMemcpyAsync(done.data(), a.done, sizeof(int) * nsys, hipMemcpyDeviceToHost, c->stream));
        IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
        return 0;
    };
    int rc;
    if (prec) hipLaunchKernelGGL(krylov_begin_kernel<true>, grid, blk, shm1, c->stream, a);
    else hipLaunchKernelGGL(krylov_begin_kernel<false>, grid, blk, shm1, c->stream, a);
    if ((rc = post_launch(c, "krylov_begin"))) return rc;
    if ((rc = fetch_done())) return rc;
    a.skip = a.done;  // a system whose loop has ended is left alone by the launches that follow
    for (int l = 0; l < c->kry_maxl; ++l) {
        bool any = false;
        for (int s = 0; s < nsys; ++s) any = any || done[s] == 0;
        if (!any) break;
        hipLaunchKernelGGL(krylov_point_kernel, grid, blk, 0, c->stream, a, l);
        if (c->kind == IDAHIP_HOST_CALLBACK) {  // the user's residual, exactly as idahip_nls_sys calls it
            const size_t cnt = (size_t)nsys * 3 * n;
            if (c->kry_host.size() < cnt) c->kry_host.resize(cnt);
            double* h = c->kry_host.data();
            IDAHIP_HIP(c, hipMemcpyAsync(h, c->kry_stage, sizeof(double) * cnt, hipMemcpyDeviceToHost, c->stream));
            IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
            for (int s = 0; s < nsys; ++s) {
                if (done[s]) continue;
                double* hs = h + (size_t)s * 3 * n;
                if (c->cb_res(hIdx[s], hTn[s], hs, hs + n, hs + 2 * n, c->cb_user) != 0)
                    return fail(c, -7, "the user's residual function failed for system %d", hIdx[s]);
            }
            IDAHIP_HIP(c, hipMemcpyAsync(c->kry_stage, h, sizeof(double) * cnt, hipMemcpyHostToDevice, c->stream));
        } else if (!with_stencil(c, [&](auto p) {
                       hipLaunchKernelGGL(krylov_res_kernel<decltype(p)::KIND>, grid, blk, 2 * sizeof(double) * n, c->stream, a);
                   })) {
            hipLaunchKernelGGL(krylov_res_kernel<IDAHIP_LINEAR_DENSE>, grid, blk, 2 * sizeof(double) * n, c->stream, a);
        }
        if (prec) hipLaunchKernelGGL(krylov_step_kernel<true>, grid, blk, shm1, c->stream, a, l);
        else hipLaunchKernelGGL(krylov_step_kernel<false>, grid, blk, shm1, c->stream, a, l);
        if ((rc = post_launch(c, "krylov_step"))) return rc;
        if ((rc = fetch_done())) return rc;
    }
    if (prec) hipLaunchKernelGGL(krylov_finish_kernel<true>, grid, blk, shm1, c->stream, a);
    else hipLaunchKernelGGL(krylov_finish_kernel<false>, grid, blk, shm1, c->stream, a);
    return post_launch(c, "krylov_finish");
}

// the staged part of idahip_krylov_solve and idahip_newton_iter_krylov (newton): `f` has passed the refusals
int krylov_call(ListCall& f, bool newton, const double* hTn, const double* hCj, const double* hTol, const double* hB, double* hX,
                double* hDelnrm, int32_t* hNli, int32_t* hFlag, double* hResNorm) {
    if (!f.stage()) return f.rc;
    idahip_ctx* c = f.c;
    const int n = c->n, nsys = f.nsys;
    KryArgs a{};
    a.idx = f.idx;
    a.cj = f.in(hCj, nsys);
    a.tol = f.in(hTol, nsys);
    a.nli = f.out<int>(nsys);
    a.flag = f.out<int>(nsys);
    a.resnorm = f.out<double>(nsys);
    a.nrm = f.out<double>(nsys);
    a.done = f.out<int>(nsys);
    if (!f.send()) return f.rc;
    a.newton = newton ? 1 : 0;
    a.b = c->kry_b;
    a.x = c->kry_x;
    if (!newton) IDAHIP_HIP(c, hipMemcpyAsync(c->kry_b, hB, sizeof(double) * nsys * n, hipMemcpyHostToDevice, c->stream));
    f.launch(newton ? IDAHIP_K_NEWTON_ITER : IDAHIP_K_SOLVE, nsys, nullptr, [&] { return krylov_launch(c, a, hTn, f.hIdx, nsys); });
    if (!f.fetch()) return f.rc;
    if (!newton) {
        IDAHIP_HIP(c, hipMemcpyAsync(hX, c->kry_x, sizeof(double) * nsys * n, hipMemcpyDeviceToHost, c->stream));
        IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    }
    const int* hn = f.host((const int*)a.nli);
    const int* hf = f.host((const int*)a.flag);
    const double* hr = f.host((const double*)a.resnorm);
    const double* hs = f.host((const double*)a.nrm);
    int any = 0, sum = 0;
    double worst = 0.0;
    for (int s = 0; s < nsys; ++s) {
        hNli[s] = hn[s];
        hFlag[s] = hf[s];
        if (hResNorm) hResNorm[s] = hr[s];
        if (newton) hDelnrm[s] = hf[s] == 0 ? sqrt(hs[s] / (double)n) : 0.0;
        if (hf[s] != 0) any = 1;
        sum += hn[s];
        if (hr[s] > worst) worst = hr[s];
    }
    c->kry_last_nli = sum;
    c->kry_last_resnorm = worst;
    return any;
}


// a preconditioned ctx solves only systems that a psetup or an upload has given factors
int krylov_prec_ready(idahip_ctx* c, const char* who, const int32_t* hIdx, int nsys) {
    if (!c->kry_prec) return 0;
    for (int s = 0; s < nsys; ++s)
        if (!c->kry_pready[hIdx[s]])
            return fail(c, -2, "%s: system %d has no preconditioner yet (idahip_krylov_psetup or idahip_krylov_upload_prec first)", who, hIdx[s]);
    return 0;
}

// the four stand-alone preconditioner calls: a Krylov ctx with the mode on
int krylov_prec_on(idahip_ctx* c, const char* who) {
    if (!c->krylov) return fail(c, -2, "%s: not a Krylov ctx (idahip_create_krylov)", who);
    if (!c->kry_prec) return fail(c, -2, "%s: the ctx has no band preconditioner (idahip_set_krylov_band_prec)", who);
    return 0;
}

}  // namespace

int idahip_set_krylov_band_prec(idahip_ctx* c, int ml, int mu) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    if (c->band) return fail(c, -2, "idahip_set_krylov_band_prec on a band ctx: not a Krylov ctx (idahip_create_krylov)");
    if (!c->krylov) return fail(c, -2, "idahip_set_krylov_band_prec on a dense ctx: not a Krylov ctx (idahip_create_krylov)");
    const bool off = ml == -1 && mu == -1;
    if (!off && c->kind == IDAHIP_LINEAR_DENSE)
        return fail(c, -2, "idahip_set_krylov_band_prec: IDAHIP_LINEAR_DENSE has no band difference-quotient Jacobian (IDAHIP_HEAT1D, IDAHIP_BRUSS1D or IDAHIP_HOST_CALLBACK)");
    if (!off && (ml < 0 || mu < 0 || ml >= c->n || mu >= c->n))
        return fail(c, -2, "idahip_set_krylov_band_prec: bandwidths ml = %d, mu = %d outside 0 <= ml, mu < n (-1, -1 turns the mode off)", ml, mu);
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    if (c->kry_pab) (void)hipFree(c->kry_pab);
    if (c->kry_ppiv) (void)hipFree(c->kry_ppiv);
    c->kry_pab = nullptr; c->kry_ppiv = nullptr;
    c->kry_prec = 0; c->kry_pml = c->kry_pmu = c->kry_pldab = 0;
    c->kry_pready.clear();
    if (off) return 0;
    const int ldab = 2 * ml + mu + 1;
    const size_t bn = (size_t)c->batch * c->n;
    if (dalloc(c, &c->kry_pab, bn * ldab) || dalloc(c, &c->kry_ppiv, bn)) {
        if (c->kry_pab) (void)hipFree(c->kry_pab);
        c->kry_pab = nullptr; c->kry_ppiv = nullptr;
        return fail(c, -100, "band preconditioner storage (%zu doubles)", bn * ldab);
    }
    IDAHIP_HIP(c, hipMemsetAsync(c->kry_pab, 0, bn * ldab * sizeof(double), c->stream));
    IDAHIP_HIP(c, hipMemsetAsync(c->kry_ppiv, 0, bn * sizeof(int64_t), c->stream));
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    c->kry_prec = 1; c->kry_pml = ml; c->kry_pmu = mu; c->kry_pldab = ldab;
    c->kry_pready.assign((size_t)c->batch, 0);
    return 0;
}

int idahip_krylov_band_prec(const idahip_ctx* c, int* ml, int* mu) {
    if (!c) return -1;
    if (c->kry_prec) {
        if (ml) *ml = c->kry_pml;
        if (mu) *mu = c->kry_pmu;
    }
    return c->kry_prec;
}

int idahip_krylov_psetup(idahip_ctx* c, const double* hTn, const double* hCj, const double* hHh, int32_t* hInfo, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (f.rc) return f.rc;
    if (int rc = krylov_prec_on(c, "idahip_krylov_psetup")) return rc;
    if (!f.args({hTn, hCj, hHh, hInfo})) return f.rc;
    if (!f.stage()) return f.rc;
    const int n = c->n;
    DqArgs d;
    fill_dq_args(c, d, c->kry_pml, c->kry_pmu, c->kry_pldab);
    d.idx = f.idx; d.cj = f.in(hCj, nsys); d.hh = f.in(hHh, nsys); d.skip = nullptr;
    d.out = c->kry_pab; d.compact = 0;
    f.launch(IDAHIP_K_JAC, nsys, nullptr, [&] {
        if (c->kind == IDAHIP_HOST_CALLBACK) return callback_dq_jac(c, d, hTn, hIdx, nsys);
        return launch_band_dq(c, d, nsys, "band DQ jac (preconditioner)");  // (idahip_set_krylov_band_prec: the stencil problems are the device kinds)
    });
    f.launch(IDAHIP_K_LU, nsys, nullptr, [&] { return band_factor(c, c->kry_pab, (long)c->kry_pldab * n, c->kry_ppiv, n, c->kry_pml, c->kry_pmu, f.idx, nsys); });
    const int rc = f.rc ? f.rc : report_info(c, hIdx, nsys, hInfo);
    for (int s = 0; s < nsys && rc >= 0; ++s) c->kry_pready[hIdx[s]] = 1;
    return rc;
}

int idahip_krylov_psolve(idahip_ctx* c, const double* hR, double* hZ, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (f.rc) return f.rc;
    if (int rc = krylov_prec_on(c, "idahip_krylov_psolve")) return rc;
    if (!f.args({hR, hZ})) return f.rc;
    if (int rc = krylov_prec_ready(c, "idahip_krylov_psolve", hIdx, nsys)) return rc;
    if (!f.stage()) return f.rc;
    if (!f.send()) return f.rc;
    const int n = c->n;
    IDAHIP_HIP(c, hipMemcpyAsync(c->kry_b, hR, sizeof(double) * nsys * n, hipMemcpyHostToDevice, c->stream));
    f.launch(IDAHIP_K_SOLVE, nsys, "krylov_psolve", [&] {
        hipLaunchKernelGGL(krylov_psolve_kernel, dim3(nsys), dim3(KRY_T), sizeof(double) * n, c->stream, (const double*)c->kry_pab,
                           (const long long*)c->kry_ppiv, n, c->kry_pml, c->kry_pmu, (const double*)c->kry_b, c->kry_x, f.idx);
    });
    if (f.rc) return f.rc;
    IDAHIP_HIP(c, hipMemcpyAsync(hZ, c->kry_x, sizeof(double) * nsys * n, hipMemcpyDeviceToHost, c->stream));
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    return f.done();
}


int idahip_krylov_download_prec(idahip_ctx* c, int sys, double* hAB, int64_t* hPiv) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    int rc = krylov_prec_on(c, "idahip_krylov_download_prec");
    if (rc) return rc;
    if (sys < 0 || sys >= c->batch) return fail(c, -2, "system out of range");
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    const size_t ne = (size_t)c->kry_pldab * c->n;
    if (hAB) IDAHIP_HIP(c, hipMemcpy(hAB, c->kry_pab + sys * ne, sizeof(double) * ne, hipMemcpyDeviceToHost));
    if (hPiv) IDAHIP_HIP(c, hipMemcpy(hPiv, c->kry_ppiv + (size_t)sys * c->n, sizeof(int64_t) * c->n, hipMemcpyDeviceToHost));
    return 0;
}

int idahip_krylov_upload_prec(idahip_ctx* c, int sys, const double* hAB, const int64_t* hPiv) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    int rc = krylov_prec_on(c, "idahip_krylov_upload_prec");
    if (rc) return rc;
    if (sys < 0 || sys >= c->batch) return fail(c, -2, "system out of range");
    if (!hAB || !hPiv) return null_argument(c);
    const int n = c->n;
    for (int j = 0; j < n; ++j) {  // the solves index the vector by the pivots: dgbtrf's range, or nothing is uploaded
        const int64_t hi = std::min<int64_t>((int64_t)n - 1, (int64_t)j + c->kry_pml);
        if (hPiv[j] < j || hPiv[j] > hi) return fail(c, -2, "pivot %lld of column %d outside [%d, %lld]", (long long)hPiv[j], j, j, (long long)hi);
    }
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    const size_t ne = (size_t)c->kry_pldab * n;
    IDAHIP_HIP(c, hipMemcpy(c->kry_pab + sys * ne, hAB, sizeof(double) * ne, hipMemcpyHostToDevice));
    IDAHIP_HIP(c, hipMemcpy(c->kry_ppiv + (size_t)sys * n, hPiv, sizeof(int64_t) * n, hipMemcpyHostToDevice));
    c->kry_pready[sys] = 1;
    return 0;
}

int idahip_krylov_solve(idahip_ctx* c, const double* hTn, const double* hCj, const double* hTol, const double* hB, double* hX, int32_t* hNli,
                        int32_t* hFlag, double* hResNorm, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (f.rc) return f.rc;
    if (!c->krylov) return fail(c, -2, "idahip_krylov_solve: not a Krylov ctx (idahip_create_krylov)");
    if (!f.args({hTn, hCj, hTol, hB, hX, hNli, hFlag, hResNorm})) return f.rc;
    if (int rc = krylov_prec_ready(c, "idahip_krylov_solve", hIdx, nsys)) return rc;
    return krylov_call(f, false, hTn, hCj, hTol, hB, hX, nullptr, hNli, hFlag, hResNorm);
}

int idahip_newton_iter_krylov(idahip_ctx* c, const double* hTn, const double* hCj, const double* hEpsNewt, double* hDelnrm, int32_t* hNli,
                              int32_t* hFlag, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (f.rc) return f.rc;
    if (!c->krylov) return fail(c, -2, "idahip_newton_iter_krylov: not a Krylov ctx (idahip_create_krylov)");
    if (!f.args({hTn, hCj, hEpsNewt, hDelnrm, hNli, hFlag})) return f.rc;
    if (int rc = krylov_prec_ready(c, "idahip_newton_iter_krylov", hIdx, nsys)) return rc;
    std::vector<double> tol((size_t)nsys);
    for (int s = 0; s < nsys; ++s) tol[s] = idakry::tolerance(c->n, hEpsNewt[s]);
    return krylov_call(f, true, hTn, hCj, tol.data(), nullptr, nullptr, hDelnrm, hNli, hFlag, nullptr);
}

// ------------------------------------------------------------------------------------------------ stepper vector ops
int idahip_init_first(idahip_ctx* c, double* hYpnorm, double* hPhi0Nrm, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hYpnorm, hPhi0Nrm})) return f.rc;
    if (int rc = missing_id(c, "idahip_init_first")) return rc;
    if (!f.stage()) return f.rc;
    double* d_out = f.out<double>(2 * (size_t)nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "init_first", [&] {
        hipLaunchKernelGGL(init_first_kernel, dim3(nsys), dim3(256), 2 * sizeof(double) * c->n, c->stream, vec_state(c), f.idx, d_out);
    });
    if (!f.fetch()) return f.rc;
    f.rms(hYpnorm, d_out, nsys, 2);
    f.rms(hPhi0Nrm, d_out + 1, nsys, 2);
    return 0;
}

int idahip_scale_phi1(idahip_ctx* c, const double* hFac, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hFac})) return f.rc;
    if (!f.stage()) return f.rc;
    const double* d_fac = f.in(hFac, nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "scale_phi1", [&] {
        hipLaunchKernelGGL(scale_phi1_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), f.idx, d_fac);
    });
    return f.done();
}

int idahip_predict(idahip_ctx* c, const int32_t* hKkNs, const double* hBeta, const double* hGamma, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hKkNs, hBeta, hGamma})) return f.rc;
    if (int rc = check_kk_ns(c, hKkNs, nsys)) return rc;
    if (!f.stage()) return f.rc;
    const int* d_kkns = f.in(hKkNs, 2 * (size_t)nsys);
    const double* d_beta = f.in(hBeta, (size_t)MXORDP1 * nsys);
    const double* d_gamma = f.in(hGamma, (size_t)MXORDP1 * nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "predict", [&] {
        hipLaunchKernelGGL(predict_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), f.idx, d_kkns, d_beta, d_gamma);
    });
    return f.done();
}

int idahip_post_newton(idahip_ctx* c, const double* hCj, const int32_t* hKk, double* hNorms, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hCj, hKk, hNorms})) return f.rc;
    if (int rc = missing_id(c, "idahip_post_newton")) return rc;
    if (int rc = check_order(c, "kk", hKk, nsys)) return rc;
    if (!f.stage()) return f.rc;
    const double* d_cj = f.in(hCj, nsys);
    const int* d_kk = f.in(hKk, nsys);
    double* d_out = f.out<double>(4 * (size_t)nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "post_newton", [&] {
        hipLaunchKernelGGL(post_newton_kernel, dim3(nsys), dim3(256), 4 * sizeof(double) * c->n, c->stream, vec_state(c), f.idx, d_cj, d_kk, d_out);
    });
    if (!f.fetch()) return f.rc;
    f.rms(hNorms, d_out, 4 * (size_t)nsys);
    return 0;
}

int idahip_post_newton_constr(idahip_ctx* c, const double* hCj, const int32_t* hKk, const double* hEpsNewt, const int32_t* hCheck,
                              double* hNorms, int32_t* hFlag, double* hRr, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hCj, hKk, hEpsNewt, hCheck, hNorms, hFlag, hRr})) return f.rc;
    if (int rc = missing_id(c, "idahip_post_newton_constr")) return rc;
    if (c->h_constr.empty()) return fail(c, -2, "idahip_post_newton_constr on a ctx without constraints (idahip_set_constraints)");
    if (int rc = check_order(c, "kk", hKk, nsys)) return rc;
    if (!f.stage()) return f.rc;
    const double* d_cj = f.in(hCj, nsys);
    const int* d_kk = f.in(hKk, nsys);
    const double* d_eps = f.in(hEpsNewt, nsys);
    const int* d_chk = f.in(hCheck, nsys);
    double* d_out = f.out<double>(4 * (size_t)nsys);
    double* d_rr = f.out<double>((size_t)nsys);
    int* d_flag = f.out<int>((size_t)nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "post_newton_constr", [&] {
        hipLaunchKernelGGL(post_newton_constr_kernel, dim3(nsys), dim3(256), 4 * sizeof(double) * c->n, c->stream, vec_state(c),
                           (const double*)c->d_constr, f.idx, d_cj, d_kk, d_eps, d_chk, d_out, d_flag, d_rr);
    });
    if (!f.fetch()) return f.rc;
    f.rms(hNorms, d_out, 4 * (size_t)nsys);
    f.copy(hFlag, d_flag, nsys);
    f.copy(hRr, d_rr, nsys);
    return 0;
}

int idahip_constr_check(idahip_ctx* c, idahip_field field, int32_t* hViolated, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hViolated})) return f.rc;
    if (c->h_constr.empty()) return fail(c, -2, "idahip_constr_check on a ctx without constraints (idahip_set_constraints)");
    const double* x = field_ptr(c, field);
    if (!x) return fail(c, -2, "unknown field %d", (int)field);
    if (!f.stage()) return f.rc;
    int* d_v = f.out<int>((size_t)nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "constr_check", [&] {
        hipLaunchKernelGGL(constr_check_kernel, dim3(nsys), dim3(256), 0, c->stream, x, (const double*)c->d_constr, c->n, f.idx, d_v);
    });
    if (!f.fetch()) return f.rc;
    f.copy(hViolated, d_v, nsys);
    return 0;
}

int idahip_restore(idahip_ctx* c, const int32_t* hKkNs, const double* hCvals, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hKkNs, hCvals})) return f.rc;
    if (int rc = check_kk_ns(c, hKkNs, nsys)) return rc;
    if (!f.stage()) return f.rc;
    const int* d_kkns = f.in(hKkNs, 2 * (size_t)nsys);
    const double* d_cv = f.in(hCvals, (size_t)MXORDP1 * nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "restore", [&] {
        hipLaunchKernelGGL(restore_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), f.idx, d_kkns, d_cv);
    });
    return f.done();
}

int idahip_complete_step(idahip_ctx* c, const int32_t* hKused, const double* hCk, int maxord, double* hPhi0Nrm, int32_t* hEwtBad,
                         const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hKused, hCk, hPhi0Nrm, hEwtBad})) return f.rc;
    if (int rc = missing_id(c, "idahip_complete_step")) return rc;
    if (maxord < 1 || maxord > 5) return fail(c, -2, "bad maxord");
    if (int rc = check_order(c, "kused", hKused, nsys, maxord)) return rc;
    if (!f.stage()) return f.rc;
    const int* d_ku = f.in(hKused, nsys);
    const double* d_ck = f.in(hCk, nsys);
    double* d_out = f.out<double>(nsys);
    int* d_bad = f.out<int>(nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "complete_step", [&] {
        hipLaunchKernelGGL(complete_step_kernel, dim3(nsys), dim3(256), sizeof(double) * c->n, c->stream, vec_state(c), f.idx, d_ku, d_ck, maxord,
                           d_out, d_bad);
    });
    if (!f.fetch()) return f.rc;
    f.rms(hPhi0Nrm, d_out, nsys);
    f.copy(hEwtBad, d_bad, nsys);
    return 0;
}

int idahip_get_solution(idahip_ctx* c, const int32_t* hKord, const double* hCvals, const double* hDvals, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hKord, hCvals, hDvals})) return f.rc;
    if (int rc = check_order(c, "kord", hKord, nsys)) return rc;
    if (!f.stage()) return f.rc;
    const int* d_ko = f.in(hKord, nsys);
    const double* d_cv = f.in(hCvals, (size_t)MXORDP1 * nsys);
    const double* d_dv = f.in(hDvals, (size_t)5 * nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "get_solution", [&] {
        hipLaunchKernelGGL(get_solution_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), f.idx, d_ko, d_cv, d_dv);
    });
    return f.done();
}

int idahip_get_dky(idahip_ctx* c, const int32_t* hKfirst, const int32_t* hKlast, const double* hCjk, double* hOut, const int32_t* hIdx,
                   int nsys) {
    ListCall f(c, hIdx, nsys);
    if (!f.args({hKfirst, hKlast, hCjk, hOut})) return f.rc;
    for (int s = 0; s < nsys; ++s)
        if (hKfirst[s] < 0 || hKfirst[s] > hKlast[s] || hKlast[s] >= MXORDP1) return fail(c, -2, "bad derivative range at list position %d", s);
    if (!f.stage()) return f.rc;
    if (!c->dky)
        if (int rc = dalloc(c, &c->dky, (size_t)c->batch * c->n)) return rc;
    const int* d_k0 = f.in(hKfirst, nsys);
    const int* d_k1 = f.in(hKlast, nsys);
    const double* d_c = f.in(hCjk, (size_t)MXORDP1 * nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "get_dky", [&] {
        hipLaunchKernelGGL(get_dky_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), f.idx, d_k0, d_k1, d_c, c->dky);
    });
    if (f.rc) return f.rc;  // the results come through ctx->dky, not the slot, and the copy below waits for the stream
    IDAHIP_HIP(c, hipMemcpyAsync(hOut, c->dky, sizeof(double) * (size_t)nsys * c->n, hipMemcpyDeviceToHost, c->stream));
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}


int idahip_snapshot_initial(idahip_ctx* c) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    const size_t bn = (size_t)c->batch * c->n;
    int rc = 0;
    if (!c->ic_y) {
        rc |= dalloc(c, &c->ic_y, bn);
        rc |= dalloc(c, &c->ic_yp, bn);
        if (rc) return fail(c, -4, "device allocation of the initial-condition copies failed");
    }
    IDAHIP_HIP(c, hipMemcpyAsync(c->ic_y, c->phi, bn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    IDAHIP_HIP(c, hipMemcpyAsync(c->ic_yp, c->phi + bn, bn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int idahip_restore_initial(idahip_ctx* c, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys);
    if (f.rc) return f.rc;
    if (!c->ic_y) return fail(c, -2, "idahip_restore_initial before idahip_snapshot_initial");
    if (!f.stage()) return f.rc;
    f.launch(IDAHIP_K_VECTOR, nsys, "restore_initial", [&] {
        hipLaunchKernelGGL(restore_initial_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), (const double*)c->ic_y,
                           (const double*)c->ic_yp, f.idx);
    });
    return f.done();
}

int idahip_reinit(idahip_ctx* c, const int32_t* hIdx, int nsys, const double* hYY0, const double* hYP0, int add) {
    ListCall f(c, hIdx, nsys);
    if (f.rc) return f.rc;
    if (!add && !f.args({hYY0, hYP0})) return f.rc;
    if (!f.stage()) return f.rc;
    // the packed rows: one copy per array into the ctx's staging buffer, which grows to the largest list seen
    const size_t rows = (size_t)nsys * c->n;
    if ((hYY0 || hYP0) && c->reinit_cap < 2 * rows) {
        IDAHIP_HIP(c, hipStreamSynchronize(c->stream));  // an earlier call's kernel may still read the old buffer
        if (c->reinit_stage) (void)hipFree(c->reinit_stage);
        c->reinit_cap = 0;
        if (int rc = dalloc(c, &c->reinit_stage, 2 * rows)) return rc;
        c->reinit_cap = 2 * rows;
    }
    const double* d_y = hYY0 ? c->reinit_stage : nullptr;
    const double* d_yp = hYP0 ? c->reinit_stage + rows : nullptr;
    if (hYY0) IDAHIP_HIP(c, hipMemcpyAsync(c->reinit_stage, hYY0, rows * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (hYP0) IDAHIP_HIP(c, hipMemcpyAsync(c->reinit_stage + rows, hYP0, rows * sizeof(double), hipMemcpyHostToDevice, c->stream));
    f.launch(IDAHIP_K_VECTOR, nsys, "reinit", [&] {
        hipLaunchKernelGGL(reinit_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), f.idx, d_y, d_yp, add ? 1 : 0, c->ic_y, c->ic_yp);
    });
    if (f.rc) return f.rc;
    // what a created system starts without and the ctx holds outside the controller record: the lock-step rounds' npe / nps of a
    // Krylov ctx, and the mark that the band preconditioner has factors for the system
    for (int s = 0; s < nsys; ++s) {
        const size_t b = (size_t)hIdx[s];
        if (b < c->kry_h_npe.size()) c->kry_h_npe[b] = 0;
        if (b < c->kry_h_nps.size()) c->kry_h_nps[b] = 0;
        if (b < c->kry_pready.size()) c->kry_pready[b] = 0;
    }
    return f.done();
}


// ------------------------------------------------------------------------------------------------ consistent initial conditions
// (ic_kernels.hpp; driven by idaens_calc_ic)
namespace {

IcVecs ic_vecs(idahip_ctx* c) {
    const size_t bn = (size_t)c->batch * c->n;
    IcVecs v;
    v.y0 = c->phi + 2 * bn; v.yp0 = c->phi + 3 * bn; v.delnew = c->phi + 4 * bn; v.savres = c->savres;
    return v;
}

// the residual kernels' IC front end: lambda == nullptr: the residual at the iterate into delta and savres; else the residual at
// the trial point into delnew and savres
void fill_ic_args(idahip_ctx* c, SysArgsIC& a, const double* d_lambda, int icopt) {
    const IcVecs v = ic_vecs(c);
    a.yypredict = v.y0; a.yppredict = v.yp0; a.yy = c->yy; a.yp = c->yp; a.ee = nullptr;
    a.delta = d_lambda ? v.delnew : c->delta;
    a.savres = c->savres; a.n = c->n; a.reset_ee = 0;
    a.dir = c->delta; a.lambda = d_lambda;
    a.id = (icopt == IDAHIP_IC_YA_YDP) ? c->d_id : nullptr;
}

// the maps of the ctx's staged factors for the IC solves (ic_solve_body), null where the factors are in the reference layout
const unsigned short* staged_ord(const idahip_ctx* c) { return lu_staged_on(c) ? (const unsigned short*)c->lu_ord : nullptr; }

// delta-like vector x <- J^-1 x with the ctx's factors, d_out[s] = sum (x_i ewt_i)^2
int launch_ic_solve(idahip_ctx* c, double* x, const int* d_idx, double* d_out, int nsys) {
    const int n = c->n;
    if (c->band) {
        const int spw = band_spw(c, nsys);
        const dim3 grid((nsys + spw - 1) / spw), blk(spw);
        if (c->ml == 1 && c->mu == 1)
            hipLaunchKernelGGL((ic_band_solve_kernel<1, 1>), grid, blk, 0, c->stream, (const double*)c->bab, (const long long*)c->piv, c->ml, c->mu, x,
                               (const double*)c->ewt, n, d_idx, nsys, d_out);
        else
            hipLaunchKernelGGL((ic_band_solve_kernel<-1, -1>), grid, blk, 0, c->stream, (const double*)c->bab, (const long long*)c->piv, c->ml, c->mu, x,
                               (const double*)c->ewt, n, d_idx, nsys, d_out);
    } else if (n <= TINY_N) {
        hipLaunchKernelGGL(ic_tiny_solve_kernel, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, (const double*)c->lu, (const long long*)c->piv, x,
                           (const double*)c->ewt, n, d_idx, nsys, d_out);
    } else if (n % 2 == 0) {
        hipLaunchKernelGGL(ic_solve_kernel<2>, dim3(nsys), dim3(256), 2 * sizeof(double) * n, c->stream, (const double*)c->lu, (const int*)c->perm, x,
                           (const double*)c->ewt, n, d_idx, d_out, staged_ord(c));
    } else {
        hipLaunchKernelGGL(ic_solve_kernel<1>, dim3(nsys), dim3(256), 2 * sizeof(double) * n, c->stream, (const double*)c->lu, (const int*)c->perm, x,
                           (const double*)c->ewt, n, d_idx, d_out, staged_ord(c));
    }
    return post_launch(c, "ic_solve");
}

// can the residual kernel of this ctx also solve (SysArgsIC::lu)? The built-in problems on a dense ctx
bool ic_fusable(const idahip_ctx* c) {
    if (c->band || c->kind == IDAHIP_HOST_CALLBACK) return false;
    // (a mass-action ctx in the wave-per-system layout has no workgroup of its own to solve with: residual and solve are two launches)
    if (c->kind == IDAHIP_MASS_ACTION) return c->n > MA_WAVE_MAX_N || (c->ma_force_wg && c->n > TINY_N);
    return c->n > TINY_N || c->kind == IDAHIP_ROBERTS || c->kind == IDAHIP_LORENZ63;
}

// the residual at the point the front end forms; with a.lu set (ic_fusable), the solve and the norm as well
int launch_ic_sys(idahip_ctx* c, const SysArgsIC& a, int nsys, const double* hTn, const int32_t* hIdx) {
    const int n = c->n;
    switch (c->kind) {
        case IDAHIP_HOST_CALLBACK:
            return callback_sys(c, a, hTn, hIdx, nsys, &a);
        case IDAHIP_ROBERTS:
            hipLaunchKernelGGL(ic_tiny_sys_kernel<IDAHIP_ROBERTS>, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, a, (const double*)nullptr, 0, nsys);
            break;
        case IDAHIP_LORENZ63:
            hipLaunchKernelGGL(ic_tiny_sys_kernel<IDAHIP_LORENZ63>, dim3((nsys + 63) / 64), dim3(64), 0, c->stream, a, (const double*)c->params, 3, nsys);
            break;
        case IDAHIP_LINEAR_DENSE: {
            const size_t shm = 2 * sizeof(double) * n;
            const double *A = c->A, *B = c->B, *C = c->C;
            if (n % 2 == 0) hipLaunchKernelGGL((linear_sys_kernel<2, false, SysArgsIC>), dim3(nsys), dim3(256), shm, c->stream, a, A, B, C, (double*)nullptr);
            else hipLaunchKernelGGL((linear_sys_kernel<1, false, SysArgsIC>), dim3(nsys), dim3(256), shm, c->stream, a, A, B, C, (double*)nullptr);
            break;
        }
        case IDAHIP_MASS_ACTION:
            if (int rc = ma_unset(c, "ic_res")) return rc;
            launch_ma_sys(c, a, nsys);
            break;
        default: {
            const size_t shm = (a.lu ? 2 : 1) * sizeof(double) * n;
            if (!with_stencil(c, [&](auto p) {
                    using P = decltype(p);
                    if (n % 2 == 0) hipLaunchKernelGGL((ic_stencil_sys_kernel<P, 2>), dim3(nsys), dim3(256), shm, c->stream, a, (const double*)c->params);
                    else hipLaunchKernelGGL((ic_stencil_sys_kernel<P, 1>), dim3(nsys), dim3(256), shm, c->stream, a, (const double*)c->params);
                }))
                return no_kernel(c, "IC residual");
            break;
        }
    }
    return post_launch(c, "ic_res");
}

int ic_check_opt(idahip_ctx* c, int icopt) {
    if (icopt != IDAHIP_IC_YA_YDP && icopt != IDAHIP_IC_Y) return fail(c, -2, "unknown icopt %d", icopt);
    if (icopt == IDAHIP_IC_YA_YDP && c->h_id.empty()) return fail(c, -2, "IDAHIP_IC_YA_YDP needs the id vector (idahip_set_id)");
    return 0;
}

// setup at the iterate, the staged part of idahip_ic_setup and idahip_ic_setup_dq (hHh != nullptr): `f` has passed the refusals
int ic_setup(ListCall& f, const double* hTn, const double* hCj, const double* hHh, int32_t* hInfo) {
    if (!f.stage()) return f.rc;
    idahip_ctx* c = f.c;
    const int nsys = f.nsys;
    const double* d_cj = f.in(hCj, nsys);
    const double* d_hh = hHh ? f.in(hHh, nsys) : nullptr;
    f.launch(IDAHIP_K_VECTOR, nsys, "ic_point", [&] {
        hipLaunchKernelGGL(ic_point_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), ic_vecs(c), f.idx);
    });
    double* work = (c->n <= TINY_N) ? c->lu : c->jw;
    f.launch(IDAHIP_K_JAC, nsys, nullptr, [&] { return launch_jac(c, work, f.idx, d_cj, nsys, hTn, hCj, f.hIdx, nullptr, d_hh); });
    return factor_and_report(f, work, hInfo);
}

}  // namespace

int idahip_ic_begin(idahip_ctx* c, double* hYpnorm, int32_t* hEwtBad, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_ic_begin");
    if (!f.args({hYpnorm, hEwtBad})) return f.rc;
    if (!f.stage()) return f.rc;
    double* d_out = f.out<double>(nsys);
    int* d_bad = f.out<int>(nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "ic_begin", [&] {
        hipLaunchKernelGGL(ic_begin_kernel, dim3(nsys), dim3(256), sizeof(double) * c->n, c->stream, vec_state(c), ic_vecs(c), f.idx, d_out, d_bad);
    });
    if (!f.fetch()) return f.rc;
    f.rms(hYpnorm, d_out, nsys);
    f.copy(hEwtBad, d_bad, nsys);
    return 0;
}

int idahip_ic_reset(idahip_ctx* c, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_ic_reset");
    if (!f.stage()) return f.rc;
    f.launch(IDAHIP_K_VECTOR, nsys, "ic_reset", [&] {
        hipLaunchKernelGGL(ic_reset_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), ic_vecs(c), f.idx);
    });
    return f.done();
}

int idahip_ic_res(idahip_ctx* c, const double* hTn, const double* hCj, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_ic_res");
    if (!f.args({hTn, hCj})) return f.rc;
    if (int rcu = ma_unset(c, "idahip_ic_res")) return rcu;
    if (!f.stage()) return f.rc;
    SysArgsIC a;
    a.idx = f.idx;
    a.tn = f.in(hTn, nsys);
    a.cj = f.in(hCj, nsys);
    fill_ic_args(c, a, nullptr, IDAHIP_IC_Y);
    f.launch(IDAHIP_K_SYS, nsys, nullptr, [&] { return launch_ic_sys(c, a, nsys, hTn, hIdx); });
    return f.done();
}

int idahip_ic_setup(idahip_ctx* c, const double* hTn, const double* hCj, int32_t* hInfo, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_ic_setup");
    if (!f.args({hTn, hCj, hInfo})) return f.rc;
    if (int rcu = ma_unset(c, "idahip_ic_setup")) return rcu;
    if (c->jac_dq) return fail(c, -2, "a DQ ctx forms its Jacobians with the step sizes: idahip_ic_setup_dq");
    return ic_setup(f, hTn, hCj, nullptr, hInfo);
}

int idahip_ic_setup_dq(idahip_ctx* c, const double* hTn, const double* hCj, const double* hHh, int32_t* hInfo, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_ic_setup_dq");
    if (!f.args({hTn, hCj, hHh, hInfo})) return f.rc;
    if (int rcu = ma_unset(c, "idahip_ic_setup_dq")) return rcu;
    if (!c->jac_dq) return fail(c, -2, "idahip_ic_setup_dq on a ctx with analytic Jacobians (idahip_set_jacobian_dq)");
    return ic_setup(f, hTn, hCj, hHh, hInfo);
}

int idahip_ic_solve(idahip_ctx* c, double* hFnorm, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_ic_solve");
    if (!f.args({hFnorm})) return f.rc;
    if (!f.stage()) return f.rc;
    double* d_out = f.out<double>(nsys);
    f.launch(IDAHIP_K_SOLVE, nsys, nullptr, [&] { return launch_ic_solve(c, c->delta, f.idx, d_out, nsys); });
    if (!f.fetch()) return f.rc;
    f.rms(hFnorm, d_out, nsys);
    return 0;
}

int idahip_ic_trial(idahip_ctx* c, int icopt, const double* hTn, const double* hCj, const double* hLambda, double* hFnormp,
                    const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_ic_trial");
    if (!f.args({hTn, hCj, hLambda, hFnormp})) return f.rc;
    if (int rcu = ma_unset(c, "idahip_ic_trial")) return rcu;
    if (int rc = ic_check_opt(c, icopt)) return rc;
    if (!f.stage()) return f.rc;
    SysArgsIC a;
    a.idx = f.idx;
    a.tn = f.in(hTn, nsys);
    a.cj = f.in(hCj, nsys);
    const double* d_lambda = f.in(hLambda, nsys);
    double* d_out = f.out<double>(nsys);
    fill_ic_args(c, a, d_lambda, icopt);
    const bool fused = ic_fusable(c);
    if (fused) {
        a.lu = c->lu; a.perm = c->perm; a.ord = staged_ord(c); a.piv = (const long long*)c->piv; a.ewt = c->ewt; a.out = d_out;
    }
    f.launch(IDAHIP_K_SYS, nsys, nullptr, [&] { return launch_ic_sys(c, a, nsys, hTn, hIdx); });
    if (!fused) f.launch(IDAHIP_K_SOLVE, nsys, nullptr, [&] { return launch_ic_solve(c, a.delta, a.idx, d_out, nsys); });
    if (!f.fetch()) return f.rc;
    f.rms(hFnormp, d_out, nsys);
    return 0;
}

int idahip_ic_accept(idahip_ctx* c, int icopt, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_ic_accept");
    if (f.rc) return f.rc;
    if (icopt != IDAHIP_IC_YA_YDP && icopt != IDAHIP_IC_Y) return fail(c, -2, "unknown icopt %d", icopt);
    if (!f.stage()) return f.rc;
    f.launch(IDAHIP_K_VECTOR, nsys, "ic_accept", [&] {
        hipLaunchKernelGGL(ic_accept_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), ic_vecs(c), icopt == IDAHIP_IC_YA_YDP ? 1 : 0, f.idx);
    });
    return f.done();
}

int idahip_ic_commit(idahip_ctx* c, int32_t* hEwtBad, const int32_t* hIdx, int nsys) {
    ListCall f(c, hIdx, nsys, "idahip_ic_commit");
    if (!f.args({hEwtBad})) return f.rc;
    if (!f.stage()) return f.rc;
    int* d_bad = f.out<int>(nsys);
    f.launch(IDAHIP_K_VECTOR, nsys, "ic_commit", [&] {
        hipLaunchKernelGGL(ic_commit_kernel, dim3(nsys), dim3(256), 0, c->stream, vec_state(c), ic_vecs(c), f.idx, d_bad);
    });
    if (!f.fetch()) return f.rc;
    f.copy(hEwtBad, d_bad, nsys);
    return 0;
}


// ---------------------------------------------------------------------------------------------- device-resident stepper (n <= 8)
__global__ void pow_batch_kernel(const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ out, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = glibc_pow::pow(x[i], y[i]);
}

int idahip_pow_batch(idahip_ctx* c, const double* hX, const double* hY, double* hOut, size_t count) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    if (!hX || !hY || !hOut) return null_argument(c);
    if (count == 0) return 0;
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    int rc = dalloc(c, &dx, count);
    if (!rc) rc = dalloc(c, &dy, count);
    if (!rc) rc = dalloc(c, &dout, count);
    if (!rc) {
        hipError_t e = hipMemcpyAsync(dx, hX, count * sizeof(double), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dy, hY, count * sizeof(double), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(pow_batch_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, (const double*)dx,
                               (const double*)dy, dout, count);
            e = hipMemcpyAsync(hOut, dout, count * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, -100, "idahip_pow_batch: %s", hipGetErrorString(e));
    }
    if (dx) (void)hipFree(dx);
    if (dy) (void)hipFree(dy);
    if (dout) (void)hipFree(dout);
    return rc;
}

static int stepper_buffers(idahip_ctx* c, const idahip_tiny_call* call, bool outputs);

// the schedule and the limits of a stepper call as the device-resident steppers take them (touts and start rounds already on
// the device)
static FlowArgs flow_args(idahip_ctx* c, const idahip_tiny_call* call) {
    FlowArgs f;
    f.touts = c->tiny_touts; f.ntout = call->ntout; f.recycle = call->recycle; f.resume = call->resume;
    f.mxstep = call->mxstep; f.maxord = call->maxord; f.maxnef = call->maxnef; f.maxncf = call->maxncf;
    f.epcon = call->epcon; f.hmax_inv = call->hmax_inv; f.t0 = call->t0;
    f.start_round = call->start_round ? (const long long*)c->tiny_start : nullptr;
    f.acc = (unsigned long long*)c->tiny_acc;
    f.batch = c->batch;
    f.nrt = call->nroots;
    for (int i = 0; i < call->nroots && i < IDAHIP_MAX_ROOTS; ++i) {
        f.rt_comp[i] = call->root_comps[i];
        f.rt_thr[i] = call->root_thresholds[i];
    }
    return f;
}

// What idahip_tiny_solve and idahip_round_solve share around their launches. stepper_call_args: the refusals that come before an
// entry point's own (extra: a further pointer it needs). stepper_call_begin: the refusals that come after them, the buffers, and the
// four uploads (records, touts, start rounds, accumulator reset). stepper_call_end: the six downloads, left on the stream.
static int stepper_call_args(idahip_ctx* c, const void* hSys, size_t sys_bytes, const idahip_tiny_call* call, const void* hRoundsDone, const void* hAcc,
                             const void* extra) {
    if (!hSys || !call || !hRoundsDone || !hAcc || !extra || !call->touts || call->ntout < 1) return null_argument(c);
    if (sys_bytes != sizeof(idactl::SysCore)) return fail(c, -2, "controller state of %zu bytes, this library expects %zu", sys_bytes, sizeof(idactl::SysCore));
    return 0;
}
static int stepper_call_begin(idahip_ctx* c, const char* who, const void* hSys, const idahip_tiny_call* call, bool outputs) {
    if (const int rcm = missing_id(c, who)) return rcm;
    if (call->recycle && (!c->ic_y || !c->ic_yp)) return fail(c, -2, "recycle needs idahip_snapshot_initial");
    if (call->recycle && call->max_rounds < 1) return fail(c, -2, "recycle needs a round limit");
    if (const int rc = stepper_buffers(c, call, outputs)) return rc;
    const int batch = c->batch;
    IDAHIP_HIP(c, hipMemcpyAsync(c->tiny_sys, hSys, (size_t)batch * sizeof(idactl::SysCore), hipMemcpyHostToDevice, c->stream));
    IDAHIP_HIP(c, hipMemcpyAsync(c->tiny_touts, call->touts, sizeof(double) * call->ntout, hipMemcpyHostToDevice, c->stream));
    if (call->start_round)
        IDAHIP_HIP(c, hipMemcpyAsync(c->tiny_start, call->start_round, sizeof(int64_t) * batch, hipMemcpyHostToDevice, c->stream));
    IDAHIP_HIP(c, hipMemsetAsync(c->tiny_acc, 0, 2 * sizeof(uint64_t), c->stream));
    return 0;
}
static int stepper_call_end(idahip_ctx* c, void* hSys, const idahip_tiny_call* call, int64_t* hRoundsDone, uint64_t* hAcc, double* hYout, double* hYPout) {
    const int batch = c->batch;
    const size_t ysz = (size_t)call->ntout * batch * c->n;
    IDAHIP_HIP(c, hipMemcpyAsync(hSys, c->tiny_sys, (size_t)batch * sizeof(idactl::SysCore), hipMemcpyDeviceToHost, c->stream));
    if (call->nroots > 0)
        IDAHIP_HIP(c, hipMemcpyAsync(call->root_states, c->tiny_roots, (size_t)batch * sizeof(idahip_root_state), hipMemcpyDeviceToHost, c->stream));
    IDAHIP_HIP(c, hipMemcpyAsync(hRoundsDone, c->tiny_rounds, sizeof(int64_t) * batch, hipMemcpyDeviceToHost, c->stream));
    IDAHIP_HIP(c, hipMemcpyAsync(hAcc, c->tiny_acc, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (hYout) IDAHIP_HIP(c, hipMemcpyAsync(hYout, c->tiny_yout, sizeof(double) * ysz, hipMemcpyDeviceToHost, c->stream));
    if (hYPout) IDAHIP_HIP(c, hipMemcpyAsync(hYPout, c->tiny_ypout, sizeof(double) * ysz, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

int idahip_tiny_solve(idahip_ctx* c, void* hSys, size_t sys_bytes, const idahip_tiny_call* call, int64_t* hRoundsDone, uint64_t* hAcc,
                      double* hYout, double* hYPout) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    if (int rca = stepper_call_args(c, hSys, sys_bytes, call, hRoundsDone, hAcc, hAcc)) return rca;
    const bool network = c->kind == IDAHIP_MASS_ACTION && c->ma_tiny;  // (the switch is granted for n <= TINY_N alone)
    if (!network && (c->n != 3 || (c->kind != IDAHIP_ROBERTS && c->kind != IDAHIP_LORENZ63)))
        return fail(c, -2, "the device-resident stepper takes the Roberts and Lorenz63 problems (n = 3), and an IDAHIP_MASS_ACTION ctx with n <= %d that opted in (idahip_set_mass_action_tiny)", TINY_N);
    if (int rcu = ma_unset(c, "idahip_tiny_solve")) return rcu;
    if (c->jac_dq && !c->h_constr.empty()) return fail(c, -2, "difference-quotient Jacobians and constraints do not combine (DESIGN.md section 4g)");
    const int batch = c->batch, n = c->n;
    int rc = stepper_call_begin(c, "idahip_tiny_solve", hSys, call, hYout || hYPout);
    if (rc) return rc;
    TinyIdaArgs a;
    a.sys = (idactl::SysCore*)c->tiny_sys;
    a.v = vec_state(c);
    a.savres = c->savres; a.lu = c->lu; a.piv = (long long*)c->piv; a.params = c->params; a.nparam = c->nparam;
    a.ic_y = c->ic_y; a.ic_yp = c->ic_yp;
    a.f = flow_args(c, call);
    a.roots = (idahip_root_state*)c->tiny_roots;
    a.jac_dq = c->jac_dq;
    a.max_rounds = call->max_rounds;
    a.round_base = call->round_base;
    a.yout = hYout ? c->tiny_yout : nullptr;
    a.ypout = hYPout ? c->tiny_ypout : nullptr;
    a.rounds_done = (long long*)c->tiny_rounds;
    {
        KTimer kt(c, IDAHIP_K_VECTOR, batch);
        // Systems per wavefront. A lane walks one system's dependent fp64 chains, and the lanes of a wavefront, each in another phase
        // of its step (one, two or four Newton iterations, a failed error test, an order change, an output), execute each
        // other's branches. A batch that does not fill the device therefore runs on more, narrower wavefronts: the fewest
        // systems per wavefront (64, 32, ... 1) that keep the wavefront count at or below one per CU. Config 2 (1024 systems,
        // same box): 64 per wavefront 57.3 M Newton iterations/s in the stream (67.1 M whole pass), 16: 63.1 (70.5), 4: 70.9 (75.8),
        // 1: 65.6 (67.5). IDAHIP_TINY_SPW overrides (measurements). The per-system program is the same: results do not depend on it.
        // LDS of one system: its controller record, and its vectors too when the device grants that much
        const size_t lds_sys = sizeof(idactl::SysCore) + sizeof(double) * tiny_lds_doubles(n);
        int spw = 64;
        {
            const int simds = c->simds > 0 ? c->simds : 1024;
            while (spw > 1 && (long)(batch + spw / 2 - 1) / (spw / 2) <= simds / 4) spw >>= 1;
            // A network's system grows with n (1184 B at n = 3, 2224 B at n = 8: 64 of those leave one wavefront per CU), so a network's
            // wavefront is also bounded by LDS: the widest of which four workgroups fit a CU (TINY_NET_LDS_PER_WG, tiny_net_ida.hpp).
            // Where the batch does not fill the device the rule above has gone below the bound already.
            // Measured (tools/network_tiny_ab.py --spw, profiles/network_tiny_spw.json):
            // lorenz, n = 3, B = 65536, seconds (medians of 7, same box): 8 0.05425, 16 0.03877, 32 0.03729, 64 0.03755, rule 0.03758
            // enzyme8, n = 8, B = 65536, seconds (medians of 7, same box): 8 0.08500, 16 0.07345, 32 0.06917, 64 0.07092, rule 0.07366
            // (the rule is 32 at n = 3 and 16 at n = 8). The bound is not the best one at n = 8: 32 systems per wavefront, two workgroups
            // per CU, are 6 % faster there than the 16 that keep four resident. Lifting it is a follow-up (DESIGN.md section 4m+).
            if (network)
                while (spw > 1 && (size_t)spw * lds_sys > TINY_NET_LDS_PER_WG) spw >>= 1;
            if (const char* e = std::getenv("IDAHIP_TINY_SPW")) {
                const int v = (int)std::strtol(e, nullptr, 10);
                if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64) spw = v;
            }
        }
        const size_t lds_state = (size_t)spw * sizeof(idactl::SysCore), lds_all = (size_t)spw * lds_sys;
        // instantiations: problem x (root finding compiled in | out -- the bracketing code costs the plain stepper registers)
        // x (the constraint check compiled in | out: the plain kernels come out as they were without it)
        const bool roots = call->nroots > 0, constr = !c->h_constr.empty();
        const double* dconstr = constr ? (const double*)c->d_constr : (const double*)nullptr;
        auto launch = [&](auto kern, auto... more) {
            const int lds_vec = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(64 * lds_sys)) == hipSuccess ? 1 : 0;
            if (!lds_vec) (void)hipGetLastError();
            hipLaunchKernelGGL(kern, dim3((batch + spw - 1) / spw), dim3(spw), lds_vec ? lds_all : lds_state, c->stream, a, lds_vec, dconstr, more...);
        };
        if (!network) {
            auto kern = c->kind == IDAHIP_ROBERTS ? (roots ? tiny_ida_kernel<IDAHIP_ROBERTS, true, false> : tiny_ida_kernel<IDAHIP_ROBERTS, false, false>)
                                                  : (roots ? tiny_ida_kernel<IDAHIP_LORENZ63, true, false> : tiny_ida_kernel<IDAHIP_LORENZ63, false, false>);
            if (constr)
                kern = c->kind == IDAHIP_ROBERTS ? (roots ? tiny_ida_kernel<IDAHIP_ROBERTS, true, true> : tiny_ida_kernel<IDAHIP_ROBERTS, false, true>)
                                                 : (roots ? tiny_ida_kernel<IDAHIP_LORENZ63, true, true> : tiny_ida_kernel<IDAHIP_LORENZ63, false, true>);
            launch(kern);
        } else {  // a network: polynomial | with rate laws, and the same twins
            auto net = [&](auto laws, const auto& m) {
                constexpr bool L = decltype(laws)::value;
                auto kern = roots ? tiny_net_ida_kernel<L, true, false> : tiny_net_ida_kernel<L, false, false>;
                if (constr) kern = roots ? tiny_net_ida_kernel<L, true, true> : tiny_net_ida_kernel<L, false, true>;
                launch(kern, m, (const double*)c->params, n);
            };
            if (ma_laws(c)) net(std::true_type{}, *c->ma_law);
            else net(std::false_type{}, *c->ma);
        }
        if ((rc = post_launch(c, "tiny_ida"))) return rc;
    }
    if ((rc = stepper_call_end(c, hSys, call, hRoundsDone, hAcc, hYout, hYPout))) return rc;
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// buffers every device-resident stepper call needs: controller states, the schedule, the stagger, counters, output slots
static int stepper_buffers(idahip_ctx* c, const idahip_tiny_call* call, bool outputs) {
    const int batch = c->batch, n = c->n;
    int rc = 0;
    // (each buffer is guarded by itself: a failed allocation must not leave a later call with one non-null pointer that
    // stands for the whole group)
    if (!c->tiny_sys) IDAHIP_HIP(c, hipMalloc(&c->tiny_sys, (size_t)batch * sizeof(idactl::SysCore)));
    if (!c->tiny_start) rc |= dalloc(c, &c->tiny_start, (size_t)batch);
    if (!c->tiny_rounds) rc |= dalloc(c, &c->tiny_rounds, (size_t)batch);
    if (!c->tiny_acc) rc |= dalloc(c, &c->tiny_acc, (size_t)2);
    if (rc) return rc;
    if (call->nroots < 0 || call->nroots > IDAHIP_MAX_ROOTS) return fail(c, -2, "the device steppers take at most %d root functions", IDAHIP_MAX_ROOTS);
    if (call->nroots > 0) {
        if (!call->root_comps || !call->root_thresholds || !call->root_states) return fail(c, -2, "root functions without their arrays");
        for (int i = 0; i < call->nroots; ++i)
            if (call->root_comps[i] < 0 || call->root_comps[i] >= n) return fail(c, -2, "root function %d watches component %d of %d", i, call->root_comps[i], n);
        if (call->recycle) return fail(c, -2, "root finding and idaens_stream's restarts do not combine");
        if (!c->tiny_roots) IDAHIP_HIP(c, hipMalloc(&c->tiny_roots, (size_t)batch * sizeof(idahip_root_state)));
        IDAHIP_HIP(c, hipMemcpyAsync(c->tiny_roots, call->root_states, (size_t)batch * sizeof(idahip_root_state), hipMemcpyHostToDevice, c->stream));
    }
    if (call->ntout > c->tiny_ntout_cap) {
        if (c->tiny_touts) (void)hipFree(c->tiny_touts);
        c->tiny_touts = nullptr;
        if ((rc = dalloc(c, &c->tiny_touts, (size_t)call->ntout))) return rc;
        c->tiny_ntout_cap = call->ntout;
    }
    if (outputs && call->ntout > c->tiny_yout_cap) {
        const size_t ysz = (size_t)call->ntout * batch * n;
        if (c->tiny_yout) (void)hipFree(c->tiny_yout);
        if (c->tiny_ypout) (void)hipFree(c->tiny_ypout);
        c->tiny_yout = c->tiny_ypout = nullptr;
        if ((rc = dalloc(c, &c->tiny_yout, ysz))) return rc;
        if ((rc = dalloc(c, &c->tiny_ypout, ysz))) return rc;
        c->tiny_yout_cap = call->ntout;
    }
    return 0;
}

// the setup launches of a round on a Krylov ctx: the residual of the systems that set up (no Jacobian is formed: nje stays) and the
// band preconditioner's setup on the device-built list
static int krylov_round_setup(idahip_ctx* c, const RoundArgs& a, SysArgs& sa) {
    const int batch = c->batch, n = c->n;
    int rc;
    {
        KTimer kt(c, IDAHIP_K_SYS, 0);
        sa.skip = a.skipL;
        if ((rc = launch_sys(c, sa, batch, nullptr))) return rc;
    }
    if (!c->kry_prec) return 0;
    {   // psetup of the listed systems at the residual sys has just left: P, then its factors
        KTimer kt(c, IDAHIP_K_JAC, 0);
        hipLaunchKernelGGL(dq_round_prep_kernel, dim3((batch + 255) / 256), dim3(256), 0, c->stream, a.sys, (const int*)a.skipL, c->dq_hh, batch,
                           (long)std::min(c->kry_pml + c->kry_pmu + 1, n));
        DqArgs d;
        fill_dq_args(c, d, c->kry_pml, c->kry_pmu, c->kry_pldab);
        d.idx = a.ident; d.cj = a.cj; d.hh = c->dq_hh; d.skip = a.skipL;
        d.out = c->kry_pab; d.compact = 0;
        if ((rc = launch_band_dq(c, d, batch, "band DQ jac (preconditioner)"))) return rc;
    }
    KTimer kt(c, IDAHIP_K_LU, 0);
    return band_factor(c, c->kry_pab, (long)c->kry_pldab * n, c->kry_ppiv, n, c->kry_pml, c->kry_pmu, a.lu_list, batch, a.lu_cnt);
}

// whether idahip_round_solve brings the LU list's length to the host and sizes the round's LU launches by it: dense direct contexts
// only; n > 1024 always (measured in round 4), up to 1024 by idahip_set_lu_count_on_host, the library's choice being LU_COUNT_ON_HOST_DEFAULT
static bool lu_count_on_host_on(const idahip_ctx* c) {
    if (c->krylov || c->band || c->n <= TINY_N) return false;
    if (c->n > LU_MAX_N) return true;
    return (c->lu_count_on_host < 0 ? LU_COUNT_ON_HOST_DEFAULT : c->lu_count_on_host) != 0;
}

// the setup launches of a round on a direct ctx: residual and Jacobian of the systems that set up, and the factorisation of the
// device-built list. lu_cnt_on_host: the list's length is on its way to the host (ev_cnt) and sizes the LU's launches. Up to
// n = 1024 the host waits for it first thing -- behind the residual sweep round_newton has just enqueued -- and a round without
// setups (idahip_set_lu_period's postponed rounds among them) launches nothing here; above, after the setups' own sweeps, as ever.
static int direct_round_setup(idahip_ctx* c, const RoundArgs& a, SysArgs& sa, bool lu_cnt_on_host) {
    const int batch = c->batch, n = c->n;
    const long nn = (long)n * n;
    int rc;
    int nlu = batch, slow_grid = 0;
    const int* d_cnt = a.lu_cnt;
    const auto count_arrives = [&]() -> int {
        const int32_t* got = c->rnd_host + 2;
        if (a.host_mail) {
            // round_lists_kernel posts the count to pinned memory itself: nothing sits in the stream between it and the residual sweep
            // behind it. The host polls; a stream that has run dry without the post (a launch that failed) ends the wait.
            got = c->rnd_mail;
            for (unsigned spins = 1; __atomic_load_n(&c->rnd_mail[2], __ATOMIC_ACQUIRE) != a.mail_seq; ++spins) {
                std::this_thread::yield();  // (the core goes to whoever wants it: the other groups' threads enqueue meanwhile)
                if ((spins & 0x3ff) != 0) continue;
                const hipError_t e = hipStreamQuery(c->stream);
                if (e == hipSuccess && __atomic_load_n(&c->rnd_mail[2], __ATOMIC_ACQUIRE) != a.mail_seq)
                    return fail(c, -4, "the round's list length never reached the host");
                if (e != hipSuccess && e != hipErrorNotReady) return fail(c, -100, "hipStreamQuery failed: %s", hipGetErrorString(e));
            }
        } else {
            IDAHIP_HIP(c, hipEventSynchronize(c->ev_cnt));
        }
        nlu = got[0];
        d_cnt = nullptr;
        if (nlu < 0 || nlu > batch) return fail(c, -4, "list length %d outside 0..%d", nlu, batch);
        if (!a.host_mail) return 0;  // (n > 1024: the redo maximum does not travel; the SLOW launches keep a wave per system)
        // the SLOW panel launches walk a list that is normally empty: clamp(2 * the last round's largest list + 32, 32, count) workgroups
        const int redo = std::min(std::max(got[1], 0), batch);
        slow_grid = c->lu_slow_grid > 0 ? c->lu_slow_grid : std::min(std::max(2 * redo + 32, 32), nlu);
        return 0;
    };
    const bool count_first = lu_cnt_on_host && a.host_mail;
    if (count_first) {
        if ((rc = count_arrives())) return rc;
        if (nlu == 0) return 0;
    }
    if (a.jac_in_lu) {  // the plain sweep for the systems that set up: the factorisation forms J from A and B itself
        KTimer kt(c, IDAHIP_K_SYS, 0);
        sa.skip = a.skipL;
        if ((rc = launch_sys(c, sa, batch, nullptr))) return rc;
    } else if (a.fused_jac) {  // J = B + cj A falls out of the same sweep
        KTimer kt(c, IDAHIP_K_SYS_JAC, 0);
        sa.skip = a.skipL;
        if ((rc = launch_sys(c, sa, batch, c->jw))) return rc;
    } else {  // no fused residual + Jacobian kernel for this problem: the residual, then the Jacobian of the same systems
        {
            KTimer kt(c, IDAHIP_K_SYS, 0);
            sa.skip = a.skipL;
            if ((rc = launch_sys(c, sa, batch, nullptr))) return rc;
        }
        KTimer kt(c, IDAHIP_K_JAC, 0);
        if (c->jac_dq)  // the systems' hh from their records, and their nre_dq
            hipLaunchKernelGGL(dq_round_prep_kernel, dim3((batch + 255) / 256), dim3(256), 0, c->stream, a.sys, (const int*)a.skipL, c->dq_hh,
                               batch, dq_evals(c));
        if ((rc = launch_jac(c, c->jw, a.ident, a.cj, batch, nullptr, nullptr, nullptr, a.skipL, c->dq_hh))) return rc;
    }
    if (lu_cnt_on_host && !count_first && (rc = count_arrives())) return rc;
    const LuJac jq{c->A, c->B, a.cj, 1};  // (cj by system id)
    KTimer kt(c, IDAHIP_K_LU, 0);
    if (c->band) rc = band_factor(c, c->bab, (long)c->ldab * n, c->piv, n, c->ml, c->mu, a.lu_list, nlu, d_cnt);
    else rc = lu_factor_batched(c, c->jw, nn, c->lu, nn, (long long*)c->piv, n, c->perm, a.lu_list, nlu, d_cnt, a.jac_in_lu ? &jq : nullptr, slow_grid);
    if (rc) return rc;
    return post_launch(c, "lu");
}

// The Newton solve of one round (round_ida.hpp): the residual of the systems that start without a linear setup, the residual and
// setup of those that start with one, the control kernel's phase 0, then MAXNLSIT passes of { iteration ; control ; residual },
// booked under the classes of the host stepper's calls. A direct ctx and a Krylov ctx (kr non-null: idahip_set_krylov_rounds) differ
// in the setup launches, the iteration launch and the control kernel's instantiation. A Krylov ctx always takes the one-launch solve
// (idahip_set_krylov_fused is ignored: the two paths are bit-identical).
static int round_newton(idahip_ctx* c, const RoundArgs& a, const KryRoundArgs* kr, SysArgs& sa, bool lu_cnt_on_host) {
    const int batch = c->batch;
    const dim3 per_sys((batch + 255) / 256), blk(256);
    const auto ctl = [&](int phase) {
        if (kr) hipLaunchKernelGGL(round_ctl_kernel<true>, per_sys, blk, 0, c->stream, a, *kr, phase);
        else hipLaunchKernelGGL(round_ctl_kernel<false>, per_sys, blk, 0, c->stream, a, NoKryArgs{}, phase);
    };
    int rc;
    {   // sys(y0), y <- y0 = 0 (newton.rs:73)
        KTimer kt(c, IDAHIP_K_SYS, 0);
        sa.reset_ee = 1; sa.skip = a.skipP;
        if ((rc = launch_sys(c, sa, batch, nullptr))) return rc;
    }
    if ((rc = kr ? krylov_round_setup(c, a, sa) : direct_round_setup(c, a, sa, lu_cnt_on_host))) return rc;
    ctl(0);
    KryArgs ka{};
    if (kr) {
        fill_kry_args(c, ka);
        ka.idx = a.ident; ka.cj = a.cj; ka.tol = kr->tol; ka.skip = a.skipI;
        ka.newton = 1;
        ka.nli = c->kry_rint; ka.flag = c->kry_rint + batch; ka.resnorm = c->kry_rres; ka.nrm = a.nrm_out;
    }
    for (int m = 1; m <= idactl::MAXNLSIT; ++m) {
        {
            KTimer kt(c, IDAHIP_K_NEWTON_ITER, 0);
            if (kr) {
                if (!launch_krylov_fused<true>(c, ka, batch)) return fail(c, -2, "no fused Krylov kernel for problem kind %d", (int)c->kind);
                if ((rc = post_launch(c, "krylov_fused (round)"))) return rc;
            } else if ((rc = launch_newton_iter(c, a.ident, a.scale, a.nrm_out, a.skipI, batch))) {
                return rc;
            }
        }
        ctl(m);
        if (m < idactl::MAXNLSIT) {
            KTimer kt(c, IDAHIP_K_SYS, 0);
            sa.reset_ee = 0; sa.skip = a.skipS;
            if ((rc = launch_sys(c, sa, batch, nullptr))) return rc;
        }
    }
    return 0;
}

int idahip_round_solve(idahip_ctx* c, void* hSys, size_t sys_bytes, const idahip_tiny_call* call, int64_t* hRoundsDone, uint64_t* hAcc,
                       double* hYout, double* hYPout, int64_t* rounds_run) {
    if (c && !c->kry_rounds)
        if (int rc = refuse_krylov(c, "idahip_round_solve")) return rc;
    DevGuard dev_guard__(c);
    if (!c) return -1;
    if (int rca = stepper_call_args(c, hSys, sys_bytes, call, hRoundsDone, hAcc, rounds_run)) return rca;
    if (int rcu = ma_unset(c, "idahip_round_solve")) return rcu;
    const KindFacts& facts = kind_facts(c->kind);
    const bool lin = c->kind == IDAHIP_LINEAR_DENSE && facts.rounds && c->n <= LU_BIG_MAX_N;
    const bool banded = facts.rounds && facts.banded && c->n <= LU_BIG_MAX_N;
    const bool network = c->kind == IDAHIP_MASS_ACTION && facts.rounds && c->n <= LU_BIG_MAX_N;
    const bool kry = c->krylov != 0;  // (idahip_set_krylov_rounds is on: no LU bounds n, the LU variant does not matter)
    if (kry && (c->n <= TINY_N || !(lin || banded) || (c->kry_prec && c->kind == IDAHIP_LINEAR_DENSE)))
        return fail(c, -2, "the device lock-step rounds of a Krylov ctx take linear dense (no preconditioner), heat and Brusselator problems with %d < n <= %d", TINY_N, LU_BIG_MAX_N);
    if (!kry && (c->n <= TINY_N || !(lin || banded || network) || c->lu_variant < 4))
        return fail(c, -2, "the device-resident lock-step stepper takes linear dense, heat, Brusselator and mass-action problems with %d < n <= %d (LU variant 4)", TINY_N, LU_BIG_MAX_N);
    if (!c->h_constr.empty()) return fail(c, -2, "the device lock-step stepper does not check constraints: the host stepper does (DESIGN.md section 4g)");
    const int batch = c->batch, n = c->n;
    int rc = stepper_call_begin(c, "idahip_round_solve", hSys, call, hYout || hYPout);
    if (rc) return rc;
    if (!c->rnd_i) rc |= dalloc(c, &c->rnd_i, (size_t)8 * batch + 8 + 2 * IDAHIP_K_COUNT);
    if (!c->rnd_d) rc |= dalloc(c, &c->rnd_d, (size_t)4 * batch);
    if (rc) return rc;
    if (!c->rnd_host) IDAHIP_HIP(c, hipHostMalloc((void**)&c->rnd_host, 4 * sizeof(int32_t)));
    const bool lu_cnt_on_host = lu_count_on_host_on(c);
    const bool lu_cnt_mail = lu_cnt_on_host && n <= LU_MAX_N;  // (above, the count comes by copy and event behind the setups' sweeps, as measured in round 4)
    if (lu_cnt_mail && !c->rnd_mail) {
        IDAHIP_HIP(c, hipHostMalloc((void**)&c->rnd_mail, 4 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(c->rnd_mail, 0, 4 * sizeof(int32_t));
    }
    // whether any system of the call has a stop time: the kernels without it are the ones that ran before there was one
    bool tstop = false;
    for (int b = 0; b < batch; ++b) tstop = tstop || static_cast<const idactl::SysCore*>(hSys)[b].tstopset;
    RoundArgs a;
    a.f = flow_args(c, call);
    a.sys = (idactl::SysCore*)c->tiny_sys;
    a.v = vec_state(c);
    a.ic_y = c->ic_y; a.ic_yp = c->ic_yp;
    a.yout = hYout ? c->tiny_yout : nullptr;
    a.ypout = hYPout ? c->tiny_ypout : nullptr;
    a.round_base = call->round_base;
    a.fused_jac = (c->kind == IDAHIP_LINEAR_DENSE && !c->jac_dq && !kry) ? 1 : 0;
    a.jac_in_lu = (a.fused_jac && jac_in_lu_on(c, false)) ? 1 : 0;
    if ((c->jac_dq || (kry && c->kry_prec)) && !c->dq_hh && (rc = dalloc(c, &c->dq_hh, (size_t)batch))) return rc;
    a.lu_period = kry ? 1 : c->lu_period;  // (a psetup is one band launch: nothing to amortise)
    KryRoundArgs kr{};
    if (kry) {
        if (!c->kry_rcnt) rc |= dalloc(c, &c->kry_rcnt, (size_t)3 * batch);
        if (!c->kry_rint) rc |= dalloc(c, &c->kry_rint, (size_t)2 * batch);
        if (!c->kry_rres) rc |= dalloc(c, &c->kry_rres, (size_t)batch);
        if (rc) return rc;
        // npe / nps are not in the controller record: they travel in arrays of their own (idahip_krylov_rounds_put / get_counters)
        c->kry_h_npe.resize((size_t)batch, 0);
        c->kry_h_nps.resize((size_t)batch, 0);
        IDAHIP_HIP(c, hipMemcpyAsync(c->kry_rcnt, c->kry_h_npe.data(), sizeof(int64_t) * batch, hipMemcpyHostToDevice, c->stream));
        IDAHIP_HIP(c, hipMemcpyAsync(c->kry_rcnt + batch, c->kry_h_nps.data(), sizeof(int64_t) * batch, hipMemcpyHostToDevice, c->stream));
        IDAHIP_HIP(c, hipMemsetAsync(c->kry_rcnt + 2 * (size_t)batch, 0, sizeof(int64_t) * batch, c->stream));
        kr.prec = c->kry_prec;
        kr.nli = c->kry_rint; kr.flag = c->kry_rint + batch;
        kr.npe = (long long*)c->kry_rcnt; kr.nps = (long long*)c->kry_rcnt + batch; kr.ready = (long long*)c->kry_rcnt + 2 * (size_t)batch;
    }
    a.roots = (idahip_root_state*)c->tiny_roots;
    int* ib = c->rnd_i;
    a.stepping = ib; a.in_newton = ib + batch; a.skipP = ib + 2 * batch; a.skipL = ib + 3 * batch; a.skipI = ib + 4 * batch;
    a.skipS = ib + 5 * batch; a.ident = ib + 6 * batch; a.lu_list = ib + 7 * batch; a.lu_cnt = ib + 8 * batch; a.summary = ib + 8 * batch + 2; a.lu_wait = ib + 8 * batch + 4;
    a.lu_redo = (n <= LU_MAX_N && !kry && !c->band) ? c->lu_redo : nullptr;  // (n > 1024: the round is the one it was; the SLOW launches, where there are any, keep a wave per system)
    a.host_mail = nullptr; a.mail_seq = 0;
    if (lu_cnt_mail) IDAHIP_HIP(c, hipHostGetDevicePointer((void**)&a.host_mail, c->rnd_mail, 0));
    a.stats = (unsigned long long*)(ib + 8 * batch + 6);  // (8 * batch + 6 ints: 8-byte aligned for even batch; checked below)
    if (((uintptr_t)a.stats & 7) != 0) a.stats = (unsigned long long*)(ib + 8 * batch + 7);
    IDAHIP_HIP(c, hipMemsetAsync(a.stats, 0, IDAHIP_K_COUNT * sizeof(unsigned long long), c->stream));
    a.lu_info = c->lu_info;
    a.tn = c->rnd_d; a.cj = c->rnd_d + batch; a.scale = c->rnd_d + 2 * batch; a.nrm_out = c->rnd_d + 3 * batch;
    a.rounds_done = (long long*)c->tiny_rounds;
    kr.tol = a.scale;  // (a Krylov ctx does not scale the correction: the slot carries the solver's tolerance)
    hipLaunchKernelGGL(round_init_kernel, dim3((batch + 255) / 256), dim3(256), 0, c->stream, a);
    IDAHIP_HIP(c, hipMemsetAsync(a.summary, 0, 2 * sizeof(int), c->stream));
    const size_t shm_wg = sizeof(double) * (4 * (size_t)n + 8);
    SysArgs sa;
    fill_sys_args(c, sa, 1);
    sa.idx = a.ident; sa.tn = a.tn; sa.cj = a.cj;
    int64_t r = 0;
    for (;; ++r) {
        if (call->max_rounds > 0 && r >= call->max_rounds) break;
        a.round = r;
        a.first_round = r == 0;
        if (a.host_mail) a.mail_seq = ++c->rnd_mail_seq;  // (what round_lists_kernel posts last and direct_round_setup waits for)
        {
            KTimer kt(c, IDAHIP_K_VECTOR, 0);
            auto kern = call->nroots > 0 ? (tstop ? round_begin_kernel<true, true> : round_begin_kernel<true, false>)
                                         : (tstop ? round_begin_kernel<false, true> : round_begin_kernel<false, false>);
            hipLaunchKernelGGL(kern, dim3(batch), dim3(WG_NT), shm_wg, c->stream, a);
            // (a Krylov ctx without the preconditioner factors nothing: no list)
            if (!kry || c->kry_prec) {
                if (a.lu_redo) hipLaunchKernelGGL(round_lists_kernel<true>, dim3(1), dim3(1024), 0, c->stream, a);
                else hipLaunchKernelGGL(round_lists_kernel<false>, dim3(1), dim3(1024), 0, c->stream, a);
            }
        }
        // n > 1024 (config 4): a factorisation is ~640 launches, most of them one workgroup per matrix, and a third of a small
        // batch needs one in any round -- launches sized for the whole batch cost more than they do at n = 512 (11.4 against
        // 12.3 k iters/s in round 4). The list's length comes back to the host (4 bytes, behind the residual kernels enqueued
        // next: the copy's round trip is hidden) and the LU's launches are sized by it, as the host stepper's are.
        // n <= 1024: the host sizes the launches too (idahip_set_lu_count_on_host), but round_lists_kernel posts
        // the count to pinned memory itself (RoundArgs::host_mail): no copy and no event in the stream. Either way the last
        // factorisation's largest redo count rides along and sizes the SLOW panel launches.
        // (the band LU is one launch: its surplus lanes leave on reading the count)
        if (lu_cnt_on_host && !lu_cnt_mail) {
            IDAHIP_HIP(c, hipMemcpyAsync(c->rnd_host + 2, a.lu_cnt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
            IDAHIP_HIP(c, hipEventRecord(c->ev_cnt, c->stream));
        }
        rc = round_newton(c, a, kry ? &kr : nullptr, sa, lu_cnt_on_host);
        if (rc) return rc;
        IDAHIP_HIP(c, hipMemsetAsync(a.summary, 0, sizeof(int), c->stream));
        {
            KTimer kt(c, IDAHIP_K_VECTOR, 0);
            auto kern = call->nroots > 0 ? (tstop ? round_end_kernel<true, true> : round_end_kernel<true, false>)
                                         : (tstop ? round_end_kernel<false, true> : round_end_kernel<false, false>);
            hipLaunchKernelGGL(kern, dim3(batch), dim3(WG_NT), shm_wg, c->stream, a);
            if ((rc = post_launch(c, "round_end"))) return rc;
        }
        if (!call->recycle) {  // one synchronisation per round: does any system still step?
            IDAHIP_HIP(c, hipMemcpyAsync(c->rnd_host, a.summary, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
            if (c->rnd_host[0] == 0) {
                ++r;
                break;
            }
        }
    }
    *rounds_run = r;
    if ((rc = stepper_call_end(c, hSys, call, hRoundsDone, hAcc, hYout, hYPout))) return rc;
    unsigned long long hstats[IDAHIP_K_COUNT];
    IDAHIP_HIP(c, hipMemcpyAsync(hstats, a.stats, sizeof hstats, hipMemcpyDeviceToHost, c->stream));
    std::vector<int64_t> kcnt;
    if (kry) {
        kcnt.resize((size_t)3 * batch);
        IDAHIP_HIP(c, hipMemcpyAsync(kcnt.data(), c->kry_rcnt, sizeof(int64_t) * kcnt.size(), hipMemcpyDeviceToHost, c->stream));
    }
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    for (int b = 0; kry && b < batch; ++b) {
        // (a system that idaens_stream created anew in the call's last round has not set up yet: its counters have restarted with it)
        const bool fresh = static_cast<const idactl::SysCore*>(hSys)[b].nsetups == 0;
        c->kry_h_npe[b] = fresh ? 0 : kcnt[b];
        c->kry_h_nps[b] = fresh ? 0 : kcnt[(size_t)batch + b];
        if (c->kry_prec && kcnt[2 * (size_t)batch + b] != 0) c->kry_pready[b] = 1;  // as after the host stepper's psetup calls
    }
    for (int k = 0; k < IDAHIP_K_COUNT; ++k) c->k_systems[k] += (int64_t)hstats[k];  // systems actually served, per kernel class
    c->k_systems[IDAHIP_K_VECTOR] += 2 * r * (int64_t)batch;
    return 0;
}

int idahip_lu_variant(const idahip_ctx* c) { return c ? c->lu_variant : -1; }
int idahip_timing_build(void) { return tb::TIMING_BUILD ? 1 : 0; }
int idahip_set_lu_superpanel(idahip_ctx* c, int on) {
    if (!c) return -1;
    c->lu_superpanel = on != 0 ? 1 : 0;
    return 0;
}
int idahip_lu_superpanel(const idahip_ctx* c) { return c ? c->lu_superpanel : -1; }
int idahip_set_lu_period(idahip_ctx* c, int rounds) {
    if (!c || rounds < 1 || rounds > 64) return -1;
    c->lu_period = rounds;
    return 0;
}
int idahip_lu_period(const idahip_ctx* c) { return c ? c->lu_period : -1; }
int idahip_set_lu_count_on_host(idahip_ctx* c, int on) {
    if (!c || on < -1 || on > 1) return -1;
    c->lu_count_on_host = on;
    return 0;
}
int idahip_lu_count_on_host(const idahip_ctx* c) { return c ? (lu_count_on_host_on(c) ? 1 : 0) : -1; }
int idahip_set_lu_slow_grid(idahip_ctx* c, int workgroups) {
    if (!c || workgroups < 0) return -1;
    c->lu_slow_grid = workgroups;
    return 0;
}

// LSolver::get_type / num_iters / res_norm of the dense direct solver (crates/linear/src/dense.rs:30-36, traits.rs:82-90)
int idahip_ls_type(const idahip_ctx* c) { return c ? (c->krylov ? IDAHIP_LS_ITERATIVE : IDAHIP_LS_DIRECT) : -1; }
int idahip_ls_num_iters(const idahip_ctx* c) { return c ? (c->krylov ? c->kry_last_nli : 0) : -1; }
double idahip_ls_res_norm(const idahip_ctx* c) { return c && c->krylov ? c->kry_last_resnorm : 0.0; }

#ifdef IDAHIP_STAMPS /* (only accepted together with -DIDAHIP_TIMING_BUILD: exp_switches.hpp) */
/* timing builds: a device buffer for in-kernel time stamps (8 per workgroup of the instrumented launch) */
void* idahip_debug_stamps(idahip_ctx* c, size_t words) {
    if (!c) return nullptr;
    if (!c->dbg_stamps && hipMalloc((void**)&c->dbg_stamps, words * 8) != hipSuccess) return nullptr;
    (void)hipMemset(c->dbg_stamps, 0, words * 8);
    return c->dbg_stamps;
}
#endif

int idahip_set_lu_variant(idahip_ctx* c, int variant) {
    DevGuard dev_guard__(c);
    if (!c || variant < 3 || variant > 4) return -1;  // 3: panel + narrow update kernels, 4: wave-per-matrix panel (default)
    c->lu_variant = variant;
    return 0;
}

int idahip_set_jac_in_lu(idahip_ctx* c, int on) {
    if (!c) return -1;
    if (on && !jac_in_lu_can(c))
        return fail(c, -2, "idahip_set_jac_in_lu: J = B + cj*A inside the LU is for a dense IDAHIP_LINEAR_DENSE ctx with %d < n <= %d", TINY_N, WP_MAX_ROWS);
    c->jac_in_lu = on ? 1 : 0;
    return 0;
}

int idahip_set_lu_staged(idahip_ctx* c, int on) {
    if (!c) return -1;
    if (on && !(c->lu_ord && c->n > TINY_N && c->n <= WP_MAX_ROWS))
        return fail(c, -2, "idahip_set_lu_staged: staged L is for a dense direct ctx with %d < n <= %d", TINY_N, WP_MAX_ROWS);
    c->lu_staged = on ? 1 : 0;
    return 0;
}

// 1: the ctx's factors are written and read staged from now on; 0: in the reference layout
int idahip_lu_staged(const idahip_ctx* c) { return c ? (lu_staged_on(c) ? 1 : 0) : -1; }

// 0: nowhere now; 1: in idahip_round_solve alone (never set, n > 448); 2: there and in the list entry points (set to 1)
int idahip_jac_in_lu(const idahip_ctx* c) { return c ? (jac_in_lu_on(c, true) ? 2 : jac_in_lu_on(c, false) ? 1 : 0) : -1; }

// ------------------------------------------------------------------------------------------------ measurement
int idahip_timing_enable(idahip_ctx* c, int on) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    c->timing = on < 0 ? 0 : (on > 2 ? 2 : on);
    return 0;
}
int idahip_timing_get(idahip_ctx* c, idahip_kclass k, double* ms, int64_t* launches, int64_t* systems) {
    DevGuard dev_guard__(c);
    if (!c || k < 0 || k >= IDAHIP_K_COUNT) return -1;
    if (ms) *ms = c->k_ms[k];
    if (launches) *launches = c->k_launches[k];
    if (systems) *systems = c->k_systems[k];
    return 0;
}
int idahip_timing_reset(idahip_ctx* c) {
    DevGuard dev_guard__(c);
    if (!c) return -1;
    for (int k = 0; k < IDAHIP_K_COUNT; ++k) {
        c->k_ms[k] = 0.0;
        c->k_launches[k] = 0;
        c->k_systems[k] = 0;
    }
    return 0;
}

}  // extern "C"
