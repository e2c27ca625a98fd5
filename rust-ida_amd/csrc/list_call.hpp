// libidahip -- the frame of an entry point over a host list of system ids (hIdx, nsys): DESIGN.md, "an entry point over a list of
// systems". ListCall owns what these entry points share -- the refusals every one of them makes, the staging slot with the device
// copy of the list, the timed launch and its error check, and how per-system results come back --, so that an entry point says
// only its own refusals, the arrays it stages, its launches and where its results go. Host code only.
#pragma once
#include <cmath>
#include <initializer_list>

#include "common.hpp"

namespace idahip {

inline int check_list(idahip_ctx* c, const int32_t* hIdx, int nsys) {
    if (!c) return -1;
    if (nsys < 0 || nsys > c->batch) return fail(c, -2, "nsys = %d out of range (batch = %d)", nsys, c->batch);
    if (nsys > 0 && !hIdx) return fail(c, -2, "null system list");
    for (int s = 0; s < nsys; ++s)
        if (hIdx[s] < 0 || hIdx[s] >= c->batch) return fail(c, -2, "system id %d out of range at list position %d", hIdx[s], s);
    // no id twice: two workgroups would factor one matrix in place, or update one system's vectors, at the same time
    uint64_t* seen = c->list_seen.data();
    int dup = -1;
    for (int s = 0; s < nsys && dup < 0; ++s) {
        const uint64_t bit = 1ull << (hIdx[s] & 63);
        if (seen[hIdx[s] >> 6] & bit) dup = s;
        seen[hIdx[s] >> 6] |= bit;
    }
    for (int s = 0; s < (dup < 0 ? nsys : dup); ++s) seen[hIdx[s] >> 6] = 0;  // leave the map clear for the next call
    if (dup >= 0) return fail(c, -2, "system id %d listed twice (again at list position %d)", hIdx[dup], dup);
    return 0;
}

inline int post_launch(idahip_ctx* c, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, -101, "launch of %s failed: %s", what, hipGetErrorString(e));
    return 0;
}

// a host pointer that a call needs is NULL
inline int null_argument(idahip_ctx* c) { return fail(c, -2, "null argument"); }

// what the calls that need a matrix answer on a Krylov ctx (a null ctx passes: the caller's null check answers that)
inline int refuse_krylov(idahip_ctx* c, const char* who) {
    if (c && c->krylov) return fail(c, -2, "%s on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix", who);
    return 0;
}

// One call of an entry point over a list. The steps, in the order the refusals are documented to win:
//   ListCall f(c, hIdx, nsys[, who]);    the ctx's device; with `who`, the Krylov-ctx refusal; the list check        -> f.rc
//   if (!f.args({p, q, ...})) return f.rc;            null_argument() unless every pointer is set
//   ... the entry point's own refusals (return fail(...)) ...
//   if (!f.stage()) return f.rc;         an empty list ends here with 0; else a staging slot and f.idx, the list on the device
//   f.in(h, count) / f.out<T>(count)     further arrays into the slot, result regions out of it (all in() before the first out())
//   f.launch(class, systems, name, body) uploads the slot before the first launch; KTimer, body(), post_launch(name)
//   return f.done();                     no results: the slot stays busy until the stream has passed this point
//   if (!f.fetch()) return f.rc;         results: the result regions are on the host; f.rms / f.copy / f.host hand them out
// A step that fails leaves its code in f.rc, and every later launch(), fetch() and done() is skipped and passes the code on.
struct ListCall {
    DevGuard guard;
    idahip_ctx* c;
    const int32_t* hIdx;
    int nsys;
    int rc;
    bool sent = false;
    ArgPack ap;
    const int* idx = nullptr;

    ListCall(idahip_ctx* ctx, const int32_t* list, int count, const char* no_krylov = nullptr)
        : guard(ctx), c(ctx), hIdx(list), nsys(count), rc(no_krylov ? refuse_krylov(ctx, no_krylov) : 0) {
        if (!rc) rc = check_list(c, hIdx, nsys);
    }

    bool args(std::initializer_list<const void*> ptrs) {
        if (rc) return false;
        for (const void* p : ptrs)
            if (!p) rc = null_argument(c);
        return rc == 0;
    }
    bool stage() {
        if (rc || nsys == 0) return false;
        if ((rc = ap.begin(c))) return false;
        idx = ap.in(hIdx, nsys);
        return true;
    }
    template <class T>
    const T* in(const T* src, size_t count) { return ap.in(src, count); }
    template <class T>
    T* out(size_t count) { return ap.out<T>(count); }

    // the slot's inputs on their way to the device (a result region that did not fit fails here, before anything is launched)
    bool send() {
        if (!rc && !sent) {
            sent = true;
            if (!(rc = ap.ok())) rc = ap.upload();
        }
        return rc == 0;
    }
    // body(): the launches booked under one timer, void or an int code; `what` names the kernel for post_launch (nullptr: body checks)
    template <class F>
    bool launch(idahip_kclass k, int systems, const char* what, F&& body) {
        if (!send()) return false;
        KTimer kt(c, k, systems);
        if constexpr (std::is_void_v<decltype(body())>) body();
        else rc = body();
        if (!rc && what) rc = post_launch(c, what);
        return rc == 0;
    }
    int done() { return rc ? rc : (rc = ap.finish_async()); }
    bool fetch() {
        if (!rc) rc = ap.fetch();
        return rc == 0;
    }

    // after fetch(): a result region on the host, and the three ways results go to the caller
    template <class T>
    const T* host(const T* d) const { return ap.host_of(d); }
    // dst[i] = the RMS norm of n components from their sum of squares src[i * stride]: divide, then sqrt, host libm (norm_rms.rs:36-37)
    void rms(double* dst, const double* d_src, size_t count, size_t stride = 1) const {
        const double* h = host(d_src);
        for (size_t i = 0; i < count; ++i) dst[i] = sqrt(h[i * stride] / (double)c->n);
    }
    template <class T>
    void copy(T* dst, const T* d_src, size_t count) const {
        const T* h = host(d_src);
        for (size_t i = 0; i < count; ++i) dst[i] = h[i];
    }
};

// the per-system info of the last factorisation (ctx->lu_info) for the listed systems; 1 if any of them is non-zero
inline int report_info(idahip_ctx* c, const int32_t* hIdx, int nsys, int32_t* hInfo) {
    std::vector<int32_t> info(c->batch);
    IDAHIP_HIP(c, hipMemcpyAsync(info.data(), c->lu_info, sizeof(int32_t) * c->batch, hipMemcpyDeviceToHost, c->stream));
    IDAHIP_HIP(c, hipStreamSynchronize(c->stream));
    int any = 0;
    for (int s = 0; s < nsys; ++s) {
        hInfo[s] = info[hIdx[s]];
        any |= hInfo[s] != 0;
    }
    return any ? 1 : 0;
}

// the order ranges of the stepper's vector calls, per list position
inline int check_kk_ns(idahip_ctx* c, const int32_t* hKkNs, int nsys) {
    for (int s = 0; s < nsys; ++s)
        if (hKkNs[2 * s] < 1 || hKkNs[2 * s] >= MXORDP1 || hKkNs[2 * s + 1] < 0) return fail(c, -2, "bad kk/ns at list position %d", s);
    return 0;
}
inline int check_order(idahip_ctx* c, const char* what, const int32_t* hK, int nsys, int kmax = MXORDP1 - 1) {
    for (int s = 0; s < nsys; ++s)
        if (hK[s] < 1 || hK[s] > kmax) return fail(c, -2, "bad %s at list position %d", what, s);
    return 0;
}

}  // namespace idahip
