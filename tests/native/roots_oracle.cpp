// TEST INFRASTRUCTURE: tests/native/tstop_oracle.cpp (oracle/capi.cpp plus the id vector and the stop time) plus the product's root
// function family on any of the oracle's problems. The oracle's own root functions are Roberts' two; `Problem` has the virtual
// num_roots() / root() pair, so a decorator that forwards the problem and answers those two with g_i = y[comp_i] - thr_i (what
// idaens_set_roots defines) gives oracle/ida.hpp's own root finding on Lorenz, the linear dense and the heat problem too
// (tests/roots_oracle.py compiles this into a temporary directory and loads it with ctypes).
#include "tstop_oracle.cpp"

namespace {

struct WithRoots : Problem {
    std::unique_ptr<Problem> inner;
    std::vector<int> comps;
    std::vector<double> thr;
    int model_size() const override { return inner->model_size(); }
    void res(double tt, const double* yy, const double* yp, double* rr) const override { inner->res(tt, yy, yp, rr); }
    void jac(double tt, double cj, const double* yy, const double* yp, const double* rr, double* J) const override {
        inner->jac(tt, cj, yy, yp, rr, J);
    }
    int num_roots() const override { return (int)comps.size(); }
    void root(double, const double* yy, const double*, double* g) const override {
        for (size_t i = 0; i < comps.size(); ++i) g[i] = yy[comps[i]] - thr[i];
    }
};

}  // namespace

extern "C" {

// oracle_ida_create's arguments, then the family: comps [nroots] (0 <= comp < n), thresholds [nroots]. nullptr for a bad component.
void* roots_oracle_create(int kind, int n, const double* params, const double* A, const double* B, const double* c, const double* yy0,
                          const double* yp0, double rtol, const double* atol, int natol, int nroots, const int32_t* comps,
                          const double* thresholds) {
    WithRoots* w = new WithRoots();
    std::unique_ptr<Problem> keep(w);
    w->inner = make_problem(kind, n, params, A, B, c);
    for (int i = 0; i < nroots; ++i) {
        if (comps[i] < 0 || comps[i] >= w->inner->model_size()) return nullptr;
        w->comps.push_back(comps[i]);
        w->thr.push_back(thresholds[i]);
    }
    Handle* h = new Handle();
    h->problem = std::move(keep);
    h->ida.reset(new Ida(h->problem.get(), yy0, yp0, make_tol(rtol, atol, natol)));
    return h;
}

}  // extern "C"
