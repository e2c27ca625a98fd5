// TEST INFRASTRUCTURE: tests/native/roots_oracle.cpp plus one creator that hands a start time to oracle/ida.hpp's `Ida` constructor
// (quirk Q13: t0 = 0 unless set explicitly) -- what IDAReInit needs from the oracle: a new object at t0 with new values and the same
// root functions (tests/reinit_oracle.py compiles this into a temporary directory and loads it with ctypes).
#include "roots_oracle.cpp"

extern "C" {

// roots_oracle_create's arguments, then t0. nroots < 0: the problem as the oracle has it, without the decorator (Roberts then keeps its
// own two functions). nullptr for a bad component.
void* reinit_oracle_create(int kind, int n, const double* params, const double* A, const double* B, const double* c, const double* yy0,
                           const double* yp0, double rtol, const double* atol, int natol, int nroots, const int32_t* comps,
                           const double* thresholds, double t0) {
    Handle* h = new Handle();
    if (nroots < 0) {
        h->problem = make_problem(kind, n, params, A, B, c);
    } else {
        WithRoots* w = new WithRoots();
        std::unique_ptr<Problem> keep(w);
        w->inner = make_problem(kind, n, params, A, B, c);
        for (int i = 0; i < nroots; ++i) {
            if (comps[i] < 0 || comps[i] >= w->inner->model_size()) {
                delete h;
                return nullptr;
            }
            w->comps.push_back(comps[i]);
            w->thr.push_back(thresholds[i]);
        }
        h->problem = std::move(keep);
    }
    h->ida.reset(new Ida(h->problem.get(), yy0, yp0, make_tol(rtol, atol, natol), t0));
    return h;
}

}  // extern "C"
