// TEST INFRASTRUCTURE: the CPU oracle's C API (oracle/capi.cpp, included as it is) plus the three switches it lacks -- the id vector,
// the stop time and a way to read whether one is set -- so that tests can drive oracle/ida.hpp's own stop tests and masked norms
// (tests/tstop_oracle.py compiles this into a temporary directory and loads it with ctypes). `suppressalg` is already reachable through
// oracle_ida_set_scalar.
#include "../../oracle/capi.cpp"

extern "C" {

// ida_id[i] = id[i] != 0 (1: differential, the component counts in the masked norms)
int tstop_oracle_set_id(void* vh, const double* id, int n) {
    Ida& ida = *((Handle*)vh)->ida;
    if (n != ida.n) return -1;
    for (int i = 0; i < n; ++i) ida.ida_id[i] = id[i] != 0.0 ? 1 : 0;
    return 0;
}
// ida_tstop = Some(t) (has != 0) or None
void tstop_oracle_set_tstop(void* vh, int has, double t) {
    Ida& ida = *((Handle*)vh)->ida;
    ida.has_tstop = has != 0;
    ida.ida_tstop = t;
}
int tstop_oracle_has_tstop(void* vh, double* t) {
    const Ida& ida = *((Handle*)vh)->ida;
    if (t) *t = ida.ida_tstop;
    return ida.has_tstop ? 1 : 0;
}

}  // extern "C"
