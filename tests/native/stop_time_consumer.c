/* The stop-time and masked-norm prototypes of include/ida_ensemble.h and include/ida_hip.h consumed from C.
 * Built by tests/test_stop_time_consumer.py with `gcc -std=c99 -Wall -Wextra -pedantic -Werror` against libidaens.so and libidahip.so;
 * the test checks that it compiles and links. With no arguments it only prints the constants; it never opens a device. */
#include <stdio.h>

#include "ida_ensemble.h"

typedef int (*set_stop_time_fn)(idaens*, const double*, int);
typedef int (*get_stop_time_fn)(const idaens*, double*);
typedef int (*set_suppress_alg_fn)(idahip_ctx*, int);
typedef int (*suppress_alg_fn)(const idahip_ctx*);
typedef int (*wrms_masked_fn)(idahip_ctx*, const double*, const double*, double*, const int32_t*, int);

int main(void) {
    set_stop_time_fn a = idaens_set_stop_time;
    get_stop_time_fn b = idaens_get_stop_time;
    set_suppress_alg_fn c = idahip_set_suppress_alg;
    suppress_alg_fn d = idahip_suppress_alg;
    wrms_masked_fn e = idahip_wrms_masked;
    double t = 0.0;
    /* null handles are refused, nothing is touched */
    int rc = a(NULL, &t, 1) + b(NULL, &t) + c(NULL, 1) + d(NULL);
    printf("TSTOP_RETURN %d BAD_TSTOP %d null_calls %d wrms_masked %d\n", IDAENS_TSTOP_RETURN, IDAENS_BAD_TSTOP, rc, e != NULL);
    return 0;
}
