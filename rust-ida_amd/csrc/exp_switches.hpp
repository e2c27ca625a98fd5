// Timing-build switches of the kernels, all in one place.
//
// The measurements behind DESIGN.md section 4 were taken with builds of libidahip.so in which one part of a kernel is removed
// or replaced (results are then garbage: such a library only serves tools/kt_libs.sh, tools/newton_time.py, tools/stamps_*.py).
// None of that may reach the shipped library by accident: a switch is only accepted together with -DIDAHIP_TIMING_BUILD, the
// default `make` defines neither (tests/test_abi_symbols.py scans the Makefile and asks the library: idahip_timing_build()
// must return 0), and the kernels only ever read the constants of namespace idahip::tb below -- in a product build every one
// of them is a compile-time `false` / product value and the guarded code folds away.
#pragma once

#if !defined(IDAHIP_TIMING_BUILD) &&                                                                                   \
    (defined(IDAHIP_EXP_NOPRO) || defined(IDAHIP_EXP_NOUPD) || defined(IDAHIP_EXP_NOGATHER) || defined(IDAHIP_EXP_NODIAG) || \
     defined(IDAHIP_EXP_NOSWEEP) || defined(IDAHIP_STAMPS) || defined(IDAHIP_TRAIL_PIPE) || defined(IDAHIP_TRAIL_QUAD) ||   \
     defined(IDAHIP_WP_RING) || defined(IDAHIP_US_PAD) || defined(IDAHIP_SYS_UNR) || defined(IDAHIP_TRAIL_AHEAD) ||         \
     defined(IDAHIP_NT_SYS) || defined(IDAHIP_NT_SOLVE) || defined(IDAHIP_NT_FINALIZE) || defined(IDAHIP_NT_TRAIL))
#error "IDAHIP_EXP_* / IDAHIP_STAMPS / IDAHIP_TRAIL_* (IDAHIP_TRAIL_AHEAD: 0..3) / IDAHIP_WP_RING / IDAHIP_US_PAD / IDAHIP_SYS_UNR / IDAHIP_NT_* are timing-build switches: add -DIDAHIP_TIMING_BUILD (the library then reports itself as one and is not a product)"
#endif

namespace idahip {
namespace tb {

#ifdef IDAHIP_TIMING_BUILD
constexpr bool TIMING_BUILD = true;
#else
constexpr bool TIMING_BUILD = false;
#endif

// lu_trail64w_kernel: no gather and no U12 solve (U12 = constants) / return before the strips / gathered entries = constants
#ifdef IDAHIP_EXP_NOPRO
constexpr bool NOPRO = true;
#else
constexpr bool NOPRO = false;
#endif
#ifdef IDAHIP_EXP_NOUPD
constexpr bool NOUPD = true;
#else
constexpr bool NOUPD = false;
#endif
#ifdef IDAHIP_EXP_NOGATHER
constexpr bool NOGATHER = true;
#else
constexpr bool NOGATHER = false;
#endif
// wg_getrs: the solve without its diagonal blocks / without its sweeps
#ifdef IDAHIP_EXP_NODIAG
constexpr bool NODIAG = true;
#else
constexpr bool NODIAG = false;
#endif
#ifdef IDAHIP_EXP_NOSWEEP
constexpr bool NOSWEEP = true;
#else
constexpr bool NOSWEEP = false;
#endif
// in-kernel time stamps (lu_panelr_kernel's first launch; lu_trail64w_kernel's launch for super-panel k0 == STAMPS): -1 = none
#ifdef IDAHIP_STAMPS
constexpr int STAMPS = IDAHIP_STAMPS;
#else
constexpr int STAMPS = -1;
#endif
// lu_trail64w_kernel: operand reads of step k+1 requested before the arithmetic of step k (product: yes); U12 solve in
// registers on all four waves (product: yes); padding of a row of Us in doubles (product: 2)
#ifdef IDAHIP_TRAIL_PIPE
constexpr bool TRAIL_PIPE = IDAHIP_TRAIL_PIPE != 0;
#else
constexpr bool TRAIL_PIPE = true;
#endif
#ifdef IDAHIP_TRAIL_QUAD
constexpr bool TRAIL_QUAD = IDAHIP_TRAIL_QUAD != 0;
#else
constexpr bool TRAIL_QUAD = true;
#endif
#ifdef IDAHIP_US_PAD
constexpr int US_PAD = IDAHIP_US_PAD;
#else
constexpr int US_PAD = 2;
#endif
// lu_trail64w_kernel, solve in registers: steps by which the LDS reads of the multipliers run ahead of step kk (product: 1, then 3)
#ifdef IDAHIP_TRAIL_AHEAD
constexpr int trail_ahead(int kk) { return IDAHIP_TRAIL_AHEAD; }
#else
constexpr int trail_ahead(int kk) { return kk < 32 ? 1 : 3; }
#endif
// lu_wavepanel_kernel: deep multiplier prefetch rings (product: depth 2 for every slot count)
#ifdef IDAHIP_WP_RING
constexpr bool WP_DEEP_RING = IDAHIP_WP_RING != 0;
#else
constexpr bool WP_DEEP_RING = false;
#endif
// linear_sys_kernel: columns of A and B in flight per thread (product: 16)
#ifdef IDAHIP_SYS_UNR
constexpr int SYS_UNR = IDAHIP_SYS_UNR;
#else
constexpr int SYS_UNR = 16;
#endif

// Cache policy of the streams a launch touches once (the non-temporal bit on loads and stores that exist anyway; results are bit
// for bit the same either way). The product values are the ones that won their A/B in the stream of four groups, alternating
// processes on one box (profiles/r07_cache_policy_ab.txt); -DIDAHIP_TIMING_BUILD -DIDAHIP_NT_...=0|1 builds
// the other side.
//   NT_SYS      (on):  linear_sys_kernel: A and B, and the J store of the fused variant (y, y', c keep the default policy)
//   NT_SOLVE    (on):  wg_getrs (newton_iter_kernel, ls_solve_kernel, the IC trial): the factors
//   NT_FINALIZE (on):  lu_finalize_kernel: the work matrix it reads, the factors it writes
//   NT_TRAIL    (off): lu_trail64w_kernel, n <= 1024: the A22 strips read and written, the U12 store to the factors (L21, L11, the
//                      pivot rows and the live list, which the column blocks of a matrix share, keep the default policy either
//                      way). Same registers, LDS and instruction counts, and 3 % slower in the stream: off.
#ifdef IDAHIP_NT_SYS
constexpr bool NT_SYS = IDAHIP_NT_SYS != 0;
#else
constexpr bool NT_SYS = true;
#endif
#ifdef IDAHIP_NT_SOLVE
constexpr bool NT_SOLVE = IDAHIP_NT_SOLVE != 0;
#else
constexpr bool NT_SOLVE = true;
#endif
#ifdef IDAHIP_NT_FINALIZE
constexpr bool NT_FINALIZE = IDAHIP_NT_FINALIZE != 0;
#else
constexpr bool NT_FINALIZE = true;
#endif
#ifdef IDAHIP_NT_TRAIL
constexpr bool NT_TRAIL = IDAHIP_NT_TRAIL != 0;
#else
constexpr bool NT_TRAIL = false;
#endif

}  // namespace tb
}  // namespace idahip
