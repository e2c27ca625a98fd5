"""rust-ida_amd/host/ida_solve_flow.hpp on the host: a stand-alone g++ program (tests/native/roots_check.cpp) instantiates the text
that the host stepper and the device steppers share -- root finding, stop tests, loop-top checks, call entry -- with a closed-form
backend (y(t) a cubic per component) and checks it against what the polynomials say: the bracket around the analytic root, the
evaluation count, g exactly 0 at t0 / at the end of a step / again just after a root (CLOSE_ROOTS), both arms of the Illinois
weight point for point against a one-function restatement of the method, hand-counted runs for the end-of-bracket clamp and for two
functions crossing in one step, a failing root function, the stop tests in both task modes and the three exits of the loop-top
checks. Built with -fsanitize=address,undefined and run as its own program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["bracket_a_root", "zero_at_t0", "reentry_after_a_root", "zero_at_thi", "illinois_arms", "failing_root_function",
         "stop_tests_and_loop_top", "call_entry"]


def test_shared_flow_against_closed_form_roots(tmp_path):
    exe = str(tmp_path / "roots_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "rust-ida_amd", "host"),
                           "-o", exe, os.path.join(ROOT, "tests", "native", "roots_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.split("\n")[:-1] == ["ok " + c for c in CASES] + ["all ok"], r.stdout
    assert r.stderr == "", r.stderr
