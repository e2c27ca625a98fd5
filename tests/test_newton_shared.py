"""The Newton flow of rust-ida_amd/host/ida_controller.hpp on the host: a stand-alone g++ program (tests/native/newton_check.cpp) runs
every script -- initial jcur, call_lsetup, the result of each linear setup, the outcome of each convergence test, up to MAXNLSIT
iterations in each of the two passes a solve can take -- through the oracle's Newton::solve (oracle/newton.hpp) and through a driver
loop over newton_begin / newton_after_ctest, the functions every stepper instantiates, and asserts the same return code, niters,
nconvfails, jcur, curiter and sequence of sys / setup / solve calls, with either flavour of the setup's bookkeeping. It also checks
conv_test_core's compile-time iterations (ctest_kernel<0>, <1>) against a restatement with std::pow, and that pow(b, 1.0) is b bit for
bit. Built with -fsanitize=address,undefined and run as its own program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["direct_setup", "nojac_setup", "pow_identity", "conv_test_core"]
FLOW_STATEMENTS = ["curiter += 1", "nconvfails += 1", "curiter >= MAXNLSIT", "s.jcur = false"]


def test_newton_flow_against_the_oracle_on_every_script(tmp_path):
    exe = str(tmp_path / "newton_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "rust-ida_amd", "host"),
                           "-I", os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(ROOT, "tests", "native", "newton_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.split("\n")[:-1] == ["ok " + c for c in CASES] + ["all ok"], r.stdout
    assert r.stderr == "", r.stderr


def test_newton_flow_is_written_once():
    """The statements of Newton::solve's bookkeeping stand in ida_controller.hpp and nowhere else under rust-ida_amd/."""
    pkg = os.path.join(ROOT, "rust-ida_amd")
    hits = []
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".hpp", ".cpp", ".hip", ".h", ".py")) and f != "ida_controller.hpp":
                with open(os.path.join(d, f), errors="replace") as fh:
                    for i, line in enumerate(fh, 1):
                        hits += [(f, i, s) for s in FLOW_STATEMENTS if s in line]
    assert hits == [], hits
    own = open(os.path.join(pkg, "host", "ida_controller.hpp")).read()
    assert all(s in own for s in FLOW_STATEMENTS)
