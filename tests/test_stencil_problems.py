"""rust-ida_amd/csrc/stencil_problems.hpp on the host: a stand-alone g++ program (tests/native/stencil_check.cpp) evaluates the two
banded device problems' descriptions -- Heat1D and Bruss1D, the text every stencil kernel instantiates -- at seeded states and prints
the bits: every row of F, every Jacobian entry inside the band, and the kernels' band predicate up to two places outside it. Compared
here, bit pattern for bit pattern, with the numpy restatements the GPU tests use (dq_ref.heat_res / analytic_jac, bruss_ref.res /
jac). Heat at n = 9, 10, 23, the Brusselator at n = 10, 12. Built with -fsanitize=address,undefined and run as its own program: the
state vectors are exactly n long, so a row that reads past an end is an error."""
import os
import subprocess

import numpy as np

import bruss_ref as BR
import dq_ref as DQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("heat", 9), ("heat", 10), ("heat", 23), ("bruss", 10), ("bruss", 12)]


def _f64(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _parse(text):
    lines = text.split("\n")
    assert lines[-2:] == ["all ok", ""], lines[-3:]
    cases = []
    for ln in lines[:-2]:
        t = ln.split()
        if t[0] == "case":
            cases.append({"name": t[1], "n": int(t[2]), "nparam": int(t[3]), "half_bw": int(t[4]), "row": {}, "jac": {}, "band": {}})
        elif t[0] in ("y", "yp", "prm", "cj"):
            cases[-1][t[0]] = _f64(t[1:])
        elif t[0] == "row":
            cases[-1]["row"][int(t[1])] = t[2]
        elif t[0] == "jac":
            cases[-1]["jac"][(int(t[1]), int(t[2]))] = t[3]
        elif t[0] == "band":
            cases[-1]["band"][(int(t[1]), int(t[2]))] = int(t[3])
        else:
            raise AssertionError(ln)
    return cases


def test_descriptions_against_the_numpy_restatements(tmp_path):
    exe = str(tmp_path / "stencil_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "rust-ida_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "stencil_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stderr == "", r.stderr
    cases = _parse(r.stdout)
    assert [(c["name"], c["n"]) for c in cases] == CASES
    for c in cases:
        name, n, hb = c["name"], c["n"], c["half_bw"]
        y, yp, prm, cj = c["y"], c["yp"], c["prm"], float(c["cj"][0])
        assert y.size == n and yp.size == n and prm.size == c["nparam"]
        assert (c["nparam"], hb) == {"heat": (1, 1), "bruss": (5, 2)}[name]
        if name == "heat":
            want_res = DQ.heat_res(float(prm[0]), y, yp)
            want_jac = DQ.analytic_jac("heat1d", {"coef": prm[0]}, cj, y)
        else:
            want_res = BR.res(prm, y, yp)
            want_jac = BR.jac(prm, cj, y)
        # every row of F
        assert sorted(c["row"]) == list(range(n))
        got_res = _f64([c["row"][i] for i in range(n)])
        assert np.array_equal(_bits(got_res), _bits(want_res)), (name, n, got_res, want_res)
        # the band predicate: every (r, c) up to two places outside the band was asked, and exactly |r - c| <= HALF_BW is inside
        asked = {(i, j) for j in range(n) for i in range(max(0, j - hb - 2), min(n - 1, j + hb + 2) + 1)}
        assert set(c["band"]) == asked
        for (i, j), inside in c["band"].items():
            assert inside == (1 if abs(i - j) <= hb else 0), (name, n, i, j, inside)
        assert any(abs(i - j) == hb + 1 for (i, j) in c["band"]) and any(abs(i - j) == hb + 2 for (i, j) in c["band"])
        # every entry the predicate lets through, +0.0 everywhere else (what the kernels write there): the whole matrix, [column][row]
        assert set(c["jac"]) == {k for k, inside in c["band"].items() if inside}
        got_jac = np.zeros((n, n))
        for (i, j), w in c["jac"].items():
            got_jac[j, i] = _f64([w])[0]
        assert np.array_equal(_bits(got_jac), _bits(want_jac)), (name, n)
