"""rust-ida_amd/host/krylov_scalar.hpp on the host: a stand-alone g++ program (tests/native/krylov_scalar_check.cpp) runs the scalar
part of the SPGMR solver -- Givens update of each Hessenberg column, the convergence decision, the rotation of g with the
back-substitution, the flags -- on columns dumped from tests/krylov_ref.py; every bit it prints equals the reference's."""
import os
import subprocess

import krylov_cases as K
import krylov_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("heat1d", 9, 1), ("heat1d", 9, 5), ("heat1d", 65, 16), ("heat1d", 257, 5), ("linear_dense", 9, 5), ("linear_dense", 64, 16),
         ("linear_dense", 300, 16)]


def test_scalar_part_equals_the_reference_bit_for_bit(tmp_path):
    exe = str(tmp_path / "krylov_scalar_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "rust-ida_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "krylov_scalar_check.cpp")])
    text, want = [], []
    flags = set()
    for kind, n, maxl in CASES:
        c = K.solve_inputs(kind, n, maxl)
        for s in range(K.B):
            dump = []
            r = KR.spgmr_solve(KR.make_res(c["prob"], s), c["b"][s], c["ewt"][s], c["yy"][s], c["yp"][s], c["savres"][s], c["tn"][s],
                               c["cj"][s], c["tol"][s], maxl, dump=dump)
            _, beta, tol = dump[0]
            text.append("S %s %s %d" % (float(beta).hex(), float(tol).hex(), maxl))
            for l, col in dump[1:]:
                text.append("C %d %s" % (l, " ".join(float(v).hex() for v in col)))
            text.append("E")
            want.append((r["flag"], r.get("krydim", 0 if r["nli"] == 0 else maxl), r["nli"], r["res_norm"], r.get("g", []),
                         r["q"][:2 * r["krydim"]] if "q" in r else None))
            flags.add((r["flag"], r["nli"] == 0))
    assert {(0, True), (0, False), (1, False), (2, False)} <= flags
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(out) == len(want) + 1
    for line, (flag, krydim, nli, rho, g, q) in zip(out, want):
        head, gs, qs = (part.split() for part in line.split("|"))
        assert [int(v) for v in head[:3]] == [flag, krydim, nli], (line, flag, krydim, nli)
        assert float.fromhex(head[3]).hex() == float(rho).hex()
        assert [float.fromhex(v).hex() for v in gs] == [float(v).hex() for v in g]
        if q is not None:
            assert [float.fromhex(v).hex() for v in qs] == [float(v).hex() for v in q]
    last = out[-1].split()
    assert float.fromhex(last[1]) == KR.eplin(300, 0.33) and float.fromhex(last[3]) == 300.0 ** 0.5
