"""The Krylov entry points at the drop-in boundary, without a device: declared in include/ida_hip.h, exported by the built libidahip.so,
present in the generated ida-hip-sys file and in the Python symbol list; null-ctx calls return -1 and touch nothing."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("idahip_create_krylov", "idahip_krylov", "idahip_set_krylov_fused", "idahip_krylov_fused", "idahip_krylov_solve",
       "idahip_newton_iter_krylov")


def test_new_symbols_in_header_library_sys_crate_and_python_list():
    import idahip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ida_hip.h")).read(), flags=re.S)
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "ida-hip-sys", "src", "lib.rs")).read()
    H = C.CDLL(idahip.LIB_HIP, mode=C.RTLD_GLOBAL)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(H, s), s
        assert re.search(r"pub fn %s\s*\(" % s, sys_rs), s
        assert s in idahip.HIP_SYMBOLS, s


def test_null_ctx_and_bad_creation_arguments():
    import idahip
    H, _ = idahip.load()
    assert H.idahip_krylov(None, None) == -1 and H.idahip_krylov_fused(None) == -1 and H.idahip_set_krylov_fused(None, 0) == -1
    assert H.idahip_krylov_solve(None, None, None, None, None, None, None, None, None, None, 0) == -1
    assert H.idahip_newton_iter_krylov(None, None, None, None, None, None, None, None, 0) == -1
    h = C.c_void_p()
    assert H.idahip_create_krylov(None, 0, 64, 1, 3, None, 5) == -1
    # refused before a device is looked for: n <= 8, n > 4096, maxl > 16, maxl > n, a kind without a Krylov form
    for n, maxl, kind in ((8, 5, 3), (4097, 5, 3), (64, 17, 3), (9, 10, 3), (3, 1, 0), (64, -1, 2)):
        assert H.idahip_create_krylov(C.byref(h), 0, n, 2, kind, None, maxl) == -2 and not h.value


def test_header_and_design_carry_the_definition():
    hdr = open(os.path.join(ROOT, "include", "ida_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (hdr, design):
        for word in ("kdot", "RES_REDUCED", "CONV_FAIL", "QRSOL_FAIL", "re-orthogonalisation"):
            assert word in text, word
    assert "4h" in design
