"""The band preconditioner's entry points at the drop-in boundary, without a device: declared in include/ida_hip.h, exported by the
built libidahip.so, present in the generated ida-hip-sys file and in the Python symbol list; null-ctx calls return -1 and touch
nothing; the two new counters are enumerated in include/ida_ensemble.h; header and DESIGN.md carry the definition."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("idahip_set_krylov_band_prec", "idahip_krylov_band_prec", "idahip_krylov_psetup", "idahip_krylov_psolve",
       "idahip_krylov_download_prec", "idahip_krylov_upload_prec")


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
    safe = open(os.path.join(ROOT, "bindings", "rust", "ida-hip", "src", "lib.rs")).read()
    assert re.search(r"pub fn with_band_prec\s*\(", safe)


def test_null_ctx_calls_return_minus_one():
    import idahip
    H, _ = idahip.load()
    assert H.idahip_set_krylov_band_prec(None, 1, 1) == -1
    assert H.idahip_krylov_band_prec(None, None, None) == -1
    assert H.idahip_krylov_psetup(None, None, None, None, None, None, 0) == -1
    assert H.idahip_krylov_psolve(None, None, None, None, 0) == -1
    assert H.idahip_krylov_download_prec(None, 0, None, None) == -1
    assert H.idahip_krylov_upload_prec(None, 0, None, None) == -1


def test_new_counters_are_enumerated():
    import idahip
    ens = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ida_ensemble.h")).read(), flags=re.S)
    assert re.search(r"\bIDAENS_C_NPE\s*=\s*19\b", ens) and re.search(r"\bIDAENS_C_NPS\s*=\s*20\b", ens)
    assert idahip.COUNTERS["npe"] == 19 and idahip.COUNTERS["nps"] == 20
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "ida-hip-sys", "src", "lib.rs")).read()
    assert "IDAENS_C_NPE" in sys_rs and "IDAENS_C_NPS" in sys_rs


def test_header_and_design_carry_the_definition():
    hdr = open(os.path.join(ROOT, "include", "ida_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (hdr, design):
        for word in ("psetup", "psolve", "IDABBDPRE", "zero-iteration", "1 + nli"):
            assert word in text, word
    assert "4i" in design
