"""The switch for the device lock-step rounds of a Krylov ctx at the drop-in boundary, without a device: declared in
include/ida_hip.h, exported by the built libidahip.so, in the Python symbol list with its two Ctx methods, in the generated
ida-hip-sys file (which is up to date with the headers) and in the ida-hip crate's ctx wrapper; null-ctx calls return -1."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = ("idahip_set_krylov_rounds", "idahip_krylov_rounds")
NEW = SWITCH + ("idahip_krylov_rounds_put_counters", "idahip_krylov_rounds_get_counters")


def test_header_declares_the_functions():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ida_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+idahip_set_krylov_rounds\s*\(\s*idahip_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", txt)
    assert re.search(r"\bint\s+idahip_krylov_rounds\s*\(\s*const\s+idahip_ctx\s*\*\s*\w*\s*\)\s*;", txt)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
    ens = open(os.path.join(ROOT, "include", "ida_ensemble.h")).read()
    assert "unless idahip_set_krylov_rounds" in ens


def test_python_binding_lists_them_and_ctx_has_the_methods():
    import idahip
    H = C.CDLL(idahip.LIB_HIP, mode=C.RTLD_GLOBAL)
    for s in NEW:
        assert s in idahip.HIP_SYMBOLS, s
        assert hasattr(H, s), s
    assert callable(idahip.Ctx.set_krylov_rounds) and callable(idahip.Ctx.krylov_rounds)
    L, _ = idahip.load()
    assert L.idahip_set_krylov_rounds(None, 1) == -1 and L.idahip_krylov_rounds(None) == -1
    assert L.idahip_krylov_rounds_put_counters(None, None, None) == -1 and L.idahip_krylov_rounds_get_counters(None, None, None) == -1


def test_generated_rust_sys_file_is_up_to_date():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"]).returncode == 0
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "ida-hip-sys", "src", "lib.rs")).read()
    for s in NEW:
        assert re.search(r"pub fn %s\s*\(" % s, sys_rs), s
    safe = open(os.path.join(ROOT, "bindings", "rust", "ida-hip", "src", "lib.rs")).read()
    assert re.search(r"pub fn set_krylov_rounds\s*\(", safe) and re.search(r"pub fn krylov_rounds\s*\(", safe)
