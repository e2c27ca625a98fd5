"""The switch that puts a reaction network of n <= 8 species on the one-thread stepper, at the drop-in boundary and without a
device: declared in include/ida_hip.h, exported by the built libidahip.so, in the Python symbol list with its two Ctx methods, in the
generated ida-hip-sys file (which is up to date with the headers) and in the ida-hip crate's ctx wrapper; null-ctx calls return -1."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("idahip_set_mass_action_tiny", "idahip_mass_action_tiny")


def test_header_declares_the_functions():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ida_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+idahip_set_mass_action_tiny\s*\(\s*idahip_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", txt)
    assert re.search(r"\bint\s+idahip_mass_action_tiny\s*\(\s*const\s+idahip_ctx\s*\*\s*\w*\s*\)\s*;", txt)
    ens = open(os.path.join(ROOT, "include", "ida_ensemble.h")).read()
    assert "Roberts, Lorenz63, and reaction networks that opted in" in ens


def test_python_binding_lists_them_and_ctx_has_the_methods():
    import idahip
    H = C.CDLL(idahip.LIB_HIP, mode=C.RTLD_GLOBAL)
    for s in NEW:
        assert s in idahip.HIP_SYMBOLS, s
        assert hasattr(H, s), s
    assert callable(idahip.Ctx.set_mass_action_tiny) and callable(idahip.Ctx.mass_action_tiny)
    L, _ = idahip.load()
    assert L.idahip_set_mass_action_tiny(None, 1) == -1 and L.idahip_mass_action_tiny(None) == -1


def test_generated_rust_sys_file_is_up_to_date():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"]).returncode == 0
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "ida-hip-sys", "src", "lib.rs")).read()
    for s in NEW:
        assert re.search(r"pub fn %s\s*\(" % s, sys_rs), s
    safe = open(os.path.join(ROOT, "bindings", "rust", "ida-hip", "src", "lib.rs")).read()
    assert re.search(r"pub fn set_mass_action_tiny\s*\(", safe) and re.search(r"pub fn mass_action_tiny\s*\(", safe)
