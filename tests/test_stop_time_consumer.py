"""The new prototypes -- idaens_set_stop_time, idaens_get_stop_time, idahip_set_suppress_alg, idahip_suppress_alg, idahip_wrms_masked
and IDAENS_BAD_TSTOP -- consumed from C99: tests/native/stop_time_consumer.c is compiled with -pedantic -Werror against both
headers and linked with both libraries. It opens no device: null handles are refused before anything else happens."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-ida_amd", "csrc")
HOST = os.path.join(ROOT, "rust-ida_amd", "host")


def test_stop_time_consumer_compiles_links_and_runs_as_c99(tmp_path):
    exe = str(tmp_path / "stop_time_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "stop_time_consumer.c"), "-L", HOST, "-lidaens", "-L", CSRC, "-lidahip",
                           "-Wl,-rpath," + HOST, "-Wl,-rpath," + CSRC])
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libidaens.so" in out and "libidahip.so" in out
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["TSTOP_RETURN", "1", "BAD_TSTOP", "-27", "null_calls", "-4", "wrms_masked", "1"], r.stdout
