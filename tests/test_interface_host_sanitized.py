"""The host side of csrc/contact_interface.hip under AddressSanitizer + UndefinedBehaviorSanitizer, as a
stand-alone program with its own main (tests/host_interface_san.cpp): the translation unit and the driver
are compiled with build.SAN_FLAGS (every -fsanitize flag behind -Xarch_host: the host compilation only,
device code unchanged, no GPU sanitizer) and linked with the sanitizer runtimes, so the program needs
no preloaded runtime. It drives every refusal and the size / offset arithmetic of the interface-label
entry points with tables of exactly `count` items and extreme sizes; nothing is launched. Any ASan
report or UBSan runtime error fails the test."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_interface_entry_points_host_code_under_asan_ubsan():
    from deepinteract_amd import build
    outdir = os.path.join(build.LIBDIR, "asan")
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "host_interface_san")
    cmd = [build.HIPCC, *build.CFLAGS, *build.SAN_FLAGS, os.path.join(build.CSRC, "contact_interface.hip"),
           os.path.join(HERE, "host_interface_san.cpp"), "-fsanitize=address", "-fsanitize=undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "halt_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    assert "host_interface_san: ok" in r.stdout, out[-2000:]
